// Per-image quality metrics of a stack of fp32 NHWC images against reference images in one launch
// (svae_op_image_metrics, include/svae_hip.h): sum (x - y)^2, sum |x - y|, mean SSIM over the valid window
// positions and channels, and the non-finite count of the two images.  Everything after the load is fp64.
//
// One block of 256 threads per image i; its reference is image i % ny of y.  Row i depends on those two images
// only: never on n, on the grid or on an address.
//
// Order of summation (fixed).
//  Elementwise columns: group G holds the image's elements 4 G .. 4 G + 3 (indices inside the image, whatever
//  its address); thread l takes the groups l, l + 256, ... in ascending order and adds element j of a group to
//  its accumulator j; the last group may be partial.  Then ((a0 + a1) + (a2 + a3)) per thread, a shuffle tree
//  over the wave (offsets 32 .. 1), the four waves in order.  A whole group is one 16-byte load per image when
//  both images are 16-byte aligned and four 4-byte loads otherwise: the same values into the same accumulators.
//  SSIM: channels in order, output tiles of TILE x TILE positions in row-major order.  A tile's (TILE + 10)^2
//  halo of x and y is staged in LDS as fp64; the horizontal pass forms the five window sums of x, y, x^2, y^2,
//  x y along a row (taps k = 0 .. 10 in order, one fma each; the product of two fp32 values is exact in fp64),
//  the vertical pass adds the rows k = 0 .. 10 in order.  Thread (r, q) of the 16 x 16 block owns position
//  (r, q) of every tile and adds its SSIM values in tile order; then the same wave tree and wave order.
// svae_op_image_metrics, with its argument checks, the window weights and the launch, ends the file.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "opentry.h"

namespace {

constexpr int IM_THREADS = 256;
constexpr int IM_WAVES = IM_THREADS / 64;
constexpr int IM_WIN = SVAE_SSIM_WINDOW;
constexpr int IM_TILE = SVAE_METRICS_TILE;
constexpr int IM_HALO = IM_TILE + IM_WIN - 1;
static_assert(IM_TILE * IM_TILE == IM_THREADS, "one thread per tile position");

struct SsimWeights {
  double g[IM_WIN];
};

struct ElemAcc {
  double sq[4], ab[4];
  int bad;
};

__device__ __forceinline__ void im_elem(float a, float b, int j, ElemAcc& acc) {
  const double d = (double)a - (double)b;
  acc.sq[j] = fma(d, d, acc.sq[j]);
  acc.ab[j] += fabs(d);
  acc.bad += (fabsf(a) <= FLT_MAX ? 0 : 1) + (fabsf(b) <= FLT_MAX ? 0 : 1);  // NaN and +-inf fail the comparison
}

__device__ __forceinline__ double im_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(IM_THREADS) void image_metrics_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ y, int ny, int h, int w,
                                                                   int c, double c1, double c2, SsimWeights wt,
                                                                   double* __restrict__ out) {
  __shared__ double tile[2][IM_HALO][IM_HALO];  // the halo of x and of y
  __shared__ double hs[5][IM_HALO][IM_TILE];    // horizontal window sums of x, y, x^2, y^2, x y
  __shared__ double red[IM_WAVES][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long per = (long long)h * w * c;
  const float* __restrict__ xi = x + (long long)blockIdx.x * per;
  const float* __restrict__ yi = y + (long long)(blockIdx.x % (unsigned)ny) * per;

  // ---- the elementwise columns
  ElemAcc acc;
#pragma unroll
  for (int j = 0; j < 4; ++j) acc.sq[j] = acc.ab[j] = 0.0;
  acc.bad = 0;
  const long long ng = per >> 2;  // whole groups
  if (((reinterpret_cast<uintptr_t>(xi) | reinterpret_cast<uintptr_t>(yi)) & 15) == 0) {
    for (long long g = tid; g < ng; g += IM_THREADS) {
      const float4 a = *reinterpret_cast<const float4*>(xi + 4 * g);
      const float4 b = *reinterpret_cast<const float4*>(yi + 4 * g);
      im_elem(a.x, b.x, 0, acc);
      im_elem(a.y, b.y, 1, acc);
      im_elem(a.z, b.z, 2, acc);
      im_elem(a.w, b.w, 3, acc);
    }
  } else {
    for (long long g = tid; g < ng; g += IM_THREADS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) im_elem(xi[4 * g + j], yi[4 * g + j], j, acc);
    }
  }
  const int rem = (int)(per & 3);  // the partial group is the last of the thread whose turn it is
  if (rem && tid == (int)(ng & (IM_THREADS - 1))) {
#pragma unroll
    for (int j = 0; j < 3; ++j)  // a static accumulator index keeps them in registers
      if (j < rem) im_elem(xi[4 * ng + j], yi[4 * ng + j], j, acc);
  }

  // ---- SSIM
  const int vh = h - (IM_WIN - 1), vw = w - (IM_WIN - 1);  // valid positions
  const int r = tid / IM_TILE, q = tid % IM_TILE;
  double ssim = 0.0;
  for (int ch = 0; ch < c; ++ch) {
    for (int ty = 0; ty < vh; ty += IM_TILE) {
      for (int tx = 0; tx < vw; tx += IM_TILE) {
        // the previous tile's readers of `tile` finished before its second barrier, those of `hs` finish
        // before this tile's first one
        for (int i = tid; i < IM_HALO * IM_HALO; i += IM_THREADS) {
          const int hr = i / IM_HALO, hq = i % IM_HALO;
          const int gy = ty + hr, gx = tx + hq;
          const bool in = gy < h && gx < w;  // outside: zeros, which only positions outside the valid region see
          const long long e = ((long long)gy * w + gx) * c + ch;
          tile[0][hr][hq] = in ? (double)xi[e] : 0.0;
          tile[1][hr][hq] = in ? (double)yi[e] : 0.0;
        }
        __syncthreads();
        for (int i = tid; i < IM_HALO * IM_TILE; i += IM_THREADS) {
          const int hr = i / IM_TILE, hq = i % IM_TILE;
          double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
          for (int k = 0; k < IM_WIN; ++k) {
            const double xv = tile[0][hr][hq + k], yv = tile[1][hr][hq + k], g = wt.g[k];
            a0 = fma(g, xv, a0);
            a1 = fma(g, yv, a1);
            a2 = fma(g, xv * xv, a2);
            a3 = fma(g, yv * yv, a3);
            a4 = fma(g, xv * yv, a4);
          }
          hs[0][hr][hq] = a0;
          hs[1][hr][hq] = a1;
          hs[2][hr][hq] = a2;
          hs[3][hr][hq] = a3;
          hs[4][hr][hq] = a4;
        }
        __syncthreads();
        if (ty + r < vh && tx + q < vw) {
          double mx = 0.0, my = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
          for (int k = 0; k < IM_WIN; ++k) {
            const double g = wt.g[k];
            mx = fma(g, hs[0][r + k][q], mx);
            my = fma(g, hs[1][r + k][q], my);
            sxx = fma(g, hs[2][r + k][q], sxx);
            syy = fma(g, hs[3][r + k][q], syy);
            sxy = fma(g, hs[4][r + k][q], sxy);
          }
          const double vx = sxx - mx * mx, vy = syy - my * my, cxy = sxy - mx * my;
          ssim += ((2.0 * mx * my + c1) * (2.0 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2));
        }
      }
    }
  }

  // ---- per thread, over the wave, the waves in order
  double col[4];
  col[0] = im_wave_sum((acc.sq[0] + acc.sq[1]) + (acc.sq[2] + acc.sq[3]));
  col[1] = im_wave_sum((acc.ab[0] + acc.ab[1]) + (acc.ab[2] + acc.ab[3]));
  col[2] = im_wave_sum(ssim);
  col[3] = im_wave_sum((double)acc.bad);  // at most 2 h w c: an integer, exact in fp64 in any order
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[wave][k] = col[k];
  }
  __syncthreads();
  if (tid < 4) {
    double v = red[0][tid];
#pragma unroll
    for (int k = 1; k < IM_WAVES; ++k) v += red[k][tid];
    if (tid == 2) v /= (double)vh * (double)vw * (double)c;
    out[(long long)blockIdx.x * 4 + tid] = v;
  }
}

}  // namespace

extern "C" {

int svae_op_image_metrics(const float* x, int n, const float* y, int ny, int h, int w, int c, float data_range,
                          double* out, void* stream) {
  if (!x || !y || !out) return op_fail(SVAE_EBADARG, "image_metrics: null pointer");
  if (n <= 0 || ny <= 0 || c <= 0) return op_fail(SVAE_EBADARG, "image_metrics: n, ny and c must be positive");
  if (n % ny != 0) return op_fail(SVAE_EBADARG, "image_metrics: n must be a multiple of ny");
  if (h < SVAE_SSIM_WINDOW || w < SVAE_SSIM_WINDOW)
    return op_fail(SVAE_EBADARG, "image_metrics: h and w must hold one " + std::to_string(SVAE_SSIM_WINDOW) +
                                     "-wide window");
  if (!(data_range > 0.f)) return op_fail(SVAE_EBADARG, "image_metrics: data_range must be > 0");
  SsimWeights wt;
  double sum = 0.0;
  for (int k = 0; k < IM_WIN; ++k) {
    const double d = (double)(k - IM_WIN / 2);
    wt.g[k] = std::exp(-(d * d) / (2.0 * SVAE_SSIM_SIGMA * SVAE_SSIM_SIGMA));
    sum += wt.g[k];
  }
  for (int k = 0; k < IM_WIN; ++k) wt.g[k] /= sum;
  const double L = (double)data_range;
  const double c1 = (SVAE_SSIM_K1 * L) * (SVAE_SSIM_K1 * L), c2 = (SVAE_SSIM_K2 * L) * (SVAE_SSIM_K2 * L);
  hipLaunchKernelGGL(image_metrics_kernel, dim3((unsigned)n), dim3(IM_THREADS), 0, (hipStream_t)stream, x, y, ny, h, w,
                     c, c1, c2, wt, out);
  return op_done();
}

}  // extern "C"
