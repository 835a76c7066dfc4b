// Binned power spectra of a stack of fp32 NHWC images, and of their differences to reference images, in one launch
// (svae_op_power_spectrum, include/svae_hip.h): a windowed two-dimensional DFT per (image, channel) straight from
// the caller's twiddle tables, the half spectrum's power with its multiplicity, and the sums over the caller's bin
// table.  Everything after the load is fp64 on the vector ALU, every operation rounded on its own (contraction is
// off in this file), in the order the header states; no atomics, no fp64 MFMA (its summation order is not stated).
//
// One block of 256 threads per (image i, channel k); the partner is image i % ny of y.  A block's rows depend on
// those two images and the tables only: never on n, on the grid or on an address.  With wu = w / 2 + 1, per plane
// (0: the image, 1: the difference x - y):
//  stage   the image is walked in groups of four consecutive floats (all channels), one 16-byte load per image
//          where the images are 16-byte aligned and four 4-byte loads where not; the elements of channel k go to
//          LDS as a[yy][xx] = (value * win_y[yy]) * win_x[xx] in fp64, and the non-finite ones are counted
//          (plane 0 counts x, plane 1 counts y: integers, exact in any order)
//  rows    T[yy][u] = sum over ascending xx of a * tw_x[(u xx) mod w], the index advanced by u and reduced by one
//          subtraction; T stays in LDS as complex fp64.  An item is (u, the two rows j and j + ceil(h / 2)), the
//          lanes of a wave along j: the twiddle is read once for both rows and is the same address in (nearly)
//          every lane, and the image rows are an odd number of doubles apart, so the lanes' reads fall in
//          different banks
//  columns F[v][u] = sum over ascending yy of T[yy][u] * tw_y[(v yy) mod h], the complex product written out as
//          (tr c - ti s, tr s + ti c); an item is (the two rows j and j + ceil(h / 2) of F, u), the lanes along u: T
//          is read once for both.  P = (Re Re + Im Im) * m(u) replaces the dead image in LDS
//  bins    thread u < wu walks its column in ascending v and adds P[v][u] to its own row part[u][bin[v][u]] (LDS,
//          zeroed before); thread b then adds part[0 .. wu - 1][b] in ascending u and writes out[b]
// Two outputs per item change which thread forms a sum, never the sum: each keeps its own accumulators and order.
// LDS: max(h (w | 1), h wu + wu n_bins) + 2 h wu + 3 (h + w) doubles (+ 16 bytes): 69 KB at 64 x 64 with 33 bins
// (two blocks per CU), 151 KB at SVAE_SPECTRUM_MAX_DIM square; all of it dynamic, the attribute is set once per
// device.
// svae_op_power_spectrum, with its argument checks, ends the file.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <mutex>

#include "common.h"
#include "opentry.h"

#pragma clang fp contract(off)

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;
static_assert(SVAE_SPECTRUM_MAX_DIM / 2 + 1 <= PS_THREADS, "one thread per column in the binning pass");

struct PsArgs {
  const float* x;
  const float* y;  // nullptr: plane 0 only
  int ny, h, w, c;
  const double *win_y, *win_x, *tw_y, *tw_x;
  const int* bin;
  int n_bins;
  double* out;
  long long* nonfinite;  // may be nullptr
};

// doubles in the region that holds the staged image, then the powers and the per-column bin partials (even: the
// complex table behind it stays 16-byte aligned)
__host__ __device__ inline int ps_region(int h, int w, int n_bins) {
  const int wu = w / 2 + 1, a = h * (w | 1), b = h * wu + wu * n_bins;  // image rows w | 1 doubles apart
  const int r = a > b ? a : b;
  return r + (r & 1);
}

inline size_t ps_lds_bytes(int h, int w, int n_bins) {
  const int wu = w / 2 + 1;
  return ((size_t)ps_region(h, w, n_bins) + 2 * (size_t)h * wu + 3 * (size_t)(h + w)) * sizeof(double) + 16;
}

__device__ __forceinline__ int ps_bad(float v) { return fabsf(v) <= FLT_MAX ? 0 : 1; }  // NaN and +-inf fail

__global__ __launch_bounds__(PS_THREADS) void power_spectrum_kernel(PsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ps_smem[];
  const int h = a.h, w = a.w, c = a.c, wu = w / 2 + 1, nb = a.n_bins;
  const int hw = h * w, hu = h * wu;
  const int wp = w | 1;          // doubles between two staged image rows
  const int hh = (h + 1) >> 1;   // an item of the two passes holds the rows j and j + hh
  double* const R = reinterpret_cast<double*>(ps_smem);
  double2* const T = reinterpret_cast<double2*>(R + ps_region(h, w, nb));
  double2* const twx = T + hu;
  double2* const twy = twx + w;
  double* const winx = reinterpret_cast<double*>(twy + h);
  double* const winy = winx + w;
  int* const red = reinterpret_cast<int*>(winy + h);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = (int)(blockIdx.x / (unsigned)c), ch = (int)(blockIdx.x % (unsigned)c);
  const long long per = (long long)hw * c;  // <= 2^31 - 1 (checked by the entry point)
  const float* __restrict__ xi = a.x + (long long)img * per;
  const float* __restrict__ yi = a.y ? a.y + (long long)(img % a.ny) * per : nullptr;

  for (int i = tid; i < w; i += PS_THREADS) {
    twx[i] = make_double2(a.tw_x[2 * i], a.tw_x[2 * i + 1]);
    winx[i] = a.win_x[i];
  }
  for (int i = tid; i < h; i += PS_THREADS) {
    twy[i] = make_double2(a.tw_y[2 * i], a.tw_y[2 * i + 1]);
    winy[i] = a.win_y[i];
  }
  __syncthreads();

  long long nonfinite = 0;  // thread 0's total over the planes
  const int planes = yi ? 2 : 1;
  for (int plane = 0; plane < planes; ++plane) {
    // ---- stage: R[yy * wp + xx] = the windowed value of channel ch (R's previous readers passed the plane's
    // last barrier)
    int bad = 0;
    // one group of four consecutive floats of the image: one division finds its first element's pixel and
    // channel, the other three follow by counting
    auto group = [&](int g, float x0, float x1, float x2, float x3, float y0, float y1, float y2, float y3, int cnt) {
      const float xv[4] = {x0, x1, x2, x3}, yv[4] = {y0, y1, y2, y3};
      int p = (4 * g) / c, r = 4 * g - p * c;
      int yy = p / w, xx = p - yy * w;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e < cnt && r == ch) {
          const double v = plane ? (double)xv[e] - (double)yv[e] : (double)xv[e];  // exact: two fp32 values
          R[yy * wp + xx] = (v * winy[yy]) * winx[xx];
          bad += ps_bad(plane ? yv[e] : xv[e]);
        }
        if (++r == c) {
          r = 0;
          if (++xx == w) {
            xx = 0;
            ++yy;
          }
        }
      }
    };
    const int ng = (int)(per >> 2);  // whole groups
    uintptr_t addr = reinterpret_cast<uintptr_t>(xi);
    if (plane) addr |= reinterpret_cast<uintptr_t>(yi);
    if ((addr & 15) == 0) {
#pragma unroll 4
      for (int g = tid; g < ng; g += PS_THREADS) {
        const float4 xv = *reinterpret_cast<const float4*>(xi + 4 * g);
        float4 yv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (plane) yv = *reinterpret_cast<const float4*>(yi + 4 * g);
        group(g, xv.x, xv.y, xv.z, xv.w, yv.x, yv.y, yv.z, yv.w, 4);
      }
    } else {
#pragma unroll 4
      for (int g = tid; g < ng; g += PS_THREADS) {
        const float* __restrict__ xg = xi + 4 * g;
        if (plane) {
          const float* __restrict__ yg = yi + 4 * g;
          group(g, xg[0], xg[1], xg[2], xg[3], yg[0], yg[1], yg[2], yg[3], 4);
        } else {
          group(g, xg[0], xg[1], xg[2], xg[3], 0.f, 0.f, 0.f, 0.f, 4);
        }
      }
    }
    const int rem = (int)(per & 3);  // the partial last group
    if (rem && tid == 0) {
      float xv[3] = {0.f, 0.f, 0.f}, yv[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        if (e < rem) {
          xv[e] = xi[4LL * ng + e];
          if (plane) yv[e] = yi[4LL * ng + e];
        }
      }
      group(ng, xv[0], xv[1], xv[2], 0.f, yv[0], yv[1], yv[2], 0.f, rem);
    }
    if (a.nonfinite) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o, 64);
      if (lane == 0) red[wave] = bad;  // read by thread 0 behind the next barrier, rewritten two barriers later
    }
    __syncthreads();
    if (a.nonfinite && tid == 0) {
#pragma unroll
      for (int k = 0; k < PS_WAVES; ++k) nonfinite += red[k];
    }

    // ---- rows: T[yy][u] = sum_xx a[yy][xx] * tw_x[(u xx) mod w]
    for (int it = tid; it < wu * hh; it += PS_THREADS) {
      const int u = it / hh, j = it - u * hh;
      const bool two = j + hh < h;  // odd h: the last item has one row (it reads that row twice, stores it once)
      const double* __restrict__ a0 = R + j * wp;
      const double* __restrict__ a1 = R + (two ? j + hh : j) * wp;
      double re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
      int k = 0;
#pragma unroll 4
      for (int xx = 0; xx < w; ++xx) {
        const double2 t = twx[k];
        const double v0 = a0[xx], v1 = a1[xx];
        re0 = re0 + v0 * t.x;
        im0 = im0 + v0 * t.y;
        re1 = re1 + v1 * t.x;
        im1 = im1 + v1 * t.y;
        k += u;  // u <= w / 2: one subtraction reduces it
        if (k >= w) k -= w;
      }
      T[j * wu + u] = make_double2(re0, im0);
      if (two) T[(j + hh) * wu + u] = make_double2(re1, im1);
    }
    __syncthreads();

    // ---- columns and power; the staged image is dead, P takes R[0, hu) and the partials R[hu, hu + wu nb)
    for (int it = tid; it < hh * wu; it += PS_THREADS) {
      const int j = it / wu, u = it - j * wu;
      const bool two = j + hh < h;
      const int v1 = two ? j + hh : j;
      double re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
      int k0 = 0, k1 = 0;
#pragma unroll 4
      for (int yy = 0; yy < h; ++yy) {
        const double2 t = T[yy * wu + u];
        const double2 q0 = twy[k0], q1 = twy[k1];
        const double pr0 = t.x * q0.x - t.y * q0.y;
        const double pi0 = t.x * q0.y + t.y * q0.x;
        const double pr1 = t.x * q1.x - t.y * q1.y;
        const double pi1 = t.x * q1.y + t.y * q1.x;
        re0 = re0 + pr0;
        im0 = im0 + pi0;
        re1 = re1 + pr1;
        im1 = im1 + pi1;
        k0 += j;  // j, v1 < h: one subtraction reduces them
        if (k0 >= h) k0 -= h;
        k1 += v1;
        if (k1 >= h) k1 -= h;
      }
      const bool once = u == 0 || 2 * u == w;
      const double p0 = re0 * re0 + im0 * im0, p1 = re1 * re1 + im1 * im1;
      R[j * wu + u] = once ? p0 : p0 * 2.0;
      if (two) R[(j + hh) * wu + u] = once ? p1 : p1 * 2.0;
    }
    for (int i = tid; i < wu * nb; i += PS_THREADS) R[hu + i] = 0.0;
    __syncthreads();

    // ---- bins: per column in ascending v, then the columns in ascending u
    if (tid < wu) {
      const double* __restrict__ pw = R + tid;      // the column's powers: [0, hu), apart from the partials
      const int* __restrict__ bcol = a.bin + tid;
      double* __restrict__ part = R + hu + tid * nb;
#pragma unroll 8
      for (int v = 0; v < h; ++v) {  // (unrolled: the table's loads and the powers' reads go out ahead of the adds)
        const int b = bcol[v * wu];
        const double pv = pw[v * wu];
        if ((unsigned)b < (unsigned)nb) part[b] = part[b] + pv;  // -1 (or any other value): skipped
      }
    }
    __syncthreads();
    double* __restrict__ o = a.out + (((long long)blockIdx.x * 2 + plane) * nb);
    for (int b = tid; b < nb; b += PS_THREADS) {
      double s = 0.0;
      for (int u = 0; u < wu; ++u) s = s + R[hu + u * nb + b];
      o[b] = s;
    }
    __syncthreads();
  }
  if (a.nonfinite && tid == 0) a.nonfinite[blockIdx.x] = nonfinite;
}

int ps_device() {
  int d = 0;
  (void)hipGetDevice(&d);
  return d >= 0 && d < 64 ? d : 0;
}

// the dynamic-LDS attribute is per device: set once each, by whichever host thread comes first, and its result kept
hipError_t ps_lds_attribute() {
  static std::once_flag once[64];
  static hipError_t attr[64];
  const int dev = ps_device();
  std::call_once(once[dev], [dev] {
    attr[dev] = hipFuncSetAttribute(
        (const void*)power_spectrum_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)ps_lds_bytes(SVAE_SPECTRUM_MAX_DIM, SVAE_SPECTRUM_MAX_DIM, SVAE_SPECTRUM_MAX_BINS));
  });
  return attr[dev];
}

}  // namespace

extern "C" {

int svae_op_power_spectrum(const float* x, int n, const float* y, int ny, int h, int w, int c, const double* win_y,
                           const double* win_x, const double* tw_y, const double* tw_x, const int32_t* bin, int n_bins,
                           double* out, int64_t* nonfinite, void* stream) {
  if (!x || !win_y || !win_x || !tw_y || !tw_x || !bin || !out)
    return op_fail(SVAE_EBADARG, "power_spectrum: null pointer");
  if (n <= 0 || ny <= 0 || c <= 0 || n_bins <= 0)
    return op_fail(SVAE_EBADARG, "power_spectrum: n, ny, c and n_bins must be positive");
  if (h < 2 || w < 2) return op_fail(SVAE_EBADARG, "power_spectrum: h and w must be at least 2");
  if (y && n % ny != 0) return op_fail(SVAE_EBADARG, "power_spectrum: n must be a multiple of ny");
  if (h > SVAE_SPECTRUM_MAX_DIM || w > SVAE_SPECTRUM_MAX_DIM || n_bins > SVAE_SPECTRUM_MAX_BINS)
    return op_fail(SVAE_EBADCONFIG, "power_spectrum: at most " + std::to_string(SVAE_SPECTRUM_MAX_DIM) +
                                        " rows and columns and " + std::to_string(SVAE_SPECTRUM_MAX_BINS) +
                                        " bins");
  if ((int64_t)h * w * c > 2147483647LL || (int64_t)n * c > 2147483647LL)
    return op_fail(SVAE_EBADCONFIG, "power_spectrum: h * w * c or n * c above 2^31 - 1");
  const hipError_t e = ps_lds_attribute();
  if (e != hipSuccess) return op_fail(SVAE_EHIP, hipGetErrorString(e));
  PsArgs a{x, y, ny, h, w, c, win_y, win_x, tw_y, tw_x, bin, n_bins, out, (long long*)nonfinite};
  hipLaunchKernelGGL(power_spectrum_kernel, dim3((unsigned)n * (unsigned)c), dim3(PS_THREADS), ps_lds_bytes(h, w, n_bins),
                     (hipStream_t)stream, a);
  return op_done();
}

}  // extern "C"
