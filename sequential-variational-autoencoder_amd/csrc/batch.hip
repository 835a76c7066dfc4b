// The training batch in one launch: gather rows of a device-resident dataset (uint8 or fp32), dequantise
// into the clean target, and corrupt a copy into the denoising input (the reference's apply_noise,
// trainer.py:71-78: pepper multiplies by 0, salt adds 1, Gaussian noise, clip to the data range).
//
// Random draws are counter-based (philox.h): flat output element e of the [n * per_image] batch belongs to
// group g = e / 4, lane j = e % 4; the 64-bit counter offset + g fills c0 / c1, c3 = 0 and c2 selects the
// stream (philox.h: normals, pepper word, salt word).  Nothing depends on the launch geometry or on the path
// (vector / scalar) the alignment selects.
// MakeBatchArgs and the pixel noise are corrupt.h's, the dequantisation pixel.h's; svae_op_make_batch ends the file.
#include <cstdint>

#include "common.h"
#include "corrupt.h"
#include "opentry.h"
#include "pixel.h"

namespace {

constexpr int MB_THREADS = 256;
constexpr int MB_TILE = MB_THREADS * 16;  // elements of one uint8 tile: one 16-byte load per lane

__device__ __forceinline__ long long mb_row(const MakeBatchArgs& a, long long b) {
  return a.idx ? (long long)a.idx[b] : a.start + b;
}

// fp32 rows, per_image % 4 == 0, every pointer 16-byte aligned: one group per lane, 16-byte load and stores
__global__ __launch_bounds__(MB_THREADS) void make_batch_f32v_kernel(MakeBatchArgs a) {
  const long long G = a.total >> 2;
  const float* __restrict__ data = (const float*)a.data;
  for (long long g = (long long)blockIdx.x * MB_THREADS + threadIdx.x; g < G; g += (long long)gridDim.x * MB_THREADS) {
    const long long e = g << 2;
    const long long b = e / a.per_image, off = e - b * a.per_image;
    const float4 x = *reinterpret_cast<const float4*>(data + mb_row(a, b) * a.per_image + off);
    const float t[4] = {x.x, x.y, x.z, x.w};
    if (a.input) {  // in place (input == data) is safe: the lane has read what it overwrites
      float o[4];
      mb_corrupt(t, g, a, o);
      *reinterpret_cast<float4*>(a.input + e) = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (a.target) *reinterpret_cast<float4*>(a.target + e) = x;
  }
}

// uint8 rows, per_image % 16 == 0, every pointer 16-byte aligned: a tile of 4096 pixels is staged through
// LDS with one 16-byte load per lane (16 pixels), then lane l takes groups l, l + 256, ... of the tile so
// that every store instruction of a wave covers 1 KiB of contiguous output
__global__ __launch_bounds__(MB_THREADS) void make_batch_u8v_kernel(MakeBatchArgs a) {
  __shared__ uint4 stage[MB_THREADS];
  const unsigned char* __restrict__ data = (const unsigned char*)a.data;
  const long long ntile = (a.total + MB_TILE - 1) / MB_TILE;
  for (long long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const long long e0 = tile * MB_TILE + (long long)threadIdx.x * 16;
    if (e0 < a.total) {  // total % 16 == 0: a 16-pixel chunk is whole, inside one row and aligned
      const long long b = e0 / a.per_image, off = e0 - b * a.per_image;
      stage[threadIdx.x] = *reinterpret_cast<const uint4*>(data + mb_row(a, b) * a.per_image + off);
    }
    __syncthreads();
    const unsigned* words = reinterpret_cast<const unsigned*>(stage);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = k * MB_THREADS + threadIdx.x;
      const long long e = tile * MB_TILE + (long long)q * 4;
      if (e < a.total) {
        float t[4];
        u8_dequant4(words[q], a.lo, a.qscale, t);
        if (a.input) {
          float o[4];
          mb_corrupt(t, e >> 2, a, o);
          *reinterpret_cast<float4*>(a.input + e) = make_float4(o[0], o[1], o[2], o[3]);
        }
        if (a.target) *reinterpret_cast<float4*>(a.target + e) = make_float4(t[0], t[1], t[2], t[3]);
      }
    }
    __syncthreads();
  }
}

// any per_image and alignment: one group per lane, element by element (groups may straddle rows; the last
// group may be partial)
template <bool U8>
__global__ __launch_bounds__(MB_THREADS) void make_batch_scalar_kernel(MakeBatchArgs a) {
  const long long G = (a.total + 3) >> 2;
  for (long long g = (long long)blockIdx.x * MB_THREADS + threadIdx.x; g < G; g += (long long)gridDim.x * MB_THREADS) {
    const long long e = g << 2;
    long long b = e / a.per_image, off = e - b * a.per_image;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e + j < a.total) {
        const long long src = mb_row(a, b) * a.per_image + off;
        t[j] = U8 ? u8_dequant(((const unsigned char*)a.data)[src], a.lo, a.qscale) : ((const float*)a.data)[src];
      }
      if (++off == a.per_image) { off = 0; ++b; }
    }
    float o[4];
    if (a.input) mb_corrupt(t, g, a, o);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (e + j < a.total) {
        if (a.input) a.input[e + j] = o[j];
        if (a.target) a.target[e + j] = t[j];
      }
  }
}

void make_batch(const MakeBatchArgs& a, hipStream_t s) {
  const bool al = al16(a.data) && al16(a.target) && al16(a.input);
  const long long cap = 16384;  // grid-stride beyond this many blocks
  if (a.data_u8 && al && a.per_image % 16 == 0) {
    const long long nb = (a.total + MB_TILE - 1) / MB_TILE;
    hipLaunchKernelGGL(make_batch_u8v_kernel, dim3((unsigned)(nb < cap ? nb : cap)), dim3(MB_THREADS), 0, s, a);
    return;
  }
  const long long nb = ((a.total + 3) / 4 + MB_THREADS - 1) / MB_THREADS;
  const dim3 grid((unsigned)(nb < cap ? nb : cap));
  if (!a.data_u8 && al && a.per_image % 4 == 0)
    hipLaunchKernelGGL(make_batch_f32v_kernel, grid, dim3(MB_THREADS), 0, s, a);
  else if (a.data_u8)
    hipLaunchKernelGGL(make_batch_scalar_kernel<true>, grid, dim3(MB_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(make_batch_scalar_kernel<false>, grid, dim3(MB_THREADS), 0, s, a);
}

}  // namespace

extern "C" {

int svae_op_make_batch(const void* data, int data_u8, const int32_t* idx, int64_t start, int n, int64_t per_image,
                       float lo, float hi, float pepper_prob, float salt_prob, float gaussian_scale, uint64_t seed,
                       uint64_t offset, float* target, float* input, void* stream) {
  if (!data) return op_fail(SVAE_EBADARG, "make_batch: null data");
  if (!target && !input) return op_fail(SVAE_EBADARG, "make_batch: target and input are both null");
  if (n <= 0 || per_image <= 0) return op_fail(SVAE_EBADARG, "make_batch: n and per_image must be positive");
  if (!(pepper_prob >= 0.f && pepper_prob <= 1.f) || !(salt_prob >= 0.f && salt_prob <= 1.f))
    return op_fail(SVAE_EBADARG, "make_batch: a probability outside [0, 1]");
  if (!(gaussian_scale >= 0.f)) return op_fail(SVAE_EBADARG, "make_batch: negative gaussian_scale");
  if (!(lo <= hi)) return op_fail(SVAE_EBADARG, "make_batch: lo > hi");
  if (!idx && start < 0) return op_fail(SVAE_EBADARG, "make_batch: negative start");
  // in place: every lane overwrites exactly what it read, which holds only for the identity gather of fp32 rows
  if (((const void*)input == data || (const void*)target == data) && (data_u8 || idx || start != 0))
    return op_fail(SVAE_EBADARG, "make_batch: in place needs fp32 data, idx == NULL and start == 0");
  MakeBatchArgs a{};
  a.data = data; a.data_u8 = data_u8 ? 1 : 0;
  a.idx = idx; a.start = start;
  a.per_image = per_image; a.total = (long long)n * per_image;
  a.lo = lo; a.hi = hi;
  a.qscale = quant_scale(lo, hi).qscale;
  a.scale = gaussian_scale;
  a.thr_pepper = prob_threshold(pepper_prob); a.thr_salt = prob_threshold(salt_prob);
  a.seed = seed; a.offset = offset;
  a.target = target; a.input = input;
  make_batch(a, (hipStream_t)stream);
  return op_done();
}

}  // extern "C"
