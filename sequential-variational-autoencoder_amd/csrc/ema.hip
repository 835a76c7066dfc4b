// Polyak (exponential moving) average of the flat parameter buffer (svae_op_ema, svae_set_ema;
// include/svae_hip.h): TF's ExponentialMovingAverage.apply in its assign_sub form
//
//   e' = e - omd * (e - w)          omd = (float)(1 - decay_t)
//
// with the difference, the product and the outer difference each rounded to fp32 on their own (no fma: the
// pragma below, as in batch.hip and tiles.hip).  Element i depends on e[i], w[i] and omd only: not on the
// launch geometry and not on the path (16-byte or element by element) the alignment selects.
//
// A pure stream: 8 bytes read and 4 written per element, no reuse, no atomics, no LDS.  A block owns
// EMA_UNROLL * 256 consecutive 16-byte groups per sweep and a lane keeps EMA_UNROLL loads of each stream in
// flight (64 bytes per lane, 16 KiB per block) before its first store; the grid is capped and strides over
// the rest.  Both streams are read once and not again before the next training step, so the loads are
// non-temporal (the hint changes the cache policy, not a value): over the 74.9 M live floats of preset celeba
// that, and the block-contiguous layout, took the kernel from 191 us to 133 us.
// ema_update is the launcher the engine calls after Adam (kernels.h); svae_op_ema, with its checks, ends the file.
#include <cstdint>

#include "common.h"
#include "kernels.h"
#include "opentry.h"

namespace {

constexpr int EMA_THREADS = 256;
constexpr int EMA_UNROLL = 2;  // 16-byte groups per lane and sweep

__device__ __forceinline__ float ema_one(float e, float w, float omd) {
#pragma clang fp contract(off)
  const float d = e - w;
  const float p = omd * d;
  return e - p;
}

typedef float ema_v4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ ema_v4 ema_four(const ema_v4& e, const ema_v4& w, float omd) {
  ema_v4 r;
  r.x = ema_one(e.x, w.x, omd);
  r.y = ema_one(e.y, w.y, omd);
  r.z = ema_one(e.z, w.z, omd);
  r.w = ema_one(e.w, w.w, omd);
  return r;
}

// e[head + 4 g], g in [0, nvec), is 16-byte aligned; WV: so is w[head + 4 g].  The head [0, head) and the
// tail [head + 4 nvec, n), fewer than 4 elements each, go element by element through the first lanes of block 0.
template <bool WV>
__global__ __launch_bounds__(EMA_THREADS) void ema_kernel(float* __restrict__ e, const float* __restrict__ w,
                                                          long long n, int head, long long nvec, float omd) {
  const long long sweep = (long long)gridDim.x * (EMA_UNROLL * EMA_THREADS);
  float* ev = e + head;
  const float* wv = w + head;
  for (long long g0 = (long long)blockIdx.x * (EMA_UNROLL * EMA_THREADS) + threadIdx.x; g0 < nvec; g0 += sweep) {
    ema_v4 a[EMA_UNROLL], b[EMA_UNROLL];
#pragma unroll
    for (int k = 0; k < EMA_UNROLL; ++k) {
      const long long g = g0 + k * EMA_THREADS;
      if (g < nvec) {
        a[k] = __builtin_nontemporal_load(reinterpret_cast<const ema_v4*>(ev + 4 * g));
        if (WV) {
          b[k] = __builtin_nontemporal_load(reinterpret_cast<const ema_v4*>(wv + 4 * g));
        } else {
          const float* q = wv + 4 * g;
          b[k].x = __builtin_nontemporal_load(q);
          b[k].y = __builtin_nontemporal_load(q + 1);
          b[k].z = __builtin_nontemporal_load(q + 2);
          b[k].w = __builtin_nontemporal_load(q + 3);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < EMA_UNROLL; ++k) {
      const long long g = g0 + k * EMA_THREADS;
      if (g < nvec) *reinterpret_cast<ema_v4*>(ev + 4 * g) = ema_four(a[k], b[k], omd);
    }
  }
  if (blockIdx.x == 0) {
    const long long t0 = head + 4 * nvec;
    const int t = threadIdx.x;
    if (t < head) e[t] = ema_one(e[t], w[t], omd);
    if (t0 + t < n && t < 4) e[t0 + t] = ema_one(e[t0 + t], w[t0 + t], omd);
  }
}

inline int mis16(const void* p) { return (int)(reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace

// the launchers' usual element-wise grid (misc.hip): one block per EMA_THREADS work items, at most 4096 blocks
static int ew_blocks(long long work, int per = EMA_THREADS, int cap = 4096) {
  long long b = (work + per - 1) / per;
  return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}

void ema_update(float* ema, const float* w, long long n, float omd, hipStream_t s) {
  if (n <= 0 || omd == 0.f) return;
  // floats are 4-byte aligned: the head brings ema to a 16-byte boundary (a buffer shorter than it is all head)
  long long head = ((16 - mis16(ema)) & 15) >> 2;
  if (head > n) head = n;
  const long long nvec = (n - head) >> 2;
  const int blocks = ew_blocks((nvec + EMA_UNROLL - 1) / EMA_UNROLL);
  if (mis16(w + head) == 0)
    hipLaunchKernelGGL(ema_kernel<true>, dim3(blocks), dim3(EMA_THREADS), 0, s, ema, w, n, (int)head, nvec, omd);
  else
    hipLaunchKernelGGL(ema_kernel<false>, dim3(blocks), dim3(EMA_THREADS), 0, s, ema, w, n, (int)head, nvec, omd);
}

extern "C" {

int svae_op_ema(float* ema, const float* w, int64_t n, float omd, void* stream) {
  if (!ema || !w) return op_fail(SVAE_EBADARG, "ema: null pointer");
  if (n <= 0) return op_fail(SVAE_EBADARG, "ema: n must be positive");
  if (!(omd >= 0.f && omd <= 1.f)) return op_fail(SVAE_EBADARG, "ema: omd must be in [0, 1]");
  if (omd == 0.f) return 0;
  ema_update(ema, w, n, omd, (hipStream_t)stream);
  return op_done();
}

}  // extern "C"
