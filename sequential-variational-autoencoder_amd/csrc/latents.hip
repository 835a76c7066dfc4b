// Log-density of nq query rows under an equal-weight mixture of nm diagonal Gaussians, per segment of dimensions
// (svae_op_mixture_logdensity, include/svae_hip.h).  Everything after the load is fp64; no [nq, nm] intermediate.
//
// A block is ML_ROWS query rows x ML_SLOTS waves: lane r of every wave owns row r of the block, wave k owns the
// k-th chunk of ML_SEGS consecutive segments of the block's group (blockIdx.y: ML_GROUP = ML_SLOTS * ML_SEGS
// consecutive segments of the caller's list), and a thread keeps a (running max, running sum) pair per segment
// of its chunk in registers.  Only the dimensions inside the group's hull [jlo, jhi) are staged: the block's z
// rows once (transposed, zs[j][row], one bank per lane), and per tile of ML_TILE components mu, 1 / sigma and
// -log sigma - log(2 pi) / 2, which every lane of a wave reads at the same address (a broadcast).
//
// Order of evaluation (fixed; contraction is off in this file, every fma is written out).  For query n,
// component m and segment S = [off, off + len):
//   u_j = (z[n][j] - mu[m][j]) * (1 / sigma[m][j]),  t_j = fma(-u_j / 2, u_j, -log sigma[m][j] - log(2 pi) / 2),
//   e = (((0 + t_off) + t_off+1) + ...) in ascending j; then, in ascending m from (M, s) = (-inf, 0):
//   x = exp(-|e - M|);  e > M: s = s x + 1, M = e;  else: s = s + x.      out = M + log s.
// None of it depends on the tile, the block, the group's other segments or the hull, so a value is a function of
// its row of z, the component list and its segment alone.
//
// The hull's width picks the instance, DMAX = 16, 64, 128 or 256 (LDS per block = (4 ML_ROWS + 20 ML_TILE) DMAX
// bytes: 9, 36, 72, 144 KB).  The host walks the groups in order and launches every run of up to
// ML_LAUNCH_GROUPS groups of one instance at once, its segments in the kernel's argument block.
// svae_op_mixture_logdensity, with its argument checks, ends the file.
#include <cmath>
#include <cstdint>

#include "common.h"
#include "opentry.h"

#pragma clang fp contract(off)

namespace {

constexpr int ML_TILE = SVAE_LATENTS_TILE;
constexpr int ML_ROWS = 64;                     // query rows per block: one per lane
constexpr int ML_SLOTS = 4;                     // waves per block, a chunk of segments each
constexpr int ML_SEGS = 4;                      // segments per thread
constexpr int ML_GROUP = ML_SLOTS * ML_SEGS;    // segments per block
constexpr int ML_THREADS = ML_ROWS * ML_SLOTS;
constexpr int ML_LAUNCH_GROUPS = 16;            // groups per launch: 2 KB of segment arguments
constexpr double ML_HALF_LOG_2PI = 0.91893853320467274178;

struct MlSegs {
  int off[ML_LAUNCH_GROUPS * ML_GROUP];
  int len[ML_LAUNCH_GROUPS * ML_GROUP];
};

// sg holds the launch's n_here segments, columns seg0 .. seg0 + n_here - 1 of out's n_seg
template <int DMAX>
__global__ __launch_bounds__(ML_THREADS) void mixture_logdensity_kernel(const float* __restrict__ z, long long nq,
                                                                        long long ldz, const float* __restrict__ mu,
                                                                        const float* __restrict__ sigma,
                                                                        long long nm, long long ldm, MlSegs sg,
                                                                        int n_here, int seg0, int n_seg,
                                                                        double* __restrict__ out) {
  __shared__ float zs[DMAX][ML_ROWS];
  __shared__ float mus[ML_TILE][DMAX];
  __shared__ double inv[ML_TILE][DMAX];
  __shared__ double cst[ML_TILE][DMAX];
  const int tid = threadIdx.x, lane = tid % ML_ROWS, slot = tid / ML_ROWS;
  const long long row0 = (long long)blockIdx.x * ML_ROWS;
  const int g0 = blockIdx.y * ML_GROUP;         // < n_here: the grid has no empty group
  const int ng = min(ML_GROUP, n_here - g0);    // the group's segments
  int jlo = sg.off[g0], jhi = jlo + sg.len[g0];
  for (int i = 1; i < ng; ++i) {
    jlo = min(jlo, sg.off[g0 + i]);
    jhi = max(jhi, sg.off[g0 + i] + sg.len[g0 + i]);
  }
  const int w = jhi - jlo;  // <= DMAX: the host chose the instance by it
  const int c0 = g0 + slot * ML_SEGS;
  const int ns = min(ML_SEGS, g0 + ng - c0);    // this wave's segments; <= 0: it only stages
  int off[ML_SEGS], len[ML_SEGS];
  double mx[ML_SEGS], sm[ML_SEGS];
#pragma unroll
  for (int s = 0; s < ML_SEGS; ++s) {
    off[s] = s < ns ? sg.off[c0 + s] - jlo : 0;
    len[s] = s < ns ? sg.len[c0 + s] : 0;
    mx[s] = -INFINITY;
    sm[s] = 0.0;
  }

  // the block's rows of z over the hull; rows past nq are zeros that nothing stores
  for (int i = tid; i < w * ML_ROWS; i += ML_THREADS) {
    const int r = i / w, j = i - r * w;
    zs[j][r] = row0 + r < nq ? z[(row0 + r) * ldz + jlo + j] : 0.f;
  }

  for (long long m0 = 0; m0 < nm; m0 += ML_TILE) {
    const int tn = (int)min((long long)ML_TILE, nm - m0);
    __syncthreads();  // the previous tile's readers are done
    for (int i = tid; i < tn * w; i += ML_THREADS) {
      const int c = i / w, j = i - c * w;
      const long long g = (m0 + c) * ldm + jlo + j;
      const double sd = (double)sigma[g];
      mus[c][j] = mu[g];
      inv[c][j] = 1.0 / sd;
      cst[c][j] = -log(sd) - ML_HALF_LOG_2PI;
    }
    __syncthreads();
    for (int c = 0; c < tn; ++c) {
#pragma unroll
      for (int s = 0; s < ML_SEGS; ++s) {
        if (s < ns) {
          double e = 0.0;
          for (int j = off[s]; j < off[s] + len[s]; ++j) {
            const double u = ((double)zs[j][lane] - (double)mus[c][j]) * inv[c][j];
            e = e + fma(-0.5 * u, u, cst[c][j]);
          }
          const double dlt = e - mx[s];
          const double x = exp(-fabs(dlt));
          if (dlt > 0.0) {
            sm[s] = sm[s] * x + 1.0;
            mx[s] = e;
          } else {
            sm[s] = sm[s] + x;  // a NaN lands here and stays
          }
        }
      }
    }
  }
  if (row0 + lane < nq) {
#pragma unroll
    for (int s = 0; s < ML_SEGS; ++s)
      if (s < ns) out[(row0 + lane) * n_seg + seg0 + c0 + s] = mx[s] + log(sm[s]);
  }
}

template <int DMAX>
void ml_launch(const float* z, long long nq, long long ldz, const float* mu, const float* sigma, long long nm,
               long long ldm, const MlSegs& sg, int n_here, int seg0, int n_seg, double* out, hipStream_t s) {
  const dim3 grid((unsigned)((nq + ML_ROWS - 1) / ML_ROWS), (unsigned)((n_here + ML_GROUP - 1) / ML_GROUP));
  hipLaunchKernelGGL((mixture_logdensity_kernel<DMAX>), grid, dim3(ML_THREADS), 0, s, z, nq, ldz, mu, sigma, nm, ldm,
                     sg, n_here, seg0, n_seg, out);
}

// seg: host (offset, length) pairs; launches on s
void mixture_logdensity(const float* z, long long nq, long long ldz, const float* mu, const float* sigma,
                        long long nm, long long ldm, const int* seg, int n_seg, double* out, hipStream_t s) {
  int first = 0;  // the run's first segment (a multiple of ML_GROUP)
  while (first < n_seg) {
    MlSegs sg;
    int n_here = 0, dmax = 0;
    while (first + n_here < n_seg && n_here < ML_LAUNCH_GROUPS * ML_GROUP) {
      const int a = first + n_here, b = a + ML_GROUP < n_seg ? a + ML_GROUP : n_seg;  // one group
      int lo = seg[2 * a], hi = lo + seg[2 * a + 1];
      for (int i = a + 1; i < b; ++i) {
        lo = seg[2 * i] < lo ? seg[2 * i] : lo;
        hi = seg[2 * i] + seg[2 * i + 1] > hi ? seg[2 * i] + seg[2 * i + 1] : hi;
      }
      const int k = hi - lo <= 16 ? 16 : hi - lo <= 64 ? 64 : hi - lo <= 128 ? 128 : 256;
      if (dmax && k != dmax) break;
      dmax = k;
      for (int i = a; i < b; ++i) {
        sg.off[i - first] = seg[2 * i];
        sg.len[i - first] = seg[2 * i + 1];
      }
      n_here = b - first;
    }
    for (int i = n_here; i < ML_LAUNCH_GROUPS * ML_GROUP; ++i) sg.off[i] = sg.len[i] = 0;
    if (dmax == 16) ml_launch<16>(z, nq, ldz, mu, sigma, nm, ldm, sg, n_here, first, n_seg, out, s);
    else if (dmax == 64) ml_launch<64>(z, nq, ldz, mu, sigma, nm, ldm, sg, n_here, first, n_seg, out, s);
    else if (dmax == 128) ml_launch<128>(z, nq, ldz, mu, sigma, nm, ldm, sg, n_here, first, n_seg, out, s);
    else ml_launch<256>(z, nq, ldz, mu, sigma, nm, ldm, sg, n_here, first, n_seg, out, s);
    first += n_here;
  }
}

}  // namespace

extern "C" {

int svae_op_mixture_logdensity(const float* z, int64_t nq, int64_t ldz, const float* mu, const float* sigma,
                               int64_t nm, int64_t ldm, int d, const int32_t* seg, int n_seg, double* out,
                               void* stream) {
  if (!z || !mu || !sigma || !seg || !out) return op_fail(SVAE_EBADARG, "mixture_logdensity: null pointer");
  if (nq <= 0 || nm <= 0 || d <= 0 || n_seg <= 0)
    return op_fail(SVAE_EBADARG, "mixture_logdensity: nq, nm, d and n_seg must be positive");
  if (d > SVAE_LATENTS_MAX_DIM || n_seg > SVAE_LATENTS_MAX_SEGMENTS || nq > 2147483647LL)
    return op_fail(SVAE_EBADCONFIG, "mixture_logdensity: at most " + std::to_string(SVAE_LATENTS_MAX_DIM) +
                                        " dimensions, " + std::to_string(SVAE_LATENTS_MAX_SEGMENTS) +
                                        " segments and 2^31 - 1 query rows");
  if (ldz < d || ldm < d) return op_fail(SVAE_EBADARG, "mixture_logdensity: a leading dimension below d");
  for (int i = 0; i < n_seg; ++i) {
    const int64_t off = seg[2 * i], len = seg[2 * i + 1];
    if (off < 0 || len < 1 || off + len > d)
      return op_fail(SVAE_EBADARG, "mixture_logdensity: segment " + std::to_string(i) + " is not inside [0, d)");
  }
  mixture_logdensity(z, nq, ldz, mu, sigma, nm, ldm, seg, n_seg, out, (hipStream_t)stream);
  return op_done();
}

}  // extern "C"
