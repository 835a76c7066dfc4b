// Row-wise statistics of the pairwise squared distances between n points x and up to four groups of points y_g
// (svae_op_pairwise_stats, include/svae_hip.h): per row and group the Gaussian-kernel sums at n_bw bandwidths, the
// nearest column and its distance.  No [n, m] intermediate reaches memory.
//
//   d2(i, j) = max(0, (a_i + b_j) - 2 g_ij)      a, b: squared norms in fp64, g: the fp32 inner product
//
// Three kernels, all on the caller's stream, no atomics:
//  1. pw_norms (pairwise_tile.h): the squared norms, one wave per row, in an order that depends on d alone.
//  2. pw_tile<RT>: one block of four waves per (row tile, column tile) of RT x PW_C = 128 x 128, column tiles
//     counted through the groups one after the other (a tile never spans two groups).  Where that grid has fewer
//     blocks than the device has CUs (PW_FILL), the row tile is RT = 32 instead, a wave owning 32 x 32: four
//     times the blocks.  A row's arithmetic does not know the row tile, so this changes no byte of the output.
//     The staging, the MFMA K loop and the accumulator tile are pw_gram_tile<RT> (pairwise_tile.h, shared with
//     knn.hip): g_ij is an fmaf chain in ascending k from 0 on v_mfma_f32_32x32x2_f32.  Two blocks fit a CU
//     (77 KB of LDS, 179 VGPRs): one block's loads and epilogue hide behind the other's MFMAs.
//     Epilogue: the accumulators go to LDS as a [RT][129] fp32 tile (over the staging area); thread t < 2 RT owns
//     row t % RT and the column half t / RT and walks its 64 columns in ascending j: d2 in fp64, the clamp,
//     exp per bandwidth, running sums, running (min, argmin).  The two halves meet in LDS, half 0 first, and
//     the row's partial for this column tile goes to scratch.
//  3. pw_reduce: one thread per (row, group) folds the group's column tiles in ascending order.
// So a row's outputs are a function of that row, the groups and the bandwidths: the position of the row in its
// tile, n, the grid and the addresses do not enter.
//
// A NaN or inf element, or an inner product that overflows fp32: d2 is NaN for every pair that reads it; the sums
// carry it, and the running minimum takes the first NaN it meets and keeps it (nn_idx names that column).
// svae_op_pairwise_scratch_bytes and svae_op_pairwise_stats, with their argument checks, end the file.
#include <cmath>
#include <cstdint>

#include "common.h"
#include "opentry.h"
#include "pairwise_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr int PW_B = SVAE_PAIRWISE_MAX_BW;

struct PwArgs : PwGroups {
  double inv[PW_B];
  int n_bw;
};

// the running minimum: the first NaN wins and stays, otherwise the first smallest value
__device__ __forceinline__ void pw_min(double& best, long long& idx, double v, long long j) {
  if (best != best) return;
  if (v != v || v < best) {
    best = v;
    idx = j;
  }
}

template <int RT>
__global__ __launch_bounds__(PW_THREADS, 2) void pw_tile(const float* __restrict__ x, long long n, long long ldx,
                                                         int d, const double* __restrict__ an,
                                                         const double* __restrict__ bn, PwArgs A,
                                                         double* __restrict__ pk, double* __restrict__ pd,
                                                         long long* __restrict__ pi) {
  __shared__ float lds[pw_lds_floats<RT>()];          // pw_gram_tile's staging, then the [RT][PW_GLD] tile
  __shared__ double bs[PW_C];                          // the tile's column norms
  __shared__ double hk[RT][PW_B];                      // column half 1's sums, minimum and index
  __shared__ double hd[RT];
  __shared__ long long hi[RT];
  const int tid = threadIdx.x;
  const int ct = blockIdx.x;
  const int g = pw_group_of(A, ct);
  const long long row0 = (long long)blockIdx.y * RT;
  const long long col0 = (long long)(ct - A.ct0[g]) * PW_C;
  const long long m = A.m[g];
  pw_gram_tile<RT>(x, n, ldx, d, A.y[g], m, A.ldy[g], bn + A.boff[g], row0, col0, lds, bs);

  const int er = tid & (RT - 1), half = tid / RT;  // half >= 2 (RT = 32): nothing to walk, nothing to store
  const long long row = row0 + er;
  const double a = row < n ? an[row] : 0.0;
  const long long skip = A.self_group == g ? row : -1;  // the excluded column of this row
  double sum[PW_B];
#pragma unroll
  for (int l = 0; l < PW_B; ++l) sum[l] = 0.0;
  double best = INFINITY;
  long long bidx = -1;
  const int c1 = half < 2 ? (int)min((long long)(half * 64 + 64), m - col0) : 0;
  for (int c = half * 64; c < c1; ++c) {
    if (col0 + c == skip) continue;
    const double d2 = pw_d2(a, bs, lds, er, c);
    if (pk) {
#pragma unroll
      for (int l = 0; l < PW_B; ++l)
        if (l < A.n_bw) sum[l] = sum[l] + exp(-(d2 * A.inv[l]));
    }
    pw_min(best, bidx, d2, col0 + c);
  }
  if (half == 1) {
#pragma unroll
    for (int l = 0; l < PW_B; ++l) hk[er][l] = sum[l];
    hd[er] = best;
    hi[er] = bidx;
  }
  __syncthreads();
  if (half == 0 && row < n) {
    const long long at = (long long)ct * n + row;
    if (pk) {
#pragma unroll
      for (int l = 0; l < PW_B; ++l)
        if (l < A.n_bw) pk[at * A.n_bw + l] = sum[l] + hk[er][l];
    }
    if (pd) {
      if (hi[er] >= 0) pw_min(best, bidx, hd[er], hi[er]);
      pd[at] = best;
      pi[at] = bidx;
    }
  }
}

__global__ __launch_bounds__(256) void pw_reduce(long long n, PwArgs A, const double* __restrict__ pk,
                                                 const double* __restrict__ pd, const long long* __restrict__ pi,
                                                 double* __restrict__ ksum, double* __restrict__ nn_d2,
                                                 long long* __restrict__ nn_idx) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * A.n_groups) return;
  const long long row = t / A.n_groups;
  const int g = (int)(t - row * A.n_groups);
  if (ksum) {
    for (int l = 0; l < A.n_bw; ++l) {
      double s = 0.0;
      for (int ct = A.ct0[g]; ct < A.ct0[g + 1]; ++ct) s = s + pk[((long long)ct * n + row) * A.n_bw + l];
      ksum[t * A.n_bw + l] = s;
    }
  }
  if (nn_d2) {
    double best = INFINITY;
    long long bidx = -1;
    for (int ct = A.ct0[g]; ct < A.ct0[g + 1]; ++ct) {
      const long long at = (long long)ct * n + row;
      if (pi[at] >= 0) pw_min(best, bidx, pd[at], pi[at]);
    }
    nn_d2[t] = best;
    nn_idx[t] = bidx;
  }
}

// scratch: a [n] and b [sum m] norms, then per (column tile, row) the n_bw sums, the minimum and its index
long long pairwise_scratch_bytes(long long n, const int64_t* m, int n_groups, int n_bw) {
  long long cols = 0;
  for (int g = 0; g < n_groups; ++g) cols += m[g];
  return 8 * (n + cols) + pw_tiles(m, n_groups) * n * (8LL * n_bw + 16);
}

// y, m, ldy, inv_two_sigma2: host arrays; launches on s
void pairwise_stats(const float* x, long long n, long long ldx, const float* const* y, const int64_t* m,
                    const int64_t* ldy, int n_groups, int d, int self_group, const double* inv_two_sigma2,
                    int n_bw, double* ksum, double* nn_d2, long long* nn_idx, void* scratch, hipStream_t s) {
  PwArgs A = {};
  const long long cols = pw_groups(A, y, m, ldy, n_groups, self_group);
  A.n_bw = n_bw;
  for (int l = 0; l < n_bw; ++l) A.inv[l] = inv_two_sigma2[l];
  const long long tiles = A.ct0[n_groups];
  double* bn = (double*)scratch + n;
  double* pk = bn + cols;
  double* pd = pk + tiles * n * n_bw;
  long long* pi = (long long*)(pd + tiles * n);
  const double* an = pw_launch_norms(x, n, ldx, d, A, (double*)scratch, bn, s);
  const long long rt128 = (n + PW_R - 1) / PW_R;
  if (rt128 * tiles >= PW_FILL)
    hipLaunchKernelGGL(pw_tile<PW_R>, dim3((unsigned)tiles, (unsigned)rt128), dim3(PW_THREADS), 0, s, x, n, ldx, d, an,
                       bn, A, ksum ? pk : nullptr, nn_d2 ? pd : nullptr, pi);
  else  // (fewer than PW_FILL blocks of 128 rows: n < 32768, so the grid's y fits)
    hipLaunchKernelGGL(pw_tile<32>, dim3((unsigned)tiles, (unsigned)((n + 31) / 32)), dim3(PW_THREADS), 0, s, x, n, ldx,
                       d, an, bn, A, ksum ? pk : nullptr, nn_d2 ? pd : nullptr, pi);
  hipLaunchKernelGGL(pw_reduce, dim3((unsigned)((n * n_groups + 255) / 256)), dim3(256), 0, s, n, A, pk, pd, pi,
                     ksum, nn_d2, nn_idx);
}

bool pairwise_shape_ok(int64_t n, const int64_t* m, int n_groups, int n_bw) {
  return n_bw >= 0 && n_bw <= SVAE_PAIRWISE_MAX_BW && pw_shape_ok(n, m, n_groups);
}

}  // namespace

extern "C" {

int64_t svae_op_pairwise_scratch_bytes(int64_t n, const int64_t* m, int n_groups, int n_bw) {
  if (!pairwise_shape_ok(n, m, n_groups, n_bw)) return -1;
  return pairwise_scratch_bytes(n, m, n_groups, n_bw);
}

int svae_op_pairwise_stats(const float* x, int64_t n, int64_t ldx, const float* const* y, const int64_t* m,
                           const int64_t* ldy, int n_groups, int64_t d, int self_group,
                           const double* inv_two_sigma2, int n_bw, double* ksum, double* nn_d2, int64_t* nn_idx,
                           void* scratch, void* stream) {
  if (!x || !y || !m || !ldy) return op_fail(SVAE_EBADARG, "pairwise_stats: null pointer");
  if (n <= 0 || d <= 0 || n_groups <= 0 || n_bw < 0)
    return op_fail(SVAE_EBADARG, "pairwise_stats: n, d and n_groups must be positive, n_bw not negative");
  if (n_groups > SVAE_PAIRWISE_MAX_GROUPS || n_bw > SVAE_PAIRWISE_MAX_BW)
    return op_fail(SVAE_EBADCONFIG, "pairwise_stats: at most " + std::to_string(SVAE_PAIRWISE_MAX_GROUPS) +
                                        " groups and " + std::to_string(SVAE_PAIRWISE_MAX_BW) + " bandwidths");
  if ((n_bw == 0) != (ksum == nullptr))
    return op_fail(SVAE_EBADARG, "pairwise_stats: ksum goes with n_bw > 0 and only with it");
  if ((nn_d2 == nullptr) != (nn_idx == nullptr))
    return op_fail(SVAE_EBADARG, "pairwise_stats: nn_d2 and nn_idx come together");
  if (!ksum && !nn_d2) return op_fail(SVAE_EBADARG, "pairwise_stats: nothing to compute");
  if (n_bw > 0 && !inv_two_sigma2) return op_fail(SVAE_EBADARG, "pairwise_stats: null bandwidths");
  if (ldx < d) return op_fail(SVAE_EBADARG, "pairwise_stats: ldx below d");
  for (int g = 0; g < n_groups; ++g) {
    if (!y[g]) return op_fail(SVAE_EBADARG, "pairwise_stats: null group " + std::to_string(g));
    if (m[g] <= 0) return op_fail(SVAE_EBADARG, "pairwise_stats: group " + std::to_string(g) + " is empty");
    if (ldy[g] < d) return op_fail(SVAE_EBADARG, "pairwise_stats: ldy below d in group " + std::to_string(g));
  }
  for (int l = 0; l < n_bw; ++l)
    if (!(inv_two_sigma2[l] > 0.0) || !std::isfinite(inv_two_sigma2[l]))
      return op_fail(SVAE_EBADARG, "pairwise_stats: bandwidth " + std::to_string(l) + " is not positive and finite");
  if (self_group >= n_groups) return op_fail(SVAE_EBADARG, "pairwise_stats: self_group names no group");
  if (self_group >= 0 && (n != m[self_group] || x != y[self_group]))
    return op_fail(SVAE_EBADARG, "pairwise_stats: self_group needs x == y[self_group] and n == m[self_group]");
  if (d > 2147483647LL || !pairwise_shape_ok(n, m, n_groups, n_bw))
    return op_fail(SVAE_EBADCONFIG, "pairwise_stats: d above 2^31 - 1, or too many row or column tiles");
  if (!scratch) return op_fail(SVAE_EBADARG, "pairwise_stats: null scratch");
  pairwise_stats(x, n, ldx, y, m, ldy, n_groups, (int)d, self_group < 0 ? -1 : self_group, inv_two_sigma2, n_bw, ksum,
                 nn_d2, (long long*)nn_idx, scratch, (hipStream_t)stream);
  return op_done();
}

}  // extern "C"
