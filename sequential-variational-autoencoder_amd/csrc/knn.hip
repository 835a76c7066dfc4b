// Row-wise order statistics and ball counts of the pairwise squared distances between n points x and up to four
// groups of points y_g (svae_op_pairwise_knn, include/svae_hip.h): per row and group the k smallest distances in
// ascending order, the number of columns whose own ball (a per-column squared radius) holds the row, and the number
// of pairs whose distance is NaN.  No [n, m] intermediate reaches memory.  The distance is svae_op_pairwise_stats'
// own, bit for bit: the norms and the tile are pairwise_tile.h's (pw_norms, pw_gram_tile, pw_d2).
//
// Three kernels, all on the caller's stream, no atomics:
//  1. pw_norms, as in pairwise.hip.
//  2. knn_tile<RT>: pairwise.hip's grid (one block per (row tile, column tile), RT = 32 below PW_FILL blocks) and
//     its tile.  Thread t < PW_C also stages the n_radii squared radii of column t next to the column norms (NaN
//     past the group's end and for a group without radii: a NaN radius admits nothing).  Epilogue: thread t < 2 RT
//     owns row t % RT and the column half t / RT and walks its 64 columns in ascending j.  A NaN d2 is counted and
//     enters nothing else.  Otherwise d2 goes through a compare-and-swap chain over the SVAE_KNN_MAX_K slots of a
//     sorted register list (static indices: no scratch memory; the chain is entered only where d2 is below the last
//     slot) and is compared with the column's radii.  Half 1 then writes its list and counts over its own 64
//     columns of its row of the tile, which no other thread reads (no second set of per-row arrays: 71 KB of LDS,
//     two blocks per CU as pw_tile); after one barrier half 0 sends half 1's values through its own chain, adds
//     the counts and stores the row's partial for this column tile to scratch.
//  3. knn_reduce: one thread per (row, group) sends the column tiles' lists through the same chain in ascending
//     tile order and adds the counts.
// The k smallest values of a multiset do not depend on the order they are met in, and the counts are integers: a
// row's outputs are a function of that row, the groups and the radii; the row tile, n, the grid and the addresses
// do not enter.  svae_op_knn_scratch_bytes and svae_op_pairwise_knn, with their argument checks, end the file.
#include <cmath>
#include <cstdint>

#include "common.h"
#include "opentry.h"
#include "pairwise_tile.h"

#pragma clang fp contract(off)

namespace {

constexpr int KN_K = SVAE_KNN_MAX_K;
constexpr int KN_R = SVAE_KNN_MAX_RADII;
constexpr int KN_HALF_WORDS = 2 * KN_K + KN_R + 1;  // half 1's partial in 32-bit words of its row of the tile
static_assert(KN_HALF_WORDS <= 64, "half 1's partial must fit its own 64 columns of the tile");

struct KnnArgs {
  const double* radius2[PW_G];
  int k, n_radii;
};

// v into the ascending list: every slot keeps the smaller of itself and what the slots before it passed on
__device__ __forceinline__ void knn_insert(double (&list)[KN_K], double v) {
  if (!(v < list[KN_K - 1])) return;
#pragma unroll
  for (int s = 0; s < KN_K; ++s) {
    const double lo = v < list[s] ? v : list[s];
    v = v < list[s] ? list[s] : v;
    list[s] = lo;
  }
}

template <int RT>
__global__ __launch_bounds__(PW_THREADS, 2) void knn_tile(const float* __restrict__ x, long long n, long long ldx,
                                                          int d, const double* __restrict__ an,
                                                          const double* __restrict__ bn, PwGroups A, KnnArgs Q,
                                                          double* __restrict__ pl, int* __restrict__ pc,
                                                          int* __restrict__ pn) {
  __shared__ float lds[pw_lds_floats<RT>()];  // pw_gram_tile's staging, then the [RT][PW_GLD] tile
  __shared__ double bs[PW_C];                  // the tile's column norms
  __shared__ double rs[PW_C][KN_R];            // the tile's squared radii
  const int tid = threadIdx.x;
  const int ct = blockIdx.x;
  const int g = pw_group_of(A, ct);
  const long long row0 = (long long)blockIdx.y * RT;
  const long long col0 = (long long)(ct - A.ct0[g]) * PW_C;
  const long long m = A.m[g];
  if (tid < PW_C) {  // (rs is not part of the staging area: no barrier needed before this)
    const double* __restrict__ rad = Q.radius2[g];
#pragma unroll
    for (int r = 0; r < KN_R; ++r)
      rs[tid][r] = rad && r < Q.n_radii && col0 + tid < m ? rad[(col0 + tid) * Q.n_radii + r] : (double)NAN;
  }
  pw_gram_tile<RT>(x, n, ldx, d, A.y[g], m, A.ldy[g], bn + A.boff[g], row0, col0, lds, bs);

  const int er = tid & (RT - 1), half = tid / RT;  // half >= 2 (RT = 32): nothing to walk, nothing to store
  const long long row = row0 + er;
  const double a = row < n ? an[row] : 0.0;
  const long long skip = A.self_group == g ? row : -1;  // the excluded column of this row
  double list[KN_K];
#pragma unroll
  for (int s = 0; s < KN_K; ++s) list[s] = INFINITY;
  int cnt[KN_R];
#pragma unroll
  for (int r = 0; r < KN_R; ++r) cnt[r] = 0;
  int bad = 0;
  const int c1 = half < 2 ? (int)min((long long)(half * 64 + 64), m - col0) : 0;
  for (int c = half * 64; c < c1; ++c) {
    if (col0 + c == skip) continue;
    const double d2 = pw_d2(a, bs, lds, er, c);
    if (d2 != d2) {
      ++bad;
      continue;
    }
    if (Q.k > 0) knn_insert(list, d2);
#pragma unroll
    for (int r = 0; r < KN_R; ++r) cnt[r] += d2 <= rs[c][r] ? 1 : 0;
  }
  // half 1's partial goes over columns 64 .. of its own row, which it alone has read
  int* mine = (int*)(lds + er * PW_GLD + 64);
  if (half == 1) {
#pragma unroll
    for (int s = 0; s < KN_K; ++s) {
      mine[2 * s] = __double2loint(list[s]);
      mine[2 * s + 1] = __double2hiint(list[s]);
    }
#pragma unroll
    for (int r = 0; r < KN_R; ++r) mine[2 * KN_K + r] = cnt[r];
    mine[2 * KN_K + KN_R] = bad;
  }
  __syncthreads();
  if (half == 0 && row < n) {
    const long long at = (long long)ct * n + row;
    if (Q.k > 0) {
#pragma unroll
      for (int s = 0; s < KN_K; ++s) knn_insert(list, __hiloint2double(mine[2 * s + 1], mine[2 * s]));
#pragma unroll
      for (int s = 0; s < KN_K; ++s)
        if (s < Q.k) pl[at * Q.k + s] = list[s];
    }
#pragma unroll
    for (int r = 0; r < KN_R; ++r)
      if (r < Q.n_radii) pc[at * Q.n_radii + r] = cnt[r] + mine[2 * KN_K + r];
    pn[at] = bad + mine[2 * KN_K + KN_R];
  }
}

__global__ __launch_bounds__(256) void knn_reduce(long long n, PwGroups A, KnnArgs Q, const double* __restrict__ pl,
                                                  const int* __restrict__ pc, const int* __restrict__ pn,
                                                  double* __restrict__ knn_d2, long long* __restrict__ inside,
                                                  long long* __restrict__ nonfinite) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * A.n_groups) return;
  const long long row = t / A.n_groups;
  const int g = (int)(t - row * A.n_groups);
  if (knn_d2) {
    double list[KN_K];
#pragma unroll
    for (int s = 0; s < KN_K; ++s) list[s] = INFINITY;
    for (int ct = A.ct0[g]; ct < A.ct0[g + 1]; ++ct) {
      const double* p = pl + ((long long)ct * n + row) * Q.k;
      for (int s = 0; s < Q.k; ++s) knn_insert(list, p[s]);
    }
#pragma unroll
    for (int s = 0; s < KN_K; ++s)
      if (s < Q.k) knn_d2[t * Q.k + s] = list[s];
  }
  if (inside) {
    for (int r = 0; r < Q.n_radii; ++r) {
      long long c = 0;
      for (int ct = A.ct0[g]; ct < A.ct0[g + 1]; ++ct) c += pc[((long long)ct * n + row) * Q.n_radii + r];
      inside[t * Q.n_radii + r] = c;
    }
  }
  if (nonfinite) {
    long long c = 0;
    for (int ct = A.ct0[g]; ct < A.ct0[g + 1]; ++ct) c += pn[(long long)ct * n + row];
    nonfinite[t] = c;
  }
}

bool knn_shape_ok(int64_t n, const int64_t* m, int n_groups, int k, int n_radii) {
  return k >= 0 && k <= KN_K && n_radii >= 0 && n_radii <= KN_R && k + n_radii > 0 && pw_shape_ok(n, m, n_groups);
}

// scratch: a [n] and b [sum m] norms, then per (column tile, row) the k values, the n_radii counts and the NaN count
long long knn_scratch_bytes(long long n, const int64_t* m, int n_groups, int k, int n_radii) {
  long long cols = 0;
  for (int g = 0; g < n_groups; ++g) cols += m[g];
  return 8 * (n + cols) + pw_tiles(m, n_groups) * n * (8LL * k + 4LL * n_radii + 4);
}

// y, m, ldy, radius2: host arrays; launches on s
void pairwise_knn(const float* x, long long n, long long ldx, const float* const* y, const int64_t* m,
                  const int64_t* ldy, int n_groups, int d, int self_group, int k, double* knn_d2,
                  const double* const* radius2, int n_radii, long long* inside, long long* nonfinite, void* scratch,
                  hipStream_t s) {
  PwGroups A = {};
  const long long cols = pw_groups(A, y, m, ldy, n_groups, self_group);
  KnnArgs Q = {};
  Q.k = k;
  Q.n_radii = n_radii;
  for (int g = 0; g < n_groups; ++g) Q.radius2[g] = n_radii > 0 ? radius2[g] : nullptr;
  const long long tiles = A.ct0[n_groups];
  double* bn = (double*)scratch + n;
  double* pl = bn + cols;
  int* pc = (int*)(pl + tiles * n * k);
  int* pn = pc + tiles * n * n_radii;
  const double* an = pw_launch_norms(x, n, ldx, d, A, (double*)scratch, bn, s);
  const long long rt128 = (n + PW_R - 1) / PW_R;
  if (rt128 * tiles >= PW_FILL)
    hipLaunchKernelGGL(knn_tile<PW_R>, dim3((unsigned)tiles, (unsigned)rt128), dim3(PW_THREADS), 0, s, x, n, ldx, d,
                       an, bn, A, Q, pl, pc, pn);
  else  // (fewer than PW_FILL blocks of 128 rows: n < 32768, so the grid's y fits)
    hipLaunchKernelGGL(knn_tile<32>, dim3((unsigned)tiles, (unsigned)((n + 31) / 32)), dim3(PW_THREADS), 0, s, x, n,
                       ldx, d, an, bn, A, Q, pl, pc, pn);
  hipLaunchKernelGGL(knn_reduce, dim3((unsigned)((n * n_groups + 255) / 256)), dim3(256), 0, s, n, A, Q, pl, pc, pn,
                     knn_d2, inside, nonfinite);
}

}  // namespace

extern "C" {

int64_t svae_op_knn_scratch_bytes(int64_t n, const int64_t* m, int n_groups, int k, int n_radii) {
  if (!knn_shape_ok(n, m, n_groups, k, n_radii)) return -1;
  return knn_scratch_bytes(n, m, n_groups, k, n_radii);
}

int svae_op_pairwise_knn(const float* x, int64_t n, int64_t ldx, const float* const* y, const int64_t* m,
                         const int64_t* ldy, int n_groups, int64_t d, int self_group, int k, double* knn_d2,
                         const double* const* radius2, int n_radii, int64_t* inside, int64_t* nonfinite,
                         void* scratch, void* stream) {
  if (!x || !y || !m || !ldy) return op_fail(SVAE_EBADARG, "pairwise_knn: null pointer");
  if (n <= 0 || d <= 0 || n_groups <= 0 || k < 0 || n_radii < 0)
    return op_fail(SVAE_EBADARG, "pairwise_knn: n, d and n_groups must be positive, k and n_radii not negative");
  if (n_groups > SVAE_PAIRWISE_MAX_GROUPS || k > SVAE_KNN_MAX_K || n_radii > SVAE_KNN_MAX_RADII)
    return op_fail(SVAE_EBADCONFIG, "pairwise_knn: at most " + std::to_string(SVAE_PAIRWISE_MAX_GROUPS) +
                                        " groups, k " + std::to_string(SVAE_KNN_MAX_K) + " and " +
                                        std::to_string(SVAE_KNN_MAX_RADII) + " radii");
  if ((k == 0) != (knn_d2 == nullptr))
    return op_fail(SVAE_EBADARG, "pairwise_knn: knn_d2 goes with k > 0 and only with it");
  if ((n_radii == 0) != (inside == nullptr))
    return op_fail(SVAE_EBADARG, "pairwise_knn: inside goes with n_radii > 0 and only with it");
  if (!knn_d2 && !inside) return op_fail(SVAE_EBADARG, "pairwise_knn: nothing to compute");
  if (n_radii > 0 && !radius2) return op_fail(SVAE_EBADARG, "pairwise_knn: null radii");
  if (ldx < d) return op_fail(SVAE_EBADARG, "pairwise_knn: ldx below d");
  for (int g = 0; g < n_groups; ++g) {
    if (!y[g]) return op_fail(SVAE_EBADARG, "pairwise_knn: null group " + std::to_string(g));
    if (m[g] <= 0) return op_fail(SVAE_EBADARG, "pairwise_knn: group " + std::to_string(g) + " is empty");
    if (ldy[g] < d) return op_fail(SVAE_EBADARG, "pairwise_knn: ldy below d in group " + std::to_string(g));
  }
  if (self_group >= n_groups) return op_fail(SVAE_EBADARG, "pairwise_knn: self_group names no group");
  if (self_group >= 0 && (n != m[self_group] || x != y[self_group]))
    return op_fail(SVAE_EBADARG, "pairwise_knn: self_group needs x == y[self_group] and n == m[self_group]");
  if (d > 2147483647LL || !knn_shape_ok(n, m, n_groups, k, n_radii))
    return op_fail(SVAE_EBADCONFIG, "pairwise_knn: d above 2^31 - 1, or too many row or column tiles");
  if (!scratch) return op_fail(SVAE_EBADARG, "pairwise_knn: null scratch");
  pairwise_knn(x, n, ldx, y, m, ldy, n_groups, (int)d, self_group < 0 ? -1 : self_group, k, knn_d2, radius2, n_radii,
               (long long*)inside, (long long*)nonfinite, scratch, (hipStream_t)stream);
  return op_done();
}

}  // extern "C"
