// The exact-fp32 distance tile shared by the row-wise pairwise ops (pairwise.hip: svae_op_pairwise_stats, knn.hip:
// svae_op_pairwise_knn): the squared norms, the column groups, and one block's [RT][PW_GLD] tile of inner products.
//
//   d2(i, j) = max(0, (a_i + b_j) - 2 g_ij)      a, b: squared norms in fp64, g: the fp32 inner product
//
//  pw_norms: one wave per row.  Lane l adds (double)v * v over k = l, l + 64, ... in ascending k, then a butterfly
//     over the 64 lanes (xor 32, 16, ... 1): the order depends on d alone.
//  pw_gram_tile<RT>: called by all PW_THREADS threads of a block of four waves that owns a (row tile, column tile)
//     of RT x PW_C = 128 x 128 or 32 x 128 (a wave owning 64 x 64 or 32 x 32).  The K loop stages PW_K = 32
//     dimensions of both operands in LDS, k-major ([k][row], stride 130: the 32 k of one row that a half-wave loads
//     land in 32 banks two apart, and the 32 rows a half-wave reads in 32 consecutive banks), with the next slab's
//     global loads in flight in registers during the MFMAs; the accumulators are v_mfma_f32_32x32x2_f32, so g_ij is
//     an fmaf chain in ascending k from 0 (rows, columns and dimensions past the end are staged as zeros, which add
//     nothing).  On return the accumulators sit in LDS as a [RT][PW_GLD] fp32 tile (over the staging area), the
//     tile's column norms in bs (0 past the group's end), and the block has synchronised: every thread may read both.
//  pw_d2: the distance of one pair from the tile, the clamp and the NaN rule.
// A row's arithmetic does not know the row tile, the grid or an address.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.h"
#include "svae_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int PW_R = SVAE_PAIRWISE_TILE_ROWS;
constexpr int PW_C = SVAE_PAIRWISE_TILE_COLS;
constexpr int PW_K = SVAE_PAIRWISE_TILE_K;
constexpr int PW_G = SVAE_PAIRWISE_MAX_GROUPS;
constexpr int PW_THREADS = 256;
constexpr double PW_DBL_MAX = 1.7976931348623157e308;
constexpr int PW_LD = 130;                       // staging stride in floats
constexpr int PW_GLD = PW_C + 1;                 // accumulator tile stride in floats
constexpr int PW_PER = PW_C * PW_K / PW_THREADS; // staged floats per thread of the column operand
constexpr int PW_FILL = 256;                     // blocks below which the small row tile is taken
static_assert(PW_R == 128 && PW_C == 128 && PW_K == 32, "the lane maps below are written for 128 x 128 x 32");

// floats of LDS pw_gram_tile<RT> needs: staging [2][PW_K][PW_LD], then the [RT][PW_GLD] tile
template <int RT>
constexpr int pw_lds_floats() {
  return RT * PW_GLD > 2 * PW_K * PW_LD ? RT * PW_GLD : 2 * PW_K * PW_LD;
}

struct PwGroups {
  const float* y[PW_G];
  long long m[PW_G], ldy[PW_G];
  long long boff[PW_G];  // the group's first norm in bn
  int ct0[PW_G + 1];     // the group's first column tile; ct0[n_groups] = all of them
  int n_groups, self_group;
};

__global__ __launch_bounds__(64) void pw_norms(const float* __restrict__ x, long long ld, int d,
                                               double* __restrict__ out) {
  const float* row = x + (long long)blockIdx.x * ld;
  double s = 0.0;
  for (int k = threadIdx.x; k < d; k += 64) {
    const double v = (double)row[k];
    s = s + v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// the group a column tile belongs to
__device__ __forceinline__ int pw_group_of(const PwGroups& A, int ct) {
  int g = 0;
  while (g + 1 < A.n_groups && ct >= A.ct0[g + 1]) ++g;
  return g;
}

template <int RT>
__device__ __forceinline__ void pw_gram_tile(const float* __restrict__ x, long long n, long long ldx, int d,
                                             const float* __restrict__ y, long long m, long long ldy,
                                             const double* __restrict__ bnorm, long long row0, long long col0,
                                             float* __restrict__ lds, double* __restrict__ bs) {
  static_assert(RT == 128 || RT == 32, "row tiles of 128 (2 x 2 waves of 64 x 64) or 32 (1 x 4 waves of 32 x 32)");
  constexpr int WCOLS = RT == 128 ? 2 : 4;             // waves side by side
  constexpr int MI = RT == 128 ? 2 : 1, NJ = PW_C / (32 * WCOLS);  // 32 x 32 accumulators per wave: MI x NJ
  constexpr int PER_A = RT * PW_K / PW_THREADS;        // staged floats per thread of the row operand
  float* As = lds;
  float* Bs = lds + PW_K * PW_LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // staging map: thread t loads dimension t % 32 of rows (columns) t / 32 + 8 e, e < RT / 8 (16)
  const int sk = tid & (PW_K - 1), sr = tid / PW_K;
  float ra[PER_A], rb[PW_PER];
  auto fetch = [&](int k0) {
    const bool kin = k0 + sk < d;
#pragma unroll
    for (int e = 0; e < PER_A; ++e) {
      const long long r = row0 + sr + 8 * e;
      ra[e] = kin && r < n ? x[r * ldx + k0 + sk] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < PW_PER; ++e) {
      const long long c = col0 + sr + 8 * e;
      rb[e] = kin && c < m ? y[c * ldy + k0 + sk] : 0.f;
    }
  };
  // MFMA map (32x32x2): lane l gives A[row l % 32][k l / 32] and B[k l / 32][col l % 32]
  const int wr = (wave / WCOLS) * 32 * MI, wc = (wave % WCOLS) * 32 * NJ, li = lane & 31, lk = lane >> 5;
  f32x16 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  fetch(0);
  for (int k0 = 0; k0 < d; k0 += PW_K) {
    __syncthreads();  // the previous slab's readers are done
#pragma unroll
    for (int e = 0; e < PER_A; ++e) As[sk * PW_LD + sr + 8 * e] = ra[e];
#pragma unroll
    for (int e = 0; e < PW_PER; ++e) Bs[sk * PW_LD + sr + 8 * e] = rb[e];
    __syncthreads();
    if (k0 + PW_K < d) fetch(k0 + PW_K);
#pragma unroll
    for (int ks = 0; ks < PW_K; ks += 2) {
      const float* ap = As + (ks + lk) * PW_LD + wr + li;
      const float* bp = Bs + (ks + lk) * PW_LD + wc + li;
      float av[MI], bv[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) av[i] = ap[32 * i];
#pragma unroll
      for (int j = 0; j < NJ; ++j) bv[j] = bp[32 * j];
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  }
  __syncthreads();  // the last slab's readers are done: the staging area becomes the tile
  // D[row (r % 4) + 8 (r / 4) + 4 (l / 32)][col l % 32]
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        lds[(wr + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk) * PW_GLD + wc + 32 * j + li] = acc[i][j][r];
  if (tid < PW_C) bs[tid] = col0 + tid < m ? bnorm[col0 + tid] : 0.0;
  __syncthreads();
}

// d2 of row norm a and the tile's column c of row er, clamped at 0; +-inf (an inf element, or an fp32 inner
// product that overflowed) is NaN like a NaN itself
__device__ __forceinline__ double pw_d2(double a, const double* __restrict__ bs, const float* __restrict__ lds,
                                        int er, int c) {
  const double d2 = (a + bs[c]) - 2.0 * (double)lds[er * PW_GLD + c];
  return fabs(d2) <= PW_DBL_MAX ? (d2 < 0.0 ? 0.0 : d2) : (double)NAN;
}

inline long long pw_tiles(const int64_t* m, int n_groups) {
  long long t = 0;
  for (int g = 0; g < n_groups; ++g) t += (m[g] + PW_C - 1) / PW_C;
  return t;
}

// the limits of the grid: row tiles in y, column tiles in x
inline bool pw_shape_ok(int64_t n, const int64_t* m, int n_groups) {
  if (!m || n <= 0 || n_groups <= 0 || n_groups > SVAE_PAIRWISE_MAX_GROUPS) return false;
  for (int g = 0; g < n_groups; ++g)
    if (m[g] <= 0) return false;
  return pw_tiles(m, n_groups) <= 2147483647LL && (n + PW_R - 1) / PW_R <= 65535;
}

// the groups as the kernels take them; returns the number of columns
inline long long pw_groups(PwGroups& A, const float* const* y, const int64_t* m, const int64_t* ldy, int n_groups,
                           int self_group) {
  A.n_groups = n_groups;
  A.self_group = self_group;
  long long cols = 0;
  A.ct0[0] = 0;
  for (int g = 0; g < n_groups; ++g) {
    A.y[g] = y[g];
    A.m[g] = m[g];
    A.ldy[g] = ldy[g];
    A.boff[g] = cols;
    A.ct0[g + 1] = A.ct0[g] + (int)((m[g] + PW_C - 1) / PW_C);
    cols += m[g];
  }
  return cols;
}

// the norms of every group into bn and of x into an on s; returns where x's norms are (a self group's own)
inline const double* pw_launch_norms(const float* x, long long n, long long ldx, int d, const PwGroups& A, double* an,
                                     double* bn, hipStream_t s) {
  for (int g = 0; g < A.n_groups; ++g)
    hipLaunchKernelGGL(pw_norms, dim3((unsigned)A.m[g]), dim3(64), 0, s, A.y[g], A.ldy[g], d, bn + A.boff[g]);
  if (A.self_group >= 0) return bn + A.boff[A.self_group];  // the same rows: the same bytes
  hipLaunchKernelGGL(pw_norms, dim3((unsigned)n), dim3(64), 0, s, x, ldx, d, an);
  return an;
}

}  // namespace
