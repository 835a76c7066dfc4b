// Per-segment statistics of one fp32 array in one pass (svae_op_tensor_stats, include/svae_hip.h): for every
// segment and y = clamp(x, -c, +c) the finite count, sum y, sum |y|, sum y^2, max |x|, the count of |x| > c and
// the non-finite count, accumulated in fp64.  A non-finite element is counted and contributes nothing else.
//
// Order of summation (fixed: the result depends on x, the segments and c, never on the launch geometry or on
// the address of x).  The plan (stats_plan, pure host) cuts every segment at the absolute indices
// (offset & ~3) + k * SVAE_STATS_CHUNK, so a chunk never crosses a segment and only the first group of a
// segment's first chunk and the last group of its last chunk can be partial.  Inside a chunk, group G holds the
// absolute indices 4 * ((begin >> 2) + G) .. + 3 that lie in the chunk; lane l of the block takes the groups
// l, l + 256, ... in ascending order and adds element j of a group to its accumulator j (four independent fp64
// chains per sum).  Then ((a0 + a1) + (a2 + a3)) per lane, a shuffle tree over the wave (offsets 32 .. 1),
// the four waves in order, one partial row per chunk; stats_finish_kernel adds a segment's rows in chunk order.
// A full group is one 16-byte load when x is 16-byte aligned (the Vec instance) and four 4-byte loads otherwise:
// the same values into the same accumulators.
// svae_op_stats_plan and svae_op_tensor_stats, with their argument checks, end the file.
#include <cfloat>
#include <cstdint>

#include "common.h"
#include "opentry.h"

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_WAVES = ST_THREADS / 64;
constexpr int FIN_BATCH = 16;  // chunk rows whose loads the finish kernel issues together

struct StatAcc {
  double s1[4], s2[4], s3[4];
  float mx;
  int nfin, nclip, nbad;
};

__device__ __forceinline__ void st_elem(float v, float c, int j, StatAcc& a) {
  const float av = fabsf(v);
  const bool fin = av <= FLT_MAX;  // false for NaN and +-inf
  const float y = fminf(fmaxf(v, -c), c);
  const double yd = fin ? (double)y : 0.0;
  a.s1[j] += yd;
  a.s2[j] += fabs(yd);
  a.s3[j] = fma(yd, yd, a.s3[j]);  // the square of an fp32 value is exact in fp64: one rounding, the addition's
  a.mx = fin ? fmaxf(a.mx, av) : a.mx;
  a.nfin += fin ? 1 : 0;
  a.nclip += (fin && av > c) ? 1 : 0;
  a.nbad += fin ? 0 : 1;
}

// a segment's first or last group (first element e): only the elements inside [begin, end) are read
__device__ __forceinline__ void st_partial(const float* __restrict__ x, long long e, long long begin, long long end,
                                           float c, StatAcc& a) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (e + j >= begin && e + j < end) st_elem(x[e + j], c, j, a);
}

__device__ __forceinline__ double st_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ int st_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ float st_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
  return v;
}

// one block per chunk (grid-stride over the chunks); partial row k = the eight columns of chunk k
template <bool Vec>
__global__ __launch_bounds__(ST_THREADS) void stats_chunk_kernel(const float* __restrict__ x,
                                                                 const long long* __restrict__ chunks,
                                                                 long long n_chunks, float c,
                                                                 double* __restrict__ part) {
  __shared__ double red[ST_WAVES][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long k = blockIdx.x; k < n_chunks; k += gridDim.x) {
    const long long begin = chunks[2 * k];
    const long long end = begin + (chunks[2 * k + 1] & 0xFFFFFFFFll);
    const long long g0 = begin >> 2;
    const int ng = (int)(((end + 3) >> 2) - g0);
    StatAcc a;
#pragma unroll
    for (int j = 0; j < 4; ++j) a.s1[j] = a.s2[j] = a.s3[j] = 0.0;
    a.mx = 0.f;
    a.nfin = a.nclip = a.nbad = 0;
    // groups [gf0, gf1) are whole; only group 0 and group ng - 1 can be partial.  Each lane still meets its
    // groups in ascending order (group 0 is lane 0's first, group ng - 1 its lane's last), and the loop over
    // the whole groups has no branch, so the loads of four iterations are in flight together.
    const int gf0 = ((g0 << 2) >= begin && (g0 << 2) + 4 <= end) ? 0 : 1;
    const int gf1 = (ng > gf0 && ((g0 + ng) << 2) > end) ? ng - 1 : ng;
    if (gf0 == 1 && threadIdx.x == 0) st_partial(x, g0 << 2, begin, end, c, a);
#pragma unroll 4
    for (int g = threadIdx.x + (threadIdx.x < gf0 ? ST_THREADS : 0); g < gf1; g += ST_THREADS) {
      const long long e = (g0 + g) << 2;
      float v[4];
      if (Vec) {
        const float4 q = *reinterpret_cast<const float4*>(x + e);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = x[e + j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) st_elem(v[j], c, j, a);
    }
    if (gf1 < ng && threadIdx.x == ((ng - 1) & (ST_THREADS - 1))) st_partial(x, (g0 + ng - 1) << 2, begin, end, c, a);
    double col[8];
    col[0] = (double)st_wave_sum(a.nfin);
    col[1] = st_wave_sum((a.s1[0] + a.s1[1]) + (a.s1[2] + a.s1[3]));
    col[2] = st_wave_sum((a.s2[0] + a.s2[1]) + (a.s2[2] + a.s2[3]));
    col[3] = st_wave_sum((a.s3[0] + a.s3[1]) + (a.s3[2] + a.s3[3]));
    col[4] = (double)st_wave_max(a.mx);
    col[5] = (double)st_wave_sum(a.nclip);
    col[6] = (double)st_wave_sum(a.nbad);
    col[7] = 0.0;
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 8; ++q) red[wave][q] = col[q];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
      const int q = threadIdx.x;
      double r = red[0][q];
#pragma unroll
      for (int w = 1; w < ST_WAVES; ++w) r = (q == 4) ? fmax(r, red[w][q]) : r + red[w][q];
      part[k * 8 + q] = r;
    }
    __syncthreads();
  }
}

// out[s][q] = the rows of segment s's chunks [first[s], first[s + 1]) combined in chunk order (a sum; column 4
// a maximum); a segment without chunks gets a zero row.  Eight lanes per segment.
__global__ __launch_bounds__(ST_THREADS) void stats_finish_kernel(const long long* __restrict__ first,
                                                                  const double* __restrict__ part, int n_seg,
                                                                  double* __restrict__ out) {
  const long long t = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  const long long s = t >> 3;
  const int q = (int)(t & 7);
  if (s >= n_seg) return;
  const long long k0 = first[s], k1 = first[s + 1];
  double r = 0.0;
  long long k = k0;
  // the additions stay one chain in chunk order; the loads of FIN_BATCH rows are issued together, or a long
  // segment would pay one memory round trip per chunk
  for (; k + FIN_BATCH <= k1; k += FIN_BATCH) {
    double p[FIN_BATCH];
#pragma unroll
    for (int i = 0; i < FIN_BATCH; ++i) p[i] = part[(k + i) * 8 + q];
#pragma unroll
    for (int i = 0; i < FIN_BATCH; ++i) r = (q == 4) ? fmax(r, p[i]) : r + p[i];
  }
  for (; k < k1; ++k) {
    const double p = part[k * 8 + q];
    r = (q == 4) ? fmax(r, p) : r + p;
  }
  out[s * 8 + q] = r;
}

// plan table (int64 words): [0, n_seg] the index of every segment's first chunk (entry n_seg = n_chunks), then
// per chunk (begin, segment << 32 | length).  stats_plan returns the chunk count (table == nullptr: count only),
// -1 for a negative, unordered or overlapping segment, -2 when cap_words < stats_plan_words().
inline long long stats_plan_words(int n_seg, long long n_chunks) { return (long long)n_seg + 1 + 2 * n_chunks; }

long long stats_plan(const long long* offsets, const long long* lengths, int n_seg, long long* table,
                     long long cap_words) {
  long long pos = 0, n_chunks = 0;
  for (int s = 0; s < n_seg; ++s) {
    const long long off = offsets[s], len = lengths[s];
    if (off < 0 || len < 0 || off < pos) return -1;
    pos = off + len;
    if (len > 0) n_chunks += ((pos - (off & ~3ll)) + SVAE_STATS_CHUNK - 1) / SVAE_STATS_CHUNK;
  }
  if (!table) return n_chunks;
  if (cap_words < stats_plan_words(n_seg, n_chunks)) return -2;
  long long* chunk = table + n_seg + 1;
  long long k = 0;
  for (int s = 0; s < n_seg; ++s) {
    table[s] = k;
    const long long off = offsets[s], end = off + lengths[s], base = off & ~3ll;
    long long b = off;
    while (b < end) {
      long long e = base + ((b - base) / SVAE_STATS_CHUNK + 1) * SVAE_STATS_CHUNK;  // the next cut
      if (e > end) e = end;
      chunk[2 * k] = b;
      chunk[2 * k + 1] = ((long long)s << 32) | (e - b);
      ++k;
      b = e;
    }
  }
  table[n_seg] = k;
  return k;
}

// part: n_chunks * 8 doubles; out: n_seg * 8 doubles; at most two launches on s
void tensor_stats(const float* x, const long long* plan, int n_seg, long long n_chunks, float c, double* part,
                  double* out, hipStream_t s) {
  if (n_seg <= 0) return;
  if (n_chunks > 0) {
    const long long cap = 65536;  // grid-stride beyond this many blocks
    const dim3 grid((unsigned)(n_chunks < cap ? n_chunks : cap));
    const long long* chunks = plan + n_seg + 1;
    if (al16(x))
      hipLaunchKernelGGL(stats_chunk_kernel<true>, grid, dim3(ST_THREADS), 0, s, x, chunks, n_chunks, c, part);
    else
      hipLaunchKernelGGL(stats_chunk_kernel<false>, grid, dim3(ST_THREADS), 0, s, x, chunks, n_chunks, c, part);
  }
  const long long nt = (long long)n_seg * 8;
  hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)((nt + ST_THREADS - 1) / ST_THREADS)), dim3(ST_THREADS), 0,
                     s, plan, part, n_seg, out);
}

}  // namespace

extern "C" {

int64_t svae_op_stats_plan(const int64_t* offsets, const int64_t* lengths, int32_t n_seg, int64_t* table,
                           int64_t cap_words) {
  if (n_seg < 0 || (n_seg > 0 && (!offsets || !lengths)) || cap_words < 0)
    return op_fail(SVAE_EBADARG, "stats_plan: null segments or a negative count");
  const long long n = stats_plan((const long long*)offsets, (const long long*)lengths, n_seg, (long long*)table,
                                 cap_words);
  if (n == -1)
    return op_fail(SVAE_EBADARG, "stats_plan: segments must be non-negative, ascending and disjoint");
  if (n == -2) {
    const long long nc = stats_plan((const long long*)offsets, (const long long*)lengths, n_seg, nullptr, 0);
    return op_fail(SVAE_EBADARG, "stats_plan: the table holds " + std::to_string((long long)cap_words) +
                                     " words, the plan needs " + std::to_string(stats_plan_words(n_seg, nc)));
  }
  return n;
}

int svae_op_tensor_stats(const float* x, const int64_t* plan, int32_t n_seg, int64_t n_chunks, float c,
                         double* partials, double* out, void* stream) {
  if (!x || !plan || !partials || !out) return op_fail(SVAE_EBADARG, "tensor_stats: null pointer");
  if (n_seg < 0 || n_chunks < 0) return op_fail(SVAE_EBADARG, "tensor_stats: negative count");
  if (!(c >= 0.f)) return op_fail(SVAE_EBADARG, "tensor_stats: the clamp must be >= 0 (+inf: none)");
  tensor_stats(x, (const long long*)plan, n_seg, n_chunks, c, partials, out, (hipStream_t)stream);
  return op_done();
}

}  // extern "C"
