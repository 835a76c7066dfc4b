// Whole-image restoration around the forward: cut overlapping tiles out of images (svae_op_extract_tiles) and
// put stacks of overlapping tiles back together, normalised, masked and re-quantised (svae_op_blend_tiles).
// The contract is in include/svae_hip.h.
//
// Geometry per axis (extent L, tile t <= L, stride 1 <= s <= t): k = ceil((L - t) / s) + 1 tiles, tile i at
// o_i = min(i s, L - t); the tiles covering a position form one contiguous index range (tl_cover).  Both ops are
// gathers along the contiguous x * c run of an image row, of which a tile row is a contiguous piece: lanes run
// along it, a block derives (image, row band) once, and no result depends on the launch geometry or on which
// accesses the alignment lets be 16 bytes wide (the same values enter the same operations in the same order).
// The dequantisation is pixel.h's; the two entry points, with their argument checks, end the file.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "opentry.h"
#include "pixel.h"

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_BAND = 8;          // output rows of one blend block, halved while the launch has too few blocks
constexpr long long TL_MIN_ITEMS = 1024;  // (four blocks per CU: 24.5 us against 38.9 at bands of 8)
constexpr int TL_UNITS = 1024;      // extract: 16-byte units (scalar path: elements) of one block

// per axis: k = ceil((L - t) / s) + 1 tiles, tile i at min(i s, L - t); tile id (m ky + i) kx + j
struct TileGeom {
  int nimg, H, W, c, th, tw, sy, sx;
  int ky, kx;                        // tiles per axis
  long long n_tiles;                 // nimg * ky * kx
};
struct ExtractTilesArgs {
  TileGeom g;
  const void* images; int data_u8;
  float lo, qscale;                  // qscale = (hi - lo) / 255 rounded to fp32 (make_batch's)
  long long first, count;
  float* tiles;
};
struct BlendTilesArgs {
  TileGeom g;
  const float* tiles; int nstack; long long stack_stride;
  const void* source; int source_u8; const unsigned char* known;   // source and known: both or neither
  float lo, qscale, qinv;            // qinv = 255 / (hi - lo) rounded to fp32
  float* out; unsigned char* out_u8; // either may be nullptr
};

// (uint8) min(max(rintf((v - lo) * qinv), 0), 255): the difference and the product each rounded to fp32
__device__ __forceinline__ unsigned tl_quant(float v, float lo, float qinv) {
#pragma clang fp contract(off)
  const float d = v - lo;
  const float r = rintf(d * qinv);
  return (unsigned)fminf(fmaxf(r, 0.f), 255.f);
}

__device__ __forceinline__ int tl_w1(int p, int t) { return min(p + 1, t - p); }
__device__ __forceinline__ int tl_origin(int i, int s, int L, int t) { return min(i * s, L - t); }

// the tiles [lo, hi] that cover position x of an axis: origins are non-decreasing, so they are contiguous; the
// clamped last tile covers everything from L - t on
__device__ __forceinline__ void tl_cover(int x, int t, int s, int L, int k, int& lo, int& hi) {
  hi = x >= L - t ? k - 1 : x / s;
  lo = x < t ? 0 : (x - t) / s + 1;
  if (lo > k - 1) lo = k - 1;
}

// One item = a band of `band` rows of one output tile.  A lane walks units tid, tid + 256, ... of the band's
// rows x units grid without a division (dp, dq: the step in rows and units).  VEC: a unit is four floats, stored
// as one float4 (tw c % 4 == 0 and tiles 16-byte aligned); the source is read 16 (fp32) or 4 (uint8) bytes wide
// where its address allows and element by element where not.
template <bool U8, bool VEC>
__global__ __launch_bounds__(TL_THREADS) void extract_tiles_kernel(ExtractTilesArgs a, int band, int nbands) {
  const TileGeom& g = a.g;
  const int n = g.tw * g.c;  // floats of a tile row
  const int units = VEC ? n >> 2 : n;
  const int W1 = VEC ? 4 : 1;
  const long long pitch = (long long)g.W * g.c;
  const int p_first = threadIdx.x / units, q_first = threadIdx.x - p_first * units;
  const int dp = TL_THREADS / units, dq = TL_THREADS - dp * units;
  const long long items = a.count * nbands;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long r = it / nbands;
    const int p0 = (int)(it - r * nbands) * band;
    const int rows = min(band, g.th - p0);
    const long long id = (a.first + r) % g.n_tiles;
    const long long mi = id / g.kx;
    const int j = (int)(id - mi * g.kx);
    const long long m = mi / g.ky;
    const int i = (int)(mi - m * g.ky);
    const int oy = tl_origin(i, g.sy, g.H, g.th), ox = tl_origin(j, g.sx, g.W, g.tw);
    const long long src0 = ((m * g.H + oy + p0) * g.W + ox) * g.c;
    float* __restrict__ dst0 = a.tiles + (r * g.th + p0) * (long long)n;
    int p = p_first, q = q_first;
    while (p < rows) {
      const long long s = src0 + p * pitch + q * W1;
      float* d = dst0 + (long long)p * n + q * W1;
      if (VEC) {
        float4 v;
        if (U8) {
          const unsigned char* sp = (const unsigned char*)a.images + s;
          unsigned w;
          if ((reinterpret_cast<uintptr_t>(sp) & 3) == 0)
            w = *reinterpret_cast<const unsigned*>(sp);
          else
            w = (unsigned)sp[0] | ((unsigned)sp[1] << 8) | ((unsigned)sp[2] << 16) | ((unsigned)sp[3] << 24);
          float t[4];
          u8_dequant4(w, a.lo, a.qscale, t);
          v = make_float4(t[0], t[1], t[2], t[3]);
        } else {
          const float* sp = (const float*)a.images + s;
          if ((reinterpret_cast<uintptr_t>(sp) & 15) == 0)
            v = *reinterpret_cast<const float4*>(sp);
          else
            v = make_float4(sp[0], sp[1], sp[2], sp[3]);
        }
        *reinterpret_cast<float4*>(d) = v;
      } else {
        *d = U8 ? u8_dequant(((const unsigned char*)a.images)[s], a.lo, a.qscale) : ((const float*)a.images)[s];
      }
      q += dq;
      p += dp;
      if (q >= units) { q -= units; ++p; }
    }
  }
}

struct BlendFlags {
  int vec_in;    // tiles 16-byte aligned, stack_stride % 4 == 0 and tw c % 4 == 0: float4 loads where a group allows
  int vec_out;   // out 16-byte aligned and W c % 4 == 0: float4 stores
  int vec_out8;  // out_u8 4-byte aligned and W c % 4 == 0: one 4-byte store per group
};

// One item = (stack k, image m, band of `band` rows, chunk of 1024 elements of the row run).  A lane owns the
// group of four consecutive elements e0 .. e0 + 3 of the run in every row of the band: their columns, covering
// tile ranges and column weight sums are derived once, then every row walks its covering tiles with the
// accumulators in registers.  Per element: i ascending outside, j ascending inside, fp64 from 0.
__global__ __launch_bounds__(TL_THREADS) void blend_tiles_kernel(BlendTilesArgs a, BlendFlags f, int band,
                                                                 int nbands, int nchunks) {
  const TileGeom& g = a.g;
  const int n = g.W * g.c;        // elements of an image row
  const int tn = g.tw * g.c;      // elements of a tile row
  const long long tile_elems = (long long)g.th * tn;
  const long long items = (long long)a.nstack * g.nimg * nbands * nchunks;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    long long rest = it / nchunks;
    const int chunk = (int)(it - rest * nchunks);
    const int b = (int)(rest % nbands);
    rest /= nbands;
    const long long m = rest % g.nimg, k = rest / g.nimg;
    const long long e0_ll = ((long long)chunk * TL_THREADS + threadIdx.x) * 4;
    if (e0_ll >= n) continue;
    const int e0 = (int)e0_ll;
    const int cnt = min(4, n - e0);
    int x[4], jlo[4], jhi[4], wsum[4];
    {
      int xx = e0 / g.c, ch = e0 - xx * g.c;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        x[q] = min(xx, g.W - 1);  // q >= cnt: unused, kept in range
        tl_cover(x[q], g.tw, g.sx, g.W, g.kx, jlo[q], jhi[q]);
        int ws = 0;
        for (int j = jlo[q]; j <= jhi[q]; ++j) ws += tl_w1(x[q] - tl_origin(j, g.sx, g.W, g.tw), g.tw);
        wsum[q] = ws;
        if (++ch == g.c) { ch = 0; ++xx; }
      }
    }
    // the four elements share their tiles and every tile row piece is 16-byte aligned: float4 loads
    bool fast = f.vec_in && cnt == 4 && jlo[0] == jlo[3] && jhi[0] == jhi[3];
    if (fast)
      for (int j = jlo[0]; j <= jhi[0]; ++j) fast = fast && ((tl_origin(j, g.sx, g.W, g.tw) * g.c) & 3) == 0;
    const float* __restrict__ stack = a.tiles + k * a.stack_stride;
    const int y_end = min((b + 1) * band, g.H);
    for (int y = b * band; y < y_end; ++y) {
      int ilo, ihi;
      tl_cover(y, g.th, g.sy, g.H, g.ky, ilo, ihi);
      int wy_sum = 0;
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      for (int i = ilo; i <= ihi; ++i) {
        const int p = y - tl_origin(i, g.sy, g.H, g.th);
        const int wy = tl_w1(p, g.th);
        wy_sum += wy;
        // row p of tile (m, i, 0); tile (m, i, j) lies j tiles further
        const float* __restrict__ trow = stack + ((m * g.ky + i) * g.kx) * tile_elems + (long long)p * tn;
        if (fast) {
          for (int j = jlo[0]; j <= jhi[0]; ++j) {
            const int ox = tl_origin(j, g.sx, g.W, g.tw);
            const float4 v = *reinterpret_cast<const float4*>(trow + j * tile_elems + (e0 - ox * g.c));
            const float t[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += (double)(wy * tl_w1(x[q] - ox, g.tw)) * (double)t[q];
          }
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (q >= cnt) continue;
            for (int j = jlo[q]; j <= jhi[q]; ++j) {
              const int ox = tl_origin(j, g.sx, g.W, g.tw);
              const float t = trow[j * tile_elems + (e0 + q - ox * g.c)];
              acc[q] += (double)(wy * tl_w1(x[q] - ox, g.tw)) * (double)t;
            }
          }
        }
      }
      float v[4];
      unsigned bytes = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = (float)(acc[q] / (double)(wy_sum * wsum[q]));
        if (q < cnt && a.known && a.known[(m * g.H + y) * g.W + x[q]]) {
          const long long s = (m * g.H + y) * (long long)n + e0 + q;
          v[q] = a.source_u8 ? u8_dequant(((const unsigned char*)a.source)[s], a.lo, a.qscale)
                             : ((const float*)a.source)[s];
        }
        if (a.out_u8) bytes |= tl_quant(v[q], a.lo, a.qinv) << (8 * q);
      }
      const long long o = ((k * g.nimg + m) * g.H + y) * (long long)n + e0;
      if (a.out) {
        if (f.vec_out) {
          *reinterpret_cast<float4*>(a.out + o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q < cnt) a.out[o + q] = v[q];
        }
      }
      if (a.out_u8) {
        if (f.vec_out8) {
          *reinterpret_cast<unsigned*>(a.out_u8 + o) = bytes;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q < cnt) a.out_u8[o + q] = (unsigned char)((bytes >> (8 * q)) & 0xFF);
        }
      }
    }
  }
}

constexpr long long TL_GRID_CAP = 1 << 20;  // grid-stride beyond this many blocks

int tile_count(int L, int t, int s) { return (int)(((int64_t)L - t + s - 1) / s) + 1; }

// the largest sum of window weights w1(p) = min(p + 1, t - p) over the tiles covering one position of an axis
// (exact = false: an upper bound in O(1): at most ceil(t / s) + 1 tiles cover a position, each with at most ceil(t / 2))
int64_t tile_axis_weight(int L, int t, int s, bool exact) {
  const int k = tile_count(L, t, s);
  if (!exact) return std::min<int64_t>(k, ((int64_t)t + s - 1) / s + 1) * (((int64_t)t + 1) / 2);
  int64_t best = 0;
  for (int64_t x = 0; x < L; ++x) {
    int64_t hi = x >= (int64_t)L - t ? k - 1 : x / s, lo = x < t ? 0 : (x - t) / s + 1, sum = 0;
    if (lo > k - 1) lo = k - 1;
    for (int64_t i = lo; i <= hi; ++i) {
      const int64_t p = x - std::min<int64_t>(i * s, (int64_t)L - t);
      sum += std::min<int64_t>(p + 1, t - p);
    }
    best = std::max(best, sum);
  }
  return best;
}

// the checks the two tile ops share; fills g.  0, or the code op_fail() returned
int tile_geometry(const char* op, int nimg, int H, int W, int c, int th, int tw, int sy, int sx, TileGeom& g) {
  const std::string who(op);
  if (nimg <= 0 || H <= 0 || W <= 0 || c <= 0 || th <= 0 || tw <= 0 || sy <= 0 || sx <= 0)
    return op_fail(SVAE_EBADARG, who + ": nimg, H, W, c, th, tw, sy and sx must be positive");
  if (th > H || tw > W) return op_fail(SVAE_EBADARG, who + ": the tile exceeds the image");
  if (sy > th || sx > tw) return op_fail(SVAE_EBADARG, who + ": the stride exceeds the tile");
  g.nimg = nimg; g.H = H; g.W = W; g.c = c; g.th = th; g.tw = tw; g.sy = sy; g.sx = sx;
  g.ky = tile_count(H, th, sy); g.kx = tile_count(W, tw, sx);
  g.n_tiles = (long long)nimg * g.ky * g.kx;
  return 0;
}

int tile_sizes(const char* op, const TileGeom& g) {
  if ((int64_t)g.th * g.tw * g.c > 2147483647LL || (int64_t)g.H * g.W * g.c > 2147483647LL)
    return op_fail(SVAE_EBADCONFIG, std::string(op) + ": at most 2^31 - 1 elements per tile and per image");
  return 0;
}

}  // namespace

extern "C" {

int svae_op_extract_tiles(const void* images, int data_u8, int nimg, int H, int W, int c, int th, int tw, int sy,
                          int sx, float lo, float hi, int64_t first, int64_t count, float* tiles, void* stream) {
  if (!images || !tiles) return op_fail(SVAE_EBADARG, "extract_tiles: null images or tiles");
  ExtractTilesArgs a{};
  if (int rc = tile_geometry("extract_tiles", nimg, H, W, c, th, tw, sy, sx, a.g)) return rc;
  if (count <= 0) return op_fail(SVAE_EBADARG, "extract_tiles: count must be positive");
  if (first < 0 || first >= a.g.n_tiles)
    return op_fail(SVAE_EBADARG, "extract_tiles: first must be in [0, n_tiles)");
  if (data_u8 && !(lo < hi)) return op_fail(SVAE_EBADARG, "extract_tiles: lo >= hi with uint8 images");
  if (int rc = tile_sizes("extract_tiles", a.g)) return rc;
  a.images = images; a.data_u8 = data_u8 ? 1 : 0;
  a.lo = lo; a.qscale = quant_scale(lo, hi).qscale;
  a.first = first; a.count = count; a.tiles = tiles;
  const int n = a.g.tw * a.g.c;
  const bool vec = n % 4 == 0 && al16(a.tiles);
  const int units = vec ? n / 4 : n;
  int band = (TL_UNITS + units - 1) / units;
  if (band > a.g.th) band = a.g.th;
  const int nbands = (a.g.th + band - 1) / band;
  const long long items = a.count * nbands;
  const dim3 grid((unsigned)(items < TL_GRID_CAP ? items : TL_GRID_CAP)), block(TL_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (a.data_u8) {
    if (vec) hipLaunchKernelGGL((extract_tiles_kernel<true, true>), grid, block, 0, s, a, band, nbands);
    else hipLaunchKernelGGL((extract_tiles_kernel<true, false>), grid, block, 0, s, a, band, nbands);
  } else {
    if (vec) hipLaunchKernelGGL((extract_tiles_kernel<false, true>), grid, block, 0, s, a, band, nbands);
    else hipLaunchKernelGGL((extract_tiles_kernel<false, false>), grid, block, 0, s, a, band, nbands);
  }
  return op_done();
}

int svae_op_blend_tiles(const float* tiles, int nstack, int64_t stack_stride, int nimg, int H, int W, int c, int th,
                        int tw, int sy, int sx, const void* source, int source_u8, const uint8_t* known, float lo,
                        float hi, float* out, uint8_t* out_u8, void* stream) {
  if (!tiles) return op_fail(SVAE_EBADARG, "blend_tiles: null tiles");
  if (!out && !out_u8) return op_fail(SVAE_EBADARG, "blend_tiles: out and out_u8 are both null");
  if ((known != nullptr) != (source != nullptr))
    return op_fail(SVAE_EBADARG, "blend_tiles: known and source come together");
  BlendTilesArgs a{};
  if (int rc = tile_geometry("blend_tiles", nimg, H, W, c, th, tw, sy, sx, a.g)) return rc;
  if (nstack <= 0) return op_fail(SVAE_EBADARG, "blend_tiles: nstack must be positive");
  if (stack_stride < 0 || (unsigned __int128)stack_stride < (unsigned __int128)a.g.n_tiles * th * tw * c)
    return op_fail(SVAE_EBADARG, "blend_tiles: stack_stride is smaller than a set of tiles");
  if ((out_u8 || (source && source_u8)) && !(lo < hi))
    return op_fail(SVAE_EBADARG, "blend_tiles: lo >= hi with a uint8 source or output");
  if (int rc = tile_sizes("blend_tiles", a.g)) return rc;
  const auto reaches = [&](bool exact) {  // both factors < 2^31 * 2^30: the comparison is made in fp64
    return (double)tile_axis_weight(H, th, sy, exact) * (double)tile_axis_weight(W, tw, sx, exact) >= 536870912.0;
  };
  if (reaches(false) && reaches(true))
    return op_fail(SVAE_EBADCONFIG, "blend_tiles: the weight sum of a pixel reaches 2^29");
  a.tiles = tiles; a.nstack = nstack; a.stack_stride = stack_stride;
  a.source = source; a.source_u8 = source_u8 ? 1 : 0; a.known = known;
  const QScale q = quant_scale(lo, hi);
  a.lo = lo; a.qscale = q.qscale; a.qinv = q.qinv;
  a.out = out; a.out_u8 = out_u8;
  const long long n = (long long)a.g.W * a.g.c;
  const int tn = a.g.tw * a.g.c;
  BlendFlags f;
  f.vec_in = al16(a.tiles) && a.stack_stride % 4 == 0 && tn % 4 == 0;
  f.vec_out = a.out && al16(a.out) && n % 4 == 0;
  f.vec_out8 = a.out_u8 && (reinterpret_cast<uintptr_t>(a.out_u8) & 3) == 0 && n % 4 == 0;
  const int nchunks = (int)((n + 4 * TL_THREADS - 1) / (4 * TL_THREADS));
  int band = TL_BAND, nbands;
  long long items;
  for (;; band >>= 1) {
    nbands = (a.g.H + band - 1) / band;
    items = (long long)a.nstack * a.g.nimg * nbands * nchunks;
    if (band == 1 || items >= TL_MIN_ITEMS) break;
  }
  const dim3 grid((unsigned)(items < TL_GRID_CAP ? items : TL_GRID_CAP)), block(TL_THREADS);
  hipLaunchKernelGGL(blend_tiles_kernel, grid, block, 0, (hipStream_t)stream, a, f, band, nbands, nchunks);
  return op_done();
}

}  // extern "C"
