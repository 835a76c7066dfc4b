// Random crops of large device-resident images as the clean training batch, in one launch (svae_op_crop_batch,
// include/svae_hip.h): per row an image, an integer box scale, one of up to eight symmetries and a window origin,
// then the means of the s x s source blocks of that window, mirrored / transposed, dequantised.
//
// Per-row draws are philox.h's philox_image on the stream PHILOX_CROPS: block 0 gives image, scale and symmetry,
// block 1 the origin; a block whose words cannot matter (every range is 1) is not drawn.  The dequantisation is
// pixel.h's.  Sums are exact integers (uint8) or fp32 in a fixed order (fp32), every fp32 operation is rounded on its
// own (contract(off)), so the result depends on the arguments alone: not on the launch, not on whether a block
// staged its source patch in LDS or read it from global memory, not on the path (16-byte / element) the alignment
// of a source row selects.
//
// One block owns a square tile of T x T output pixels of one row b (T = 32 or 16, chosen by the host from the LDS
// the largest listed scale needs).  The source pixels of a tile form a rectangle under every symmetry (a transposed
// tile reads the transposed rectangle), so lanes run along the contiguous source rows when it is staged and along
// the contiguous output rows when it is reduced; the symmetry is an index map on the LDS read.  A staged source row
// keeps its distance to the 16-byte boundary below it (slot r holds it at byte (address & 15)), so an aligned
// 16-byte chunk of global memory goes to LDS as one 16-byte load and store.  The chunks at a row's two ends carry
// neighbouring bytes of the images along, which nothing reads; only a chunk that would leave the images
// (before the first image's first byte, past the last one's last) is peeled element by element: nothing outside
// the images is read.
// A block whose patch does not fit what the launch reserved (no LDS at all when the largest scale's patch exceeds
// 64 KB less the header at T = 16; a scale beyond the listed ones in explicit crops) reduces from global memory
// instead: the same values enter the same operations in the same order.
// svae_op_crop_batch, with its argument checks, ends the file.
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "opentry.h"
#include "philox.h"
#include "pixel.h"

namespace {

// row b of the batch = the h x w window at (y0, x0) of image m, box-averaged by s and mapped by symmetry g, with
// (m, s, g, y0, x0) = crops[b], or drawn when crops == nullptr
struct CropArgs {
  const void* images; int data_u8;
  int nimg, H, W, c, h, w;
  int n_scales, scales[4], smax;     // smax: the largest listed scale (what the LDS patch is sized for)
  int symmetries;
  const int* crops;
  unsigned long long seed, offset;
  int n;
  float lo, qscale;                  // qscale = (hi - lo) / 255 rounded to fp32 (make_batch's)
  float* target; unsigned char* target_u8; int* meta;   // target or target_u8 may be nullptr, meta may be
};

constexpr int CR_THREADS = 256;
constexpr int CR_HDR = 32;                 // bytes ahead of the patch: the row's five parameters
constexpr long long CR_LDS_MAX = 65536 - CR_HDR;  // the patch of a 16 x 16 tile must fit this, or nothing is staged
constexpr long long CR_LDS_WIDE = 32768;   // a 32 x 32 tile is used while its patch fits this (four blocks a CU)
constexpr long long CR_GRID_CAP = 1 << 20;  // grid-stride beyond this many blocks

// (m, s, g, y0, x0) of row b: crops[b] as it is, or the draws
__device__ __forceinline__ void cr_params(const CropArgs& a, long long b, int p[5]) {
  if (a.crops) {
#pragma unroll
    for (int k = 0; k < 5; ++k) p[k] = a.crops[b * 5 + k];
    return;
  }
  unsigned w[4];
  p[0] = 0; p[1] = a.scales[0]; p[2] = 0; p[3] = 0; p[4] = 0;
  if (a.nimg > 1 || a.n_scales > 1 || a.symmetries > 1) {
    philox_image(a.seed, a.offset, b, PHILOX_CROPS, 0, w);
    p[0] = (int)__umulhi(w[0], (unsigned)a.nimg);
    const int k = (int)__umulhi(w[1], (unsigned)a.n_scales);
    p[1] = k == 0 ? a.scales[0] : (k == 1 ? a.scales[1] : (k == 2 ? a.scales[2] : a.scales[3]));
    p[2] = (int)__umulhi(w[2], (unsigned)a.symmetries);
  }
  const unsigned ny = (unsigned)(a.H - p[1] * a.h + 1), nx = (unsigned)(a.W - p[1] * a.w + 1);
  if (ny > 1 || nx > 1) {
    philox_image(a.seed, a.offset, b, PHILOX_CROPS, 1, w);
    p[3] = (int)__umulhi(w[0], ny);
    p[4] = (int)__umulhi(w[1], nx);
  }
}

// The mean of the s x s block whose first element is k0 elements into patch row r0, and its stores.  LDS: patch row
// r lies at src + r * pitch + ((mis0 + r * rb16) & 15); else at src + r * pitch (pitch: the image's row in bytes).
template <bool U8, bool LDS>
__device__ __forceinline__ void cr_pixel(const CropArgs& a, const unsigned char* src, long long pitch, int mis0, int rb16,
                                         int r0, int k0, int s, long long o) {
#pragma clang fp contract(off)
  const int c = a.c;
  if (U8) {
    unsigned sum = 0;
    for (int p = 0; p < s; ++p) {
      const int r = r0 + p;
      const unsigned char* row = src + r * pitch + (LDS ? ((mis0 + r * rb16) & 15) : 0) + k0;
      for (int q = 0; q < s; ++q) sum += row[q * c];
    }
    float mean = (float)sum;  // exact: at most 64 * 255
    if (s > 1) mean = __fdiv_rn(mean, (float)(s * s));
    if (a.target) a.target[o] = u8_dequant(mean, a.lo, a.qscale);
    if (a.target_u8) a.target_u8[o] = (unsigned char)fminf(255.f, rintf(mean));
  } else {
    const unsigned char* row = src + r0 * pitch + (LDS ? ((mis0 + r0 * rb16) & 15) : 0);
    float v = reinterpret_cast<const float*>(row)[k0];
    if (s > 1) {
      float acc = 0.f;
      for (int p = 0; p < s; ++p) {
        const int r = r0 + p;
        const float* rp = reinterpret_cast<const float*>(src + r * pitch + (LDS ? ((mis0 + r * rb16) & 15) : 0)) + k0;
        for (int q = 0; q < s; ++q) acc = acc + rp[q * c];
      }
      v = __fdiv_rn(acc, (float)(s * s));
    }
    a.target[o] = v;
  }
}

// tile: T.  lds_rows x lds_chunks 16-byte chunks of LDS follow the header (0: nothing is staged).
template <bool U8>
__global__ __launch_bounds__(CR_THREADS) void crop_batch_kernel(CropArgs a, int tile, int lds_rows, int lds_chunks) {
  extern __shared__ uint4 cr_lds4[];
  unsigned char* sm = reinterpret_cast<unsigned char*>(cr_lds4);
  int* hdr = reinterpret_cast<int*>(sm);
  unsigned char* patch = sm + CR_HDR;
  const int tid = threadIdx.x;
  const int ES = U8 ? 1 : 4;
  const int nty = (a.h + tile - 1) / tile, ntx = (a.w + tile - 1) / tile;
  const long long items = (long long)a.n * nty * ntx;
  const long long img_pitch = (long long)a.W * a.c * ES;  // bytes of an image row
  const int rb16 = (int)(img_pitch & 15);
  const long long img_bytes = (long long)a.nimg * a.H * img_pitch;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long b = it / (nty * ntx);
    const int t = (int)(it - b * (nty * ntx));
    const int i0 = (t / ntx) * tile, j0 = (t % ntx) * tile;
    const int i1 = min(i0 + tile, a.h), j1 = min(j0 + tile, a.w);
    // the row's parameters, once per block
    if (tid == 0) {
      int p[5];
      cr_params(a, b, p);
#pragma unroll
      for (int k = 0; k < 5; ++k) hdr[k] = p[k];
      if (a.meta && t == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) a.meta[b * 5 + k] = p[k];
      }
    }
    __syncthreads();
    const int m = hdr[0], s = hdr[1], g = hdr[2], y0 = hdr[3], x0 = hdr[4];
    // the tile's source pixels [pa0, pa1) x [pb0, pb1) in units of blocks (i', j')
    int pa0 = (g & 4) ? j0 : i0, pa1 = (g & 4) ? j1 : i1;
    int pb0 = (g & 4) ? i0 : j0, pb1 = (g & 4) ? i1 : j1;
    if (g & 2) { const int lo = a.h - pa1, hi = a.h - pa0; pa0 = lo; pa1 = hi; }
    if (g & 1) { const int lo = a.w - pb1, hi = a.w - pb0; pb0 = lo; pb1 = hi; }
    const int nr = (pa1 - pa0) * s;               // patch rows
    const int nb = (pb1 - pb0) * s * a.c * ES;    // bytes of a patch row
    const unsigned char* g0 = (const unsigned char*)a.images +
                              ((((long long)m * a.H + y0 + (long long)s * pa0) * a.W + x0 + (long long)s * pb0) * a.c) * ES;
    const int mis0 = (int)(reinterpret_cast<uintptr_t>(g0) & 15);
    const int nch = (nb + 15) / 16 + 1;           // chunks that cover a row at any distance to the boundary
    const bool staged = nr <= lds_rows && nch <= lds_chunks;  // block-uniform
    const int lds_pitch = lds_chunks * 16;
    if (staged) {
      // lanes along the source row: chunk k of row r is LDS bytes [16 k, 16 k + 16) of slot r.  First the chunks
      // that lie inside the images, four in flight per lane (loaded, then stored); then those that leave them,
      // peeled, in a loop of their own so that no wait of theirs sits between the wide loads
      const int nchunk = nr * nch;
      const long long gofs = g0 - (const unsigned char*)a.images;  // the patch's first byte within the images
      // chunk q as (row, first byte relative to the patch row, LDS offset): 1 wide, 2 peeled, 0 holds no patch byte
      auto chunk = [&](int q, int& r, int& lo, int& dst) -> int {
        r = q / nch;
        const int k = q - r * nch;
        lo = 16 * k - ((mis0 + r * rb16) & 15);
        dst = r * lds_pitch + 16 * k;
        if (q >= nchunk || lo >= nb) return 0;
        const long long at = gofs + r * img_pitch + lo;
        return at >= 0 && at + 16 <= img_bytes ? 1 : 2;
      };
      for (int base = tid; base < nchunk; base += 4 * CR_THREADS) {
        uint4 v0, v1, v2, v3;
        int r, lo, d0, d1, d2, d3;
        const bool w0 = chunk(base, r, lo, d0) == 1;
        if (w0) v0 = *reinterpret_cast<const uint4*>(g0 + r * img_pitch + lo);
        const bool w1 = chunk(base + CR_THREADS, r, lo, d1) == 1;
        if (w1) v1 = *reinterpret_cast<const uint4*>(g0 + r * img_pitch + lo);
        const bool w2 = chunk(base + 2 * CR_THREADS, r, lo, d2) == 1;
        if (w2) v2 = *reinterpret_cast<const uint4*>(g0 + r * img_pitch + lo);
        const bool w3 = chunk(base + 3 * CR_THREADS, r, lo, d3) == 1;
        if (w3) v3 = *reinterpret_cast<const uint4*>(g0 + r * img_pitch + lo);
        if (w0) *reinterpret_cast<uint4*>(patch + d0) = v0;
        if (w1) *reinterpret_cast<uint4*>(patch + d1) = v1;
        if (w2) *reinterpret_cast<uint4*>(patch + d2) = v2;
        if (w3) *reinterpret_cast<uint4*>(patch + d3) = v3;
      }
      for (int q = tid; q < nchunk; q += CR_THREADS) {
        int r, lo, dst;
        if (chunk(q, r, lo, dst) != 2) continue;
        const unsigned char* grow = g0 + r * img_pitch;
        unsigned char* at = patch + dst - lo;  // the LDS address of byte 0 of the patch row
        const int e0 = max(lo, 0), e1 = min(lo + 16, nb);
        for (int x = e0; x < e1; x += ES) {
          if (U8) at[x] = grow[x];
          else *reinterpret_cast<float*>(at + x) = *reinterpret_cast<const float*>(grow + x);
        }
      }
      __syncthreads();
    }
    // lanes along the output rows of the tile
    const int ntj = j1 - j0, per = ntj * a.c, total = (i1 - i0) * per;
    for (int e = tid; e < total; e += CR_THREADS) {
      const int ti = e / per, rest = e - ti * per;
      const int tj = rest / a.c, ch = rest - tj * a.c;
      const int i = i0 + ti, j = j0 + tj;
      int ip = (g & 4) ? j : i, jp = (g & 4) ? i : j;
      if (g & 2) ip = a.h - 1 - ip;
      if (g & 1) jp = a.w - 1 - jp;
      const int r0 = (ip - pa0) * s, k0 = (jp - pb0) * s * a.c + ch;
      const long long o = ((b * a.h + i) * a.w + j) * a.c + ch;
      if (staged) cr_pixel<U8, true>(a, patch, lds_pitch, mis0, rb16, r0, k0, s, o);
      else cr_pixel<U8, false>(a, g0, img_pitch, 0, 0, r0, k0, s, o);
    }
    __syncthreads();  // the header and the patch are the next item's
  }
}

// bytes of LDS behind the header for tiles of T pixels at the largest listed scale: rows and 16-byte chunks a row
inline void cr_patch(const CropArgs& a, int T, int& rows, int& chunks) {
  const long long side = (long long)a.smax * T;
  rows = (int)side;
  chunks = (int)((side * a.c * (a.data_u8 ? 1 : 4) + 15) / 16 + 1);
}

}  // namespace

extern "C" {

int svae_op_crop_batch(const void* images, int data_u8, int nimg, int H, int W, int c, int h, int w,
                       const svae_crop_spec* spec, const int32_t* crops, uint64_t seed, uint64_t offset, int n,
                       float lo, float hi, float* target, uint8_t* target_u8, int32_t* meta, void* stream) {
  if (!images || !spec) return op_fail(SVAE_EBADARG, "crop_batch: null images or spec");
  if (!target && !target_u8) return op_fail(SVAE_EBADARG, "crop_batch: target and target_u8 are both null");
  if (target_u8 && !data_u8) return op_fail(SVAE_EBADARG, "crop_batch: target_u8 needs uint8 images");
  if (nimg <= 0 || H <= 0 || W <= 0 || c <= 0 || h <= 0 || w <= 0 || n <= 0)
    return op_fail(SVAE_EBADARG, "crop_batch: nimg, H, W, c, h, w and n must be positive");
  const svae_crop_spec& p = *spec;
  if (p.n_scales < 1 || p.n_scales > 4) return op_fail(SVAE_EBADARG, "crop_batch: n_scales must be in 1 .. 4");
  int smax = 0;
  for (int k = 0; k < p.n_scales; ++k) {
    const int s = p.scales[k];
    if (s < 1 || s > 8) return op_fail(SVAE_EBADARG, "crop_batch: a scale outside 1 .. 8");
    for (int j = 0; j < k; ++j)
      if (p.scales[j] == s) return op_fail(SVAE_EBADARG, "crop_batch: a scale is listed twice");
    if ((int64_t)s * h > H || (int64_t)s * w > W)
      return op_fail(SVAE_EBADARG, "crop_batch: a scaled tile exceeds the image");
    smax = std::max(smax, s);
  }
  if (p.symmetries != 1 && p.symmetries != 2 && p.symmetries != 4 && p.symmetries != 8)
    return op_fail(SVAE_EBADARG, "crop_batch: symmetries must be 1, 2, 4 or 8");
  if (p.symmetries == 8 && h != w) return op_fail(SVAE_EBADARG, "crop_batch: the dihedral group needs h == w");
  if (data_u8 && !(lo < hi)) return op_fail(SVAE_EBADARG, "crop_batch: lo >= hi with uint8 images");
  if ((int64_t)H * W * c > 2147483647LL || (int64_t)h * w * c > 2147483647LL)
    return op_fail(SVAE_EBADCONFIG, "crop_batch: at most 2^31 - 1 elements per image and per tile");
  CropArgs a{};
  a.images = images; a.data_u8 = data_u8 ? 1 : 0;
  a.nimg = nimg; a.H = H; a.W = W; a.c = c; a.h = h; a.w = w;
  a.n_scales = p.n_scales; a.smax = smax; a.symmetries = p.symmetries;
  for (int k = 0; k < 4; ++k) a.scales[k] = k < p.n_scales ? p.scales[k] : p.scales[0];
  a.crops = crops; a.seed = seed; a.offset = offset; a.n = n;
  a.lo = lo; a.qscale = quant_scale(lo, hi).qscale;
  a.target = target; a.target_u8 = target_u8; a.meta = meta;
  int tile = 16, rows = 0, chunks = 0;
  cr_patch(a, 32, rows, chunks);
  if ((long long)rows * chunks * 16 <= CR_LDS_WIDE) {
    tile = 32;
  } else {
    cr_patch(a, 16, rows, chunks);
    if ((long long)rows * chunks * 16 > CR_LDS_MAX) rows = chunks = 0;  // every block reduces from global memory
  }
  const long long items = (long long)a.n * ((a.h + tile - 1) / tile) * ((a.w + tile - 1) / tile);
  const dim3 grid((unsigned)(items < CR_GRID_CAP ? items : CR_GRID_CAP)), block(CR_THREADS);
  const size_t lds = (size_t)CR_HDR + (size_t)rows * chunks * 16;
  hipStream_t s = (hipStream_t)stream;
  if (a.data_u8) hipLaunchKernelGGL(crop_batch_kernel<true>, grid, block, lds, s, a, tile, rows, chunks);
  else hipLaunchKernelGGL(crop_batch_kernel<false>, grid, block, lds, s, a, tile, rows, chunks);
  return op_done();
}

}  // extern "C"
