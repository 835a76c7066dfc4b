// JPEG compression artefacts on a device batch in one launch (svae_op_jpeg_batch, include/svae_hip.h): per image
// a gate and an IJG quality, then 8-bit levels, JFIF YCbCr, optional 4:2:0 chroma means, the 8 x 8 block DCT, the
// quality-scaled Annex K quantiser, the inverse transform, chroma replication, RGB and the dequantisation of
// svae_op_make_batch.  No entropy coding: only the decoded pixels exist.
//
// The per-image draw is philox.h's philox_image on the stream PHILOX_JPEG, block 0: image b is compressed iff word 0
// is below thr, at quality q_lo + mulhi(word 1, q_hi - q_lo + 1).  The dequantisation is pixel.h's.
// Every sum has a fixed order and every operation is rounded on its own (contract(off)), so the result depends on
// the arguments alone: not on the launch and not on the path (16-byte / scalar) the alignment selects.
//
// One block owns one 16 x 16 pixel tile of one image: two by two 8 x 8 blocks per plane, which is one coding unit
// under 4:2:0 and four under 4:4:4, so no block of the transform straddles two thread blocks and width never
// decides whether LDS suffices.  The gate and the quality are block-uniform.  A block
//   1 stages the in-image part of its tile's interleaved rows in LDS (`raw`; 16-byte loads, or element by element),
//   2 one lane per pixel: levels and YCbCr into the planes' 8 x 8 blocks (`blk`; pixels beyond the image read the
//     tile's last row / column: the contract's replication), under 4:2:0 the chroma means through `chr`,
//   3 one lane per row of eight values held in registers: the forward row pass,
//   4 one lane per column: the forward column pass, the quantiser and the inverse column pass (a lane holds all
//     eight coefficients of its column, so nothing leaves its registers in between),
//   5 one lane per row: the inverse row pass, + 128, rounded and clamped,
//   6 one lane per pixel: chroma replicated, RGB, dequantised into `raw`,
//   7 writes the rows of `raw` (16-byte stores, or element by element).
// Every value written comes from what the block staged, and no other block reads these pixels: in == out is legal.
// The block of an image that is not compressed does steps 1 and 7 alone, or nothing when in == out.
//
// LDS layout: an 8 x 8 block keeps its rows 12 floats apart (a row is two 16-byte accesses) and blocks lie 104
// floats apart.  The column walks of step 4 (lane (block, u) at block * 104 + y * 12 + u) then fall on 32 different
// banks for 32 consecutive lanes (104 mod 32 = 8), where rows 8 apart would put eight lanes on one bank.
// svae_op_jpeg_batch, with its argument checks and the launch, ends the file.
#include <cstdint>

#include "common.h"
#include "opentry.h"
#include "philox.h"
#include "pixel.h"

namespace {

// in [n,h,w,c] -> out (may be in), quality [n] (may be nullptr), one launch
struct JpegArgs {
  const float* in; float* out; int* quality;
  int n, h, w, c;
  unsigned thr;
  int q_lo, q_hi, subsample;         // subsample 2 only with c == 3 (the entry point makes it 1 for c == 1)
  float lo, qscale, qinv;            // qscale = (hi - lo) / 255, qinv = 255 / (hi - lo), each rounded to fp32
  unsigned long long seed, offset;
};

constexpr int JP_THREADS = 128;
constexpr int JP_TILE = 16;
constexpr int JP_ROW = 12;    // floats between the rows of an 8 x 8 block
constexpr int JP_BLK = 104;   // floats between 8 x 8 blocks
constexpr int JP_RAW = 52;    // floats between staged rows: 16 pixels of 3 channels, + 4
constexpr long long JP_GRID_CAP = 1 << 20;  // grid-stride beyond this many blocks

// The JPEG standard's Annex K quantisation tables in natural order ([v][u], v the vertical frequency):
// luminance, then chrominance
__constant__ int JP_BASE[128] = {
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99,
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99};

// The eight magnitudes of the DCT matrix: 1 / sqrt(8), then cos(m pi / 16) / 2 for m = 1 .. 7
constexpr float jp_mag(int m) {
  return m == 0 ? 0.353553391f
       : m == 1 ? 0.490392640f
       : m == 2 ? 0.461939766f
       : m == 3 ? 0.415734806f
       : m == 4 ? 0.353553391f
       : m == 5 ? 0.277785117f
       : m == 6 ? 0.191341716f
                : 0.0975451610f;
}

// C[u][x] = cos((2 x + 1) u pi / 16) / 2, C[0][x] = 1 / sqrt(8): the angle folded into the first octant
constexpr float jp_c(int u, int x) {
  if (u == 0) return jp_mag(0);
  int m = ((2 * x + 1) * u) % 32;
  if (m > 16) m = 32 - m;
  const bool neg = m > 8;
  if (neg) m = 16 - m;
  return neg ? -jp_mag(m) : jp_mag(m);
}

__device__ __forceinline__ float jp_level(float v) { return fminf(fmaxf(rintf(v), 0.f), 255.f); }

// out[k] = sum_j in[j] * C[k][j] (FWD: a forward pass over a row or a column) or sum_j in[j] * C[j][k] (an inverse
// pass), from 0 in ascending j, every product and sum rounded on its own
template <bool FWD>
__device__ __forceinline__ void jp_pass(const float in[8], float out[8]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = in[j] * (FWD ? jp_c(k, j) : jp_c(j, k));
      acc = acc + p;
    }
    out[k] = acc;
  }
}

__device__ __forceinline__ void jp_load_row(const float* row, float v[8]) {
  const float4 a = reinterpret_cast<const float4*>(row)[0], b = reinterpret_cast<const float4*>(row)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__device__ __forceinline__ void jp_store_row(float* row, const float v[8]) {
  reinterpret_cast<float4*>(row)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(row)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// element (y, x) of the 16 x 16 plane whose four blocks start at block b0
__device__ __forceinline__ int jp_at16(int b0, int y, int x) {
  return (b0 + (y >> 3) * 2 + (x >> 3)) * JP_BLK + (y & 7) * JP_ROW + (x & 7);
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_batch_kernel(JpegArgs a, int vec_in, int vec_out) {
#pragma clang fp contract(off)
  __shared__ float4 jp_raw4[JP_TILE * JP_RAW / 4];
  __shared__ float4 jp_blk4[12 * JP_BLK / 4];
  __shared__ float jp_chr[2 * JP_TILE * JP_TILE];  // full-resolution Cb and Cr ahead of the 4:2:0 means
  __shared__ float jp_qt[128];                     // the scaled tables: luminance, chrominance
  __shared__ int jp_hdr[1];
  float* raw = reinterpret_cast<float*>(jp_raw4);
  float* blk = reinterpret_cast<float*>(jp_blk4);
  const int tid = threadIdx.x;
  const int c = a.c, WC = a.w * c;
  const long long P = (long long)a.h * WC;
  const int nty = (a.h + JP_TILE - 1) / JP_TILE, ntx = (a.w + JP_TILE - 1) / JP_TILE;
  const long long items = (long long)a.n * nty * ntx;
  const bool sub2 = a.subsample == 2;
  const int nblk = c == 1 ? 4 : (sub2 ? 6 : 12);
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long b = it / (nty * ntx);
    const int t = (int)(it - b * (nty * ntx));
    const int i0 = (t / ntx) * JP_TILE, j0 = (t % ntx) * JP_TILE;
    const int nr = min(JP_TILE, a.h - i0), nc = min(JP_TILE, a.w - j0), nf = nc * c;
    // the image's draws, once per block
    if (tid == 0) {
      unsigned w[4];
      philox_image(a.seed, a.offset, b, PHILOX_JPEG, 0, w);
      const int q = w[0] < a.thr ? a.q_lo + (int)__umulhi(w[1], (unsigned)(a.q_hi - a.q_lo + 1)) : 0;
      jp_hdr[0] = q;
      if (a.quality && t == 0) a.quality[b] = q;
    }
    __syncthreads();
    const int q = jp_hdr[0];
    if (q != 0 || a.out != a.in) {  // block-uniform
      const float* __restrict__ src = a.in + b * P + (long long)i0 * WC + j0 * c;
      float* dst = a.out + b * P + (long long)i0 * WC + j0 * c;
      // 1: the tile's rows.  j0 is a multiple of 16 and, on the 16-byte path, W C one of 4: so is nf
      if (vec_in) {
        const int q4 = nf >> 2;
        for (int e = tid; e < nr * q4; e += JP_THREADS) {
          const int r = e / q4, k = e - r * q4;
          jp_raw4[r * (JP_RAW / 4) + k] = *reinterpret_cast<const float4*>(src + (long long)r * WC + 4 * k);
        }
      } else {
        for (int e = tid; e < nr * nf; e += JP_THREADS) {
          const int r = e / nf, k = e - r * nf;
          raw[r * JP_RAW + k] = src[(long long)r * WC + k];
        }
      }
      if (q != 0) {
        // IJG's scaling of the base tables, all integer
        const int s = q < 50 ? 5000 / q : 200 - 2 * q;
        for (int e = tid; e < 128; e += JP_THREADS) jp_qt[e] = (float)min(max((JP_BASE[e] * s + 50) / 100, 1), 255);
      }
      __syncthreads();
      if (q != 0) {
        // 2: levels and colour, one lane per pixel of the 16 x 16 tile
        for (int p = tid; p < JP_TILE * JP_TILE; p += JP_THREADS) {
          const int ty = p >> 4, tx = p & 15;
          const float* px = raw + min(ty, nr - 1) * JP_RAW + min(tx, nc - 1) * c;
          if (c == 1) {
            const float d = px[0] - a.lo;
            blk[jp_at16(0, ty, tx)] = jp_level(d * a.qinv);
          } else {
            const float dr = px[0] - a.lo, dg = px[1] - a.lo, db = px[2] - a.lo;
            const float R = jp_level(dr * a.qinv), G = jp_level(dg * a.qinv), B = jp_level(db * a.qinv);
            const float y0 = 0.299f * R, y1 = 0.587f * G, y2 = 0.114f * B;
            const float Y = (y0 + y1) + y2;
            const float u0 = 0.168735892f * R, u1 = 0.331264108f * G, u2 = 0.5f * B;
            const float Cb = ((128.f - u0) - u1) + u2;
            const float v0 = 0.5f * R, v1 = 0.418687589f * G, v2 = 0.081312411f * B;
            const float Cr = ((128.f + v0) - v1) - v2;
            blk[jp_at16(0, ty, tx)] = jp_level(Y);
            if (sub2) {
              jp_chr[p] = jp_level(Cb);
              jp_chr[JP_TILE * JP_TILE + p] = jp_level(Cr);
            } else {
              blk[jp_at16(4, ty, tx)] = jp_level(Cb);
              blk[jp_at16(8, ty, tx)] = jp_level(Cr);
            }
          }
        }
        __syncthreads();
        if (sub2 && c == 3) {
          // the means of the in-image pixels of every 2 x 2 block; chroma beyond the plane replicates its last
          // row / column
          const int nch = (nr + 1) >> 1, ncw = (nc + 1) >> 1;
          for (int e = tid; e < 128; e += JP_THREADS) {
            const int pl = e >> 6, cy = (e >> 3) & 7, cx = e & 7;
            const int r0 = 2 * min(cy, nch - 1), r1 = min(r0 + 2, nr);
            const int c0 = 2 * min(cx, ncw - 1), c1 = min(c0 + 2, nc);
            const float* plane = jp_chr + pl * JP_TILE * JP_TILE;
            float acc = 0.f;
            for (int ii = r0; ii < r1; ++ii)
              for (int jj = c0; jj < c1; ++jj) acc = acc + plane[ii * JP_TILE + jj];
            blk[(4 + pl) * JP_BLK + cy * JP_ROW + cx] = __fdiv_rn(acc, (float)((r1 - r0) * (c1 - c0)));
          }
          __syncthreads();
        }
        // 3: forward row pass, one lane per row
        for (int e = tid; e < nblk * 8; e += JP_THREADS) {
          float* row = blk + (e >> 3) * JP_BLK + (e & 7) * JP_ROW;
          float f[8], tr[8];
          jp_load_row(row, f);
#pragma unroll
          for (int x = 0; x < 8; ++x) f[x] = f[x] - 128.f;
          jp_pass<true>(f, tr);
          jp_store_row(row, tr);
        }
        __syncthreads();
        // 4: forward column pass, quantiser, inverse column pass, one lane per column
        for (int e = tid; e < nblk * 8; e += JP_THREADS) {
          const int bk = e >> 3, u = e & 7;
          float* col = blk + bk * JP_BLK + u;
          const float* qt = jp_qt + (bk >= 4 ? 64 : 0) + u;  // blocks 0 .. 3 are Y's in every layout
          float tv[8], F[8], sv[8];
#pragma unroll
          for (int y = 0; y < 8; ++y) tv[y] = col[y * JP_ROW];
          jp_pass<true>(tv, F);
#pragma unroll
          for (int v = 0; v < 8; ++v) {
            const float T = qt[v * 8];
            const float k = rintf(__fdiv_rn(F[v], T));
            F[v] = k * T;
          }
          jp_pass<false>(F, sv);
#pragma unroll
          for (int y = 0; y < 8; ++y) col[y * JP_ROW] = sv[y];
        }
        __syncthreads();
        // 5: inverse row pass, one lane per row
        for (int e = tid; e < nblk * 8; e += JP_THREADS) {
          float* row = blk + (e >> 3) * JP_BLK + (e & 7) * JP_ROW;
          float sv[8], g[8];
          jp_load_row(row, sv);
          jp_pass<false>(sv, g);
#pragma unroll
          for (int x = 0; x < 8; ++x) g[x] = jp_level(g[x] + 128.f);
          jp_store_row(row, g);
        }
        __syncthreads();
        // 6: chroma up, colour back, dequantisation: the in-image pixels into raw
        for (int p = tid; p < JP_TILE * JP_TILE; p += JP_THREADS) {
          const int ty = p >> 4, tx = p & 15;
          if (ty >= nr || tx >= nc) continue;
          float* px = raw + ty * JP_RAW + tx * c;
          const float Y = blk[jp_at16(0, ty, tx)];
          if (c == 1) {
            px[0] = u8_dequant(Y, a.lo, a.qscale);
          } else {
            float Cb, Cr;
            if (sub2) {
              Cb = blk[4 * JP_BLK + (ty >> 1) * JP_ROW + (tx >> 1)];
              Cr = blk[5 * JP_BLK + (ty >> 1) * JP_ROW + (tx >> 1)];
            } else {
              Cb = blk[jp_at16(4, ty, tx)];
              Cr = blk[jp_at16(8, ty, tx)];
            }
            const float db = Cb - 128.f, dr = Cr - 128.f;
            const float r0 = 1.402f * dr;
            const float g0 = 0.344136286f * db, g1 = 0.714136286f * dr;
            const float b0 = 1.772f * db;
            const float R = jp_level(Y + r0), G = jp_level((Y - g0) - g1), B = jp_level(Y + b0);
            px[0] = u8_dequant(R, a.lo, a.qscale);
            px[1] = u8_dequant(G, a.lo, a.qscale);
            px[2] = u8_dequant(B, a.lo, a.qscale);
          }
        }
        __syncthreads();
      }
      // 7: the tile's rows
      if (vec_out) {
        const int q4 = nf >> 2;
        for (int e = tid; e < nr * q4; e += JP_THREADS) {
          const int r = e / q4, k = e - r * q4;
          *reinterpret_cast<float4*>(dst + (long long)r * WC + 4 * k) = jp_raw4[r * (JP_RAW / 4) + k];
        }
      } else {
        for (int e = tid; e < nr * nf; e += JP_THREADS) {
          const int r = e / nf, k = e - r * nf;
          dst[(long long)r * WC + k] = raw[r * JP_RAW + k];
        }
      }
    }
    __syncthreads();  // the header, the tables and the tile are the next item's
  }
}

}  // namespace

extern "C" {

int svae_op_jpeg_batch(const float* in, int n, int h, int w, int c, float lo, float hi, const svae_jpeg_spec* spec,
                       uint64_t seed, uint64_t offset, float* out, int32_t* quality, void* stream) {
  if (!in || !out || !spec) return op_fail(SVAE_EBADARG, "jpeg_batch: null in, out or spec");
  if (n <= 0 || h <= 0 || w <= 0) return op_fail(SVAE_EBADARG, "jpeg_batch: n, h and w must be positive");
  if (c != 1 && c != 3) return op_fail(SVAE_EBADARG, "jpeg_batch: c must be 1 or 3");
  const svae_jpeg_spec& p = *spec;
  if (!(p.p >= 0.f && p.p <= 1.f)) return op_fail(SVAE_EBADARG, "jpeg_batch: a probability outside [0, 1]");
  if (p.q_lo < 1 || p.q_hi > 100 || p.q_lo > p.q_hi)
    return op_fail(SVAE_EBADARG, "jpeg_batch: need 1 <= q_lo <= q_hi <= 100");
  if (p.subsample != 1 && p.subsample != 2) return op_fail(SVAE_EBADARG, "jpeg_batch: subsample must be 1 or 2");
  if (!(lo < hi)) return op_fail(SVAE_EBADARG, "jpeg_batch: lo >= hi");
  if ((int64_t)h * w * c > 2147483647LL)
    return op_fail(SVAE_EBADCONFIG, "jpeg_batch: at most 2^31 - 1 elements per image");
  JpegArgs a{};
  a.in = in; a.out = out; a.quality = quality;
  a.n = n; a.h = h; a.w = w; a.c = c;
  a.thr = prob_threshold(p.p);
  a.q_lo = p.q_lo; a.q_hi = p.q_hi; a.subsample = c == 3 ? p.subsample : 1;
  const QScale q = quant_scale(lo, hi);
  a.lo = lo; a.qscale = q.qscale; a.qinv = q.qinv;
  a.seed = seed; a.offset = offset;
  const long long items = (long long)n * ((h + JP_TILE - 1) / JP_TILE) * ((w + JP_TILE - 1) / JP_TILE);
  const int row4 = (w * c) % 4 == 0;
  hipLaunchKernelGGL(jpeg_batch_kernel, dim3((unsigned)(items < JP_GRID_CAP ? items : JP_GRID_CAP)),
                     dim3(JP_THREADS), 0, (hipStream_t)stream, a, al16(in) && row4 ? 1 : 0, al16(out) && row4 ? 1 : 0);
  return op_done();
}

}  // extern "C"
