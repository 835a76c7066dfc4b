// Structured corruptions of a clean batch in one launch (svae_op_degrade_batch, include/svae_hip.h): per image a
// Gaussian blur, a box down-sampling replicated back to full size and cut-out boxes, then svae_op_make_batch's
// pixel noise and clip (corrupt.h: the one copy of it).
//
// Per-image draws are philox.h's philox_image on the stream PHILOX_DEGRADE: block 0 gives the three gates and
// sigma, block 1 + k the integer geometry of box k.  Every sum has a fixed order and every operation is rounded
// on its own (contract(off)), so the result depends on the arguments alone: not on the launch, not on whether
// the band kernel or the global-memory kernel ran, not on the path (16-byte / scalar) the alignment selects.
//
// Band kernel: a block owns one image and a band of rows (a multiple of 8, so no down-sample block straddles two
// blocks).  It stages the band and r halo rows above and below into LDS (edge rows replicated), blurs horizontally
// LDS -> LDS over all staged rows, vertically over the band's rows, averages the down-sample blocks through LDS and
// walks the band's share of the flat batch in groups of four for the cut-out, the pixel noise and the store.
// svae_op_degrade_batch, with its argument checks and the bound rmax the LDS band is sized for, ends the file.
#include <cstdint>

#include "common.h"
#include "corrupt.h"
#include "opentry.h"

namespace {

// target [n,h,w,c] -> input (and mask [n,h,w], may be nullptr); nz carries the pixel noise (what mb_corrupt reads)
struct DegradeArgs {
  const float* target; float* input; float* mask;
  int n, h, w, c;
  unsigned thr_blur, thr_down, thr_cut;
  float sigma_lo, sigma_hi, fill;
  int factor, boxes, min_side, max_side;
  int rmax;                          // min(ceil(3 sigma_hi), 12), 0 without blur: what the LDS band is sized for
  MakeBatchArgs nz;
};

constexpr int DG_THREADS = 512;  // band kernel: 8 waves a block, two blocks a CU at CelebA geometry (LDS bound)
constexpr int DG_RMAX = 12;  // taps reach min(ceil(3 sigma), 12) pixels
constexpr int DG_HDR = 64;   // words ahead of the two row buffers: draws [0, 4), boxes [4, 20), weights [32, 45)
constexpr long long DG_LDS_MAX = 65536;

struct DgDraws {
  int down, cut, r;
  float sigma;
};

// block 0: the gates, sigma and the tap radius
__device__ __forceinline__ DgDraws dg_draws(const DegradeArgs& a, long long b) {
#pragma clang fp contract(off)
  unsigned w[4];
  philox_image(a.nz.seed, a.nz.offset, b, PHILOX_DEGRADE, 0, w);
  DgDraws d;
  const float u = (float)(w[1] >> 8) * 5.9604644775390625e-8f;  // 2^-24: exact
  const float span = a.sigma_hi - a.sigma_lo;
  const float up = u * span;
  d.sigma = a.sigma_lo + up;
  d.r = 0;
  if (w[0] < a.thr_blur) {
    const int r = (int)ceilf(3.f * d.sigma);
    d.r = min(min(r, DG_RMAX), a.rmax);  // sigma <= sigma_hi, so rmax never binds: it is the bound the LDS was sized for
  }
  d.down = (w[2] < a.thr_down && a.factor > 1) ? 1 : 0;
  d.cut = (w[3] < a.thr_cut && a.boxes > 0) ? 1 : 0;
  return d;
}

// block 1 + k: box k as (y0, x0, height, width), all integer
__device__ __forceinline__ void dg_box(const DegradeArgs& a, long long b, int k, int box[4]) {
  unsigned w[4];
  philox_image(a.nz.seed, a.nz.offset, b, PHILOX_DEGRADE, 1u + (unsigned)k, w);
  const unsigned span = (unsigned)(a.max_side - a.min_side) + 1u;
  const int bh = min(a.h, a.min_side + (int)__umulhi(w[0], span));
  const int bw = min(a.w, a.min_side + (int)__umulhi(w[1], span));
  box[0] = (int)__umulhi(w[2], (unsigned)(a.h - bh + 1));
  box[1] = (int)__umulhi(w[3], (unsigned)(a.w - bw + 1));
  box[2] = bh;
  box[3] = bw;
}

// wt[k] = g_k / (g_0 + 2 sum_{k >= 1} g_k), g_k = expf(-k^2 / (2 sigma^2)), k = 0 .. r (r >= 1)
__device__ __forceinline__ void dg_weights(float sigma, int r, float* wt) {
#pragma clang fp contract(off)
  const float den = 2.f * sigma * sigma;
  float s = 0.f;
  wt[0] = 1.f;
  for (int k = 1; k <= r; ++k) {
    wt[k] = expf(-(float)(k * k) / den);
    s = s + wt[k];
  }
  const float norm = 1.f + 2.f * s;
  for (int k = 0; k <= r; ++k) wt[k] = wt[k] / norm;
}

__device__ __forceinline__ int dg_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the same test on boxes held as (y0, x0 c, y1, x1 c) against a flat column xc = x c + ch of the row
__device__ __forceinline__ bool dg_inside_flat(const int* boxes, int nbox, int y, int xc) {
  bool in = false;
  for (int k = 0; k < nbox; ++k) {
    const int* q = boxes + 4 * k;
    in = in || (y >= q[0] && y < q[2] && xc >= q[1] && xc < q[3]);
  }
  return in;
}

__device__ __forceinline__ bool dg_inside(const int* boxes, int nbox, int y, int x) {
  bool in = false;
  for (int k = 0; k < nbox; ++k) {
    const int* q = boxes + 4 * k;
    in = in || (y >= q[0] && y < q[0] + q[2] && x >= q[1] && x < q[1] + q[3]);
  }
  return in;
}

// Both blur passes of a band in LDS, for a radius r <= RB.  The 2 RB + 1 taps are loaded at once (unrolled: the
// loads' latency overlaps) and the taps beyond r are left out of the sum by a select, so the sum is the contract's:
// from 0, k = -r .. r ascending, every product and sum rounded on its own.  Index arithmetic is kept off the
// per-tap path: (slot, column) advance incrementally with the loop, the horizontal clamp acts on the flat column
// xc + k c within [ch, W C - c + ch] (monotone in x + k, so it is clamp(x + k, 0, W - 1) c + ch), and the tap offsets
// k c and k W C are wave-uniform.
template <int RB>
__device__ __forceinline__ void dg_blur_band(float* A, float* Bf, const float* wt, int r, int nrows, int nr, int w, int c,
                                             int tid) {
#pragma clang fp contract(off)
  const int WC = w * c;
  float wr[RB + 1];
#pragma unroll
  for (int k = 0; k <= RB; ++k) wr[k] = k <= r ? wt[k] : 0.f;
  // horizontal pass over every staged row, A -> Bf
  const int ds = DG_THREADS / WC, dxc = DG_THREADS - ds * WC, dch = dxc % c;
  int s = tid / WC, xc = tid - s * WC, ch = xc % c;
  for (int i = tid; i < nrows * WC; i += DG_THREADS) {
    const float* row = A + s * WC;
    const int lo = ch, hi = WC - c + ch;
    float v[2 * RB + 1];
#pragma unroll
    for (int k = -RB; k <= RB; ++k) v[k + RB] = row[min(max(xc + k * c, lo), hi)];
    float acc = 0.f;
#pragma unroll
    for (int k = -RB; k <= RB; ++k) {
      const int ak = k < 0 ? -k : k;
      const float p = wr[ak] * v[k + RB];
      const float sum = acc + p;
      acc = ak <= r ? sum : acc;
    }
    Bf[i] = acc;
    s += ds; xc += dxc;
    if (xc >= WC) { xc -= WC; ++s; }
    ch += dch;  // W C is a multiple of c: the wrap leaves the channel alone
    if (ch >= c) ch -= c;
  }
  __syncthreads();
  // vertical pass over the band's rows, Bf -> A (band row s is slot s + r of Bf, slot s of A from here on); a tap
  // beyond r reads the centre slot instead (always staged) and is not summed
  for (int i = tid; i < nr * WC; i += DG_THREADS) {
    const float* col = Bf + i + r * WC;
    float v[2 * RB + 1];
#pragma unroll
    for (int k = -RB; k <= RB; ++k) v[k + RB] = col[(k < 0 ? -k : k) <= r ? k * WC : 0];
    float acc = 0.f;
#pragma unroll
    for (int k = -RB; k <= RB; ++k) {
      const int ak = k < 0 ? -k : k;
      const float p = wr[ak] * v[k + RB];
      const float sum = acc + p;
      acc = ak <= r ? sum : acc;
    }
    A[i] = acc;
  }
  __syncthreads();
}

__global__ __launch_bounds__(DG_THREADS) void degrade_band_kernel(DegradeArgs a, int band, int lds_rows, int vec_in,
                                                                   int vec_out) {
#pragma clang fp contract(off)
  extern __shared__ float4 dg_lds4[];
  float* sm = reinterpret_cast<float*>(dg_lds4);
  int* hdr = reinterpret_cast<int*>(sm);
  float* wt = sm + 32;
  const int tid = threadIdx.x;
  const int WC = a.w * a.c;
  const long long P = (long long)a.h * WC;
  const int nband = (a.h + band - 1) / band;
  const long long b = blockIdx.x / nband;
  const int row0 = (int)(blockIdx.x % nband) * band;
  const int row1 = min(row0 + band, a.h);
  const int nr = row1 - row0;

  // the image's draws, once per block
  if (tid == 0) {
    const DgDraws d = dg_draws(a, b);
    hdr[0] = d.r; hdr[1] = d.down; hdr[2] = d.cut;
    if (d.r > 0) dg_weights(d.sigma, d.r, wt);
  } else if (tid <= a.boxes) {
    // the box as (y0, x0 c, y0 + bh, (x0 + bw) c): rows, and flat columns of a row of W C floats
    int q[4];
    dg_box(a, b, tid - 1, q);
    int* o = hdr + 4 * tid;
    o[0] = q[0]; o[1] = q[1] * a.c; o[2] = q[0] + q[2]; o[3] = (q[1] + q[3]) * a.c;
  }
  __syncthreads();
  const int r = hdr[0], down = hdr[1], cut = hdr[2];
  float* A = sm + DG_HDR;
  float* Bf = A + (long long)lds_rows * WC;
  const float* __restrict__ img = a.target + b * P;

  // stage rows row0 - r .. row1 + r - 1 (clamped into the image: edge replicate) as slots 0 .. nrows - 1 of A
  const int nrows = nr + 2 * r;  // <= lds_rows: r <= rmax
  if (vec_in) {
    const int q = WC >> 2;
#pragma unroll 4
    for (int i = tid; i < nrows * q; i += DG_THREADS) {
      const int s = i / q, x4 = i - s * q;
      const int y = dg_clamp(row0 - r + s, a.h - 1);
      reinterpret_cast<float4*>(A)[i] = *reinterpret_cast<const float4*>(img + (long long)y * WC + 4 * x4);
    }
  } else {
#pragma unroll 4
    for (int i = tid; i < nrows * WC; i += DG_THREADS) {
      const int s = i / WC, xc = i - s * WC;
      const int y = dg_clamp(row0 - r + s, a.h - 1);
      A[i] = img[(long long)y * WC + xc];
    }
  }
  __syncthreads();

  if (r > 0) {
    if (r <= 3) dg_blur_band<3>(A, Bf, wt, r, nrows, nr, a.w, a.c, tid);
    else if (r <= 6) dg_blur_band<6>(A, Bf, wt, r, nrows, nr, a.w, a.c, tid);
    else dg_blur_band<DG_RMAX>(A, Bf, wt, r, nrows, nr, a.w, a.c, tid);
  }

  const float* src = A;
  if (down) {
    // one lane per (block, channel): sequential row-major sum of the in-image pixels, one division, replicated
    const int f = a.factor;
    const int nbi = (nr + f - 1) / f, nbj = (a.w + f - 1) / f;
    for (int i = tid; i < nbi * nbj * a.c; i += DG_THREADS) {
      const int ch = i % a.c, t = i / a.c;
      const int bj = t % nbj, bi = t / nbj;
      const int i0 = bi * f, i1 = min(i0 + f, nr), j0 = bj * f, j1 = min(j0 + f, a.w);
      float acc = 0.f;
      for (int ii = i0; ii < i1; ++ii)
        for (int jj = j0; jj < j1; ++jj) acc = acc + A[(ii * a.w + jj) * a.c + ch];
      const float m = __fdiv_rn(acc, (float)((i1 - i0) * (j1 - j0)));
      for (int ii = i0; ii < i1; ++ii)
        for (int jj = j0; jj < j1; ++jj) Bf[(ii * a.w + jj) * a.c + ch] = m;
    }
    __syncthreads();
    src = Bf;
  }

  // the band's elements [E0, E1) of the flat batch, in the groups of four make_batch's noise is drawn for
  const long long E0 = b * P + (long long)row0 * WC, E1 = b * P + (long long)row1 * WC;
  const int* boxes = hdr + 4;
  for (long long g = (E0 >> 2) + tid; g <= ((E1 - 1) >> 2); g += DG_THREADS) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    bool in[4];
    // (band row, flat column) of the group's first element inside the band: one division a group
    const long long ef = (g << 2) > E0 ? (g << 2) : E0;
    const int lf = (int)(ef - E0), yf = lf / WC, xf = lf - yf * WC;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = (g << 2) + j;
      in[j] = e >= E0 && e < E1;
      if (in[j]) {
        const int l = (int)(e - E0);
        float v = src[l];
        if (cut || a.mask) {
          int yl = yf, xc = xf + (l - lf);
          while (xc >= WC) { xc -= WC; ++yl; }
          const bool hit = cut && dg_inside_flat(boxes, a.boxes, row0 + yl, xc);
          if (hit) v = a.fill;
          if (a.mask && xc % a.c == 0) a.mask[(b * a.h + row0 + yl) * a.w + xc / a.c] = hit ? 1.f : 0.f;
        }
        t[j] = v;
      }
    }
    float o[4];
    mb_corrupt(t, g, a.nz, o);
    if (vec_out && in[0] && in[3]) {
      *reinterpret_cast<float4*>(a.input + (g << 2)) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (in[j]) a.input[(g << 2) + j] = o[j];
    }
  }
}

// ---- any shape: every element recomputed from global memory, the same operations in the same order ----
__device__ float dg_hpass_g(const float* row, int x, int ch, int r, const float* wt, int w, int c) {
#pragma clang fp contract(off)
  float acc = 0.f;
  for (int k = -r; k <= r; ++k) {
    const float p = wt[k < 0 ? -k : k] * row[dg_clamp(x + k, w - 1) * c + ch];
    acc = acc + p;
  }
  return acc;
}

__device__ float dg_blur_g(const float* img, int y, int x, int ch, int r, const float* wt, const DegradeArgs& a) {
#pragma clang fp contract(off)
  const int WC = a.w * a.c;
  if (r == 0) return img[(long long)y * WC + x * a.c + ch];
  float acc = 0.f;
  for (int k = -r; k <= r; ++k) {
    const float p =
        wt[k < 0 ? -k : k] * dg_hpass_g(img + (long long)dg_clamp(y + k, a.h - 1) * WC, x, ch, r, wt, a.w, a.c);
    acc = acc + p;
  }
  return acc;
}

__global__ __launch_bounds__(DG_THREADS) void degrade_global_kernel(DegradeArgs a) {
#pragma clang fp contract(off)
  const int WC = a.w * a.c;
  const long long P = (long long)a.h * WC;
  const long long total = (long long)a.n * P;
  const long long G = (total + 3) >> 2;
  for (long long g = (long long)blockIdx.x * DG_THREADS + threadIdx.x; g < G; g += (long long)gridDim.x * DG_THREADS) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    long long cur = -1;  // the image whose draws are held (a group may straddle two images)
    DgDraws d{};
    float wt[DG_RMAX + 1];
    int boxes[16];
    for (int j = 0; j < 4; ++j) {
      const long long e = (g << 2) + j;
      if (e >= total) break;
      const long long b = e / P;
      const int l = (int)(e - b * P);
      if (b != cur) {
        cur = b;
        d = dg_draws(a, b);
        if (d.r > 0) dg_weights(d.sigma, d.r, wt);
        if (d.cut)
          for (int k = 0; k < a.boxes; ++k) dg_box(a, b, k, boxes + 4 * k);
      }
      const float* img = a.target + b * P;
      const int p = l / a.c, ch = l - p * a.c;
      const int y = p / a.w, x = p - y * a.w;
      float v;
      if (d.down) {
        const int f = a.factor;
        const int i0 = (y / f) * f, i1 = min(i0 + f, a.h), j0 = (x / f) * f, j1 = min(j0 + f, a.w);
        float acc = 0.f;
        for (int ii = i0; ii < i1; ++ii)
          for (int jj = j0; jj < j1; ++jj) acc = acc + dg_blur_g(img, ii, jj, ch, d.r, wt, a);
        v = __fdiv_rn(acc, (float)((i1 - i0) * (j1 - j0)));
      } else {
        v = dg_blur_g(img, y, x, ch, d.r, wt, a);
      }
      const bool hit = d.cut && dg_inside(boxes, a.boxes, y, x);
      if (hit) v = a.fill;
      if (a.mask && ch == 0) a.mask[b * a.h * a.w + p] = hit ? 1.f : 0.f;
      t[j] = v;
    }
    float o[4];
    mb_corrupt(t, g, a.nz, o);
    for (int j = 0; j < 4; ++j)
      if ((g << 2) + j < total) a.input[(g << 2) + j] = o[j];
  }
}

// bytes of LDS the band kernel needs for bands of `band` rows (degrade_batch falls back to global memory above 64 KB)
long long degrade_lds_bytes(const DegradeArgs& a, int band) {
  const long long rows = (long long)(band < a.h ? band : a.h) + 2 * a.rmax;
  return 4 * (DG_HDR + 2 * rows * a.w * a.c);
}

void degrade_batch(const DegradeArgs& a, hipStream_t s) {
  int band = 0;
  for (int cand : {16, 8})
    if (!band && degrade_lds_bytes(a, cand) <= DG_LDS_MAX) band = cand;
  const long long nband = band ? (a.h + band - 1) / band : 0;
  if (band && nband * a.n <= 2147483647LL) {
    const int lds_rows = (band < a.h ? band : a.h) + 2 * a.rmax;
    const int vec_in = al16(a.target) && (a.w * a.c) % 4 == 0;
    hipLaunchKernelGGL(degrade_band_kernel, dim3((unsigned)(nband * a.n)), dim3(DG_THREADS),
                       (size_t)degrade_lds_bytes(a, band), s, a, band, lds_rows, vec_in, al16(a.input) ? 1 : 0);
    return;
  }
  const long long total = (long long)a.n * a.h * a.w * a.c;
  const long long nb = ((total + 3) / 4 + DG_THREADS - 1) / DG_THREADS;
  const long long cap = 16384;  // grid-stride beyond this many blocks
  hipLaunchKernelGGL(degrade_global_kernel, dim3((unsigned)(nb < cap ? nb : cap)), dim3(DG_THREADS), 0, s, a);
}

}  // namespace

extern "C" {

int svae_op_degrade_batch(const float* target, int n, int h, int w, int c, float lo, float hi,
                          const svae_degrade_spec* spec, uint64_t seed, uint64_t offset, float* input, float* mask,
                          void* stream) {
  if (!target || !input || !spec) return op_fail(SVAE_EBADARG, "degrade_batch: null target, input or spec");
  if (input == target) return op_fail(SVAE_EBADARG, "degrade_batch: in place is not possible (the blur reads neighbours)");
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return op_fail(SVAE_EBADARG, "degrade_batch: n, h, w and c must be positive");
  const int64_t per_image = (int64_t)h * w * c;
  if (per_image < 4) return op_fail(SVAE_EBADARG, "degrade_batch: h * w * c must be at least 4");
  if (per_image > 2147483647LL) return op_fail(SVAE_EBADCONFIG, "degrade_batch: at most 2^31 - 1 elements per image");
  const svae_degrade_spec& p = *spec;
  auto prob = [](float v) { return v >= 0.f && v <= 1.f; };
  if (!prob(p.p_blur) || !prob(p.p_down) || !prob(p.p_cut) || !prob(p.pepper_prob) || !prob(p.salt_prob))
    return op_fail(SVAE_EBADARG, "degrade_batch: a probability outside [0, 1]");
  if (!(p.sigma_lo >= 0.f) || !(p.sigma_lo <= p.sigma_hi) || !(p.sigma_hi <= 4.f))
    return op_fail(SVAE_EBADARG, "degrade_batch: need 0 <= sigma_lo <= sigma_hi <= 4");
  if (p.factor != 1 && p.factor != 2 && p.factor != 4 && p.factor != 8)
    return op_fail(SVAE_EBADARG, "degrade_batch: factor must be 1, 2, 4 or 8");
  if (p.boxes < 0 || p.boxes > 4) return op_fail(SVAE_EBADARG, "degrade_batch: boxes must be in 0 .. 4");
  if (p.min_side < 1 || p.min_side > p.max_side)
    return op_fail(SVAE_EBADARG, "degrade_batch: need 1 <= min_side <= max_side");
  if (!(p.gaussian_scale >= 0.f)) return op_fail(SVAE_EBADARG, "degrade_batch: negative gaussian_scale");
  if (!(lo <= hi)) return op_fail(SVAE_EBADARG, "degrade_batch: lo > hi");
  DegradeArgs a{};
  a.target = target; a.input = input; a.mask = mask;
  a.n = n; a.h = h; a.w = w; a.c = c;
  a.thr_blur = prob_threshold(p.p_blur); a.thr_down = prob_threshold(p.p_down); a.thr_cut = prob_threshold(p.p_cut);
  a.sigma_lo = p.sigma_lo; a.sigma_hi = p.sigma_hi; a.fill = p.fill;
  a.factor = p.factor; a.boxes = p.boxes; a.min_side = p.min_side; a.max_side = p.max_side;
  // the largest tap radius a draw can give: sigma <= sigma_hi, and the kernel forms ceilf(3.f * sigma) alike
  const int rmax = (int)std::ceil(3.f * p.sigma_hi);
  a.rmax = a.thr_blur ? (rmax < 12 ? rmax : 12) : 0;
  a.nz.lo = lo; a.nz.hi = hi; a.nz.scale = p.gaussian_scale;
  a.nz.thr_pepper = prob_threshold(p.pepper_prob); a.nz.thr_salt = prob_threshold(p.salt_prob);
  a.nz.seed = seed; a.nz.offset = offset;
  degrade_batch(a, (hipStream_t)stream);
  return op_done();
}

}  // extern "C"
