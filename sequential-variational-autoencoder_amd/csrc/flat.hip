// Flat-convolution generator kernels (generator_flat, sequential_vae.py:1880-1936): 4x4 stride-1
// TF-SAME convolutions at full image resolution with a handful of channels (3 -> 6 -> 12 -> 24 -> 12
// -> 6 -> 3), in exact fp32 on v_mfma_f32_16x16x4_f32 in every dtype mode (a k-ordered fmaf chain).
//
// One block of 4 waves owns R whole output rows of one image (R * W <= 256 pixels; the whole image when
// H * W < 256) and stages the (R+3) x (W+3) x C window of the gathered tensor in LDS once: TF SAME at
// stride 1 for k = 4 pads 1 row / column before and 2 after (the adjoint: 2 before, 1 after, taps
// flipped).  The window is written as the tensor the convolution sees, so the padding is zeros of the
// ACTIVATED tensor and what the producer left undone is applied while staging:
//   forward      lrelu(bn(pre)) of the previous layer from its pre-BN tensor + mean / invstd / beta
//   dgrad, wgrad d pre = invstd * (dz - S/n - xhat * Q/n) from dz = d act * lrelu'(y), pre and the sums
// so no full-resolution BN apply or BN-backward apply pass exists: every full-resolution tensor is
// written once.  GEMM views:
//   forward / dgrad  M = the block's pixels (16 per MFMA tile, 4 tiles per wave = 4 independent
//                    accumulator chains per N tile), K = 16 * C (tap-major), N = channels out padded to 16 / 32
//   wgrad            M = 16 * Cin rows (tap, cin) = Cin tiles dealt over the waves, N = Cout padded,
//                    K = the block's pixels; per-block slabs summed in block order by flat_wsum
// Epilogues: the forward writes the pre-BN output and per-block (sum, sum^2) partials; the input
// gradient multiplies by lrelu'(y) of the layer below and writes the (sum dz, sum dz * xhat) partials.
// Partials are fp64, combined lane -> wave -> block in a fixed order and finished by sd_stat_fin
// (chain.hip) in block order: bit-deterministic, no float atomics.
#include <algorithm>

#include "kernels.h"

#define FLAT_TPB 256
#define FLAT_MAXC 32

namespace {

struct FlatGeo {
  int N, H, Wd, R, bpi;  // images, image size, rows per block, blocks per image
  FastDiv dWP;           // window row length W + 3
};

// what a staged element is made from (see the header)
struct FlatLoad {
  const float* src;   // gathered tensor [N, H, W, ld]
  int ld, C;
  int mode;           // 0 raw, 1 lrelu(bn(src)), 2 d pre from dz = src
  const float* pre;   // mode 2: the layer's pre-BN tensor [.., C]
  const float *mean, *invstd, *beta, *sums;
  float inv_n;
  FastDiv dC;
};

__device__ __forceinline__ float flat_load(const FlatLoad& L, long long p, int c) {
  const float v = L.src[p * L.ld + c];
  if (L.mode == 0) return v;
  if (L.mode == 1) return lrelu_f(bn_y1(v, L.mean[c], L.invstd[c], L.beta[c]));
  const float is = L.invstd[c];
  const float xh = (L.pre[p * L.C + c] - L.mean[c]) * is;
  return is * (v - L.sums[2 * c] * L.inv_n - xh * (L.sums[2 * c + 1] * L.inv_n));
}

// window [R+3][W+3][C] of rows oy0 - pb .. of image n, zeros outside the image.  The global loads of a
// batch of 16 elements per thread are issued before its LDS stores.
__device__ __forceinline__ void flat_stage_window(const FlatLoad& L, const FlatGeo& g, int n, int oy0, int pb,
                                                  float* win) {
  const int WP = g.Wd + 3, C = L.C;
  const int tot = (g.R + 3) * WP * C;
  const long long img = (long long)n * g.H * g.Wd;
  for (int base = 0; base < tot; base += FLAT_TPB * 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = base + u * FLAT_TPB + threadIdx.x;
      v[u] = 0.f;
      if (i < tot) {
        const int q = fdiv(i, L.dC), c = i - q * C;
        const int rr = fdiv(q, g.dWP), col = q - rr * WP;
        const int iy = oy0 - pb + rr, ix = col - pb;
        if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.Wd) v[u] = flat_load(L, img + (long long)iy * g.Wd + ix, c);
      }
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = base + u * FLAT_TPB + threadIdx.x;
      if (i < tot) win[i] = v[u];
    }
  }
}

struct FlatConvArgs {
  FlatLoad in;
  FlatGeo g;
  const float* W;     // TF [4][4][Cin][Cout]
  int Cd;             // channels written
  int adj;            // 0: y = conv(in, W) (in.C = Cin, Cd = Cout); 1: dx = conv^T(in, W) (in.C = Cout, Cd = Cin)
  const float* bias;  // optional, added to the stored value (not to the statistics)
  float* dst;
  int ldd;
  // adj epilogue: dst = acc * lrelu'(bn(opre)) and the partials (sum dz, sum dz * xhat) of the layer below
  const float *opre, *omean, *oinvstd, *obeta;
  double* part;       // [blocks][Cd][2] or null
};

// forward conv / input gradient.  LDS: win | wl [16 * C][16 * NT] | koff [16 * C] | red [4][16 * NT][2] fp64
template <int NT>
__global__ __launch_bounds__(FLAT_TPB) void flat_conv_kernel(const FlatConvArgs a) {
  extern __shared__ __align__(16) char flat_sm[];
  constexpr int NP = 16 * NT;
  const FlatGeo g = a.g;
  const int C = a.in.C, K = 16 * C, WP = g.Wd + 3;
  const int nwin = (g.R + 3) * WP * C;
  double* red = (double*)flat_sm;                 // (first: 8-byte aligned)
  float* win = (float*)(red + 4 * NP * 2);
  float* wl = win + nwin;
  int* koff = (int*)(wl + K * NP);
  const int n = blockIdx.x / g.bpi;
  const int oy0 = (blockIdx.x % g.bpi) * g.R;
  const int rows = min(g.R, g.H - oy0);
  const int npix = rows * g.Wd;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

  flat_stage_window(a.in, g, n, oy0, a.adj ? 2 : 1, win);
  for (int i = threadIdx.x; i < K * NP; i += FLAT_TPB) {
    const int j = i % NP, k = i / NP;
    const int tap = fdiv(k, a.in.dC), c = k - tap * C;
    float w = 0.f;
    if (j < a.Cd) w = a.adj ? a.W[((15 - tap) * a.Cd + j) * C + c] : a.W[(tap * C + c) * a.Cd + j];
    wl[i] = w;
  }
  for (int k = threadIdx.x; k < K; k += FLAT_TPB) {
    const int tap = k / C, c = k % C;
    koff[k] = ((tap >> 2) * WP + (tap & 3)) * C + c;
  }
  __syncthreads();

  f32x4 acc[4][NT];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mi][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (wv * 64 < npix) {  // (wave-uniform: a wave whose 64 pixels are all past the block's has no work)
    int pb[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      int pix = wv * 64 + mi * 16 + (lane & 15);
      if (pix >= npix) pix = 0;  // (reads stay inside the window; the rows are dropped below)
      pb[mi] = ((pix / g.Wd) * WP + pix % g.Wd) * C;
    }
    const int kq = lane >> 4, jn = lane & 15;
    for (int k0 = 0; k0 < K; k0 += 4) {
      const int k = k0 + kq;
      const int ko = koff[k];
      float bv[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bv[nt] = wl[k * NP + nt * 16 + jn];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const float av = win[pb[mi] + ko];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mi][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[nt], acc[mi][nt], 0, 0, 0);
      }
    }
  }
  // epilogue: D[row 4 * (lane >> 4) + r][col lane & 15]
  const long long pix0 = ((long long)n * g.H + oy0) * g.Wd;
  double s1[NT], s2[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    s1[nt] = 0.0;
    s2[nt] = 0.0;
    const int ch = nt * 16 + (lane & 15);
    const bool chok = ch < a.Cd;
    float om = 0.f, ois = 0.f, ob = 0.f, bi = 0.f;
    if (chok && a.opre) { om = a.omean[ch]; ois = a.oinvstd[ch]; ob = a.obeta[ch]; }
    if (chok && a.bias) bi = a.bias[ch];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pix = wv * 64 + mi * 16 + 4 * (lane >> 4) + r;
        if (!chok || pix >= npix) continue;
        const long long p = pix0 + pix;
        float v = acc[mi][nt][r];
        if (a.opre) {
          const float x = a.opre[p * a.Cd + ch];
          v *= dact_from_y(bn_y1(x, om, ois, ob), ACT_LRELU);
          s1[nt] += (double)v;
          s2[nt] += (double)(v * ((x - om) * ois));
        } else {
          s1[nt] += (double)v;
          s2[nt] += (double)v * (double)v;
        }
        a.dst[p * a.ldd + ch] = v + bi;
      }
  }
  if (!a.part) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    s1[nt] += __shfl_xor(s1[nt], 16);
    s1[nt] += __shfl_xor(s1[nt], 32);
    s2[nt] += __shfl_xor(s2[nt], 16);
    s2[nt] += __shfl_xor(s2[nt], 32);
    if (lane < 16) {
      red[(wv * NP + nt * 16 + lane) * 2] = s1[nt];
      red[(wv * NP + nt * 16 + lane) * 2 + 1] = s2[nt];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * a.Cd) {
    double s = 0.0;
    for (int w = 0; w < 4; ++w) s += red[w * NP * 2 + threadIdx.x];
    a.part[(long long)blockIdx.x * 2 * a.Cd + threadIdx.x] = s;
  }
}

struct FlatWgradArgs {
  FlatLoad in;   // the layer's input (C = Cin)
  FlatLoad dy;   // its d pre (C = Cout)
  FlatGeo g;
  int G;         // row groups (of <= 256 pixels) per block: fewer, larger slabs at large batches
  float* part;   // [blocks][16 * Cin * Cout]
};

// weight-gradient slab of one block: the sum over its G row groups (accumulated in registers, groups in
// order).  LDS: win | dp [256][16 * NT] | koff [16 * Cin] | poff [256]; wave w owns the M tiles w, w + 4, ...
// (TPW of them at most)
template <int NT, int TPW>
__global__ __launch_bounds__(FLAT_TPB) void flat_wgrad_kernel(const FlatWgradArgs a) {
  extern __shared__ __align__(16) char flat_sm[];
  constexpr int NP = 16 * NT;
  const FlatGeo g = a.g;
  const int Ci = a.in.C, Co = a.dy.C, K = 16 * Ci, WP = g.Wd + 3;
  const int nwin = (g.R + 3) * WP * Ci;
  float* win = (float*)flat_sm;
  float* dp = win + nwin;
  int* koff = (int*)(dp + FLAT_TPB * NP);
  int* poff = koff + K;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ngrp = g.N * g.bpi;

  for (int k = threadIdx.x; k < K; k += FLAT_TPB) {
    const int tap = k / Ci, c = k % Ci;
    koff[k] = ((tap >> 2) * WP + (tap & 3)) * Ci + c;
  }
  f32x4 acc[TPW][NT];
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[j][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int gi = 0; gi < a.G; ++gi) {
    const int grp = blockIdx.x * a.G + gi;
    if (grp >= ngrp) break;  // (block-uniform)
    const int n = grp / g.bpi;
    const int oy0 = (grp % g.bpi) * g.R;
    const int rows = min(g.R, g.H - oy0);
    const int npix = rows * g.Wd;
    const long long pix0 = ((long long)n * g.H + oy0) * g.Wd;
    if (gi) __syncthreads();  // the previous group's reads of win / dp / poff
    flat_stage_window(a.in, g, n, oy0, 1, win);
    for (int base = 0; base < FLAT_TPB * NP; base += FLAT_TPB * 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = base + u * FLAT_TPB + threadIdx.x;
        const int co = i % NP, pix = i / NP;
        v[u] = (i < FLAT_TPB * NP && pix < npix && co < Co) ? flat_load(a.dy, pix0 + pix, co) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = base + u * FLAT_TPB + threadIdx.x;
        if (i < FLAT_TPB * NP) dp[i] = v[u];
      }
    }
    {
      const int pix = threadIdx.x < npix ? threadIdx.x : 0;
      poff[threadIdx.x] = ((pix / g.Wd) * WP + pix % g.Wd) * Ci;
    }
    __syncthreads();
    if (wv < Ci) {
      int ko[TPW];
#pragma unroll
      for (int j = 0; j < TPW; ++j) ko[j] = wv + 4 * j < Ci ? koff[(wv + 4 * j) * 16 + (lane & 15)] : 0;
      const int kq = lane >> 4, jn = lane & 15;
      const int kend = (npix + 3) & ~3;
      for (int k0 = 0; k0 < kend; k0 += 4) {
        const int pix = k0 + kq;
        const int po = poff[pix];
        float bv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = dp[pix * NP + nt * 16 + jn];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          if (wv + 4 * j < Ci) {
            const float av = win[po + ko[j]];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[j][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[nt], acc[j][nt], 0, 0, 0);
          }
        }
      }
    }
  }
  float* out = a.part + (long long)blockIdx.x * K * Co;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int mt = wv + 4 * j;
    if (mt >= Ci) continue;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int co = nt * 16 + (lane & 15);
      if (co >= Co) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(mt * 16 + 4 * (lane >> 4) + r) * Co + co] = acc[j][nt][r];
    }
  }
}

// out0[j] (j < n0) / out1[j - n0] = fp64 sum over the block slabs: 16 columns x 16 interleaved slab
// slices per block, each slice summed in slab order, the slices in slice order
__global__ __launch_bounds__(FLAT_TPB) void flat_wsum_kernel(const float* part, int nblk, int nw, float* out0, int n0,
                                                             float* out1) {
  __shared__ double red[16][17];
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int j = blockIdx.x * 16 + cl;
  double s = 0.0;
  if (j < nw)
    for (int b = sl; b < nblk; b += 16) s += part[(long long)b * nw + j];
  red[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && j < nw) {
    double t = 0.0;
    for (int i = 0; i < 16; ++i) t += red[i][cl];
    if (j < n0) out0[j] = (float)t;
    else out1[j - n0] = (float)t;
  }
}

// per-block column sums of X [rows][ld] (C <= 32 columns), fp64 partials [blocks][C][2] (second slot 0):
// xor-shuffle sums inside each wave, the four waves added in wave order
__global__ __launch_bounds__(FLAT_TPB) void flat_colsum_kernel(const float* X, int ld, long long rows, int C,
                                                               double* part) {
  __shared__ double red[FLAT_MAXC][FLAT_TPB / 64];
  const long long p = (long long)blockIdx.x * FLAT_TPB + threadIdx.x;
  for (int c = 0; c < C; ++c) {
    double v = p < rows ? (double)X[p * ld + c] : 0.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < C) {
    double t = 0.0;
    for (int w = 0; w < FLAT_TPB / 64; ++w) t += red[threadIdx.x][w];
    part[((long long)blockIdx.x * C + threadIdx.x) * 2] = t;
    part[((long long)blockIdx.x * C + threadIdx.x) * 2 + 1] = 0.0;
  }
}

const size_t kFlatLdsMax = 160 * 1024;
constexpr int kMaxDev = 64;
int cur_device() {
  int d = 0;
  (void)hipGetDevice(&d);
  return d >= 0 && d < kMaxDev ? d : 0;
}

FlatGeo flat_geo(int N, int H) {
  FlatGeo g;
  g.N = N; g.H = H; g.Wd = H;
  g.R = std::max(1, std::min(H, FLAT_TPB / H));
  g.bpi = (H + g.R - 1) / g.R;
  g.dWP = make_fastdiv(H + 3);
  return g;
}

size_t conv_lds(const FlatGeo& g, int C, int NT) {
  return (size_t)4 * 16 * NT * 2 * sizeof(double) +
         ((size_t)(g.R + 3) * (g.Wd + 3) * C + (size_t)16 * C * 16 * NT + 16 * C) * sizeof(float);
}
size_t wgrad_lds(const FlatGeo& g, int Ci, int NT) {
  return ((size_t)(g.R + 3) * (g.Wd + 3) * Ci + (size_t)FLAT_TPB * 16 * NT + 16 * Ci + FLAT_TPB) * sizeof(float);
}

bool shape_ok(int N, int H, int Cs, int Cd) {
  return N >= 1 && H >= 1 && H <= FLAT_TPB && Cs >= 1 && Cs <= FLAT_MAXC && Cd >= 1 && Cd <= FLAT_MAXC &&
         (long long)N * H * H < (1LL << 31) / FLAT_MAXC;
}

template <int NT>
void launch_conv(const FlatConvArgs& a, size_t lds, hipStream_t s) {
  static bool attr[kMaxDev] = {};  // the attribute is per device
  const int dev = cur_device();
  if (!attr[dev]) {
    (void)hipFuncSetAttribute((const void*)flat_conv_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFlatLdsMax);
    attr[dev] = true;
  }
  hipLaunchKernelGGL(flat_conv_kernel<NT>, dim3(a.g.N * a.g.bpi), dim3(FLAT_TPB), lds, s, a);
}

// row groups per weight-gradient block: 1 until the launch has over two blocks per CU's worth of groups
// (512), then as many as keep 512 blocks, 8 at most -- fewer slabs to write and to sum
int wgrad_groups(const FlatGeo& g) { return std::max(1, std::min(8, g.N * g.bpi / 512)); }
int wgrad_blocks(const FlatGeo& g, int G) { return (g.N * g.bpi + G - 1) / G; }

template <int NT, int TPW>
void launch_wgrad(const FlatWgradArgs& a, size_t lds, hipStream_t s) {
  static bool attr[kMaxDev] = {};
  const int dev = cur_device();
  if (!attr[dev]) {
    (void)hipFuncSetAttribute((const void*)flat_wgrad_kernel<NT, TPW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)kFlatLdsMax);
    attr[dev] = true;
  }
  hipLaunchKernelGGL((flat_wgrad_kernel<NT, TPW>), dim3(wgrad_blocks(a.g, a.G)), dim3(FLAT_TPB), lds, s, a);
}

FlatLoad make_load(const FlatIn& f, int C) {
  FlatLoad L{};
  L.src = f.p; L.ld = f.ld ? f.ld : C; L.C = C; L.mode = f.mode;
  L.pre = f.pre; L.mean = f.mean; L.invstd = f.invstd; L.beta = f.beta; L.sums = f.sums; L.inv_n = f.inv_n;
  L.dC = make_fastdiv(C);
  return L;
}

}  // namespace

int flat_blocks(int N, int H) { return N * flat_geo(N, H).bpi; }

bool flat_conv_ok(int N, int H, int Cs, int Cd) {
  return shape_ok(N, H, Cs, Cd) && conv_lds(flat_geo(N, H), Cs, Cd > 16 ? 2 : 1) <= kFlatLdsMax;
}
bool flat_wgrad_ok(int N, int H, int Ci, int Co) {
  return shape_ok(N, H, Ci, Co) && wgrad_lds(flat_geo(N, H), Ci, Co > 16 ? 2 : 1) <= kFlatLdsMax;
}

int flat_conv(const FlatIn& in, int N, int H, int Cs, const float* W, int Cd, int adj, const float* bias, float* dst,
              int ldd, const FlatOut& o, double* part, hipStream_t s) {
  if (!flat_conv_ok(N, H, Cs, Cd)) return -1;
  FlatConvArgs a{};
  a.in = make_load(in, Cs);
  a.g = flat_geo(N, H);
  a.W = W; a.Cd = Cd; a.adj = adj; a.bias = bias; a.dst = dst; a.ldd = ldd ? ldd : Cd;
  a.opre = o.pre; a.omean = o.mean; a.oinvstd = o.invstd; a.obeta = o.beta;
  a.part = part;
  const int NT = Cd > 16 ? 2 : 1;
  const size_t lds = conv_lds(a.g, Cs, NT);
  if (NT == 1) launch_conv<1>(a, lds, s);
  else launch_conv<2>(a, lds, s);
  return 0;
}

int flat_wgrad(const FlatIn& in, const FlatIn& dy, int N, int H, int Ci, int Co, float* part, float* dW,
               hipStream_t s) {
  if (!flat_wgrad_ok(N, H, Ci, Co)) return -1;
  FlatWgradArgs a{};
  a.in = make_load(in, Ci);
  a.dy = make_load(dy, Co);
  a.g = flat_geo(N, H);
  a.G = wgrad_groups(a.g);
  a.part = part;
  const int NT = Co > 16 ? 2 : 1;
  const size_t lds = wgrad_lds(a.g, Ci, NT);
  const int tpw = (Ci + 3) / 4;
#define FLAT_WG(NT_, TPW_) launch_wgrad<NT_, TPW_>(a, lds, s)
  if (NT == 1) {
    if (tpw <= 1) FLAT_WG(1, 1);
    else if (tpw <= 2) FLAT_WG(1, 2);
    else if (tpw <= 4) FLAT_WG(1, 4);
    else FLAT_WG(1, 8);
  } else {
    if (tpw <= 1) FLAT_WG(2, 1);
    else if (tpw <= 2) FLAT_WG(2, 2);
    else if (tpw <= 4) FLAT_WG(2, 4);
    else FLAT_WG(2, 8);
  }
#undef FLAT_WG
  const int nw = 16 * Ci * Co;
  hipLaunchKernelGGL(flat_wsum_kernel, dim3((nw + 15) / 16), dim3(FLAT_TPB), 0, s, part, wgrad_blocks(a.g, a.G), nw, dW,
                     nw, (float*)nullptr);
  return 0;
}

int flat_colsum_blocks(long long rows) { return (int)((rows + FLAT_TPB - 1) / FLAT_TPB); }
void flat_colsum(const float* X, int ld, long long rows, int C, double* part, hipStream_t s) {
  hipLaunchKernelGGL(flat_colsum_kernel, dim3(flat_colsum_blocks(rows)), dim3(FLAT_TPB), 0, s, X, ld, rows, C, part);
}
