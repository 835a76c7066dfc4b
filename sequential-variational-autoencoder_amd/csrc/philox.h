// Counter-based Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and
// the Box-Muller normals every random draw of the library is formed with (misc.hip philox_normal_kernel,
// batch.hip make_batch_kernel).  A draw is a function of (key, counter) alone, never of the launch.
#pragma once
#include <hip/hip_runtime.h>

// Counter word c2 of every draw made for a batch under one (seed, offset): the stream.  Two draws of a batch are
// independent because they differ here, so a new per-batch draw takes the next number and no number is reused.
enum PhiloxStream : unsigned {
  PHILOX_NORMALS = 0,  // corrupt.h: the Gaussian pixel noise
  PHILOX_PEPPER = 1,   // corrupt.h
  PHILOX_SALT = 2,     // corrupt.h
  PHILOX_DEGRADE = 3,  // degrade.hip: gates, sigma and boxes per image
  PHILOX_CROPS = 4,    // crops.hip: image, scale, symmetry and origin per row
  PHILOX_JPEG = 5,     // jpeg.hip: gate and quality per image
};

__device__ __forceinline__ void philox(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0,
                                       unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    unsigned h0 = (unsigned)(p0 >> 32), l0 = (unsigned)p0;
    unsigned h1 = (unsigned)(p1 >> 32), l1 = (unsigned)p1;
    unsigned n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the four words of a per-image draw: counter (offset + b in c0 / c1, c2 = stream, c3 = block) under the key
// (lo32(seed), hi32(seed))
__device__ __forceinline__ void philox_image(unsigned long long seed, unsigned long long offset, long long b,
                                             PhiloxStream stream, unsigned block, unsigned w[4]) {
  const unsigned long long ctr = offset + (unsigned long long)b;
  w[0] = (unsigned)ctr; w[1] = (unsigned)(ctr >> 32); w[2] = stream; w[3] = block;
  philox(w[0], w[1], w[2], w[3], (unsigned)seed, (unsigned)(seed >> 32));
}

// four N(0,1) from the four words of one Philox output: u = (w + 0.5) 2^-32 in fp32, Box-Muller on words
// (0, 1) -> v[0], v[1] and on words (2, 3) -> v[2], v[3]
__device__ __forceinline__ void philox_box_muller(unsigned c0, unsigned c1, unsigned c2, unsigned c3, float v[4]) {
  const float inv = 2.3283064365386963e-10f;
  float u0 = (c0 + 0.5f) * inv, u1 = (c1 + 0.5f) * inv, u2 = (c2 + 0.5f) * inv, u3 = (c3 + 0.5f) * inv;
  float r0 = sqrtf(-2.f * __logf(u0)), r1 = sqrtf(-2.f * __logf(u2));
  v[0] = r0 * __cosf(6.2831853f * u1);
  v[1] = r0 * __sinf(6.2831853f * u1);
  v[2] = r1 * __cosf(6.2831853f * u3);
  v[3] = r1 * __sinf(6.2831853f * u3);
}
