// Counter-based Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and
// the Box-Muller normals every random draw of the library is formed with (misc.hip philox_normal_kernel,
// batch.hip make_batch_kernel).  A draw is a function of (key, counter) alone, never of the launch.
#pragma once
#include <hip/hip_runtime.h>

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
