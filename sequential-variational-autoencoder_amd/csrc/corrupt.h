// The pixel noise of svae_op_make_batch's contract, shared by batch.hip and degrade.hip: pepper multiplies by 0,
// salt adds 1, Gaussian noise, clip to the data range.  One copy, so both ops round alike.
#pragma once
#include "philox.h"

// make_batch's kernel arguments (degrade.hip fills the fields mb_corrupt reads):
// row b of the batch = data[idx ? idx[b] : start + b] (uint8 or fp32 rows of per_image elements);
// target = lo + u8 * qscale (fp32 rows: as they are); input = clip(target * keep + salt + scale * N(0,1), lo, hi)
// with keep = (pepper word >= thr_pepper), salt = (salt word < thr_salt), Philox counters offset + e / 4
struct MakeBatchArgs {
  const void* data; int data_u8;
  const int* idx; long long start;
  long long per_image, total;        // total = n * per_image
  float lo, hi, qscale, scale;       // qscale = (hi - lo) / 255
  unsigned thr_pepper, thr_salt;
  unsigned long long seed, offset;
  float* target; float* input;       // either may be nullptr
};

// the four outputs of group g from its four clean values
__device__ __forceinline__ void mb_corrupt(const float t[4], long long g, const MakeBatchArgs& a, float o[4]) {
#pragma clang fp contract(off)
  const unsigned long long ctr = a.offset + (unsigned long long)g;
  const unsigned lo32 = (unsigned)ctr, hi32 = (unsigned)(ctr >> 32);
  const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
  float nrm[4] = {0.f, 0.f, 0.f, 0.f};
  unsigned pw[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};  // keep (thr_pepper = 0: every word keeps)
  unsigned sw[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};  // no salt (thr_salt = 0: no word salts)
  if (a.scale != 0.f) {  // the normals are finite, so a zero scale adds exactly +-0
    unsigned c0 = lo32, c1 = hi32, c2 = PHILOX_NORMALS, c3 = 0;
    philox(c0, c1, c2, c3, k0, k1);
    philox_box_muller(c0, c1, c2, c3, nrm);
  }
  if (a.thr_pepper) {
    pw[0] = lo32; pw[1] = hi32; pw[2] = PHILOX_PEPPER; pw[3] = 0;
    philox(pw[0], pw[1], pw[2], pw[3], k0, k1);
  }
  if (a.thr_salt) {
    sw[0] = lo32; sw[1] = hi32; sw[2] = PHILOX_SALT; sw[3] = 0;
    philox(sw[0], sw[1], sw[2], sw[3], k0, k1);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float keep = pw[j] >= a.thr_pepper ? 1.f : 0.f;
    const float salt = sw[j] < a.thr_salt ? 1.f : 0.f;
    // each operation rounded on its own (contract(off) above), in the order the contract states
    float v = t[j] * keep + salt;
    const float gn = a.scale * nrm[j];
    v = v + gn;
    o[j] = fminf(fmaxf(v, a.lo), a.hi);
  }
}
