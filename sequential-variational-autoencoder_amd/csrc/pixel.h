// The uint8 dequantisation of svae_op_make_batch's contract, shared by every op that turns 8-bit levels into the
// data range (batch.hip, crops.hip, jpeg.hip, tiles.hip).  One copy, so they round alike: crop_batch at scale 1
// equals make_batch and blend_tiles(extract_tiles(img)) is img, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// lo + q * qscale with the product and the sum each rounded to fp32 (the *_rn intrinsics are plain operators
// to the compiler, which would contract them into one fma: the pragma keeps the two roundings the contract states).
// q: a level in [0, 255], whole (a stored byte) or not (crop_batch's block means)
__device__ __forceinline__ float u8_dequant(float q, float lo, float qscale) {
#pragma clang fp contract(off)
  const float p = q * qscale;
  return lo + p;
}

// the four bytes of a little-endian word, lowest first
__device__ __forceinline__ void u8_dequant4(unsigned w, float lo, float qscale, float t[4]) {
  t[0] = u8_dequant((float)(w & 0xFF), lo, qscale);
  t[1] = u8_dequant((float)((w >> 8) & 0xFF), lo, qscale);
  t[2] = u8_dequant((float)((w >> 16) & 0xFF), lo, qscale);
  t[3] = u8_dequant((float)(w >> 24), lo, qscale);
}
