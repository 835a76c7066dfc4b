// What a context-free entry point (svae_op_*: no svae_ctx) needs besides its own checks.  Such an entry point
// lives in the .hip that launches its kernel, as an extern "C" function after the anonymous namespace, and reports
// through svae_last_error(NULL).  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "svae_hip.h"

void svae_tls_error(const std::string& msg);  // engine.cpp: the thread's message behind svae_last_error(NULL)

inline int op_fail(int code, const std::string& msg) {
  svae_tls_error(msg);
  return code;
}

// after the last launch of an op: 0, or SVAE_EHIP with the runtime's own text
inline int op_done() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : op_fail(SVAE_EHIP, hipGetErrorString(e));
}

// thr(p) = min(floor(p 2^32), 2^32 - 1): a word w < thr(p) with probability p
inline uint32_t prob_threshold(float p) {
  const double t = std::floor((double)p * 4294967296.0);
  return t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
}

// the uint8 level spacing of the data range and its inverse, each formed in double and rounded to fp32 once
struct QScale {
  float qscale, qinv;  // (hi - lo) / 255, 255 / (hi - lo)
};
inline QScale quant_scale(float lo, float hi) {
  return {(float)(((double)hi - (double)lo) / 255.0), (float)(255.0 / ((double)hi - (double)lo))};
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
