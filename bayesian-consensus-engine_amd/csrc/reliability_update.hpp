// reliability_update.hpp -- compute_update / update_reliability for one participant
// (reliability.py:163-173), shared by the single-step kernels (elementwise.hip) and the chain
// kernels (settle.hip) so the arithmetic exists once.  FP contraction off (CPython rounding).
#pragma once
#pragma clang fp contract(off)

#include "bce_device.hpp"

namespace bce {

// reliability.py:163-169: the capped step and the [0, 1] clamp.
__device__ __forceinline__ void update_rel(double& r, bool correct) {
  const double direction = correct ? 1.0 : -1.0;
  const double raw = 0.15 * direction;                      // _BASE_LEARNING_RATE
  const double capped = py_max(-0.10, py_min(0.10, raw));   // MAX_UPDATE_STEP
  r = py_max(0.0, py_min(1.0, r + capped));
}

// update_rel under another rule.  With direction = +-1.0, learning rate >= 0 and cap >= 0 the
// reference's capped step max(-cap, min(cap, rate * direction)) is exactly +-delta with delta =
// min(cap, rate): selection and negation, no arithmetic, so one double per rule is bit-exact.
__device__ __forceinline__ void update_rel_step(double& r, bool correct, double delta) {
  r = py_max(0.0, py_min(1.0, r + (correct ? delta : -delta)));
}

// reliability.py:172-173: each update closes 10% of the gap to 1.0.
__device__ __forceinline__ void update_conf(double& c) { c = py_min(1.0, c + (1.0 - c) * 0.10); }

__device__ __forceinline__ void update_one(double& r, double& c, bool correct) {
  update_rel(r, correct);
  update_conf(c);
}

}  // namespace bce
