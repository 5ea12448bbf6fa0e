// consensus_history.hpp -- the pieces consensus_history.hip and consensus_leave_one_out.hip write the
// same way: both sort a market once by (sid, position) and read the table through a clamped row.
#pragma once
#pragma clang fp contract(off)

#include "consensus_common.hpp"

namespace bce {

constexpr int kHistMaxThreads = 1024;  // workgroup of the long kernels (one market each)

// A signal's sid as its table row: clamped into [0, n_sources) (unsigned compare, so a negative
// sid clamps to the last row); `bad` is set when it was outside.
__device__ __forceinline__ unsigned hist_row(int32_t sid, int32_t n_sources, bool& bad) {
  const unsigned smax = n_sources > 0 ? (unsigned)(n_sources - 1) : 0u;
  const unsigned s = (unsigned)sid;
  bad = bad || s > smax || n_sources <= 0;
  return s < smax ? s : smax;
}
__device__ __forceinline__ double2 hist_gather(const ConsArgs& a, unsigned row) {
  return a.n_sources > 0 ? a.relconf[row] : make_double2(0.0, 0.0);
}

}  // namespace bce
