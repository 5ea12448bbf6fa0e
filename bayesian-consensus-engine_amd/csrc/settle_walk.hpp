// settle_walk.hpp -- the chain walk of one source's correctness bits, shared by the settlement
// kernels (settle.hip) and the walk-forward trace (walk_forward.hip) so it exists once.
#pragma once
#include "bce_device.hpp"
#include "bce_internal.hpp"
#include "consensus_common.hpp"
#include "reliability_update.hpp"

#pragma clang fp contract(off)

namespace bce {

constexpr int kSyncRun = 11;  // equal outcomes in a row that pin the reliability to 1.0 / 0.0

struct SettleArgs {
  const unsigned long long* bits;
  int64_t n_bits;
  const int64_t* start;  // [S + 1] bit offset of every source's chain
  const int32_t* order;  // [T] touched sources, longest chain first
  int64_t T;
  int64_t n_long;        // the first n_long sources of `order` take the chunked path
  int32_t S;
  double* rel;
  double* conf;
  int64_t* t_us;
  uint8_t* present;      // nullable: every row exists
  int64_t now_us;
  double default_rel;
  double default_conf;
  double2* snap;         // [n_long] {rel, conf} the long chains start from
  int* fault;
};

// The chain of source order[q] as a bit range; false (and the fault word) when the plan is not
// one: the lane then reads and writes nothing.
__device__ __forceinline__ bool settle_range(const SettleArgs& a, int64_t q, int32_t& s, int64_t& b0,
                                             int64_t& b1) {
  s = a.order[q];
  if (s < 0 || s >= a.S) {
    if (a.fault) atomicCAS(a.fault, 0, kFaultSid);
    return false;
  }
  b0 = a.start[s];
  b1 = a.start[s + 1];
  if (b0 < 0 || b1 < b0 || b1 > a.n_bits) {
    if (a.fault) atomicCAS(a.fault, 0, kFaultOffsets);
    return false;
  }
  return b1 > b0;
}

// n confidence updates from c: the chain stops once a step returns its input bit for bit (from
// the cold start 0.25 after 331 steps, at 0.9999999999999996) -- every later step is that step.
__device__ __forceinline__ double settle_conf(double c, int64_t n) {
  for (int64_t k = 0; k < n; ++k) {
    double next = c;
    update_conf(next);
    if (__double_as_longlong(next) == __double_as_longlong(c)) break;
    c = next;
  }
  return c;
}

// The update rule a chain is walked under: the step of one bit, and whether a run of equal bits
// has pinned the reliability.  FixedRule is the reference's constants, compiled in.
struct FixedRule {
  __device__ __forceinline__ void step(double& r, bool correct) const { update_rel(r, correct); }
  __device__ __forceinline__ bool pinned(int run) const { return run >= kSyncRun; }
};

// One point of an update-rule grid: the step delta = min(cap, rate) and the run of equal bits
// that pins r to exactly 1.0 / 0.0 under it (the caller's bound; kNeverSync: no run does).
constexpr int kNeverSync = 0x7fffffff;
struct StepRule {
  double delta;
  int sync;
  __device__ __forceinline__ void step(double& r, bool correct) const { update_rel_step(r, correct, delta); }
  __device__ __forceinline__ bool pinned(int run) const { return run >= sync; }
};

// Chain positions [p0, p1) of the chain that starts at bit b0, word by word (the lane streams its
// own words).  WALK: every bit is one step of `rule` on r.  TRACK: run / prev follow the length of
// the current run of equal bits; the first position that completes a pinning run ends the span
// (its bit already applied) and is returned, else -1.
template <bool WALK, bool TRACK, class Rule>
__device__ __forceinline__ int64_t settle_span(const unsigned long long* __restrict__ bits, int64_t b0, int64_t p0,
                                               int64_t p1, double& r, int& run, bool& prev, const Rule& rule) {
  int64_t g = b0 + p0;
  const int64_t gend = b0 + p1;
  while (g < gend) {
    const int sh = (int)(g & 63);
    unsigned long long w = bits[g >> 6] >> sh;
    const int64_t left = gend - g;
    const int n = left < 64 - sh ? (int)left : 64 - sh;
    for (int k = 0; k < n; ++k) {
      const bool bit = (w & 1ull) != 0;
      w >>= 1;
      if (WALK) rule.step(r, bit);
      if (TRACK) {
        run = (run > 0 && bit == prev) ? run + 1 : 1;
        prev = bit;
        if (rule.pinned(run)) return g + k - b0;
      }
    }
    g += n;
  }
  return -1;
}

// Under the reference's constants: a run of kSyncRun equal bits pins.
template <bool WALK, bool TRACK>
__device__ __forceinline__ int64_t settle_span(const unsigned long long* __restrict__ bits, int64_t b0, int64_t p0,
                                               int64_t p1, double& r, int& run, bool& prev) {
  return settle_span<WALK, TRACK>(bits, b0, p0, p1, r, run, prev, FixedRule{});
}

}  // namespace bce
