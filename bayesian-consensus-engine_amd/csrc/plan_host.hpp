// plan_host.hpp -- the host-side decisions of the planned consensus launch: the length bins,
// the long-market scratch size and WHICH launches a planned batch makes (plan_schedule).  Plain
// C++17, no HIP: the C entries (consensus_api.hip) launch what plan_schedule lists,
// bce_plan_schedule (plan.hip) hands the same list to sharding._rank_main_us, and
// tests/test_plan_schedule.py pins it without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/bce.h"

namespace bce {

constexpr int kLongMaxLds = 4096;  // longest market the LDS kernels take; beyond: global scratch
static_assert(BCE_NBINS == 13, "bin table");
constexpr int64_t kBinMax[BCE_NBINS - 1] = {8, 16, 32, 64, 128, 256, 512, 1024, 1536, 2048, 3072, kLongMaxLds};
constexpr int kBinNp2Lo = 8, kBinNp2Hi = 10;  // the 1536 and 3072 bins
static_assert(kBinMax[kBinNp2Lo] == 1536 && kBinMax[kBinNp2Hi] == 3072, "non-power-of-two bins");
constexpr int kPlanSideLast = 3;  // bins 0..3 (n <= 64) run on the side stream
constexpr double kMergeRounds = 6.0;  // merge a small call's bins below this many resident rounds
inline int bin_of(int64_t n) {
  for (int b = 0; b < BCE_NBINS - 1; ++b)
    if (n <= kBinMax[b]) return b;
  return BCE_NBINS - 1;
}

constexpr int kHugeGrid = 512;  // workgroups of the global-scratch long kernel (one slice each)

inline int64_t next_pow2(int64_t n) {
  int64_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// Scratch of the global-scratch long kernel for `count` (> 0) markets of at most max_len
// signals: four arrays of next_pow2(max_len) 8-byte keys per workgroup ...
inline int64_t long_scratch_grid(int64_t count) { return count < kHugeGrid ? count : kHugeGrid; }
inline int64_t long_scratch_bytes(int64_t count, int64_t max_len) {
  return long_scratch_grid(count) * 4 * next_pow2(max_len) * 8;
}
// ... and the keys per workgroup slice that `bytes` of it give the same launch.
inline int64_t long_scratch_stride(int64_t count, int64_t bytes) { return bytes / (long_scratch_grid(count) * 4 * 8); }

// One kernel launch of a planned batch: the markets of bins b0..b1 in one kernel sized for bin
// b1 (its own markets first, then the shorter bins' -- consensus_wide_kernel's list_hi).
struct PlanLaunch {
  int b0, b1;
  bool side;  // on the side stream
};
struct PlanSchedule {
  PlanLaunch launch[BCE_NBINS];  // in issue order
  int n = 0;
  bool fork = false;  // the side stream is forked from / joined into the caller's
};

// The launches of a planned batch.  resident(b): resident workgroups of wide bin b's kernel
// (wide_resident); asked only about a range that holds markets.
//
// bin_start (host int64[BCE_NBINS + 1]) given -- bce_consensus_planned:
//   The short-market bins (n <= 64) are small latency-bound launches: they run on a side
//   stream while the long bins run on the caller's, longest first (joined before return).
//   Measured on C3: 1.73 -> 1.65 ms; moving wide bins to the side stream too, or forking every
//   bin over 2-8 streams, was slower (profiles/r02_c3_plan_streams.jsonl); so was dealing every
//   bin over 2 or 4 streams with the resident grid shared out by estimated work (round 5,
//   profiles/archive/r05b/: one 8th of C3 0.233 -> 0.294 / 0.307 ms), and a small call's 65..1024
//   launches on a second side stream (0.2188 -> 0.2325 ms, profiles/archive/r05f/).
//   Fork only when both streams get work: a batch of only short or only long markets runs on
//   the caller's stream alone, without the fork / join events (~10 us of step boundary,
//   DESIGN.md §5).
//   Merges:
//     EXACT: the non-power-of-two bins (1025..1536, 2049..3072) always ride in the launch of the
//     power-of-two bin above them: the exact kernel's LDS chain buffers allow two workgroups per
//     CU at 3/6 waves as at 4/8, so the smaller workgroup only loses latency hiding, and a
//     separate launch adds a tail.
//     Small calls (a market shard, kMergeRounds): a launch whose markets would fill fewer than
//     kMergeRounds rounds of its resident grid costs a ramp and a tail for little work, so FAST
//     merges the non-power-of-two bins the same way and the 65..512 bins run as one 1-wave
//     launch -- fewer, fuller launches for a 1/8 shard of C3.
//   Order: longest bins first, except that the 2049..3072 bin precedes the 3073..4096 one: its
//   6-wave workgroups leave 4 of a CU's 16 wave slots free (two per CU at 128 VGPRs), which the
//   side stream's short-market kernels then fill (C3 fast -1.3%,
//   profiles/archive/r03x/order_ab.txt) -- and every main-stream launch that fills fewer than
//   kMergeRounds rounds of its resident grid (a shard's cut piece of a bin) moves behind the
//   full ones.  A small launch first ends while the side stream still holds CUs, and the big
//   persistent launch behind it, whose workgroups stride statically over its markets, then
//   starts part of its grid late and drags a tail (a planned C3 shard: 0.226 vs 0.15 ms for the
//   same bin-11 markets, profiles/r06c/).  Ordering every launch by estimated work instead cost
//   the full C3 batch 2% (1.325 vs 1.298 ms, profiles/r06e/).  The side bins come last; empty
//   launches are dropped.
//
// bin_start NULL -- bce_consensus_planned_device, the counts are on the device: the full
// batch's structure.  EXACT runs the non-power-of-two bins in the launch of the bin above, FAST
// gives every bin its own launch (no small-call merges), longest bins first, bins 0..3 on the
// side stream, always forked; no launch for bin 12 (markets longer than 4096 are not computed).
template <class Resident>
PlanSchedule plan_schedule(const int64_t* bin_start, int32_t mode, Resident&& resident) {
  static const int kClassic[BCE_NBINS] = {12, 10, 11, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0};
  const bool dev = bin_start == nullptr;
  auto cnt = [&](int b0, int b1) { return bin_start[b1 + 1] - bin_start[b0]; };
  auto few = [&](int b0, int b1) {
    return !dev && cnt(b0, b1) > 0 && (double)cnt(b0, b1) < kMergeRounds * (double)resident(b1);
  };
  int lo[BCE_NBINS];  // bin b's launch takes bins lo[b]..b
  for (int b = 0; b < BCE_NBINS; ++b) lo[b] = b;
  for (int b : {kBinNp2Lo + 1, kBinNp2Hi + 1})
    if (mode == BCE_MODE_EXACT || few(b - 1, b)) lo[b] = b - 1;
  if (few(kPlanSideLast + 1, kPlanSideLast + 3)) lo[kPlanSideLast + 3] = kPlanSideLast + 1;  // 65..512 as one
  // when bin b's launch is issued: 0 with the full main-stream launches, 1 with the small
  // ones, 2 with the side bins; -1: none (merged into the launch of the bin above, or empty)
  int pass[BCE_NBINS] = {};
  for (int b = 0; b < BCE_NBINS; ++b)
    for (int k = lo[b]; k < b; ++k) pass[k] = -1;
  for (int b : kClassic) {
    if (pass[b] < 0) continue;
    if (dev ? b == BCE_NBINS - 1 : cnt(lo[b], b) == 0) pass[b] = -1;
    else if (b <= kPlanSideLast) pass[b] = 2;
    else if (b < BCE_NBINS - 1 && few(lo[b], b)) pass[b] = 1;
  }
  PlanSchedule s;
  for (int p = 0; p < 3; ++p)
    for (int b : kClassic)
      if (pass[b] == p) s.launch[s.n++] = {lo[b], b, b <= kPlanSideLast};
  s.fork = dev || (cnt(0, kPlanSideLast) > 0 && cnt(kPlanSideLast + 1, BCE_NBINS - 1) > 0);
  return s;
}

}  // namespace bce
