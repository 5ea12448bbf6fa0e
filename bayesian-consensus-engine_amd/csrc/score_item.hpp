// score_item.hpp -- what bce_score_groups and bce_score_bootstrap share (include/bce.h, DESIGN
// §4.20 / §4.24): the item rule (class and per-item terms), the cut of a group into segments and
// the checked item range of a segment.  One copy, so the two entry points cannot drift apart.
#pragma once
#include "bce_device.hpp"
#include "bce_internal.hpp"
#include "consensus_common.hpp"

#pragma clang fp contract(off)

namespace bce {

constexpr int kScoreT = 256;
constexpr int kScoreSeg = BCE_SCORE_SEG;

enum { kScScored = 0, kScHit = 1, kScUnresolved = 2, kScNull = 3, kScBad = 4 };

// The segments a group of `len` items is cut into (an empty group keeps one, which writes zeros).
__host__ __device__ inline int64_t score_segments(int64_t len) {
  return len <= 0 ? 1 : (len + kScoreSeg - 1) / kScoreSeg;
}

// The items [*i0, *i1) of segment `seg` (empty on any fault).  Returns the fault code: the
// segment table is no partition (the row is zeros), or the group's offsets decrease or leave
// [0, n_items] (the group reads as empty).
__device__ __forceinline__ int score_segment_items(const int64_t* goff, int64_t G, const int64_t* seg_start,
                                                   const int64_t* seg_group, int64_t n_items, int64_t seg,
                                                   int64_t* i0, int64_t* i1) {
  *i0 = *i1 = 0;
  const int64_t g = seg_group[seg];  // one load: a search of seg_start costs ~20 dependent ones
  int64_t j = -1;
  if (g >= 0 && g < G && seg < seg_start[g + 1]) j = seg - seg_start[g];
  if (j < 0) return kFaultOffsets;
  const int64_t b = goff[g], e = goff[g + 1];
  if (b < 0 || e < b || e > n_items) return kFaultOffsets;
  if (j < score_segments(e - b)) {
    *i0 = b + j * kScoreSeg;
    *i1 = *i0 + kScoreSeg < e ? *i0 + kScoreSeg : e;
  }
  return 0;
}

// The class of an item whose indices are inside their arrays: the first rule that applies.
__device__ __forceinline__ int score_class(double v, int o, int ok, bool has_base, double bs) {
  if (o < 0) return kScUnresolved;
  if (!ok) return kScNull;
  if (!(v >= 0.0 && v <= 1.0) || (has_base && !(bs >= 0.0 && bs <= 1.0))) return kScBad;
  return kScScored;
}

struct ScoreTerms {
  double brier, logloss, brier_base;
  bool hit;
};

// The terms of a scored item: difference, then product (no contraction); brier_base 0.0 without
// a base.
__device__ __forceinline__ ScoreTerms score_terms(double v, int o, bool has_base, double bs, double eps) {
  ScoreTerms t;
  const double od = (double)o;
  const double d = v - od;
  t.brier = d * d;
  const double q = o ? v : 1.0 - v;
  t.logloss = -log(q < eps ? eps : q);
  t.brier_base = 0.0;
  if (has_base) {
    const double db = bs - od;
    t.brier_base = db * db;
  }
  t.hit = (v >= 0.5) == (o == 1);  // market.py:298-301
  return t;
}

}  // namespace bce
