// trace_walk.hpp -- the traced chain walk: a source's settlement chain walked from its start row,
// the raw {rel, conf} stored at every query position it passes.  Shared by the walk-forward trace
// (walk_forward.hip) and the update-rule grid trace (trace_grid.hip) so it exists once.
#pragma once
#include "reliability_update.hpp"
#include "settle_walk.hpp"

#pragma clang fp contract(off)

namespace bce {

struct TraceArgs {
  SettleArgs s;           // the chains and the start table (read only; t_us / now_us / snap unused)
  const int64_t* qstart;  // [S + 1] query range of every source
  const int64_t* qpos;    // [E] chain position whose before-state the query reads, ascending per source
  const int32_t* qentry;  // [E] the entry a query answers
  int64_t E;
  double2* trace;         // [E] by entry
};

// A worker's place in its source's queries, and the confidence chain it advances between them.
struct TraceCursor {
  int64_t qi, qe;
  double c;    // confidence after cn steps
  int64_t cn;
};

__device__ __forceinline__ void trace_fault(const TraceArgs& a) {
  if (a.s.fault) atomicCAS(a.s.fault, 0, kFaultOffsets);
}

// The queries of source s behind chain position pos (qpos > pos: query pos itself belongs to the
// worker that applied bit pos - 1, query 0 to walk_read_kernel); false when qstart is not a range.
__device__ __forceinline__ bool trace_queries(const TraceArgs& a, int32_t s, int64_t pos, TraceCursor& cur) {
  const int64_t qs = a.qstart[s], qe = a.qstart[s + 1];
  if (qs < 0 || qe < qs || qe > a.E) {
    trace_fault(a);
    return false;
  }
  int64_t lo = qs, hi = qe;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a.qpos[mid] <= pos) lo = mid + 1; else hi = mid;
  }
  cur.qi = lo;
  cur.qe = qe;
  return true;
}

// Every query at chain position p: the state after p bits, one 16-byte store each.
__device__ __forceinline__ void trace_emit(const TraceArgs& a, int64_t p, double r, TraceCursor& cur) {
  while (cur.qi < cur.qe && a.qpos[cur.qi] == p) {
    if (cur.cn != p) {
      cur.c = settle_conf(cur.c, p - cur.cn);
      cur.cn = p;
    }
    const int32_t e = a.qentry[cur.qi];
    if (e < 0 || e >= a.E) trace_fault(a); else a.trace[e] = make_double2(r, cur.c);
    ++cur.qi;
  }
}

// settle_span<true, TRACK> over [p, pend) under `rule`, cut at the query positions in (p, pend],
// which are stored on the way.  TRACK: the position whose bit completed a sync run (the walk ends
// behind it, the query there stored), else -1.
template <bool TRACK, class Rule = FixedRule>
__device__ __forceinline__ int64_t trace_span(const TraceArgs& a, int64_t b0, int64_t p, int64_t pend, double& r,
                                              int& run, bool& prev, TraceCursor& cur, const Rule& rule = Rule{}) {
  while (p < pend) {
    int64_t stop = pend;
    if (cur.qi < cur.qe) {
      const int64_t k = a.qpos[cur.qi];
      if (k <= p) {  // not ascending, or negative: the query is not answered
        trace_fault(a);
        ++cur.qi;
        continue;
      }
      if (k < stop) stop = k;
    }
    const int64_t hit = settle_span<true, TRACK>(a.s.bits, b0, p, stop, r, run, prev, rule);
    if (TRACK && hit >= 0) {
      trace_emit(a, hit + 1, r, cur);
      return hit;
    }
    p = stop;
    trace_emit(a, p, r, cur);
  }
  return -1;
}

__device__ __forceinline__ void trace_start_row(const SettleArgs& a, int32_t s, double& r, double& c) {
  const bool pres = a.present ? a.present[s] != 0 : true;
  r = pres ? a.rel[s] : a.default_rel;  // reliability.py:133-140 cold start
  c = pres ? a.conf[s] : a.default_conf;
}

}  // namespace bce
