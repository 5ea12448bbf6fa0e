// trace_grid.hip -- the settlement trace of walk_forward.hip under a grid of update rules at once.
//
// The learning rate and the step cap of update_reliability (reliability.py:163-169) change every
// chain state, so a grid of K rules is K traces -- but all K walk the same correctness bits and
// meet the same queries; only the double a lane carries differs.  With Kp = K rounded up to a
// power of two (at most 64), a wave holds 64 / Kp chains (or chunks): lane c * Kp + k walks chain
// c under rule k, lanes with k >= K are idle (they load and store nothing).  The lanes of one
// chain read the same bit word and the same query at the same address -- one request -- and lane k
// stores {rel, conf} to trace[k * E + entry]: K traces [E] back to back, so slice k is exactly
// what bce_settle_trace writes and bce_walk_read_lag reads it unchanged.
//
//   trace_grid_chain_kernel  trace_chain_kernel per (chain, rule): the lanes of a chain run in
//                            lockstep, the short path has no data-dependent branch
//   trace_grid_long_kernel   trace_long_kernel per (chunk, rule), sync_run[k] in place of
//                            kSyncRun: the lanes of a chunk sync at different positions and
//                            diverge.  Per rule the worker argument of trace_long_kernel holds
//                            unchanged -- every query is stored once per rule.
//
// The confidence chain does not depend on the rule; every lane recomputes it (settle_conf).
// final (optional): {rel, conf} behind every touched source's whole chain, by the lane -- on the
// long path, the one worker -- that reaches the chain's end.
#include "trace_walk.hpp"

#pragma clang fp contract(off)

namespace bce {

struct GridArgs {
  TraceArgs t;              // t.trace: [K * E], rule-major
  const double* step;       // [K] delta = min(cap, rate) >= 0
  const int64_t* sync_run;  // [K] equal bits that pin r under delta, <= 0: none do
  int K;
  int kshift;               // log2(Kp)
  double2* final;           // nullable [K * S]
};

// Lane `lane` of the launch as (item, rule): the rule loaded, the trace moved to the rule's
// slice.  false: an idle lane, or a step that is no step (negative or NaN: the fault word).
__device__ __forceinline__ bool grid_lane(const GridArgs& g, int64_t lane, int64_t& item, int& k, TraceArgs& a,
                                          StepRule& rule) {
  k = (int)(lane & ((1ll << g.kshift) - 1));
  item = lane >> g.kshift;
  if (k >= g.K) return false;
  a = g.t;
  const double d = g.step[k];
  if (!(d >= 0.0)) {
    trace_fault(a);
    return false;
  }
  const int64_t sr = g.sync_run[k];
  rule.delta = d;
  rule.sync = sr >= 1 && sr < kNeverSync ? (int)sr : kNeverSync;
  a.trace += (int64_t)k * a.E;
  return true;
}

__device__ __forceinline__ void grid_final(const GridArgs& g, int k, int32_t s, double r, const TraceCursor& cur,
                                           int64_t L) {
  if (g.final) g.final[(int64_t)k * g.t.s.S + s] = make_double2(r, settle_conf(cur.c, L - cur.cn));
}

__global__ __launch_bounds__(64) void trace_grid_chain_kernel(GridArgs g) {
  int64_t item;
  int k;
  TraceArgs a;
  StepRule rule;
  if (!grid_lane(g, (int64_t)blockIdx.x * 64 + threadIdx.x, item, k, a, rule)) return;
  const int64_t q = a.s.n_long + item;  // the long chains: trace_grid_long_kernel
  if (q >= a.s.T) return;
  int32_t s;
  int64_t b0, b1;
  if (!settle_range(a.s, q, s, b0, b1)) return;
  double r, c;
  trace_start_row(a.s, s, r, c);
  TraceCursor cur{0, 0, c, 0};
  if (!trace_queries(a, s, 0, cur)) return;
  int run = 0;
  bool prev = false;
  trace_span<false>(a, b0, 0, b1 - b0, r, run, prev, cur, rule);
  if (cur.qi < cur.qe) trace_fault(a);  // a query behind the chain's end
  grid_final(g, k, s, r, cur, b1 - b0);
}

__global__ __launch_bounds__(64) void trace_grid_long_kernel(GridArgs g, const int64_t* __restrict__ chunk_start,
                                                             int64_t n_chunks, int64_t C) {
  int64_t wk;
  int k;
  TraceArgs a;
  StepRule rule;
  if (!grid_lane(g, (int64_t)blockIdx.x * 64 + threadIdx.x, wk, k, a, rule)) return;
  if (wk >= n_chunks) return;
  // the long source this chunk belongs to: the last q with chunk_start[q] <= wk
  int64_t lo = 0, hi = a.s.n_long;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (chunk_start[mid] <= wk) lo = mid; else hi = mid;
  }
  const int64_t q = lo, j = wk - chunk_start[q];
  int32_t s;
  int64_t b0, b1;
  if (j < 0 || !settle_range(a.s, q, s, b0, b1)) return;
  const int64_t L = b1 - b0;
  if (j > (L - 1) / C) return;  // more chunks than the chain has: nothing to do
  const int64_t home_end = (j + 1) * C < L ? (j + 1) * C : L;
  double r, c;
  trace_start_row(a.s, s, r, c);
  int run = 0;
  bool prev = false;
  int64_t pos = j * C;
  if (j > 0) {  // the first pinning run that lies inside the home chunk
    if (rule.sync > C) return;  // longer than a chunk: no run does, worker 0 walks the whole chain
    const int64_t p = settle_span<false, true>(a.s.bits, b0, pos, home_end, r, run, prev, rule);
    if (p < 0) return;    // none: the worker before walks through this chunk and owns its queries
    r = prev ? 1.0 : 0.0; // exact whatever came before
    pos = p + 1;          // bit p was applied by the worker before: query p + 1 is theirs
  }
  TraceCursor cur{0, 0, c, 0};
  if (!trace_queries(a, s, pos, cur)) return;
  trace_span<false>(a, b0, pos, home_end, r, run, prev, cur, rule);  // the rest of the home chunk
  for (int64_t cb = home_end; cb < L; cb += C) {  // later chunks, until one has a sync run of its own
    const int64_t cend = cb + C < L ? cb + C : L;
    run = 0;  // a run counts from its chunk's first bit
    if (trace_span<true>(a, b0, cb, cend, r, run, prev, cur, rule) >= 0) return;  // that chunk's worker goes on
  }
  if (cur.qi < cur.qe) trace_fault(a);  // the one worker that reaches the chain's end
  grid_final(g, k, s, r, cur, L);
}

}  // namespace bce

using namespace bce;

extern "C" int bce_settle_trace_grid(const uint64_t* bits, int64_t n_bits, const int64_t* start, const int32_t* order,
                                     int64_t n_touched, int64_t n_long, const int64_t* chunk_start, int64_t n_chunks,
                                     int64_t chunk_bits, int32_t n_sources, const double* rel, const double* conf,
                                     const uint8_t* present, double default_rel, double default_conf,
                                     const int64_t* qstart, const int64_t* qpos, const int32_t* qentry,
                                     int64_t n_entries, const double* step, const int64_t* sync_run, int32_t n_points,
                                     double* trace, double* final, void* stream) {
  BCE_REQUIRE(n_bits >= 0 && n_touched >= 0 && n_sources > 0 && n_touched <= n_sources && n_entries >= 0,
              "settle_trace_grid: bad shape");
  BCE_REQUIRE(n_entries < (1ll << 31), "settle_trace_grid: n_entries >= 2^31");
  BCE_REQUIRE(n_points >= 1 && n_points <= BCE_UPDATE_MAX_POINTS,
              "settle_trace_grid: n_points %d outside [1, %d]", (int)n_points, BCE_UPDATE_MAX_POINTS);
  BCE_REQUIRE(step && sync_run, "settle_trace_grid: NULL step or sync_run");
  BCE_REQUIRE(n_long >= 0 && n_long <= n_touched && n_chunks >= 0, "settle_trace_grid: bad long-chain split");
  if (n_touched == 0 || (n_entries == 0 && !final)) return BCE_OK;
  BCE_REQUIRE(bits && start && order && rel && conf, "settle_trace_grid: NULL argument");
  BCE_REQUIRE(qstart && (n_entries == 0 || (qpos && qentry && trace)), "settle_trace_grid: NULL query argument");
  BCE_REQUIRE((uintptr_t)trace % 16 == 0 && (uintptr_t)final % 16 == 0,
              "settle_trace_grid: trace and final must be 16-byte aligned");
  if (n_long > 0) {
    BCE_REQUIRE(chunk_start, "settle_trace_grid: long chains need chunk_start");
    BCE_REQUIRE(chunk_bits >= 64 && chunk_bits < (1ll << 31), "settle_trace_grid: chunk_bits outside [64, 2^31)");
    BCE_REQUIRE(n_chunks >= n_long, "settle_trace_grid: fewer chunks than long chains");
  }
  int kshift = 0;
  while ((1 << kshift) < n_points) ++kshift;
  const int64_t per = 64 >> kshift;  // chains (chunks) of a wave
  const int64_t blocks = (n_touched - n_long + per - 1) / per, lblocks = (n_chunks + per - 1) / per;
  BCE_REQUIRE(blocks < (1ll << 31) && lblocks < (1ll << 31), "settle_trace_grid: grid too large");
  GridArgs g{};
  // the trace kernels only read the table: the shared argument block is settle's, which writes it
  g.t.s = SettleArgs{reinterpret_cast<const unsigned long long*>(bits), n_bits, start, order, n_touched, n_long,
                     n_sources, const_cast<double*>(rel), const_cast<double*>(conf), nullptr,
                     const_cast<uint8_t*>(present), 0, default_rel, default_conf, nullptr, fault_word()};
  g.t.qstart = qstart;
  g.t.qpos = qpos;
  g.t.qentry = qentry;
  g.t.E = n_entries;
  g.t.trace = reinterpret_cast<double2*>(trace);
  g.step = step;
  g.sync_run = sync_run;
  g.K = n_points;
  g.kshift = kshift;
  g.final = reinterpret_cast<double2*>(final);
  if (blocks > 0) {
    hipLaunchKernelGGL(trace_grid_chain_kernel, dim3((unsigned)blocks), dim3(64), 0, as_stream(stream), g);
    const int rc = check_launch("trace_grid_chain_kernel");
    if (rc != BCE_OK) return rc;
  }
  if (n_long == 0) return BCE_OK;
  hipLaunchKernelGGL(trace_grid_long_kernel, dim3((unsigned)lblocks), dim3(64), 0, as_stream(stream), g, chunk_start,
                     n_chunks, chunk_bits);
  return check_launch("trace_grid_long_kernel");
}
