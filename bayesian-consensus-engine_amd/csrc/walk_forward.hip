// walk_forward.hip -- walk-forward consensus: every market of a chronological batch reads the
// reliability table as it stood after the markets before it were settled.
//
// The reference run online is, per market m: get_reliability(s, scope, apply_decay=True) for every
// source of m with the clock at the market's time (reliability.py:104-140, decay.py:90-145), then
// compute_consensus, then -- if m is resolved -- update_reliability for every signal of m
// (reliability.py:142-233), which stamps updated_at with that time.  The state a source is read in
// at market m is therefore a PREFIX state of its settlement chain (settle.hip): the state after
// the `qpos` bits that belong to earlier markets.  One query per unique (market, source) pair
// ("entry"), the queries of a source contiguous and ascending in qpos.
//
//   trace_chain_kernel  one lane per short chain of `order`: walks the chain as settle_chain_kernel
//                       does and stores {rel, conf} -- raw, not decayed -- into trace[qentry] at
//                       every query position it passes
//   trace_long_kernel   one lane per chunk of a long chain, the workers of settle_long_kernel.
//                       Every chain position is walked (WALK) by exactly one worker whose state is
//                       the true state there: worker 0 from the start row to the first sync point,
//                       worker j from its sync point (exactly 1.0 / 0.0) to the next.  The worker
//                       that applies bit k - 1 owns query k and stores it, once; no atomics, no
//                       communication.  Neither kernel writes the table.
//   walk_read_kernel    one lane per entry: the read side.  qlast >= 0: the traced state, stamped
//                       with the time of market qlast; qlast < 0 (no earlier bit, qpos == 0): the
//                       start row, or the cold defaults where none exists.  Decays to the entry's
//                       own market time and packs the consensus table over the entry index, the
//                       present bits from one ballot per wave as pair_resolve_kernel does.  With
//                       resolution lag the stamp is the market's resolve time and the read time
//                       its forecast time (bce_walk_read_lag); otherwise the two are one array.
//   walk_lag_queries_kernel  one lane per query: the query order of a batch with resolution lag,
//                       the visible prefix of the source's chain by bisection over the resolve
//                       times of its bits.
#include "reliability_update.hpp"
#include "scope_lookup.hpp"
#include "settle_walk.hpp"
#include "trace_walk.hpp"

#pragma clang fp contract(off)

namespace bce {

__global__ __launch_bounds__(64) void trace_chain_kernel(TraceArgs a) {
  const int64_t q = a.s.n_long + (int64_t)blockIdx.x * 64 + threadIdx.x;  // the long chains: trace_long_kernel
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
  trace_span<false>(a, b0, 0, b1 - b0, r, run, prev, cur);
  if (cur.qi < cur.qe) trace_fault(a);  // a query behind the chain's end
}

__global__ __launch_bounds__(64) void trace_long_kernel(TraceArgs a, const int64_t* __restrict__ chunk_start,
                                                        int64_t n_chunks, int64_t C) {
  const int64_t wk = (int64_t)blockIdx.x * 64 + threadIdx.x;
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
  if (j > 0) {  // the first run of kSyncRun equal bits that lies inside the home chunk
    const int64_t p = settle_span<false, true>(a.s.bits, b0, pos, home_end, r, run, prev);
    if (p < 0) return;    // none: the worker before walks through this chunk and owns its queries
    r = prev ? 1.0 : 0.0; // exact whatever came before
    pos = p + 1;          // bit p was applied by the worker before: query p + 1 is theirs
  }
  TraceCursor cur{0, 0, c, 0};
  if (!trace_queries(a, s, pos, cur)) return;
  trace_span<false>(a, b0, pos, home_end, r, run, prev, cur);  // the rest of the home chunk
  for (int64_t cb = home_end; cb < L; cb += C) {  // later chunks, until one has a sync run of its own
    const int64_t cend = cb + C < L ? cb + C : L;
    run = 0;  // a run counts from its chunk's first bit
    if (trace_span<true>(a, b0, cb, cend, r, run, prev, cur) >= 0) return;  // that chunk's worker goes on
  }
  if (cur.qi < cur.qe) trace_fault(a);  // the one worker that reaches the chain's end
}

struct WalkReadArgs {
  int64_t E;
  const int32_t* usid;     // [E] source of every entry
  const int32_t* emarket;  // [E]
  const int32_t* qlast;    // [E] market of the last bit before the entry, -1: none
  const double2* trace;    // [E]
  const int64_t* stamp;    // [M] the time a market's updates stamp updated_at with
  const int64_t* now;      // [M] the time a market is read at (the same array without resolution lag)
  int64_t M;
  const double* rel;       // [S] the start table
  const double* conf;
  const int64_t* t_us;
  const uint8_t* present;  // nullable: every row exists
  int32_t S;
  DecayConst k;            // now_us is set per entry
  int mark_cold;
  int clamped;             // the caller clamped a sid while building the entries
  double2* relconf;        // [E], may be `trace` itself
  uint32_t* bits;          // [ceil(E / 32)]
  uint8_t* exists;         // [E] nullable: a row existed at read time
  int* fault;
};

constexpr int kWalkGridCap = 8192;  // workgroups, striding like pair_resolve_kernel

__global__ __launch_bounds__(256) void walk_read_kernel(WalkReadArgs a) {
  __shared__ unsigned long long sExp[256];
  stage_exp_table(sExp);
  if (a.clamped && a.fault && blockIdx.x == 0 && threadIdx.x == 0) atomicCAS(a.fault, 0, kFaultSid);
  for (int64_t base = (int64_t)blockIdx.x * 256; base < a.E; base += (int64_t)gridDim.x * 256) {
    const int64_t e = base + threadIdx.x;
    const bool in = e < a.E;
    int code = 0;
    bool exists = false;
    if (in) {
      const int64_t m = clamp_market(a.emarket[e], a.M, code);
      const int32_t s = clamp_sid(a.usid[e], a.S, code);
      int64_t ql = a.qlast[e];
      if (ql < -1 || ql >= a.M) {  // not a market: read as "no earlier bit"
        code = kFaultOffsets;
        ql = -1;
      }
      double r = a.k.default_rel, c = a.k.default_conf;
      int64_t t = BCE_NO_TIMESTAMP;
      if (ql >= 0) {  // settled by an earlier market of the batch: updated_at is that market's time
        const double2 st = a.trace[e];
        r = st.x;
        c = st.y;
        t = a.stamp[ql];
        exists = true;
      } else if (a.present == nullptr || a.present[s]) {
        r = a.rel[s];
        c = a.conf[s];
        t = a.t_us[s];
        exists = true;
      }
      if (exists) {  // reliability.py:114-123; a missing row is the cold start, undecayed
        DecayConst k = a.k;
        k.now_us = a.now[m];
        r = decayed(r, t, k, sExp);
      }
      a.relconf[e] = make_double2(r, c);
      if (a.exists) a.exists[e] = exists ? 1 : 0;
    }
    store_present_bits(a.bits, base, a.E, in && (!a.mark_cold || exists));
    if (code && a.fault) atomicCAS(a.fault, 0, code);
  }
}

// Resolution lag: market j is read at forecast[j] and settles at resolve[j] >= forecast[j].  A
// source's chain holds its bits in (resolve time, market, position) order, and entry (j, s) sees
// the bits whose market m has (resolve[m], m) < (forecast[j], j): a prefix of the chain, found by
// bisection.  Without lag the prefix is "the markets before j" and the host counts it by a scan.
struct LagQueryArgs {
  int64_t Q;
  const int32_t* qentry;      // [Q] the entry a query answers
  const int32_t* usid;        // [E]
  const int32_t* emarket;     // [E]
  int64_t E;
  const int64_t* start;       // [S + 1] bit range of every source's chain
  int32_t S;
  const int32_t* bit_market;  // [n_bits] the market of every chain bit, in chain order
  int64_t n_bits;
  const int64_t* forecast;    // [M]
  const int64_t* resolve;     // [M] read for resolved markets only
  int64_t M;
  int64_t* qpos;              // [Q] by query, relative to the chain
  int32_t* qlast;             // [E] by entry: the market of bit qpos - 1, -1: none
  int64_t* slast;             // [S] the market of the chain's last bit, -1: none
  int* fault;
};

// The chain of source s as a range of bit_market; false where start is no range inside [0, n_bits].
__device__ __forceinline__ bool lag_chain(const LagQueryArgs& a, int32_t s, int64_t& b0, int64_t& b1) {
  b0 = a.start[s];
  b1 = a.start[s + 1];
  return b0 >= 0 && b1 >= b0 && b1 <= a.n_bits;
}

// One lane per query, then one lane per source; every load is bounds-checked first, and a query
// that meets bad input reads as "no earlier bit".  The position the bisection ends on has the
// last probe that held on its left and the last that failed on its right -- bit qpos - 1 satisfies
// the predicate and bit qpos does not, for any array -- so the neighbours need no second look;
// what can go wrong is a range or an index, and those raise the fault word.
__global__ __launch_bounds__(256) void walk_lag_queries_kernel(LagQueryArgs a) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t q = first; q < a.Q; q += stride) {
    const int64_t e = a.qentry[q];
    bool ok = e >= 0 && e < a.E;
    int64_t pos = 0, last = -1;
    if (ok) {
      const int64_t s = a.usid[e], j = a.emarket[e];
      int64_t b0 = 0, b1 = 0;
      ok = s >= 0 && s < a.S && j >= 0 && j < a.M && lag_chain(a, (int32_t)s, b0, b1);
      if (ok) {
        const int64_t tj = a.forecast[j];
        int64_t lo = b0, hi = b1;
        while (lo < hi) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          const int64_t m = a.bit_market[mid];
          if (m < 0 || m >= a.M) {
            ok = false;
            break;
          }
          const int64_t tm = a.resolve[m];
          if (tm < tj || (tm == tj && m < j)) {
            lo = mid + 1;
            last = m;  // the rightmost probe that held: bit lo - 1
          } else {
            hi = mid;
          }
        }
        pos = lo - b0;
      }
      if (!ok) {
        pos = 0;
        last = -1;
      }
      a.qlast[e] = (int32_t)last;
    }
    a.qpos[q] = pos;
    if (!ok && a.fault) atomicCAS(a.fault, 0, kFaultOffsets);
  }
  for (int64_t s = first; s < a.S; s += stride) {
    int64_t b0, b1, last = -1;
    bool ok = lag_chain(a, (int32_t)s, b0, b1);
    if (ok && b1 > b0) {
      last = a.bit_market[b1 - 1];
      if (last < 0 || last >= a.M) {
        ok = false;
        last = -1;
      }
    }
    a.slast[s] = last;
    if (!ok && a.fault) atomicCAS(a.fault, 0, kFaultOffsets);
  }
}

}  // namespace bce

using namespace bce;

extern "C" int bce_settle_trace(const uint64_t* bits, int64_t n_bits, const int64_t* start, const int32_t* order,
                                int64_t n_touched, int64_t n_long, const int64_t* chunk_start, int64_t n_chunks,
                                int64_t chunk_bits, int32_t n_sources, const double* rel, const double* conf,
                                const uint8_t* present, double default_rel, double default_conf,
                                const int64_t* qstart, const int64_t* qpos, const int32_t* qentry,
                                int64_t n_entries, double* trace, void* stream) {
  BCE_REQUIRE(n_bits >= 0 && n_touched >= 0 && n_sources > 0 && n_touched <= n_sources && n_entries >= 0,
              "settle_trace: bad shape");
  BCE_REQUIRE(n_entries < (1ll << 31), "settle_trace: n_entries >= 2^31");
  BCE_REQUIRE(n_long >= 0 && n_long <= n_touched && n_chunks >= 0, "settle_trace: bad long-chain split");
  if (n_touched == 0 || n_entries == 0) return BCE_OK;
  BCE_REQUIRE(bits && start && order && rel && conf, "settle_trace: NULL argument");
  BCE_REQUIRE(qstart && qpos && qentry && trace, "settle_trace: NULL query argument");
  BCE_REQUIRE((uintptr_t)trace % 16 == 0, "settle_trace: trace must be 16-byte aligned");
  if (n_long > 0) {
    BCE_REQUIRE(chunk_start, "settle_trace: long chains need chunk_start");
    BCE_REQUIRE(chunk_bits >= 64, "settle_trace: chunk_bits < 64");
    BCE_REQUIRE(n_chunks >= n_long, "settle_trace: fewer chunks than long chains");
  }
  const int64_t blocks = (n_touched - n_long + 63) / 64, lblocks = (n_chunks + 63) / 64;
  BCE_REQUIRE(blocks < (1ll << 31) && lblocks < (1ll << 31), "settle_trace: grid too large");
  TraceArgs a{};
  // the trace kernels only read the table: the shared argument block is settle's, which writes it
  a.s = SettleArgs{reinterpret_cast<const unsigned long long*>(bits), n_bits, start, order, n_touched, n_long,
                   n_sources, const_cast<double*>(rel), const_cast<double*>(conf), nullptr,
                   const_cast<uint8_t*>(present), 0, default_rel, default_conf, nullptr, fault_word()};
  a.qstart = qstart;
  a.qpos = qpos;
  a.qentry = qentry;
  a.E = n_entries;
  a.trace = reinterpret_cast<double2*>(trace);
  if (blocks > 0) {
    hipLaunchKernelGGL(trace_chain_kernel, dim3((unsigned)blocks), dim3(64), 0, as_stream(stream), a);
    const int rc = check_launch("trace_chain_kernel");
    if (rc != BCE_OK) return rc;
  }
  if (n_long == 0) return BCE_OK;
  hipLaunchKernelGGL(trace_long_kernel, dim3((unsigned)lblocks), dim3(64), 0, as_stream(stream), a, chunk_start,
                     n_chunks, chunk_bits);
  return check_launch("trace_long_kernel");
}

// bce_walk_read_lag holds the launch; bce_walk_read is the same with the two time arrays equal.
extern "C" int bce_walk_read_lag(int64_t n_entries, const int32_t* usid, const int32_t* emarket,
                                 const int32_t* qlast, const double* trace, const int64_t* stamp_time_us,
                                 const int64_t* now_time_us, int64_t n_markets, const double* rel,
                                 const double* conf, const int64_t* t_us, const uint8_t* present, int32_t n_sources,
                                 double half_life_days, double min_rel, double default_rel, double default_conf,
                                 int mark_cold, int sid_clamped, double* relconf, uint32_t* present_bits,
                                 uint8_t* exists, void* stream) {
  BCE_REQUIRE(n_entries >= 0 && n_markets >= 0 && n_sources > 0, "walk_read: bad shape");
  BCE_REQUIRE(n_entries < (1ll << 31) && n_markets < (1ll << 31), "walk_read: n_entries or n_markets >= 2^31");
  BCE_REQUIRE(n_markets > 0 || n_entries == 0, "walk_read: entries without markets");
  if (n_entries == 0 && !sid_clamped) return BCE_OK;
  BCE_REQUIRE(n_entries == 0 ||
                  (usid && emarket && qlast && trace && stamp_time_us && now_time_us && rel && conf && t_us),
              "walk_read: NULL argument");
  BCE_REQUIRE(n_entries == 0 || (relconf && present_bits), "walk_read: NULL output");
  BCE_REQUIRE((uintptr_t)relconf % 16 == 0 && (uintptr_t)trace % 16 == 0,
              "walk_read: trace and relconf must be 16-byte aligned");
  WalkReadArgs a{};
  a.E = n_entries;
  a.usid = usid;
  a.emarket = emarket;
  a.qlast = qlast;
  a.trace = reinterpret_cast<const double2*>(trace);
  a.stamp = stamp_time_us;
  a.now = now_time_us;
  a.M = n_markets;
  a.rel = rel;
  a.conf = conf;
  a.t_us = t_us;
  a.present = present;
  a.S = n_sources;
  a.k = DecayConst{0, half_life_days, min_rel, default_rel, default_conf};
  a.mark_cold = mark_cold;
  a.clamped = sid_clamped;
  a.relconf = reinterpret_cast<double2*>(relconf);
  a.bits = present_bits;
  a.exists = exists;
  a.fault = fault_word();
  const int64_t g = (n_entries + 255) / 256;
  hipLaunchKernelGGL(walk_read_kernel, dim3((unsigned)(g < 1 ? 1 : (g < kWalkGridCap ? g : kWalkGridCap))), dim3(256),
                     0, as_stream(stream), a);
  return check_launch("walk_read_kernel");
}

extern "C" int bce_walk_read(int64_t n_entries, const int32_t* usid, const int32_t* emarket, const int32_t* qlast,
                             const double* trace, const int64_t* market_time_us, int64_t n_markets,
                             const double* rel, const double* conf, const int64_t* t_us, const uint8_t* present,
                             int32_t n_sources, double half_life_days, double min_rel, double default_rel,
                             double default_conf, int mark_cold, int sid_clamped, double* relconf,
                             uint32_t* present_bits, uint8_t* exists, void* stream) {
  return bce_walk_read_lag(n_entries, usid, emarket, qlast, trace, market_time_us, market_time_us, n_markets, rel,
                           conf, t_us, present, n_sources, half_life_days, min_rel, default_rel, default_conf,
                           mark_cold, sid_clamped, relconf, present_bits, exists, stream);
}

extern "C" int bce_walk_lag_queries(int64_t n_queries, const int32_t* qentry, const int32_t* usid,
                                    const int32_t* emarket, int64_t n_entries, const int64_t* start,
                                    int32_t n_sources, const int32_t* bit_market, int64_t n_bits,
                                    const int64_t* forecast_time_us, const int64_t* resolve_time_us,
                                    int64_t n_markets, int64_t* qpos, int32_t* qlast, int64_t* slast, void* stream) {
  BCE_REQUIRE(n_queries >= 0 && n_entries >= 0 && n_bits >= 0 && n_markets >= 0 && n_sources > 0,
              "walk_lag_queries: bad shape");
  BCE_REQUIRE(n_entries < (1ll << 31) && n_markets < (1ll << 31), "walk_lag_queries: n_entries or n_markets >= 2^31");
  BCE_REQUIRE(n_queries <= n_entries, "walk_lag_queries: more queries than entries");
  BCE_REQUIRE(n_markets > 0 || (n_entries == 0 && n_bits == 0), "walk_lag_queries: entries or bits without markets");
  BCE_REQUIRE(start && slast, "walk_lag_queries: NULL start or slast");
  BCE_REQUIRE(n_bits == 0 || bit_market, "walk_lag_queries: NULL bit_market");
  BCE_REQUIRE(n_queries == 0 || (qentry && usid && emarket && forecast_time_us && resolve_time_us && qpos && qlast),
              "walk_lag_queries: NULL argument");
  LagQueryArgs a{n_queries, qentry, usid, emarket, n_entries, start, n_sources, bit_market, n_bits,
                 forecast_time_us, resolve_time_us, n_markets, qpos, qlast, slast, fault_word()};
  const int64_t lanes = n_queries > n_sources ? n_queries : (int64_t)n_sources;
  const int64_t g = (lanes + 255) / 256;
  hipLaunchKernelGGL(walk_lag_queries_kernel, dim3((unsigned)(g < kWalkGridCap ? g : kWalkGridCap)), dim3(256), 0,
                     as_stream(stream), a);
  return check_launch("walk_lag_queries_kernel");
}
