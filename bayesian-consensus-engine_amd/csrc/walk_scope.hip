// walk_scope.hip -- the read side of the NAMESPACED walk-forward: every entry of a chronological
// batch is fetched as NamespacedReliabilityStore.get_reliability(s, market_id, domain,
// apply_decay=True) would fetch it at its market's turn (reliability_abstraction.py:119-188), after
// the resolved markets before it ran update_reliability(s, correct, domain=, update_global=)
// (:190-239) at domain and / or global scope.
//
// Two chain families are traced beforehand by bce_settle_trace (walk_forward.hip, unchanged), each
// into a buffer of its own over the entry index: the (domain, source) chains of a DomainPlan and
// the per-source global chains.  Market-scope rows are read only.  Whether a scope's row "exists"
// for the fallback is decided per read, as of the entry's turn: a chain that has a bit before the
// entry's market (qlast >= 0) was stamped by that market, so it exists whatever its start row was;
// otherwise the start row decides with its `has` flag (updated_at truthy).
//
//   walk_scope_read_kernel  one lane per entry: the market row (binary search of the sid in the
//                           market's segment), else the entry's domain chain, else its global chain,
//                           else the cold start; the picked state decayed from its own stamp to the
//                           entry's market time, packed as the consensus table over the entry index,
//                           the present bits from one ballot per wave as walk_read_kernel.  With
//                           resolution lag a traced state is stamped with the RESOLVE time of market
//                           qlast and the entry is read at its market's FORECAST time
//                           (bce_walk_scope_read_lag); otherwise the two are one array.
#include "scope_lookup.hpp"

#pragma clang fp contract(off)

namespace bce {

struct WalkScopeArgs {
  int64_t E;
  const int32_t* usid;      // [E] source of every entry
  const int32_t* emarket;   // [E]
  const int64_t* stamp;     // [M] the time a market's updates stamp updated_at with
  const int64_t* now;       // [M] the time a market is read at (the same array without resolution lag)
  int64_t M;
  int32_t S;
  const int64_t* poffsets;  // [M + 1] NULL: no market scope (market_id=None)
  const int32_t* psid;      // [P]
  NsScope prow;             // [P] the market-scope rows
  int64_t P;
  const int32_t* dentry;    // [E] the (domain, source) chain of every entry, -1: none; NULL: no domain scope
  const int32_t* dqlast;    // [E] market of the last domain bit before the entry, -1: none
  const double2* dtrace;    // [E]
  NsScope dstart;           // [F] the domain chains' start rows; has = updated_at truthy
  int64_t F;
  const int32_t* gqlast;    // [E] the same for the global chain; NULL: no global bit in the batch
  const double2* gtrace;    // [E]
  NsScope gstart;           // [S] the dense global start table, rel == NULL: scope not requested
  DecayConst k;             // now_us is set per entry
  int mark_cold;
  int clamped;              // the caller clamped a sid while building the entries
  double2* relconf;         // [E], may be dtrace or gtrace itself: a lane reads both before it stores
  uint32_t* bits;           // [ceil(E / 32)]
  uint8_t* scope;           // [E]
  int* fault;
};

// qlast of one family: a market of the batch, or -1; anything else reads as "no earlier bit".
__device__ __forceinline__ int64_t walk_scope_qlast(const int32_t* __restrict__ qlast, int64_t e, int64_t M,
                                                    int& code) {
  if (!qlast) return -1;
  const int64_t ql = qlast[e];
  if (ql < -1 || ql >= M) {
    code = kFaultOffsets;
    return -1;
  }
  return ql;
}

__global__ __launch_bounds__(256) void walk_scope_read_kernel(WalkScopeArgs a) {
  __shared__ unsigned long long sExp[256];
  stage_exp_table(sExp);
  if (a.clamped && a.fault && blockIdx.x == 0 && threadIdx.x == 0) atomicCAS(a.fault, 0, kFaultSid);
  for (int64_t base = (int64_t)blockIdx.x * 256; base < a.E; base += (int64_t)gridDim.x * 256) {
    const int64_t e = base + threadIdx.x;
    const bool in = e < a.E;
    int code = 0;
    int sc = 3;  // cold start
    if (in) {
      const int64_t m = clamp_market(a.emarket[e], a.M, code);
      const int32_t s = clamp_sid(a.usid[e], a.S, code);
      // the three per-entry indices are loaded (coalesced) and checked whichever scope answers
      int64_t f = a.dentry ? (int64_t)a.dentry[e] : -1;
      if (f < -1 || f >= a.F) {  // no such chain: the market has no domain
        code = kFaultOffsets;
        f = -1;
      }
      const int64_t dql = a.dentry ? walk_scope_qlast(a.dqlast, e, a.M, code) : -1;
      const int64_t gql = walk_scope_qlast(a.gqlast, e, a.M, code);
      double r = a.k.default_rel, c = a.k.default_conf;
      int64_t t = BCE_NO_TIMESTAMP;
      // 1. the market row: seeded per (source, market), never written during the walk
      if (a.poffsets) {
        int64_t p0 = a.poffsets[m], p1 = a.poffsets[m + 1];
        if (!clamp_segment(p0, p1, a.P)) code = kFaultOffsets;  // searched as empty
        bool hit = false;
        const int64_t lo = sorted_lower_bound(a.psid, p0, p1, s, hit);
        if (hit && a.prow.has[lo]) {
          r = a.prow.rel[lo];
          c = a.prow.conf[lo];
          t = a.prow.t_us[lo];
          sc = 0;
        }
      }
      // 2. the domain chain: stamped by an earlier market of the batch, else its start row
      if (sc == 3 && f >= 0) {
        if (dql >= 0) {
          const double2 st = a.dtrace[e];
          r = st.x;
          c = st.y;
          t = a.stamp[dql];
          sc = 1;
        } else if (a.dstart.has[f]) {
          r = a.dstart.rel[f];
          c = a.dstart.conf[f];
          t = a.dstart.t_us[f];
          sc = 1;
        }
      }
      // 3. the global chain, likewise
      if (sc == 3 && a.gstart.rel) {
        if (gql >= 0) {
          const double2 st = a.gtrace[e];
          r = st.x;
          c = st.y;
          t = a.stamp[gql];
          sc = 2;
        } else if (a.gstart.has[s]) {
          r = a.gstart.rel[s];
          c = a.gstart.conf[s];
          t = a.gstart.t_us[s];
          sc = 2;
        }
      }
      if (sc != 3) {  // 4. else the cold start, undecayed
        DecayConst k = a.k;
        k.now_us = a.now[m];
        r = decayed(r, t, k, sExp);
      }
      a.relconf[e] = make_double2(r, c);
      a.scope[e] = (uint8_t)sc;
    }
    store_present_bits(a.bits, base, a.E, in && (!a.mark_cold || sc != 3));
    if (code && a.fault) atomicCAS(a.fault, 0, code);
  }
}

}  // namespace bce

using namespace bce;

// bce_walk_scope_read_lag holds the launch; bce_walk_scope_read is the same with the two time arrays equal.
extern "C" int bce_walk_scope_read_lag(int64_t n_entries, const int32_t* usid, const int32_t* emarket,
                                       const int64_t* stamp_time_us, const int64_t* now_time_us, int64_t n_markets,
                                       int32_t n_sources, const int64_t* poffsets, const int32_t* psid,
                                       const double* prel, const double* pconf, const int64_t* pt_us,
                                       const uint8_t* phas, int64_t n_rows, const int32_t* dentry,
                                       const int32_t* dqlast, const double* dtrace, const double* drel,
                                       const double* dconf, const int64_t* dt_us, const uint8_t* dhas,
                                       int64_t n_dentries, const int32_t* gqlast, const double* gtrace,
                                       const double* grel, const double* gconf, const int64_t* gt_us,
                                       const uint8_t* ghas, double half_life_days, double min_rel, double default_rel,
                                       double default_conf, int mark_cold, int sid_clamped, double* relconf,
                                       uint32_t* present_bits, uint8_t* scope, void* stream) {
  BCE_REQUIRE(n_entries >= 0 && n_markets >= 0 && n_sources > 0 && n_rows >= 0 && n_dentries >= 0,
              "walk_scope_read: bad shape");
  BCE_REQUIRE(n_entries < (1ll << 31) && n_markets < (1ll << 31) && n_dentries < (1ll << 31),
              "walk_scope_read: n_entries, n_markets or n_dentries >= 2^31");
  BCE_REQUIRE(n_markets > 0 || n_entries == 0, "walk_scope_read: entries without markets");
  if (n_entries == 0 && !sid_clamped) return BCE_OK;
  BCE_REQUIRE(n_entries == 0 || (usid && emarket && stamp_time_us && now_time_us),
              "walk_scope_read: NULL argument");
  BCE_REQUIRE(n_entries == 0 || (relconf && present_bits && scope), "walk_scope_read: NULL output");
  BCE_REQUIRE(poffsets || n_rows == 0, "walk_scope_read: market rows without poffsets");
  if (n_rows > 0) {
    BCE_REQUIRE(psid && prel && pconf && pt_us && phas, "walk_scope_read: NULL market table array");
  }
  if (dentry) {
    BCE_REQUIRE(dqlast && dtrace, "walk_scope_read: the domain scope needs dqlast and dtrace");
    BCE_REQUIRE(n_dentries == 0 || (drel && dconf && dt_us && dhas), "walk_scope_read: NULL domain start row array");
  }
  if (grel) {
    BCE_REQUIRE(gconf && gt_us && ghas, "walk_scope_read: global scope: NULL array");
  }
  BCE_REQUIRE(gqlast == nullptr || (grel && gtrace), "walk_scope_read: gqlast needs the global table and gtrace");
  BCE_REQUIRE((uintptr_t)relconf % 16 == 0 && (uintptr_t)dtrace % 16 == 0 && (uintptr_t)gtrace % 16 == 0,
              "walk_scope_read: the traces and relconf must be 16-byte aligned");
  WalkScopeArgs a{};
  a.E = n_entries;
  a.usid = usid;
  a.emarket = emarket;
  a.stamp = stamp_time_us;
  a.now = now_time_us;
  a.M = n_markets;
  a.S = n_sources;
  a.poffsets = poffsets;
  a.psid = psid;
  a.prow = NsScope{prel, pconf, pt_us, phas};
  a.P = n_rows;
  a.dentry = dentry;
  a.dqlast = dqlast;
  a.dtrace = reinterpret_cast<const double2*>(dtrace);
  a.dstart = NsScope{drel, dconf, dt_us, dhas};
  a.F = n_dentries;
  a.gqlast = gqlast;
  a.gtrace = reinterpret_cast<const double2*>(gtrace);
  a.gstart = NsScope{grel, gconf, gt_us, ghas};
  a.k = DecayConst{0, half_life_days, min_rel, default_rel, default_conf};
  a.mark_cold = mark_cold;
  a.clamped = sid_clamped;
  a.relconf = reinterpret_cast<double2*>(relconf);
  a.bits = present_bits;
  a.scope = scope;
  a.fault = fault_word();
  const int64_t g = (n_entries + 255) / 256;
  hipLaunchKernelGGL(walk_scope_read_kernel, dim3((unsigned)(g < 1 ? 1 : (g < kLookupGridCap ? g : kLookupGridCap))),
                     dim3(256), 0, as_stream(stream), a);
  return check_launch("walk_scope_read_kernel");
}

extern "C" int bce_walk_scope_read(int64_t n_entries, const int32_t* usid, const int32_t* emarket,
                                   const int64_t* market_time_us, int64_t n_markets, int32_t n_sources,
                                   const int64_t* poffsets, const int32_t* psid, const double* prel,
                                   const double* pconf, const int64_t* pt_us, const uint8_t* phas, int64_t n_rows,
                                   const int32_t* dentry, const int32_t* dqlast, const double* dtrace,
                                   const double* drel, const double* dconf, const int64_t* dt_us,
                                   const uint8_t* dhas, int64_t n_dentries, const int32_t* gqlast,
                                   const double* gtrace, const double* grel, const double* gconf,
                                   const int64_t* gt_us, const uint8_t* ghas, double half_life_days, double min_rel,
                                   double default_rel, double default_conf, int mark_cold, int sid_clamped,
                                   double* relconf, uint32_t* present_bits, uint8_t* scope, void* stream) {
  return bce_walk_scope_read_lag(n_entries, usid, emarket, market_time_us, market_time_us, n_markets, n_sources,
                                 poffsets, psid, prel, pconf, pt_us, phas, n_rows, dentry, dqlast, dtrace, drel, dconf,
                                 dt_us, dhas, n_dentries, gqlast, gtrace, grel, gconf, gt_us, ghas, half_life_days,
                                 min_rel, default_rel, default_conf, mark_cold, sid_clamped, relconf, present_bits,
                                 scope, stream);
}
