// domain_scope.hip -- the namespaced lookup of a batch whose markets belong to different domains.
//
// NamespacedReliabilityStore.get_reliability(sid, market_id=m, domain=domain_of(m), apply_decay)
// (reliability_abstraction.py:119-188) for every unique (market, source) pair of a batch in one
// launch: the pair's market row, else the row of the source in the MARKET'S domain, else the
// global row, else the cold start.  A domain's rows are sparse like a market's, so the domain
// table has the pair table's layout with the domain index in the place of the market
// (doffsets / dsid ascending inside a domain); market_domain[m] names the domain of market m,
// -1 = none (a falsy domain, :150).  bce_pair_resolve takes one dense domain for the whole batch;
// this entry stands beside it and leaves it alone.
//
//   scope_resolve_kernel  one lane per query entry, as pair_resolve_kernel: the entry's market,
//                         a binary search in the market's row segment, a second one in the
//                         segment of the market's domain, the first scope whose row has a truthy
//                         updated_at, decayed by its own t_us.  Present bits from one ballot.
#include "scope_lookup.hpp"

#pragma clang fp contract(off)

namespace bce {

struct ScopeArgs : LookupArgs {  // poffsets == NULL: no market scope (market_id=None)
  const int32_t* mdom;      // [M] domain index of every market, -1: none
  const int64_t* doffsets;  // [D + 1]
  int64_t D;
  const int32_t* dsid;      // [R]
  NsScope drow;             // [R] the domain-scope rows
  int64_t R;
  int64_t* dlb;
  uint8_t* dmatched;
};

__global__ __launch_bounds__(256) void scope_resolve_kernel(ScopeArgs a) {
  __shared__ unsigned long long sExp[256];
  stage_exp_table(sExp);
  int64_t n = a.Q > a.M ? a.Q : a.M;
  n = n > a.D ? n : a.D;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t e = base + threadIdx.x;
    int code = 0;
    // every market's offset pairs and domain index, and every domain's offset pair, are checked
    // once, by the lane of that index
    if (e < a.M) {
      if (!is_segment(a.qoffsets[e], a.qoffsets[e + 1], a.Q)) code = kFaultOffsets;
      if (a.poffsets && !is_segment(a.poffsets[e], a.poffsets[e + 1], a.P)) code = kFaultOffsets;
      const int64_t d = a.mdom[e];
      if (d < -1 || d >= a.D) code = kFaultOffsets;
    }
    if (e < a.D && !is_segment(a.doffsets[e], a.doffsets[e + 1], a.R)) code = kFaultOffsets;
    const bool in = e < a.Q;
    int sc = 3;  // cold start
    if (in) {
      const int64_t m = entry_market(a.emarket, a.qoffsets, a.M, e, code);
      const int32_t s = clamp_sid(a.qsid[e], a.S, code);
      // the market's row (absent table: market_id=None)
      bool hit = false;
      int64_t lo = 0;
      if (a.poffsets) {
        int64_t p0 = a.poffsets[m], p1 = a.poffsets[m + 1];
        if (!clamp_segment(p0, p1, a.P)) code = kFaultOffsets;  // searched as empty
        lo = sorted_lower_bound(a.psid, p0, p1, s, hit);
      }
      if (a.lb) a.lb[e] = lo;
      if (a.matched) a.matched[e] = hit ? 1 : 0;
      // the row of the market's domain
      bool dhit = false;
      int64_t dlo = 0;
      int64_t d = a.mdom[m];
      if (d < -1 || d >= a.D) {  // no such domain: the market has none
        code = kFaultOffsets;
        d = -1;
      }
      if (d >= 0) {
        int64_t d0 = a.doffsets[d], d1 = a.doffsets[d + 1];
        if (!clamp_segment(d0, d1, a.R)) code = kFaultOffsets;  // searched as empty
        dlo = sorted_lower_bound(a.dsid, d0, d1, s, dhit);
      }
      if (a.dlb) a.dlb[e] = dlo;
      if (a.dmatched) a.dmatched[e] = dhit ? 1 : 0;
      // the first scope whose row has a truthy updated_at
      const NsScope* pick = nullptr;
      int64_t at = 0;
      if (hit && a.row.has[lo]) {
        pick = &a.row;
        at = lo;
        sc = 0;
      } else if (dhit && a.drow.has[dlo]) {
        pick = &a.drow;
        at = dlo;
        sc = 1;
      } else if (a.glob.rel && a.glob.has[s]) {
        pick = &a.glob;
        at = s;
        sc = 2;
      }
      double r = a.k.default_rel, c = a.k.default_conf;
      read_scope(pick, at, a.apply_decay, a.k, sExp, r, c);
      if (a.relconf) a.relconf[e] = make_double2(r, c);
      if (a.scope) a.scope[e] = (uint8_t)sc;
    }
    if (a.bits) store_present_bits(a.bits, base, a.Q, in && (!a.mark_cold || sc != 3));
    if (code && a.fault) atomicCAS(a.fault, 0, code);
  }
}

}  // namespace bce

using namespace bce;

extern "C" int bce_scope_resolve(const int64_t* qoffsets, int64_t n_markets, const int32_t* qsid,
                                 const int32_t* emarket, int64_t n_queries, const int64_t* poffsets,
                                 const int32_t* psid, const double* prel, const double* pconf,
                                 const int64_t* pt_us, const uint8_t* phas, int64_t n_rows,
                                 const int32_t* market_domain, const int64_t* doffsets, int64_t n_domains,
                                 const int32_t* dsid, const double* drel, const double* dconf,
                                 const int64_t* dt_us, const uint8_t* dhas, int64_t n_drows, int32_t n_sources,
                                 const double* grel, const double* gconf, const int64_t* gt_us,
                                 const uint8_t* ghas, int apply_decay, int64_t now_us, double half_life_days,
                                 double min_rel, double default_rel, double default_conf, int mark_cold,
                                 int64_t* lb, uint8_t* matched, int64_t* dlb, uint8_t* dmatched, double* relconf,
                                 uint32_t* present_bits, uint8_t* scope, void* stream) {
  BCE_REQUIRE(n_markets >= 0 && n_queries >= 0 && n_rows >= 0 && n_domains >= 0 && n_drows >= 0 && n_sources > 0,
              "scope_resolve: bad shape");
  BCE_REQUIRE(n_markets < (1ll << 31) && n_domains < (1ll << 31), "scope_resolve: n_markets / n_domains >= 2^31");
  BCE_REQUIRE(n_markets > 0 || (n_queries == 0 && n_rows == 0), "scope_resolve: entries or rows without markets");
  BCE_REQUIRE(n_domains > 0 || n_drows == 0, "scope_resolve: rows without domains");
  if (n_markets == 0) return BCE_OK;
  BCE_REQUIRE(qoffsets && market_domain, "scope_resolve: NULL qoffsets / market_domain");
  BCE_REQUIRE(n_queries == 0 || qsid, "scope_resolve: NULL qsid");
  BCE_REQUIRE(poffsets || n_rows == 0, "scope_resolve: market rows without poffsets");
  if (n_rows > 0) {
    BCE_REQUIRE(psid && prel && pconf && phas, "scope_resolve: NULL market table array");
    BCE_REQUIRE(pt_us || !apply_decay, "scope_resolve: the market table needs t_us");
  }
  BCE_REQUIRE(doffsets || n_domains == 0, "scope_resolve: NULL doffsets");
  if (n_drows > 0) {
    BCE_REQUIRE(dsid && drel && dconf && dhas, "scope_resolve: NULL domain table array");
    BCE_REQUIRE(dt_us || !apply_decay, "scope_resolve: the domain table needs t_us");
  }
  if (grel) {
    BCE_REQUIRE(gconf && ghas && (gt_us || !apply_decay), "scope_resolve: global scope: NULL array");
  }
  ScopeArgs a{};
  const int rc = fill_lookup_args("scope_resolve", a, qoffsets, n_markets, qsid, emarket, n_queries, poffsets, psid,
                                  {prel, pconf, pt_us, phas}, n_rows, n_sources, {grel, gconf, gt_us, ghas},
                                  apply_decay, mark_cold, {now_us, half_life_days, min_rel, default_rel, default_conf},
                                  lb, matched, relconf, present_bits, scope);
  if (rc != BCE_OK) return rc;
  a.mdom = market_domain;
  a.doffsets = doffsets;
  a.D = n_domains;
  a.dsid = dsid;
  a.drow = NsScope{drel, dconf, dt_us, dhas};
  a.R = n_drows;
  a.dlb = dlb;
  a.dmatched = dmatched;
  const int64_t n = n_queries > n_markets ? n_queries : n_markets;
  hipLaunchKernelGGL(scope_resolve_kernel, lookup_grid(n > n_domains ? n : n_domains), dim3(256), 0,
                     as_stream(stream), a);
  return check_launch("scope_resolve_kernel");
}
