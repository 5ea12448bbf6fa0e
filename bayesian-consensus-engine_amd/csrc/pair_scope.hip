// pair_scope.hip -- market-scope reliability rows: the (source, market) rows of the store as a
// sparse table in HBM, looked up for every unique (market, source) pair of a batch.
//
// The reference keeps one row per (source_id, market_id) and reads it once per pair:
// MarketStore.compute_all_consensus -> get_reliability(sid, str(market.id), apply_decay=True)
// (market.py:200-221, reliability.py:104-140); NamespacedReliabilityStore.get_reliability with a
// market id tries that row first (reliability_abstraction.py:137-188); compute_update starts from
// it undecayed (reliability.py:161).  The table is CSR by market over the batch's market index
// (poffsets / psid ascending inside a market), the queries are the batch's unique pairs in the
// same layout (qoffsets / qsid: ReestimateCsrPlan's uoffsets / usid).
//
//   pair_resolve_kernel  one lane per query entry: its market from emarket (or a search of
//                        qoffsets), a binary search of its sid inside the market's row segment,
//                        then the mode's outputs.  Whole waves walk 64 consecutive entries, so
//                        the present bits come from one ballot (namespace_resolve_kernel).
#include "scope_lookup.hpp"

#pragma clang fp contract(off)

namespace bce {

struct PairArgs : LookupArgs {
  int mode;
  NsScope dom;  // [S] dense like glob, rel == NULL: not requested
  double* orel;
  double* oconf;
  int64_t* ot;
  uint8_t* opresent;
};

__global__ __launch_bounds__(256) void pair_resolve_kernel(PairArgs a) {
  __shared__ unsigned long long sExp[256];
  stage_exp_table(sExp);
  const int64_t n = a.Q > a.M ? a.Q : a.M;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t e = base + threadIdx.x;
    int code = 0;
    // every market's two offset pairs are checked once, by the lane of that index
    if (e < a.M && !(is_segment(a.qoffsets[e], a.qoffsets[e + 1], a.Q) &&
                     is_segment(a.poffsets[e], a.poffsets[e + 1], a.P)))
      code = kFaultOffsets;
    const bool in = e < a.Q;
    double r = a.k.default_rel, c = a.k.default_conf;
    int64_t t = BCE_NO_TIMESTAMP;
    int sc = 3;  // cold start
    bool hit = false;
    if (in) {
      const int64_t m = entry_market(a.emarket, a.qoffsets, a.M, e, code);
      int64_t p0 = a.poffsets[m], p1 = a.poffsets[m + 1];
      if (!clamp_segment(p0, p1, a.P)) code = kFaultOffsets;  // searched as empty
      const int32_t s = clamp_sid(a.qsid[e], a.S, code);
      const int64_t lo = sorted_lower_bound(a.psid, p0, p1, s, hit);
      if (a.lb) a.lb[e] = lo;
      if (a.matched) a.matched[e] = hit ? 1 : 0;
      if (a.mode == BCE_PAIR_RAW) {  // compute_update's start state (reliability.py:161)
        if (hit) {
          r = a.row.rel[lo];
          c = a.row.conf[lo];
          t = a.row.t_us[lo];
        }
        if (a.orel) a.orel[e] = r;
        if (a.oconf) a.oconf[e] = c;
        if (a.ot) a.ot[e] = t;
        if (a.opresent) a.opresent[e] = hit ? 1 : 0;
      } else {
        const NsScope* pick = nullptr;
        int64_t at = 0;
        if (a.mode == BCE_PAIR_STORE) {  // a row that exists, whatever its updated_at
          if (hit) {
            pick = &a.row;
            at = lo;
            sc = 0;
          }
        } else {  // the first scope whose row has a truthy updated_at
          if (hit && a.row.has[lo]) {
            pick = &a.row;
            at = lo;
            sc = 0;
          } else if (a.dom.rel && a.dom.has[s]) {
            pick = &a.dom;
            at = s;
            sc = 1;
          } else if (a.glob.rel && a.glob.has[s]) {
            pick = &a.glob;
            at = s;
            sc = 2;
          }
        }
        read_scope(pick, at, a.apply_decay, a.k, sExp, r, c);
        if (a.relconf) a.relconf[e] = make_double2(r, c);
        if (a.scope) a.scope[e] = (uint8_t)sc;
      }
    }
    if (a.bits && a.mode != BCE_PAIR_RAW) store_present_bits(a.bits, base, a.Q, in && (!a.mark_cold || sc != 3));
    if (code && a.fault) atomicCAS(a.fault, 0, code);
  }
}

}  // namespace bce

using namespace bce;

extern "C" int bce_pair_resolve(int32_t mode, const int64_t* qoffsets, int64_t n_markets, const int32_t* qsid,
                                const int32_t* emarket, int64_t n_queries, const int64_t* poffsets,
                                const int32_t* psid, const double* prel, const double* pconf,
                                const int64_t* pt_us, const uint8_t* phas, int64_t n_rows, int32_t n_sources,
                                const double* drel, const double* dconf, const int64_t* dt_us,
                                const uint8_t* dhas, const double* grel, const double* gconf,
                                const int64_t* gt_us, const uint8_t* ghas, int apply_decay, int64_t now_us,
                                double half_life_days, double min_rel, double default_rel, double default_conf,
                                int mark_cold, int64_t* lb, uint8_t* matched, double* relconf,
                                uint32_t* present_bits, uint8_t* scope, double* out_rel, double* out_conf,
                                int64_t* out_t_us, uint8_t* out_present, void* stream) {
  BCE_REQUIRE(mode == BCE_PAIR_STORE || mode == BCE_PAIR_NAMESPACED || mode == BCE_PAIR_RAW,
              "pair_resolve: unknown mode %d", (int)mode);
  BCE_REQUIRE(n_markets >= 0 && n_queries >= 0 && n_rows >= 0 && n_sources > 0, "pair_resolve: bad shape");
  BCE_REQUIRE(n_markets < (1ll << 31), "pair_resolve: n_markets >= 2^31");
  BCE_REQUIRE(n_markets > 0 || (n_queries == 0 && n_rows == 0), "pair_resolve: entries or rows without markets");
  if (n_markets == 0) return BCE_OK;
  BCE_REQUIRE(qoffsets && poffsets, "pair_resolve: NULL offsets");
  BCE_REQUIRE(n_queries == 0 || qsid, "pair_resolve: NULL qsid");
  if (n_rows > 0) {
    BCE_REQUIRE(psid && prel && pconf, "pair_resolve: NULL table array");
    BCE_REQUIRE(pt_us || (mode != BCE_PAIR_RAW && !apply_decay), "pair_resolve: the table needs t_us");
    BCE_REQUIRE(phas || mode != BCE_PAIR_NAMESPACED, "pair_resolve: the namespaced mode needs has");
  }
  const NsScope dense[2] = {{drel, dconf, dt_us, dhas}, {grel, gconf, gt_us, ghas}};
  for (int q = 0; q < 2; ++q) {
    if (dense[q].rel == nullptr) continue;  // scope not requested (falsy domain)
    BCE_REQUIRE(mode == BCE_PAIR_NAMESPACED, "pair_resolve: a dense scope needs BCE_PAIR_NAMESPACED");
    BCE_REQUIRE(dense[q].conf && dense[q].has && (dense[q].t_us || !apply_decay),
                "pair_resolve: dense scope %d: NULL array", q + 1);
  }
  PairArgs a{};
  const int rc = fill_lookup_args("pair_resolve", a, qoffsets, n_markets, qsid, emarket, n_queries, poffsets, psid,
                                  {prel, pconf, pt_us, phas}, n_rows, n_sources, dense[1], apply_decay, mark_cold,
                                  {now_us, half_life_days, min_rel, default_rel, default_conf}, lb, matched, relconf,
                                  present_bits, scope);
  if (rc != BCE_OK) return rc;
  a.mode = mode;
  a.dom = dense[0];
  a.orel = out_rel;
  a.oconf = out_conf;
  a.ot = out_t_us;
  a.opresent = out_present;
  hipLaunchKernelGGL(pair_resolve_kernel, lookup_grid(n_queries > n_markets ? n_queries : n_markets), dim3(256), 0,
                     as_stream(stream), a);
  return check_launch("pair_resolve_kernel");
}
