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
#include "bce_device.hpp"
#include "bce_internal.hpp"
#include "consensus_common.hpp"
#include "decay_device.hpp"

#pragma clang fp contract(off)

namespace bce {

struct PairArgs {
  int mode;
  const int64_t* qoffsets;  // [M + 1]
  int64_t M;
  const int32_t* qsid;      // [Q]
  const int32_t* emarket;   // [Q], nullable: search qoffsets
  int64_t Q;
  const int64_t* poffsets;  // [M + 1]
  const int32_t* psid;      // [P]
  NsScope row;              // [P] the market-scope rows
  int64_t P;
  int32_t S;
  NsScope dom, glob;        // [S] dense scopes, rel == NULL: not requested
  int apply_decay;
  int mark_cold;
  DecayConst k;
  int64_t* lb;
  uint8_t* matched;
  double2* relconf;
  uint32_t* bits;
  uint8_t* scope;
  double* orel;
  double* oconf;
  int64_t* ot;
  uint8_t* opresent;
  int* fault;
};

constexpr int kPairGridCap = 8192;  // workgroups (32 per CU), striding like namespace_resolve_kernel

// Lower bound of s in psid[lo, hi) (strictly ascending); hit = psid[lower bound] == s.  Binary: a
// 4-ary search (three independent probes per step, the match decided by the last step's loads) was
// measured and did not pay (measurements/pair_scope_4ary_search.txt).
__device__ __forceinline__ int64_t pair_lower_bound(const int32_t* __restrict__ psid, int64_t lo, int64_t hi,
                                                    int32_t s, bool& hit) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (psid[mid] < s) lo = mid + 1; else hi = mid;
  }
  hit = lo < end && psid[lo] == s;
  return lo;
}

__global__ __launch_bounds__(256) void pair_resolve_kernel(PairArgs a) {
  __shared__ unsigned long long sExp[256];  // the exp table in LDS (see replay_step_kernel)
  sExp[threadIdx.x] = kExpTab[threadIdx.x];
  __syncthreads();
  const int64_t n = a.Q > a.M ? a.Q : a.M;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t e = base + threadIdx.x;
    int code = 0;
    // every market's two offset pairs are checked once, by the lane of that index
    if (e < a.M) {
      const int64_t q0 = a.qoffsets[e], q1 = a.qoffsets[e + 1];
      const int64_t p0 = a.poffsets[e], p1 = a.poffsets[e + 1];
      if (q0 < 0 || q1 < q0 || q1 > a.Q || p0 < 0 || p1 < p0 || p1 > a.P) code = kFaultOffsets;
    }
    const bool in = e < a.Q;
    double r = a.k.default_rel, c = a.k.default_conf;
    int64_t t = BCE_NO_TIMESTAMP;
    int sc = 3;  // cold start
    bool hit = false;
    if (in) {
      int64_t m;
      if (a.emarket) {
        m = a.emarket[e];
      } else {  // the last m with qoffsets[m] <= e
        int64_t lo = 0, hi = a.M;  // qoffsets[lo] <= e is assumed for lo = 0
        while (hi - lo > 1) {
          const int64_t mid = (lo + hi) >> 1;
          if (a.qoffsets[mid] <= e) lo = mid; else hi = mid;
        }
        m = lo;
      }
      if (m < 0 || m >= a.M) {
        code = kFaultOffsets;
        m = m < 0 ? 0 : a.M - 1;
      }
      if (e < a.qoffsets[m] || e >= a.qoffsets[m + 1]) code = kFaultOffsets;  // not this market's entry
      int64_t p0 = a.poffsets[m], p1 = a.poffsets[m + 1];
      if (p0 < 0 || p1 < p0 || p1 > a.P) {  // not a segment of the table: searched as empty
        code = kFaultOffsets;
        p0 = p0 < 0 ? 0 : (p0 > a.P ? a.P : p0);
        p1 = p0;
      }
      int32_t s = a.qsid[e];
      if (s < 0 || s >= a.S) {
        code = code ? code : kFaultSid;
        s = s < 0 ? 0 : a.S - 1;
      }
      const int64_t lo = pair_lower_bound(a.psid, p0, p1, s, hit);
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
        if (pick) {
          r = pick->rel[at];
          c = pick->conf[at];
          if (a.apply_decay) r = decayed(r, pick->t_us[at], a.k, sExp);
        }
        if (a.relconf) a.relconf[e] = make_double2(r, c);
        if (a.scope) a.scope[e] = (uint8_t)sc;
      }
    }
    if (a.bits && a.mode != BCE_PAIR_RAW) {
      const unsigned long long w = __ballot(in && (!a.mark_cold || sc != 3));
      const int ln = (int)(threadIdx.x & 63);
      const int64_t w0 = (base + (threadIdx.x & ~63)) >> 5;
      const int64_t nw = (a.Q + 31) >> 5;
      if (ln < 2 && w0 + ln < nw) a.bits[w0 + ln] = (uint32_t)(w >> (32 * ln));
    }
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
  BCE_REQUIRE(relconf == nullptr || (uintptr_t)relconf % 16 == 0, "pair_resolve: relconf must be 16-byte aligned");
  PairArgs a{};
  a.mode = mode;
  a.qoffsets = qoffsets;
  a.M = n_markets;
  a.qsid = qsid;
  a.emarket = emarket;
  a.Q = n_queries;
  a.poffsets = poffsets;
  a.psid = psid;
  a.row = NsScope{prel, pconf, pt_us, phas};
  a.P = n_rows;
  a.S = n_sources;
  a.dom = dense[0];
  a.glob = dense[1];
  a.apply_decay = apply_decay;
  a.mark_cold = mark_cold;
  a.k = DecayConst{now_us, half_life_days, min_rel, default_rel, default_conf};
  a.lb = lb;
  a.matched = matched;
  a.relconf = reinterpret_cast<double2*>(relconf);
  a.bits = present_bits;
  a.scope = scope;
  a.orel = out_rel;
  a.oconf = out_conf;
  a.ot = out_t_us;
  a.opresent = out_present;
  a.fault = fault_word();
  const int64_t n = n_queries > n_markets ? n_queries : n_markets;
  const int64_t g = (n + 255) / 256;
  hipLaunchKernelGGL(pair_resolve_kernel, dim3((unsigned)(g < kPairGridCap ? g : kPairGridCap)), dim3(256), 0,
                     as_stream(stream), a);
  return check_launch("pair_resolve_kernel");
}
