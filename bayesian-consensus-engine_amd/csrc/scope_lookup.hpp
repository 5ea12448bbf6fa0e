// scope_lookup.hpp -- the building blocks of the scoped-reliability lookups, once: what
// pair_resolve_kernel (pair_scope.hip), scope_resolve_kernel (domain_scope.hip), walk_read_kernel
// (walk_forward.hip) and namespace_resolve_kernel (elementwise.hip) do per entry, and the half of
// the argument block that bce_pair_resolve and bce_scope_resolve share.
#pragma once
#include "bce_device.hpp"
#include "bce_internal.hpp"
#include "consensus_common.hpp"
#include "decay_device.hpp"

#pragma clang fp contract(off)

namespace bce {

// One scope table: dense over the S ranks (bce_namespace_resolve, the dense scopes of
// bce_pair_resolve) or the rows of a sparse pair / domain table.
struct NsScope {
  const double* rel;
  const double* conf;
  const int64_t* t_us;
  const uint8_t* has;
};

// The exp table in LDS (see replay_step_kernel); workgroups of 256 threads.
__device__ __forceinline__ void stage_exp_table(unsigned long long (&sExp)[256]) {
  sExp[threadIdx.x] = kExpTab[threadIdx.x];
  __syncthreads();
}

// Whole waves walk 64 consecutive entries from `base` (the workgroup's first), so the present bits
// of a wave are one ballot: two 32-bit words of the ceil(n / 32) the table has.
__device__ __forceinline__ void store_present_bits(uint32_t* bits, int64_t base, int64_t n, bool pred) {
  const unsigned long long w = __ballot(pred);
  const int ln = (int)(threadIdx.x & 63);
  const int64_t w0 = (base + (threadIdx.x & ~63)) >> 5;
  const int64_t nw = (n + 31) >> 5;
  if (ln < 2 && w0 + ln < nw) bits[w0 + ln] = (uint32_t)(w >> (32 * ln));
}

// Lower bound of s in ids[lo, hi) (strictly ascending); hit = ids[lower bound] == s.  Binary: a
// 4-ary search (three independent probes per step, the match decided by the last step's loads) was
// measured and did not pay (measurements/pair_scope_4ary_search.txt).  A domain
// segment is long (up to S rows), but the lanes of a wave are consecutive entries of mostly one
// market, so their first probes are the same words.
__device__ __forceinline__ int64_t sorted_lower_bound(const int32_t* __restrict__ ids, int64_t lo, int64_t hi,
                                                      int32_t s, bool& hit) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ids[mid] < s) lo = mid + 1; else hi = mid;
  }
  hit = lo < end && ids[lo] == s;
  return lo;
}

// [o0, o1) is a segment of a table of n rows: the pair does not decrease and stays in [0, n].
__device__ __forceinline__ bool is_segment(int64_t o0, int64_t o1, int64_t n) {
  return o0 >= 0 && o1 >= o0 && o1 <= n;
}

// The same, and where it is none an empty segment inside the table in its place.
__device__ __forceinline__ bool clamp_segment(int64_t& o0, int64_t& o1, int64_t n) {
  if (is_segment(o0, o1, n)) return true;
  o0 = o0 < 0 ? 0 : (o0 > n ? n : o0);
  o1 = o0;
  return false;
}

__device__ __forceinline__ int64_t clamp_market(int64_t m, int64_t M, int& code) {
  if (m < 0 || m >= M) {
    code = kFaultOffsets;
    m = m < 0 ? 0 : M - 1;
  }
  return m;
}

// The first fault code of an entry wins.
__device__ __forceinline__ int32_t clamp_sid(int32_t s, int32_t S, int& code) {
  if (s < 0 || s >= S) {
    code = code ? code : kFaultSid;
    s = s < 0 ? 0 : S - 1;
  }
  return s;
}

// The market of entry e: emarket[e], or the last m with qoffsets[m] <= e; clamped into [0, M).
__device__ __forceinline__ int64_t entry_market(const int32_t* __restrict__ emarket,
                                                const int64_t* __restrict__ qoffsets, int64_t M, int64_t e,
                                                int& code) {
  int64_t m;
  if (emarket) {
    m = emarket[e];
  } else {
    int64_t lo = 0, hi = M;  // qoffsets[lo] <= e is assumed for lo = 0
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (qoffsets[mid] <= e) lo = mid; else hi = mid;
    }
    m = lo;
  }
  m = clamp_market(m, M, code);
  if (e < qoffsets[m] || e >= qoffsets[m + 1]) code = kFaultOffsets;  // not this market's entry
  return m;
}

// Row `at` of the picked scope, decayed by its own t_us; no scope: r and c keep the cold start.
__device__ __forceinline__ void read_scope(const NsScope* pick, int64_t at, int apply_decay, const DecayConst& k,
                                           const unsigned long long* sExp, double& r, double& c) {
  if (!pick) return;
  r = pick->rel[at];
  c = pick->conf[at];
  if (apply_decay) r = decayed(r, pick->t_us[at], k, sExp);
}

// What bce_pair_resolve and bce_scope_resolve both take: the queries, the market table, the
// global scope, the decay and the per-entry outputs.  Leading base of PairArgs and ScopeArgs.
struct LookupArgs {
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
  NsScope glob;             // [S] dense, rel == NULL: not requested
  int apply_decay;
  int mark_cold;
  DecayConst k;
  int64_t* lb;
  uint8_t* matched;
  double2* relconf;
  uint32_t* bits;
  uint8_t* scope;
  int* fault;
};

// Fills it after the one check that is the last of both entries; `who` prefixes the message.
inline int fill_lookup_args(const char* who, LookupArgs& a, const int64_t* qoffsets, int64_t n_markets,
                            const int32_t* qsid, const int32_t* emarket, int64_t n_queries,
                            const int64_t* poffsets, const int32_t* psid, const NsScope& row, int64_t n_rows,
                            int32_t n_sources, const NsScope& glob, int apply_decay, int mark_cold,
                            const DecayConst& k, int64_t* lb, uint8_t* matched, double* relconf,
                            uint32_t* present_bits, uint8_t* scope) {
  BCE_REQUIRE(relconf == nullptr || (uintptr_t)relconf % 16 == 0, "%s: relconf must be 16-byte aligned", who);
  a = LookupArgs{qoffsets, n_markets, qsid, emarket, n_queries, poffsets, psid, row, n_rows, n_sources, glob,
                 apply_decay, mark_cold, k, lb, matched, reinterpret_cast<double2*>(relconf), present_bits, scope,
                 fault_word()};
  return BCE_OK;
}

// The capped grid of both lookups: 8192 workgroups (32 per CU) of 256, striding like
// namespace_resolve_kernel.
constexpr int kLookupGridCap = 8192;
inline dim3 lookup_grid(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return dim3((unsigned)(g < kLookupGridCap ? g : kLookupGridCap));
}

}  // namespace bce
