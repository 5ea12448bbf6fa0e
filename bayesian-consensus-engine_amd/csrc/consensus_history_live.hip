// consensus_history_live.hip -- the consensus history with the reliabilities re-read at every
// arrival: point k of market j (stored at CSR position offsets[j] + k) is core.compute_consensus
// of the market's first k + 1 signals with every source fetched by get_reliability(s, scope,
// apply_decay=True) with the clock at the point's own arrival time, after every market that
// resolved before that arrival was settled -- a Market used online while other markets resolve
// around it.
//
// The chains are compiled in (resolve time, market, position) order and every prefix state of
// every chain is traced once (bce_settle_trace_all: states[g] behind chain bit g).  Point i of
// market j sees bit b of source s iff (resolve[bit_market[b]], bit_market[b]) < (arrival[i], j)
// lexicographically; the visible bits are a prefix of the chain, found by bisection.  With pos
// visible bits the row is states[start[s] + pos - 1] stamped with the resolve time of that bit's
// market, else the start row with its t_us, else the cold defaults (undecayed); then decayed() to
// the arrival: walk_read_kernel's logic per (point, source) instead of per entry.  No per-(point,
// source) array exists in memory: a point reads a source's row where the source's sorted run
// closes with at least one of the point's signals in it, and uses it at once.
//
// The per-run window: arrivals do not decrease inside a market, so what any point of the market
// sees of a chain lies between what its first and its last arrival see.  At staging every sorted
// run bisects its chain twice, at those two times, and keeps [lo, hi] in LDS; a point bisects
// inside the window only.  A market's life is short beside a chain's, so the window is mostly
// empty and most reads cost no probe.  BCE_LIVE_WINDOW=0 compiles the kernels without it (every
// read bisects the whole chain): the measurement's other side, not a run-time switch.
//
//  live_short_kernel<G>  n <= G in {8, 16, 32, 64}: G lanes per market, lane k owns point k
//  live_long_kernel      65 <= n <= 4096: one workgroup per market, 32 B of LDS per signal (key,
//                        probability, window; no row is staged), thread t takes points t, t +
//                        blockDim, ...
//
// The front (claim, loads, rank by counting, or key fill and bitonic sort) is consensus_sorted.hpp's;
// the walk is history_point's (consensus_history.hip) with the staged row replaced by the live
// read.  Every index is checked before it is used, as walk_lag_queries_kernel does: a chain range
// outside [0, n_bits] or a bit_market outside [0, M) reads as "no visible bit" and raises
// kFaultOffsets; a sid outside [0, n_sources) is clamped and raises kFaultSid; a market over the
// launch's bound is left untouched and raises kFaultTooLong.  No floating-point atomics; every
// output element has exactly one writer.
#include "consensus_common.hpp"
#include "consensus_sorted.hpp"
#include "decay_device.hpp"

#pragma clang fp contract(off)

#ifndef BCE_LIVE_WINDOW
#define BCE_LIVE_WINDOW 1
#endif

namespace bce {
namespace {

constexpr bool kLiveWindow = BCE_LIVE_WINDOW != 0;
constexpr int kLiveElemBytes = kLiveWindow ? 32 : 16;  // LDS per signal of the long kernel: key, probability, window

struct LiveArgs {
  const int64_t* arrival;     // [N] arrival time of every signal
  const int64_t* start;       // [S + 1] bit range of every source's chain
  const int32_t* bit_market;  // [n_bits] the market of every chain bit, in chain order
  int64_t n_bits;
  const int64_t* resolve;     // [M] read for the markets of chain bits only
  int64_t M;
  const double2* states;      // [n_bits] {rel, conf} behind every chain bit
  const double* rel;          // [S] the start table
  const double* conf;
  const int64_t* t_us;
  const uint8_t* present;     // nullable: every row exists
  DecayConst k;               // now_us is set per read
};

// A range of absolute bit positions inside one chain; lo < 0: the chain is no range (reported).
struct LiveWindow {
  int64_t lo, hi;
};

__device__ __forceinline__ void stage_exp(unsigned long long* sExp, int tid, int NT) {
  for (int i = tid; i < 256; i += NT) sExp[i] = kExpTab[i];
}

// The whole chain of table row s as a window.
__device__ __forceinline__ LiveWindow live_chain(const LiveArgs& L, unsigned s, bool& badchain) {
  const int64_t b0 = L.start[s], b1 = L.start[s + 1];
  if (b0 >= 0 && b1 >= b0 && b1 <= L.n_bits) return LiveWindow{b0, b1};
  badchain = true;
  return LiveWindow{-1, -1};
}

// The first bit of [lo, hi) that (t, j) does not see, hi where it sees all; ok = false (and lo)
// where a probed bit names no market.
__device__ __forceinline__ int64_t live_visible(const LiveArgs& L, int64_t lo, int64_t hi, int64_t t, int64_t j,
                                                bool& ok) {
  const int64_t lo0 = lo;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int64_t m = L.bit_market[mid];
    if (m < 0 || m >= L.M) {
      ok = false;
      return lo0;
    }
    const int64_t tm = L.resolve[m];
    if (tm < t || (tm == t && m < j)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// What the points of market j, which arrive in [t_first, t_last], can see of the chain of row s.
__device__ __forceinline__ LiveWindow live_window(const LiveArgs& L, unsigned s, int64_t j, int64_t t_first,
                                                  int64_t t_last, bool& badchain) {
  LiveWindow w = live_chain(L, s, badchain);
  if (w.lo < 0) return w;
  bool ok = true;
  const int64_t lo = live_visible(L, w.lo, w.hi, t_first, j, ok);
  const int64_t hi = ok ? live_visible(L, lo, w.hi, t_last, j, ok) : lo;
  if (ok) return LiveWindow{lo, hi};
  badchain = true;
  return LiveWindow{-1, -1};
}

// get_reliability(s, scope, apply_decay=True) as point (t_arr, j) sees it; s is a table row and w
// a window of its chain that holds the end of what the point sees.
__device__ __forceinline__ double2 live_row(const LiveArgs& L, unsigned s, int64_t j, int64_t t_arr, LiveWindow w,
                                            const unsigned long long* sExp, bool& badchain) {
  int64_t last = -1, pos = 0;
  if (w.lo >= 0) {
    bool ok = true;
    pos = live_visible(L, w.lo, w.hi, t_arr, j, ok);
    if (ok && pos > L.start[s]) {  // the market of bit pos - 1 stamps the state
      last = L.bit_market[pos - 1];
      ok = last >= 0 && last < L.M;
    }
    if (!ok) {
      badchain = true;
      last = -1;
    }
  }
  double r = L.k.default_rel, c = L.k.default_conf;
  int64_t t = BCE_NO_TIMESTAMP;
  bool exists = false;
  if (last >= 0) {  // settled by a market that resolved before the arrival: updated_at is its resolve time
    const double2 st = L.states[pos - 1];
    r = st.x;
    c = st.y;
    t = L.resolve[last];
    exists = true;
  } else if (L.present == nullptr || L.present[s]) {
    r = L.rel[s];
    c = L.conf[s];
    t = L.t_us[s];
    exists = true;
  }
  if (exists) {  // reliability.py:114-123; a missing row is the cold start, undecayed
    DecayConst k = L.k;
    k.now_us = t_arr;
    r = decayed(r, t, k, sExp);
  }
  return make_double2(r, c);
}

// history_point (consensus_history.hip) with the row of a source read live where its run closes
// with cnt > 0: point k of market j of n signals sorted by (sid, position), at CSR position `at`;
// win[e] is the window of the run that closes at sorted element e (kLiveWindow).
constexpr int kLiveChunk = 4;
__device__ __forceinline__ void live_point(const ConsArgs& a, const LiveArgs& L, int64_t at, int64_t j,
                                           const unsigned long long* key, const double* prob, const LiveWindow* win,
                                           int n, unsigned k, const unsigned long long* sExp, bool& badchain) {
  constexpr int C = kLiveChunk;
  const int64_t t_arr = L.arrival[at];
  double total = 0.0, ws = 0.0, cs = 0.0, s = 0.0;
  int cnt = 0, u = 0;
  for (int e0 = 0; e0 < n; e0 += C) {
    unsigned long long kk[C + 1];  // kk[c + 1]: the element behind e0 + c (past the end: no sid)
    double pp[C];
#pragma unroll
    for (int c = 0; c <= C; ++c) {
      const unsigned long long v = key[e0 + c < n ? e0 + c : n - 1];
      kk[c] = e0 + c < n ? v : kSent64;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) pp[c] = prob[e0 + c < n ? e0 + c : n - 1];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (e0 + c < n) {
        if ((unsigned)kk[c] <= k) {
          s += pp[c];
          ++cnt;
        }
        if ((unsigned)(kk[c + 1] >> 32) != (unsigned)(kk[c] >> 32) && cnt > 0) {  // the last of its source's run
          const double avg = cnt > 1 ? s / (double)cnt : s;  // core.py:116; s / 1 == s
          const unsigned row = (unsigned)(kk[c] >> 32);
          const LiveWindow w = kLiveWindow ? win[e0 + c] : live_chain(L, row, badchain);
          const double2 rc = live_row(L, row, j, t_arr, w, sExp, badchain);
          total += rc.x;       // core.py:119-120
          ws += avg * rc.x;    // core.py:136
          cs += rc.y * rc.x;   // core.py:142
          ++u;
          s = 0.0;
          cnt = 0;
        }
      }
    }
  }
  store_market(a, at, total, ws, cs, u);
}

// ------------------------------------------------------------------------------------
// short markets: G lanes per market
// ------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(64) void live_short_kernel(ConsArgs a, LiveArgs L) {
  dev_range(a);
  static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lanes per market");
  constexpr int SPR = kWave / G;  // markets per wave and round
  __shared__ unsigned sRaw[kWave];
  __shared__ unsigned long long sKey[kWave];
  __shared__ double sProb[kWave];
  __shared__ LiveWindow sWin[kLiveWindow ? kWave : 1];
  __shared__ unsigned long long sExp[256];

  const int lane = lane_id();
  stage_exp(sExp, lane, kWave);
  const int t = lane & (G - 1);
  const int base = lane - t;  // the market's first LDS slot
  const int64_t n_rounds = (a.n_list + SPR - 1) / SPR;
  bool badsid = false, badchain = false;
  for (int64_t r = blockIdx.x; r < n_rounds; r += gridDim.x) {
    const ShortFront f = short_front<G>(a, r, lane, sRaw, badsid);
    if (f.valid) {
      sKey[base + f.rank] = ((unsigned long long)f.s << 32) | (unsigned)t;
      sProb[base + f.rank] = f.p;
    }
    wave_sync_lds();
    if (kLiveWindow) {
      if (f.valid) {  // lane t: the run that closes at sorted element t, if one does
        const unsigned row = (unsigned)(sKey[base + t] >> 32);
        if (t + 1 == f.n || (unsigned)(sKey[base + t + 1] >> 32) != row)
          sWin[base + t] = live_window(L, row, f.m, L.arrival[f.off], L.arrival[f.off + f.n - 1], badchain);
      }
      wave_sync_lds();
    }
    if (f.valid)
      live_point(a, L, f.off + t, f.m, sKey + base, sProb + base, sWin + (kLiveWindow ? base : 0), f.n, (unsigned)t,
                 sExp, badchain);
    wave_sync_lds();  // the next round overwrites the slots
  }
  if (ballot(badsid)) raise_fault(a.fault, kFaultSid);
  if (ballot(badchain)) raise_fault(a.fault, kFaultOffsets);
}

// ------------------------------------------------------------------------------------
// long markets: workgroup per market, P = LDS capacity in signals (a power of two)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHistMaxThreads) void live_long_kernel(ConsArgs a, LiveArgs L, int P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char live_lds[];
  __shared__ unsigned long long sExp[256];
  unsigned long long* const key = reinterpret_cast<unsigned long long*>(live_lds);
  double* const prob = reinterpret_cast<double*>(live_lds + 8 * (size_t)P);
  LiveWindow* const win = reinterpret_cast<LiveWindow*>(live_lds + 16 * (size_t)P);  // kLiveWindow
  const int tid = threadIdx.x, NT = blockDim.x;

  stage_exp(sExp, tid, NT);  // ordered before its first read by the barriers of the first market
  report_plan_too_long(a, tid);
  dev_range(a);
  bool badsid = false, badchain = false;
  for (int64_t li = blockIdx.x; li < a.n_list; li += gridDim.x) {
    int64_t m, off;
    int n;
    if (!claim_market(a, li, P, tid, m, off, n)) continue;
    if (n == 0) continue;
    // ---- keys in arrival order, sorted by sid, then arrival position ----------------------
    const int Pm = fill_keys(a, key, off, n, tid, NT, badsid, [](int) {});
    __syncthreads();
    block_bitonic_sort_u64(key, Pm, tid, NT);
    // ---- probabilities in sorted order, the window of every run ------------------------------
    const int64_t t_first = L.arrival[off], t_last = L.arrival[off + n - 1];
    for (int e = tid; e < n; e += NT) {
      const unsigned long long ke = key[e];
      prob[e] = a.prob[off + (unsigned)ke];
      if (kLiveWindow && (e + 1 == n || (unsigned)(key[e + 1] >> 32) != (unsigned)(ke >> 32)))
        win[e] = live_window(L, (unsigned)(ke >> 32), m, t_first, t_last, badchain);
    }
    __syncthreads();
    // ---- the points ------------------------------------------------------------------------
    for (int k = tid; k < n; k += NT) live_point(a, L, off + k, m, key, prob, win, n, (unsigned)k, sExp, badchain);
    __syncthreads();  // the next market overwrites the LDS
  }
  if (ballot(badsid)) raise_fault(a.fault, kFaultSid);
  if (ballot(badchain)) raise_fault(a.fault, kFaultOffsets);
}

int launch_live_short(int max_len, const ConsArgs& a, const LiveArgs& L, hipStream_t st) {
  const int G = max_len <= 8 ? 8 : max_len <= 16 ? 16 : max_len <= 32 ? 32 : 64;
  const int64_t rounds = ceil_div(a.n_list, kWave / G);
  switch (G) {
    case 8: return launch_persistent(live_short_kernel<8>, 64, 8, rounds, "live_short_kernel<8>", st, a, L);
    case 16: return launch_persistent(live_short_kernel<16>, 64, 8, rounds, "live_short_kernel<16>", st, a, L);
    case 32: return launch_persistent(live_short_kernel<32>, 64, 8, rounds, "live_short_kernel<32>", st, a, L);
    default: return launch_persistent(live_short_kernel<64>, 64, 8, rounds, "live_short_kernel<64>", st, a, L);
  }
}

}  // namespace
}  // namespace bce

using namespace bce;

extern "C" int bce_consensus_history_live(
    const int64_t* offsets, int64_t n_markets, const int32_t* sid, const double* prob, int64_t n_signals,
    const double* states, const uint32_t* present_bits, int32_t n_sources, const int32_t* market_list, int64_t n_list,
    const int64_t* bin_start_host, const int64_t* bin_start_dev, int32_t max_len, double* consensus,
    double* confidence, double* total_weight, int32_t* n_unique, const int64_t* arrival_us, const int64_t* start,
    const int32_t* bit_market, int64_t n_bits, const int64_t* resolve_time_us, const double* rel, const double* conf,
    const int64_t* t_us, const uint8_t* present, double half_life_days, double min_rel, double default_rel,
    double default_conf, void* stream) {
  (void)present_bits;  // a source without a row reads the cold defaults through `present`
  hipStream_t st = as_stream(stream);
  const bool nothing = n_markets == 0 || n_signals == 0;
  BCE_REQUIRE(n_bits >= 0, "history_live: negative size");
  if (!nothing) {
    BCE_REQUIRE(n_sources > 0, "history_live: n_sources must be positive");
    BCE_REQUIRE(arrival_us && start && rel && conf && t_us, "history_live: NULL argument");
    BCE_REQUIRE(n_bits == 0 || (bit_market && resolve_time_us && states), "history_live: NULL chain argument");
  }
  LiveArgs L{arrival_us, start, bit_market, n_bits, resolve_time_us, n_markets,
             reinterpret_cast<const double2*>(states), rel, conf, t_us, present,
             DecayConst{0, half_life_days, min_rel, default_rel, default_conf}};
  PerSignalCall c{offsets, n_markets, sid, prob, n_signals, states, n_sources, market_list, n_list,
                  bin_start_host, bin_start_dev, max_len, consensus, confidence, total_weight, n_unique};
  c.rows_optional = true;  // states is NULL where no chain has a bit
  return per_signal_launch(
      "history_live", "per-point", c, nothing,
      [&](int bound, const ConsArgs& a) { return launch_live_short(bound, a, L, st); },
      [&](int64_t bound, const ConsArgs& a) {
        return launch_market_block(live_long_kernel, kLiveElemBytes, bound, a.n_list, "live_long_kernel", st, a, L);
      });
}
