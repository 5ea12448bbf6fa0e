// consensus_history.hip -- the consensus of every market after each of its signals arrived:
// point k of market m (stored at CSR position offsets[m] + k) is core.compute_consensus
// (core.py:63-180) of the market's first k + 1 signals, the online use of the reference's Market
// (market.py: add_signal, then compute_consensus, then add_signal again).  Four values per point:
// consensus, confidence (0.0 where the reference returns None), total_weight, n_unique.
//
// The n prefixes of a market share the sort, the table gather and the memory traffic; they do not
// share arithmetic, because a source that sorts in front of the others changes every rounding
// behind it: each prefix is its own ordered sum (core.py:107-144).  So a market is sorted ONCE by
// (sid, arrival position), staged in LDS with its gathered {reliability, confidence} rows, and
// every point walks the sorted elements, skipping those that arrived after it.
//
//  history_short_kernel<G>  n <= G in {8, 16, 32, 64}: G lanes per market (64 / G markets per
//                           wave), lane k owns point k.  Keys are unique, so the sort is a rank
//                           by counting over LDS.  In each step of the walk the lanes of a market
//                           read one LDS address (a broadcast).
//  history_long_kernel      65 <= n <= 4096: one workgroup per market, the (sid, position)
//                           bitonic sort of consensus_long_kernel in LDS (32 B per signal: 128 KiB
//                           at 4096), thread t takes points t, t + blockDim, ...
//
// The work is QUADRATIC in the market length by construction: n points of n steps each, 16.8M
// steps for a 4096-signal market, spread over the workgroup.  Markets longer than 4096 signals
// are left untouched and raise kFaultTooLong.  A sid outside [0, n_sources) has its row read
// clamped and raises kFaultSid.  Keys are 64 bits wide ((sid << 32) | position): any table size.
// No floating-point atomics; every output element has exactly one writer.
#include "consensus_common.hpp"
#include "consensus_history.hpp"
#include "plan_host.hpp"

#pragma clang fp contract(off)

namespace bce {
namespace {

constexpr int kHistElemBytes = 32;  // LDS per signal of the long kernel: key, probability, row

// Point k of a market of n signals sorted by (sid, position): key[e] = (sid << 32) | position,
// prob[e] and row[e] the probability and the table row of sorted element e.  The elements with
// position <= k are the point's signals, added per source in arrival order (core.py:115-116); a
// source's run closes behind its last sorted element (for every point at the same e), then the
// ordered sums over the sources (core.py:120,136,142).  The sorted elements come from LDS kHistChunk
// at a time, read unconditionally ahead of the steps that use them: one LDS round trip per chunk
// instead of three dependent ones per step.
constexpr int kHistChunk = 4;
__device__ __forceinline__ void history_point(const ConsArgs& a, int64_t at, const unsigned long long* key,
                                              const double* prob, const double2* row, int n, unsigned k) {
  constexpr int C = kHistChunk;
  double total = 0.0, ws = 0.0, cs = 0.0, s = 0.0;
  int cnt = 0, j = 0;
  for (int e0 = 0; e0 < n; e0 += C) {
    unsigned long long kk[C + 1];  // kk[c + 1]: the element behind e0 + c (past the end: no sid)
    double pp[C];
    double2 rr[C];
#pragma unroll
    for (int c = 0; c <= C; ++c) {
      const unsigned long long v = key[e0 + c < n ? e0 + c : n - 1];
      kk[c] = e0 + c < n ? v : kSent64;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int e = e0 + c < n ? e0 + c : n - 1;
      pp[c] = prob[e];
      rr[c] = row[e];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (e0 + c < n) {
        if ((unsigned)kk[c] <= k) {
          s += pp[c];
          ++cnt;
        }
        if ((unsigned)(kk[c + 1] >> 32) != (unsigned)(kk[c] >> 32)) {  // the last of its source's run
          // core.py:116; s / 1 == s, so the wave divides only where one of its points saw the source twice
          double avg = s;
          if (ballot(cnt > 1)) avg = cnt > 1 ? s / (double)cnt : s;
          if (cnt > 0) {
            total += rr[c].x;       // core.py:119-120
            ws += avg * rr[c].x;    // core.py:136
            cs += rr[c].y * rr[c].x;  // core.py:142
            ++j;
            s = 0.0;
            cnt = 0;
          }
        }
      }
    }
  }
  store_market(a, at, total, ws, cs, j);
}

// ------------------------------------------------------------------------------------
// short markets: G lanes per market
// ------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(64) void history_short_kernel(ConsArgs a) {
  dev_range(a);
  static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lanes per market");
  constexpr int SPR = kWave / G;  // markets per wave and round
  __shared__ unsigned sRaw[kWave];
  __shared__ unsigned long long sKey[kWave];
  __shared__ double sProb[kWave];
  __shared__ double2 sRow[kWave];

  const int lane = lane_id();
  const int t = lane & (G - 1);
  const int base = lane - t;  // the market's first LDS slot
  const int64_t n_rounds = (a.n_list + SPR - 1) / SPR;
  bool badsid = false;
  for (int64_t r = blockIdx.x; r < n_rounds; r += gridDim.x) {
    const int64_t li = r * SPR + lane / G;
    int64_t off = 0;
    int n = 0;
    if (li < a.n_list) {
      const int64_t m = a.list ? a.list[li] : li;
      off = a.offsets[m];
      const int64_t len = a.offsets[m + 1] - off;
      if (len < 0 || len > G) {  // longer than the launch's bound: report, leave untouched
        if (a.fault) atomicCAS(a.fault, 0, kFaultTooLong);
      } else {
        n = (int)len;
      }
    }
    const bool valid = t < n;
    unsigned s = 0;
    double p = 0.0;
    double2 rc = make_double2(0.0, 0.0);
    if (valid) {
      s = hist_row(a.sid[off + t], a.n_sources, badsid);
      p = a.prob[off + t];
      rc = hist_gather(a, s);  // core.py:110-112 (cold-start defaults are baked into the table)
    }
    sRaw[lane] = s;
    wave_sync_lds();
    // rank among the market's unique (sid, position) keys
    int rank = 0;
#pragma unroll
    for (int q = 0; q < G; ++q) {  // no short circuit: every read is issued before the first compare
      const unsigned sq = sRaw[base + q];
      rank += (int)((q < n) & ((sq < s) | ((sq == s) & (q < t))));
    }
    if (valid) {
      sKey[base + rank] = ((unsigned long long)s << 32) | (unsigned)t;
      sProb[base + rank] = p;
      sRow[base + rank] = rc;
    }
    wave_sync_lds();
    if (valid) history_point(a, off + t, sKey + base, sProb + base, sRow + base, n, (unsigned)t);
    wave_sync_lds();  // the next round overwrites the slots
  }
  if (ballot(badsid)) raise_fault(a.fault, kFaultSid);
}

// ------------------------------------------------------------------------------------
// long markets: workgroup per market, P = LDS capacity in signals (a power of two)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHistMaxThreads) void history_long_kernel(ConsArgs a, int P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hist_lds[];
  double2* const row = reinterpret_cast<double2*>(hist_lds);
  unsigned long long* const key = reinterpret_cast<unsigned long long*>(hist_lds + 16 * (size_t)P);
  double* const prob = reinterpret_cast<double*>(hist_lds + 24 * (size_t)P);
  const int tid = threadIdx.x, NT = blockDim.x;

  // a device-resident plan: its last bin holds the markets longer than 4096, which get no launch
  if (a.dev_bins && blockIdx.x == 0 && tid == 0 && a.dev_bins[BCE_NBINS] > a.dev_bins[BCE_NBINS - 1] && a.fault)
    atomicCAS(a.fault, 0, kFaultTooLong);
  dev_range(a);
  bool badsid = false;
  for (int64_t li = blockIdx.x; li < a.n_list; li += gridDim.x) {
    const int64_t m = a.list ? a.list[li] : li;
    const int64_t off = a.offsets[m];
    const int64_t len = a.offsets[m + 1] - off;
    if (len < 0 || len > P) {  // uniform over the workgroup
      if (tid == 0 && a.fault) atomicCAS(a.fault, 0, kFaultTooLong);
      continue;
    }
    const int n = (int)len;
    if (n == 0) continue;
    int Pm = 64;  // this market's padded size
    while (Pm < n) Pm <<= 1;

    // ---- keys in arrival order --------------------------------------------------------
    for (int i = tid; i < Pm; i += NT)
      key[i] = i < n ? ((unsigned long long)hist_row(a.sid[off + i], a.n_sources, badsid) << 32) | (unsigned)i
                     : kSent64;
    __syncthreads();
    // ---- bitonic sort: ascending sid, then arrival position (core.py:103,115) -----------
    for (int k = 2; k <= Pm; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int c = tid; c < (Pm >> 1); c += NT) {
          const int lo = ((c & ~(j - 1)) << 1) | (c & (j - 1));
          const int hi = lo | j;
          const bool up = (lo & k) == 0;
          const unsigned long long x = key[lo], y = key[hi];
          if ((x > y) == up) {
            key[lo] = y;
            key[hi] = x;
          }
        }
        __syncthreads();
      }
    }
    // ---- probabilities and table rows in sorted order -----------------------------------
    for (int e = tid; e < n; e += NT) {
      const unsigned long long ke = key[e];
      prob[e] = a.prob[off + (unsigned)ke];
      row[e] = hist_gather(a, (unsigned)(ke >> 32));  // core.py:110-112
    }
    __syncthreads();
    // ---- the points ------------------------------------------------------------------------
    for (int k = tid; k < n; k += NT) history_point(a, off + k, key, prob, row, n, (unsigned)k);
    __syncthreads();  // the next market overwrites the LDS
  }
  if (ballot(badsid)) raise_fault(a.fault, kFaultSid);
}

int launch_hist_short(int max_len, const ConsArgs& a, hipStream_t st) {
  const int G = max_len <= 8 ? 8 : max_len <= 16 ? 16 : max_len <= 32 ? 32 : 64;
  const int64_t rounds = ceil_div(a.n_list, kWave / G);
  switch (G) {
    case 8: return launch_persistent(history_short_kernel<8>, 64, 8, rounds, "history_short_kernel<8>", a, st);
    case 16: return launch_persistent(history_short_kernel<16>, 64, 8, rounds, "history_short_kernel<16>", a, st);
    case 32: return launch_persistent(history_short_kernel<32>, 64, 8, rounds, "history_short_kernel<32>", a, st);
    default: return launch_persistent(history_short_kernel<64>, 64, 8, rounds, "history_short_kernel<64>", a, st);
  }
}

int launch_hist_long(int64_t max_len, const ConsArgs& a, hipStream_t st) {
  if (a.n_list == 0) return BCE_OK;
  int64_t P = next_pow2(max_len < 64 ? 64 : max_len);
  if (P > kLongMaxLds) P = kLongMaxLds;
  const int threads = (int)(P < kHistMaxThreads ? P : kHistMaxThreads);
  const size_t lds = (size_t)kHistElemBytes * (size_t)P;
  const void* fn = reinterpret_cast<const void*>(&history_long_kernel);
  const int rc = ensure_dynamic_lds(fn, kHistElemBytes * kLongMaxLds);
  if (rc) return rc;
  const int per_cu = blocks_per_cu(fn, threads, lds, 1, "history_long_kernel");
  const int64_t cap = (int64_t)cu_count() * per_cu;
  const int grid = (int)(a.n_list < cap ? a.n_list : cap);
  hipLaunchKernelGGL(history_long_kernel, dim3(grid), dim3(threads), lds, st, a, (int)P);
  return check_launch("history_long_kernel");
}

}  // namespace
}  // namespace bce

using namespace bce;

extern "C" int bce_consensus_history(const int64_t* offsets, int64_t n_markets, const int32_t* sid,
                                     const double* prob, int64_t n_signals, const double* relconf,
                                     const uint32_t* present_bits, int32_t n_sources, const int32_t* market_list,
                                     int64_t n_list, const int64_t* bin_start_host, const int64_t* bin_start_dev,
                                     int32_t max_len, double* consensus, double* confidence, double* total_weight,
                                     int32_t* n_unique, void* stream) {
  (void)present_bits;  // cold sources already carry their defaults in relconf
  BCE_REQUIRE(n_markets >= 0 && n_signals >= 0 && n_sources >= 0 && n_list >= 0, "history: negative size");
  BCE_REQUIRE(max_len >= 0 && max_len <= kLongMaxLds, "history: max_len %d outside [0, %d]", max_len, kLongMaxLds);
  BCE_REQUIRE(n_markets == 0 || offsets, "history: offsets is NULL");
  BCE_REQUIRE(n_signals == 0 || (sid && prob), "history: sid/prob NULL");
  BCE_REQUIRE(n_signals == 0 || (consensus && confidence && total_weight && n_unique),
              "history: per-point outputs must be non-NULL");
  BCE_REQUIRE(n_sources == 0 || relconf, "history: source table is NULL");
  BCE_REQUIRE((uintptr_t)relconf % 16 == 0, "history: relconf must be 16-byte aligned");
  BCE_REQUIRE(!(bin_start_host && bin_start_dev), "history: one plan, host or device bin boundaries");
  const bool planned = bin_start_host || bin_start_dev;
  BCE_REQUIRE(!planned || market_list || n_markets == 0, "history: a plan needs its market order");
  if (n_markets == 0 || n_signals == 0) return BCE_OK;
  ConsArgs base{};
  base.offsets = offsets; base.sid = sid; base.prob = prob;
  base.relconf = reinterpret_cast<const double2*>(relconf);
  base.n_sources = n_sources; base.n_signals = n_signals;
  base.consensus = consensus; base.confidence = confidence; base.total_weight = total_weight;
  base.n_unique = n_unique;
  base.fault = fault_word();
  hipStream_t st = as_stream(stream);
  if (!planned) {  // one launch sized by max_len (0: unknown, as 4096)
    base.list = market_list;
    base.n_list = market_list ? n_list : n_markets;
    if (base.n_list == 0) return BCE_OK;
    return (max_len > 0 && max_len <= 64) ? launch_hist_short(max_len, base, st)
                                          : launch_hist_long(max_len > 0 ? max_len : kLongMaxLds, base, st);
  }
  // a length-binned plan: one launch per bin, longest bins first; the > 4096 bin runs in the
  // 4096 launch, which reports its markets and leaves them untouched
  int rc = BCE_OK;
  for (int b = BCE_NBINS - 1; b >= 0 && !rc; --b) {
    if (bin_start_dev && b == BCE_NBINS - 1) continue;  // reported by the long launches
    ConsArgs a = base;
    if (bin_start_host) {
      a.list = market_list + bin_start_host[b];
      a.n_list = bin_start_host[b + 1] - bin_start_host[b];
      if (a.n_list == 0) continue;
    } else {
      a.list = market_list;    // the whole plan order: the range is read on the device
      a.n_list = n_markets;    // upper bound: sizes the grid
      a.dev_bins = bin_start_dev;
      a.dev_b0 = a.dev_b1 = b;
    }
    const int64_t bound = b < BCE_NBINS - 1 ? kBinMax[b] : kLongMaxLds;
    rc = b <= kPlanSideLast ? launch_hist_short((int)bound, a, st) : launch_hist_long(bound, a, st);
  }
  return rc;
}
