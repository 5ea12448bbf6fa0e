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
// This file holds what only the history does: history_point, the walk of one point, and what the
// two kernels stage for it.  The market claim, the loads and the rank of the short kernel, the
// claim, the key fill and the sort of the long one, the launchers and the body of the C entry are
// consensus_sorted.hpp's, shared with consensus_leave_one_out.hip.
//
// The work is QUADRATIC in the market length by construction: n points of n steps each, 16.8M
// steps for a 4096-signal market, spread over the workgroup.  Markets longer than 4096 signals
// are left untouched and raise kFaultTooLong.  A sid outside [0, n_sources) has its row read
// clamped and raises kFaultSid.  Keys are 64 bits wide ((sid << 32) | position): any table size.
// No floating-point atomics; every output element has exactly one writer.
#include "consensus_common.hpp"
#include "consensus_sorted.hpp"

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
    const ShortFront f = short_front<G>(a, r, lane, sRaw, badsid);
    if (f.valid) {
      sKey[base + f.rank] = ((unsigned long long)f.s << 32) | (unsigned)t;
      sProb[base + f.rank] = f.p;
      sRow[base + f.rank] = f.rc;
    }
    wave_sync_lds();
    if (f.valid) history_point(a, f.off + t, sKey + base, sProb + base, sRow + base, f.n, (unsigned)t);
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

  report_plan_too_long(a, tid);
  dev_range(a);
  bool badsid = false;
  for (int64_t li = blockIdx.x; li < a.n_list; li += gridDim.x) {
    int64_t m, off;
    int n;
    if (!claim_market(a, li, P, tid, m, off, n)) continue;
    if (n == 0) continue;
    // ---- keys in arrival order, sorted by sid, then arrival position ----------------------
    const int Pm = fill_keys(a, key, off, n, tid, NT, badsid, [](int) {});
    __syncthreads();
    block_bitonic_sort_u64(key, Pm, tid, NT);
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
  hipStream_t st = as_stream(stream);
  const PerSignalCall c{offsets, n_markets, sid, prob, n_signals, relconf, n_sources, market_list, n_list,
                        bin_start_host, bin_start_dev, max_len, consensus, confidence, total_weight, n_unique};
  return per_signal_launch(
      "history", "per-point", c, n_markets == 0 || n_signals == 0,
      [&](int bound, const ConsArgs& a) { return launch_hist_short(bound, a, st); },
      [&](int64_t bound, const ConsArgs& a) {
        return launch_market_block(history_long_kernel, kHistElemBytes, bound, a.n_list, "history_long_kernel", st, a);
      });
}
