// consensus_leave_one_out.hip -- every source's marginal effect on its market's consensus: the
// signal at CSR position p, of source x in market m, gets core.compute_consensus (core.py:63-180)
// of m's signals whose source is NOT x.  Four values per signal -- consensus, confidence (0.0
// where the reference returns None), total_weight, n_unique -- the same for all signals of one
// source in one market; and, when asked for, the market's own consensus per market (full_*).
//
// What the leave-outs of a market share: the sort by (sid, position), the table gather, and
// every source's closed run -- avg = s / cnt (core.py:116), w = rel, avg * w, conf * w
// (core.py:119,136,142) do not depend on which source is left out.  What they cannot share is
// the three ordered sums over the sources (core.py:120,136,142): dropping a source changes every
// rounding behind it.  So a market is sorted ONCE, its U unique sources are compacted into LDS as
// {w, avg * w, conf * w}, and leave-out j is the left-to-right sum of the three columns over the
// entries e != j: O(n + U^2) per market.  The walk that leaves out the LAST entry is the full
// sum's prefix: adding the last entry to it gives the market's own consensus, bit for bit.
//
//  loo_short_kernel<G>  n <= G in {8, 16, 32, 64}: G lanes per market (64 / G markets per wave),
//                       the history kernel's rank by counting; lane j walks leave-out j, lane t
//                       then copies the result of its signal's source to position t.
//  loo_long_kernel      65 <= n <= 4096: one workgroup per market, the (sid, position) bitonic
//                       sort in LDS, the leaders of the sorted runs close them and a block scan
//                       compacts them; thread t walks leave-outs t, t + blockDim, ... and writes
//                       the positions of its source's signals.
//
// This file holds what only the leave-outs do: loo_walk, the run closing and the compaction into
// {w, avg * w, conf * w}, and the copy of every leave-out to its source's signals.  The market
// claim, the loads and the rank of the short kernel, the claim, the key fill, the sort and the
// compact index of the long one, the launchers and the body of the C entry are
// consensus_sorted.hpp's, shared with consensus_history.hip.
//
// Markets longer than 4096 signals (or than a max_len <= 64 launch takes) are left untouched and
// raise kFaultTooLong; a sid outside [0, n_sources) has its row read clamped and raises
// kFaultSid.  No floating-point atomics; every output element has exactly one writer.
#include "consensus_common.hpp"
#include "consensus_sorted.hpp"

#pragma clang fp contract(off)

namespace bce {
namespace {

// The market's own consensus, one row per market: all four NULL, or all four set.
struct LooFull {
  double* consensus;
  double* confidence;
  double* total_weight;
  int32_t* n_unique;
};

constexpr int kLooElemBytes = 36;  // LDS per signal of the long kernel (loo_long_kernel)

// Leave-out j of a market's U compact entries: the ordered sums (core.py:120,136,142) over the
// entries e != j.  The entries come from LDS kLooChunk at a time, read unconditionally ahead of
// the steps that use them (every lane of a market reads one address: a broadcast).
constexpr int kLooChunk = 4;
__device__ __forceinline__ void loo_walk(const double* W, const double* AW, const double* CW, int U, int j,
                                         double& total, double& ws, double& cs) {
  constexpr int C = kLooChunk;
  total = ws = cs = 0.0;
  for (int e0 = 0; e0 < U; e0 += C) {
    double w[C], x[C], c[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const int e = e0 + i < U ? e0 + i : U - 1;
      w[i] = W[e];
      x[i] = AW[e];
      c[i] = CW[e];
    }
#pragma unroll
    for (int i = 0; i < C; ++i) {
      if (e0 + i < U && e0 + i != j) {
        total += w[i];
        ws += x[i];
        cs += c[i];
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// short markets: G lanes per market
// ------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(64) void loo_short_kernel(ConsArgs a, LooFull f) {
  dev_range(a);
  static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lanes per market");
  constexpr int SPR = kWave / G;  // markets per wave and round
  constexpr unsigned long long kGroup = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
  __shared__ unsigned sRaw[kWave];  // sids in arrival order
  __shared__ unsigned sSid[kWave];  // ... and sorted by (sid, position), with probability and row
  __shared__ double sProb[kWave];
  __shared__ double2 sRow[kWave];
  __shared__ double cW[kWave], cAW[kWave], cCW[kWave];         // the compact entries of every market
  __shared__ double rCons[kWave], rConf[kWave], rTot[kWave];   // the result of every leave-out

  const int lane = lane_id();
  const int t = lane & (G - 1);
  const int base = lane - t;  // the market's first LDS slot
  const int64_t n_rounds = (a.n_list + SPR - 1) / SPR;
  bool badsid = false;
  for (int64_t r = blockIdx.x; r < n_rounds; r += gridDim.x) {
    const ShortFront sf = short_front<G>(a, r, lane, sRaw, badsid);
    const int64_t off = sf.off, m = sf.m;  // m >= 0: the market is processed (it may be empty)
    const int n = sf.n, rank = sf.rank;
    const bool valid = sf.valid;
    if (valid) {
      sSid[base + rank] = sf.s;
      sProb[base + rank] = sf.p;
      sRow[base + rank] = sf.rc;
    }
    wave_sync_lds();
    // lane t now looks at SORTED element t: the first of its source's run is the run's leader
    unsigned ss = 0;
    bool first = false;
    if (valid) {
      ss = sSid[lane];
      first = t == 0 || sSid[lane - 1] != ss;
    }
    const unsigned long long fm = (ballot(first) >> base) & kGroup;  // the market's leaders
    const int U = __popcll(fm);
    const int jrun = __popcll(fm & (~0ull >> (63 - t))) - 1;      // the run of sorted element t
    const int jmine = __popcll(fm & (~0ull >> (63 - rank))) - 1;  // ... and of the signal at position t
    // the leaders add their run's probabilities in arrival order (core.py:115-116)
    double sum = 0.0;
    int cnt = 0;
    bool open = first;
    for (int d = 0; d < G; ++d) {
      const int q = base + (t + d < n ? t + d : t);
      open = open && t + d < n && sSid[q] == ss;
      if (!ballot(open)) break;
      if (open) {
        sum += sProb[q];
        ++cnt;
      }
    }
    if (first) {
      const double2 row = sRow[lane];
      const double avg = cnt > 1 ? sum / (double)cnt : sum;  // s / 1 == s
      cW[base + jrun] = row.x;            // core.py:119
      cAW[base + jrun] = avg * row.x;     // core.py:136
      cCW[base + jrun] = row.y * row.x;   // core.py:142
    }
    wave_sync_lds();
    // lane j < U walks leave-out j
    if (t < U) {
      double total, ws, cs;
      loo_walk(cW + base, cAW + base, cCW + base, U, t, total, ws, cs);
      const bool null_ = (total == 0.0);  // core.py:131-133
      rCons[lane] = null_ ? 0.0 : ws / total;
      rConf[lane] = null_ ? 0.0 : cs / total;
      rTot[lane] = total;
      if (t == U - 1 && f.consensus) {  // its sums are the full sums' prefix in front of the last entry
        total += cW[lane];
        ws += cAW[lane];
        cs += cCW[lane];
        store_row(f.consensus, f.confidence, f.total_weight, f.n_unique, m, total, ws, cs, U);
      }
    }
    if (m >= 0 && n == 0 && t == 0 && f.consensus)
      store_row(f.consensus, f.confidence, f.total_weight, f.n_unique, m, 0.0, 0.0, 0.0, 0);
    wave_sync_lds();
    if (valid) {  // consecutive lanes, consecutive addresses; duplicates of a source get copies
      const int64_t at = off + t;
      a.consensus[at] = rCons[base + jmine];
      a.confidence[at] = rConf[base + jmine];
      a.total_weight[at] = rTot[base + jmine];
      a.n_unique[at] = U - 1;
    }
    wave_sync_lds();  // the next round overwrites the slots
  }
  if (ballot(badsid)) raise_fault(a.fault, kFaultSid);
}

// ------------------------------------------------------------------------------------
// long markets: workgroup per market, P = LDS capacity in signals (a power of two)
// ------------------------------------------------------------------------------------
// LDS, 36 B per signal: the sorted keys (8 B; from the compaction on the W column), the
// probabilities in arrival order (8 B), the AW and CW columns (8 B each), the arrival position of
// every sorted element and the first sorted element of every run (2 B each: positions < 4096).
__global__ __launch_bounds__(kHistMaxThreads) void loo_long_kernel(ConsArgs a, LooFull f, int P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char loo_lds[];
  unsigned long long* const key = reinterpret_cast<unsigned long long*>(loo_lds);
  double* const W = reinterpret_cast<double*>(loo_lds);
  double* const Pr = reinterpret_cast<double*>(loo_lds + 8 * (size_t)P);
  double* const AW = reinterpret_cast<double*>(loo_lds + 16 * (size_t)P);
  double* const CW = reinterpret_cast<double*>(loo_lds + 24 * (size_t)P);
  unsigned short* const sPos = reinterpret_cast<unsigned short*>(loo_lds + 32 * (size_t)P);
  unsigned short* const rStart = reinterpret_cast<unsigned short*>(loo_lds + 34 * (size_t)P);
  __shared__ int sCnt[kHistMaxThreads / kWave];
  const int tid = threadIdx.x, NT = blockDim.x;
  const int lane = lane_id(), wv = tid / kWave, NW = NT / kWave;

  report_plan_too_long(a, tid);
  dev_range(a);
  bool badsid = false;
  for (int64_t li = blockIdx.x; li < a.n_list; li += gridDim.x) {
    int64_t m, off;
    int n;
    if (!claim_market(a, li, P, tid, m, off, n)) continue;
    if (n == 0) {
      if (tid == 0 && f.consensus)
        store_row(f.consensus, f.confidence, f.total_weight, f.n_unique, m, 0.0, 0.0, 0.0, 0);
      continue;
    }
    // ---- keys and probabilities in arrival order, the keys then sorted by sid, then position
    const int Pm = fill_keys(a, key, off, n, tid, NT, badsid, [&](int i) { Pr[i] = a.prob[off + i]; });
    __syncthreads();
    block_bitonic_sort_u64(key, Pm, tid, NT);
    // ---- the leaders (first sorted element of a source's run), before the keys are overwritten
    unsigned leads = 0;  // bit c: sorted element c * NT + tid leads a run
    for (int c0 = 0, c = 0; c0 < n; c0 += NT, ++c) {
      const int e = c0 + tid;
      if (e < n && (e == 0 || (unsigned)(key[e - 1] >> 32) != (unsigned)(key[e] >> 32))) leads |= 1u << c;
    }
    __syncthreads();
    // ---- close the runs, compact them: NT sorted elements at a time ---------------------------
    // The W column lies on the keys.  Entry j of a leader at sorted element e has j <= e, the
    // elements of this pass are read before the barrier and written behind it, and a later pass
    // reads only elements behind this one's.
    int U = 0;
    for (int c0 = 0, c = 0; c0 < n; c0 += NT, ++c) {
      const int e = c0 + tid;
      const bool first = (leads >> c) & 1u;
      unsigned pos = 0;
      double w = 0.0, aw = 0.0, cw = 0.0;
      if (e < n) {
        const unsigned long long ke = key[e];
        pos = (unsigned)ke;
        if (first) {
          const unsigned ss = (unsigned)(ke >> 32);
          double s = 0.0;  // core.py:116: the run's probabilities in arrival order
          int cnt = 0;
          for (int q = e; q < n; ++q) {
            const unsigned long long kq = key[q];
            if ((unsigned)(kq >> 32) != ss) break;
            s += Pr[(unsigned)kq];
            ++cnt;
          }
          const double avg = cnt > 1 ? s / (double)cnt : s;
          const double2 row = hist_gather(a, ss);  // core.py:110-112
          w = row.x;           // core.py:119
          aw = avg * row.x;    // core.py:136
          cw = row.y * row.x;  // core.py:142
        }
      }
      const int j = block_compact_index(first, sCnt, wv, NW, lane, U);
      if (e < n) sPos[e] = (unsigned short)pos;
      if (first) {
        W[j] = w;
        AW[j] = aw;
        CW[j] = cw;
        rStart[j] = (unsigned short)e;
      }
      __syncthreads();
    }
    // ---- the leave-outs ------------------------------------------------------------------------
    for (int j = tid; j < U; j += NT) {
      double total, ws, cs;
      loo_walk(W, AW, CW, U, j, total, ws, cs);
      const bool null_ = (total == 0.0);  // core.py:131-133
      const double cons = null_ ? 0.0 : ws / total, conf = null_ ? 0.0 : cs / total;
      const int q1 = j + 1 < U ? rStart[j + 1] : n;
      for (int q = rStart[j]; q < q1; ++q) {  // every signal of the source gets a copy
        const int64_t at = off + sPos[q];
        a.consensus[at] = cons;
        a.confidence[at] = conf;
        a.total_weight[at] = total;
        a.n_unique[at] = U - 1;
      }
      if (j == U - 1 && f.consensus) {  // its sums are the full sums' prefix in front of the last entry
        total += W[j];
        ws += AW[j];
        cs += CW[j];
        store_row(f.consensus, f.confidence, f.total_weight, f.n_unique, m, total, ws, cs, U);
      }
    }
    __syncthreads();  // the next market overwrites the LDS
  }
  if (ballot(badsid)) raise_fault(a.fault, kFaultSid);
}

int launch_loo_short(int max_len, const ConsArgs& a, const LooFull& f, hipStream_t st) {
  const int G = max_len <= 8 ? 8 : max_len <= 16 ? 16 : max_len <= 32 ? 32 : 64;
  const int64_t rounds = ceil_div(a.n_list, kWave / G);
  switch (G) {
    case 8: return launch_persistent(loo_short_kernel<8>, 64, 8, rounds, "loo_short_kernel<8>", st, a, f);
    case 16: return launch_persistent(loo_short_kernel<16>, 64, 8, rounds, "loo_short_kernel<16>", st, a, f);
    case 32: return launch_persistent(loo_short_kernel<32>, 64, 8, rounds, "loo_short_kernel<32>", st, a, f);
    default: return launch_persistent(loo_short_kernel<64>, 64, 8, rounds, "loo_short_kernel<64>", st, a, f);
  }
}

}  // namespace
}  // namespace bce

using namespace bce;

extern "C" int bce_consensus_leave_one_out(const int64_t* offsets, int64_t n_markets, const int32_t* sid,
                                           const double* prob, int64_t n_signals, const double* relconf,
                                           const uint32_t* present_bits, int32_t n_sources,
                                           const int32_t* market_list, int64_t n_list,
                                           const int64_t* bin_start_host, const int64_t* bin_start_dev,
                                           int32_t max_len, double* consensus, double* confidence,
                                           double* total_weight, int32_t* n_unique, double* full_consensus,
                                           double* full_confidence, double* full_total_weight,
                                           int32_t* full_n_unique, void* stream) {
  (void)present_bits;  // cold sources already carry their defaults in relconf
  const int n_full = (full_consensus != nullptr) + (full_confidence != nullptr) + (full_total_weight != nullptr) +
                     (full_n_unique != nullptr);
  BCE_REQUIRE(n_full == 0 || n_full == 4, "leave_one_out: the full_* outputs are all NULL or all non-NULL");
  const LooFull full{full_consensus, full_confidence, full_total_weight, full_n_unique};
  hipStream_t st = as_stream(stream);
  const PerSignalCall c{offsets, n_markets, sid, prob, n_signals, relconf, n_sources, market_list, n_list,
                        bin_start_host, bin_start_dev, max_len, consensus, confidence, total_weight, n_unique};
  // without signals every market is empty: only the full_* rows (zeros) are left to write
  return per_signal_launch(
      "leave_one_out", "per-signal", c, n_markets == 0 || (n_signals == 0 && n_full == 0),
      [&](int bound, const ConsArgs& a) { return launch_loo_short(bound, a, full, st); },
      [&](int64_t bound, const ConsArgs& a) {
        return launch_market_block(loo_long_kernel, kLooElemBytes, bound, a.n_list, "loo_long_kernel", st, a, full);
      });
}
