// consensus_sorted.hpp -- one copy of what the kernels that sort a market ONCE by (sid, position)
// write the same way: consensus_history.hip and consensus_leave_one_out.hip (the per-signal
// analyses: the clamped table row, the fronts of their short and long kernels, their launchers and
// the body of their C entries) and consensus_long_kernel in consensus.hip (the u64 bitonic sort and
// the block compaction).  What a kernel does behind the sort stays in its own file.
#pragma once
#pragma clang fp contract(off)

#include "consensus_common.hpp"
#include "plan_host.hpp"

namespace bce {

constexpr int kHistMaxThreads = 1024;  // workgroup of the per-signal long kernels (one market each)

// A signal's sid as its table row: clamped into [0, n_sources) (unsigned compare, so a negative
// sid clamps to the last row); `bad` is set when it was outside.
__device__ __forceinline__ unsigned hist_row(int32_t sid, int32_t n_sources, bool& bad) {
  const unsigned smax = n_sources > 0 ? (unsigned)(n_sources - 1) : 0u;
  const unsigned s = (unsigned)sid;
  bad = bad || s > smax || n_sources <= 0;
  return s < smax ? s : smax;
}
__device__ __forceinline__ double2 hist_gather(const ConsArgs& a, unsigned row) {
  return a.n_sources > 0 ? a.relconf[row] : make_double2(0.0, 0.0);
}

// ------------------------------------------------------------------------------------
// workgroup pieces
// ------------------------------------------------------------------------------------
// Ascending bitonic sort of P (a power of two) u64 keys by the NT threads of a workgroup, a
// barrier behind every stage: keys (sid << 32) | position sort by sid, then arrival position
// (core.py:103,115).  Inlined into its caller, so `key` keeps the address space it has there
// (LDS accesses for an LDS array, global ones for a scratch slice).
__device__ __forceinline__ void block_bitonic_sort_u64(unsigned long long* key, int P, int tid, int NT) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int c = tid; c < (P >> 1); c += NT) {
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
}

// One pass of a block compaction: the compact index of this thread's element if it is a `first`
// (its rank among the firsts of the pass, behind the `total` of the passes before), and `total`
// advanced by the pass's count.  `cnt`: one LDS word per wave; the barrier between its store and
// its reads is in here, the one that lets the next pass overwrite it stays with the caller.
__device__ __forceinline__ int block_compact_index(bool first, int* cnt, int wv, int NW, int lane, int& total) {
  const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const unsigned long long bm = ballot(first);
  if (lane == 0) cnt[wv] = __popcll(bm);
  __syncthreads();
  int before = total, pass = 0;
  for (int q = 0; q < NW; ++q) {
    const int cq = cnt[q];
    if (q < wv) before += cq;
    pass += cq;
  }
  total += pass;
  return before + __popcll(bm & below);
}

// ------------------------------------------------------------------------------------
// the front of the per-signal short kernels: G lanes per market, 64 / G markets per wave
// ------------------------------------------------------------------------------------
struct ShortFront {
  int64_t off;  // the market's first CSR position
  int64_t m;    // the market, -1 where the group has none (past the list, or too long)
  int n;        // its signals (0 for no market)
  bool valid;   // lane t holds signal t
  unsigned s;   // ... its table row, probability and {reliability, confidence}
  double p;
  double2 rc;
  int rank;     // the signal's place among the market's (sid, position) keys
};

// Lane t = lane & (G - 1) of round r: claims the group's market (one longer than G is reported
// and left untouched), loads signal t, publishes its row to sRaw[lane] and ranks it by counting.
template <int G>
__device__ __forceinline__ ShortFront short_front(const ConsArgs& a, int64_t r, int lane, unsigned* sRaw,
                                                  bool& badsid) {
  const int t = lane & (G - 1);
  const int base = lane - t;  // the market's first LDS slot
  ShortFront f;
  f.off = 0;
  f.m = -1;
  f.n = 0;
  const int64_t li = r * (kWave / G) + lane / G;
  if (li < a.n_list) {
    const int64_t mk = a.list ? a.list[li] : li;
    f.off = a.offsets[mk];
    const int64_t len = a.offsets[mk + 1] - f.off;
    if (len < 0 || len > G) {  // longer than the launch's bound: report, leave untouched
      if (a.fault) atomicCAS(a.fault, 0, kFaultTooLong);
    } else {
      f.n = (int)len;
      f.m = mk;
    }
  }
  f.valid = t < f.n;
  f.s = 0;
  f.p = 0.0;
  f.rc = make_double2(0.0, 0.0);
  if (f.valid) {
    f.s = hist_row(a.sid[f.off + t], a.n_sources, badsid);
    f.p = a.prob[f.off + t];
    f.rc = hist_gather(a, f.s);  // core.py:110-112 (cold-start defaults are baked into the table)
  }
  sRaw[lane] = f.s;
  wave_sync_lds();
  // rank among the market's unique (sid, position) keys
  f.rank = 0;
#pragma unroll
  for (int q = 0; q < G; ++q) {  // no short circuit: every read is issued before the first compare
    const unsigned sq = sRaw[base + q];
    f.rank += (int)((q < f.n) & ((sq < f.s) | ((sq == f.s) & (q < t))));
  }
  return f;
}

// ------------------------------------------------------------------------------------
// the front of the per-signal long kernels: one workgroup per market, P keys of LDS
// ------------------------------------------------------------------------------------
// A device-resident plan: its last bin holds the markets longer than 4096, which get no launch.
// Called at kernel entry, ahead of dev_range.
__device__ __forceinline__ void report_plan_too_long(const ConsArgs& a, int tid) {
  if (a.dev_bins && blockIdx.x == 0 && tid == 0 && a.dev_bins[BCE_NBINS] > a.dev_bins[BCE_NBINS - 1] && a.fault)
    atomicCAS(a.fault, 0, kFaultTooLong);
}

// Market li of the launch's list: false (uniform over the workgroup) for one longer than P, which
// is reported and left untouched.  An empty market is claimed (n == 0).
__device__ __forceinline__ bool claim_market(const ConsArgs& a, int64_t li, int P, int tid, int64_t& m,
                                             int64_t& off, int& n) {
  m = a.list ? a.list[li] : li;
  off = a.offsets[m];
  const int64_t len = a.offsets[m + 1] - off;
  if (len < 0 || len > P) {
    if (tid == 0 && a.fault) atomicCAS(a.fault, 0, kFaultTooLong);
    return false;
  }
  n = (int)len;
  return true;
}

// The market's keys in arrival order, padded with kSent64 to Pm, its padded size (a power of two
// >= 64, returned); each(i) runs beside the key store of every signal i < n.  No barrier.
template <class Each>
__device__ __forceinline__ int fill_keys(const ConsArgs& a, unsigned long long* key, int64_t off, int n, int tid,
                                         int NT, bool& badsid, Each each) {
  int Pm = 64;
  while (Pm < n) Pm <<= 1;
  for (int i = tid; i < Pm; i += NT) {
    key[i] = i < n ? ((unsigned long long)hist_row(a.sid[off + i], a.n_sources, badsid) << 32) | (unsigned)i
                   : kSent64;
    if (i < n) each(i);
  }
  return Pm;
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
// The launch of a long kernel `fn(args..., P)`: P = the padded bound (64..4096 keys of
// `elem_bytes` of dynamic LDS each), min(P, 1024) threads, a grid of min(n_list, resident
// workgroups).
template <class... KA, class... A>
int launch_market_block(void (*fn)(KA...), int elem_bytes, int64_t max_len, int64_t n_list, const char* name,
                        hipStream_t st, const A&... args) {
  if (n_list == 0) return BCE_OK;
  int64_t P = next_pow2(max_len < 64 ? 64 : max_len);
  if (P > kLongMaxLds) P = kLongMaxLds;
  const int threads = (int)(P < kHistMaxThreads ? P : kHistMaxThreads);
  const size_t lds = (size_t)elem_bytes * (size_t)P;
  const void* f = reinterpret_cast<const void*>(fn);
  const int rc = ensure_dynamic_lds(f, elem_bytes * kLongMaxLds);
  if (rc) return rc;
  const int per_cu = blocks_per_cu(f, threads, lds, 1, name);
  const int64_t cap = grid_cap(per_cu);
  const int grid = (int)(n_list < cap ? n_list : cap);
  hipLaunchKernelGGL(fn, dim3(grid), dim3(threads), lds, st, args..., (int)P);
  return check_launch(name);
}

// What bce_consensus_history and bce_consensus_leave_one_out take alike.
struct PerSignalCall {
  const int64_t* offsets; int64_t n_markets;
  const int32_t* sid; const double* prob; int64_t n_signals;
  const double* relconf; int32_t n_sources;
  const int32_t* market_list; int64_t n_list;
  const int64_t* bin_start_host; const int64_t* bin_start_dev; int32_t max_len;
  double* consensus; double* confidence; double* total_weight; int32_t* n_unique;
  bool rows_optional = false;  // relconf may be NULL with n_sources > 0 (the live history: no chain has a bit)
};

// The body of both entries: the shared argument checks (messages "<op>: ...", the outputs named
// `outs`), `nothing` (the entry's own early-out) once they pass, then one launch sized by max_len
// or one per length bin of the plan.  launch_short(max_len, args) takes a bound <= 64,
// launch_long(max_len, args) one of 65..4096.
template <class Short, class Long>
int per_signal_launch(const char* op, const char* outs, const PerSignalCall& c, bool nothing, Short launch_short,
                      Long launch_long) {
  BCE_REQUIRE(c.n_markets >= 0 && c.n_signals >= 0 && c.n_sources >= 0 && c.n_list >= 0, "%s: negative size", op);
  BCE_REQUIRE(c.max_len >= 0 && c.max_len <= kLongMaxLds, "%s: max_len %d outside [0, %d]", op, c.max_len,
              kLongMaxLds);
  BCE_REQUIRE(c.n_markets == 0 || c.offsets, "%s: offsets is NULL", op);
  BCE_REQUIRE(c.n_signals == 0 || (c.sid && c.prob), "%s: sid/prob NULL", op);
  BCE_REQUIRE(c.n_signals == 0 || (c.consensus && c.confidence && c.total_weight && c.n_unique),
              "%s: %s outputs must be non-NULL", op, outs);
  BCE_REQUIRE(c.n_sources == 0 || c.relconf || c.rows_optional, "%s: source table is NULL", op);
  BCE_REQUIRE((uintptr_t)c.relconf % 16 == 0, "%s: relconf must be 16-byte aligned", op);
  BCE_REQUIRE(!(c.bin_start_host && c.bin_start_dev), "%s: one plan, host or device bin boundaries", op);
  const bool planned = c.bin_start_host || c.bin_start_dev;
  BCE_REQUIRE(!planned || c.market_list || c.n_markets == 0, "%s: a plan needs its market order", op);
  if (nothing) return BCE_OK;
  ConsArgs base{};
  base.offsets = c.offsets; base.sid = c.sid; base.prob = c.prob;
  base.relconf = reinterpret_cast<const double2*>(c.relconf);
  base.n_sources = c.n_sources; base.n_signals = c.n_signals;
  base.consensus = c.consensus; base.confidence = c.confidence; base.total_weight = c.total_weight;
  base.n_unique = c.n_unique;
  base.fault = fault_word();
  if (!planned) {  // one launch sized by max_len (0: unknown, as 4096)
    base.list = c.market_list;
    base.n_list = c.market_list ? c.n_list : c.n_markets;
    if (base.n_list == 0) return BCE_OK;
    return (c.max_len > 0 && c.max_len <= 64) ? launch_short((int)c.max_len, base)
                                              : launch_long(c.max_len > 0 ? c.max_len : kLongMaxLds, base);
  }
  // a length-binned plan: one launch per bin, longest bins first; the > 4096 bin runs in the
  // 4096 launch, which reports its markets and leaves them untouched
  int rc = BCE_OK;
  for (int b = BCE_NBINS - 1; b >= 0 && !rc; --b) {
    if (c.bin_start_dev && b == BCE_NBINS - 1) continue;  // reported by the long launches
    ConsArgs a = base;
    if (c.bin_start_host) {
      a.list = c.market_list + c.bin_start_host[b];
      a.n_list = c.bin_start_host[b + 1] - c.bin_start_host[b];
      if (a.n_list == 0) continue;
    } else {
      a.list = c.market_list;  // the whole plan order: the range is read on the device
      a.n_list = c.n_markets;  // upper bound: sizes the grid
      a.dev_bins = c.bin_start_dev;
      a.dev_b0 = a.dev_b1 = b;
    }
    const int64_t bound = b < BCE_NBINS - 1 ? kBinMax[b] : kLongMaxLds;
    rc = b <= kPlanSideLast ? launch_short((int)bound, a) : launch_long(bound, a);
  }
  return rc;
}

}  // namespace bce
