// consensus.hip -- batched core.compute_consensus (core.py:63-179) over CSR markets: the seg
// and long kernels, their launchers, and launch_seg_for_len, which picks the kernel for markets
// of up to 64 signals (the lane-per-market kernels are consensus_lane.hip, the LDS-table kernel
// is consensus_tab.hip, the wide one consensus_wide.hip over wide_sort.hpp and ordered_chain.hpp;
// the C entries are consensus_api.hip).
//
// Kernels by market length (launch_seg_for_len / launch_wide_len pick them):
//  consensus_pipe_kernel<G>    contiguous markets, n <= G in {8,16,32}, all outputs
//  consensus_flat_kernel<G>    contiguous markets, n <= 32, compact outputs or huge tables
//  consensus_lpm_kernel<G>     market lists (planned ragged batches), n <= 32
//                              (all three lane = market: consensus_lane.hip)
//  consensus_seg_kernel<64,8>  33 <= n <= 64: cooperative lane-per-signal phase (bitonic
//                              sort, ballots) then lane-per-market ordered sums from LDS.
//  consensus_wide_kernel       64 < n <= 4096 (consensus_wide.hip): one workgroup per
//                              market, register bitonic network over packed (sid, index)
//                              keys, exact chains or BCE_MODE_FAST fixed-order trees.
//  consensus_long_kernel<LDS>  fallback for long markets (LDS or global-scratch sort),
//                              BCE_MODE_FAST fixed-order trees.
// Every kernel sums in the reference's order in BCE_MODE_EXACT (bit-exact outputs).
// FP contraction is off for the whole file: every mul/add rounds like CPython.
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include <algorithm>

#include "consensus_common.hpp"
#include "consensus_sorted.hpp"
#include "plan_host.hpp"

#pragma clang fp contract(off)

constexpr int kSegWPE = 1;   // __launch_bounds__ min waves per SIMD for the segment kernel

namespace bce {

// ------------------------------------------------------------------------------------
// short markets: wave-per-tile, lane-per-signal then lane-per-market
// ------------------------------------------------------------------------------------
template <int G, int TM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kSegWPE, 8)))
void consensus_seg_kernel(ConsArgs a) {
  dev_range(a);
  static_assert(G == 8 || G == 16 || G == 32 || G == 64, "segment width");
  constexpr int SPR = kWave / G;   // segments (markets) per round
  constexpr int R = TM / SPR;      // rounds per tile
  static_assert(R * SPR == TM, "tile must be a whole number of rounds");
  constexpr int LOGG = (G == 8) ? 3 : (G == 16) ? 4 : (G == 32) ? 5 : 6;
  constexpr int RS = G + 1;        // padded LDS row stride (conflict-free transposed reads)
  constexpr int NI = (TM * G + 3 + 4 * kWave - 1) / (4 * kWave);  // 16-B sid chunks per lane
  constexpr int NP = (TM * G + 1 + 2 * kWave - 1) / (2 * kWave);  // 16-B prob chunks per lane

  // One LDS array, carved by hand (cdna guide §5 trap 4a): W | A | B rows (fp64,
  // TM x RS each), then usid rows, per-market scalars and the present bitmask.
  constexpr int ROWS = TM * RS;
  __shared__ double sWAB[3 * ROWS];
  __shared__ int32_t sU[ROWS];
  __shared__ int64_t sOff[TM];
  __shared__ int32_t sN[TM];
  __shared__ int32_t sM[TM];
  __shared__ int32_t sNU[TM];
  __shared__ int32_t sErr[TM];
  __shared__ double sTot[TM];
  __shared__ uint32_t sBits[kBitsLds];
  double* const sW = sWAB;
  double* const sA = sWAB + ROWS;
  double* const sB = sWAB + 2 * ROWS;

  const int lane = lane_id();
  const int seg = lane / G;
  const int t = lane & (G - 1);
  const int seg_base = seg * G;
  const unsigned long long segmask =
      (G >= 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << seg_base);
  const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

  // present bitmask: staged once per (persistent) workgroup when it fits in LDS
  const int nwords = (a.n_sources + 31) >> 5;
  const bool bits_in_lds = nwords <= kBitsLds;
  if (bits_in_lds)
    for (int i = lane; i < nwords; i += kWave) sBits[i] = a.pbits[i];
  // input staging for contiguous tiles, aliased onto the W|A|B rows (dead until the
  // cooperative phase): sids at sStageI[e - a0] in W, probabilities at sStageP[e - a0p]
  // from A on.
  static_assert(ROWS * 8 >= NI * 4 * kWave * 4, "sid staging fits in the W rows");
  static_assert(2 * ROWS * 8 >= NP * 2 * kWave * 8, "prob staging fits in the A|B rows");
  int32_t* sStageI = reinterpret_cast<int32_t*>(sW);
  double* sStageP = sA;

  const int64_t n_tiles = (a.n_list + TM - 1) / TM;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    // ---- tile metadata -------------------------------------------------------------
    if (lane < TM) {
      const int64_t li = tile * TM + lane;
      int32_t m = -1;
      int64_t off = 0;
      int32_t n = 0;
      if (li < a.n_list) {
        m = a.list ? a.list[li] : (int32_t)li;
        off = a.offsets[m];
        n = (int32_t)(a.offsets[m + 1] - off);
        if (n < 0 || n > G) {  // longer than the launch's max_len: report, skip
          if (a.fault) atomicCAS(a.fault, 0, kFaultTooLong);
          n = 0;
        }
      }
      sM[lane] = m;
      sOff[lane] = off;
      sN[lane] = n;
    }
    __syncthreads();

    // ---- load every round's signals; all loads in flight before the first use -------
    int32_t sidv[R];
    double pv[R];
    bool valid[R];
    if (a.list == nullptr) {
      // contiguous tile: [base, end) streamed with 16-B loads into LDS, then each lane
      // picks its (market, slot) element.
      const int64_t base = sOff[0];
      int64_t end = base;
#pragma unroll
      for (int q = 0; q < TM; ++q) end = (sN[q] > 0) ? sOff[q] + sN[q] : end;
      const int64_t a0 = base & ~3ll, a0p = base & ~1ll;
      int4 vi[NI];
      double2 vp[NP];
#pragma unroll
      for (int q = 0; q < NI; ++q) {
        const int64_t e = a0 + 4 * (lane + kWave * q);
        vi[q] = make_int4(0, 0, 0, 0);
        if (e < end) {
          if (e + 4 <= a.n_signals) {
            vi[q] = *reinterpret_cast<const int4*>(a.sid + e);
          } else {
            vi[q].x = a.sid[e];
            if (e + 1 < a.n_signals) vi[q].y = a.sid[e + 1];
            if (e + 2 < a.n_signals) vi[q].z = a.sid[e + 2];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const int64_t e = a0p + 2 * (lane + kWave * q);
        vp[q] = make_double2(0.0, 0.0);
        if (e < end) {
          if (e + 2 <= a.n_signals) vp[q] = *reinterpret_cast<const double2*>(a.prob + e);
          else vp[q].x = a.prob[e];
        }
      }
#pragma unroll
      for (int q = 0; q < NI; ++q)
        *reinterpret_cast<int4*>(sStageI + 4 * (lane + kWave * q)) = vi[q];
#pragma unroll
      for (int q = 0; q < NP; ++q)
        *reinterpret_cast<double2*>(sStageP + 2 * (lane + kWave * q)) = vp[q];
      __syncthreads();
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int mk = r * SPR + seg;
        valid[r] = t < sN[mk];
        const int64_t p = sOff[mk] + t;
        sidv[r] = valid[r] ? sStageI[p - a0] : 0;
        pv[r] = valid[r] ? sStageP[p - a0p] : 0.0;
      }
      __syncthreads();  // staging (aliased on sA/sB) is dead from here on
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int mk = r * SPR + seg;
        const int32_t n = sN[mk];
        valid[r] = t < n;
        sidv[r] = 0;
        pv[r] = 0.0;
        if (valid[r]) {
          const int64_t p = sOff[mk] + t;
          sidv[r] = a.sid[p];
          pv[r] = a.prob[p];
        }
      }
    }

    // ---- source-table gathers for every round, by ORIGINAL lane, all in flight ------
    // (core.py:110-112): one 16-B {reliability, confidence} load per signal; the sorted
    // lanes later pull the values of the lane that holds the same sid (ds_bpermute), so
    // no L2 round trip sits inside the per-round dependency chain.
    double2 rc[R];
    uint32_t pw[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      rc[r] = make_double2(0.5, 0.25);
      pw[r] = 0xffffffffu;
      if (valid[r]) {
        rc[r] = a.relconf[sidv[r]];
        if (!bits_in_lds) pw[r] = a.pbits[sidv[r] >> 5];
      }
    }

    // ---- cooperative phase -----------------------------------------------------------
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int mk = r * SPR + seg;
      unsigned key = valid[r] ? (((unsigned)sidv[r] << LOGG) | (unsigned)t) : kSent32;
      key = bitonic_sort_seg<G>(key, t);
      const bool kv = key != kSent32;
      const int ssid = (int)(key >> LOGG);
      const int src = seg_base + (int)(key & (G - 1));  // lane holding this signal
      const double ps = pull_f64(pv[r], src);            // probability in sorted order
      const int prev = wave_shr1(ssid, -1);
      const bool first = kv && (t == 0 || prev != ssid);
      const unsigned long long fm = ballot(first);
      const unsigned long long vm = ballot(kv);
      const int j = __popcll(fm & segmask & below);
      // run length of a leader: distance to the next leader / invalid lane / segment end
      const unsigned long long bnd = fm | ~vm;
      const unsigned long long above = (lane == 63) ? 0ull : (bnd >> (lane + 1));
      const int seg_end = seg_base + G;
      int run = above ? (__builtin_ctzll(above) + 1) : (64 - lane);
      if (lane + run > seg_end) run = seg_end - lane;
      const int myrun = first ? run : 1;
      double s = 0.0 + ps;  // builtin sum() starts from int 0 (core.py:116)
      double avg = s;
      if (ballot(myrun > 1)) {  // duplicates: sum the run in input order
        for (int k = 1; k < G; ++k) {
          const int sl = (lane + k < 64) ? lane + k : 63;
          const double pk = pull_f64(ps, sl);
          if (k < myrun) s += pk;
          if (!ballot(k + 1 < myrun)) break;
        }
        avg = (myrun > 1) ? s / (double)myrun : s;
      }
      const double w = pull_f64(rc[r].x, src);  // core.py:111,119
      const double c = pull_f64(rc[r].y, src);  // core.py:112
      const uint32_t word = bits_in_lds ? sBits[ssid >> 5] : (uint32_t)pull_i32((int)pw[r], src);
      if (first) {
        const bool cold = ((word >> (ssid & 31)) & 1u) == 0;  // core.py:167-170
        const int o = mk * RS + j;
        sW[o] = w;
        sA[o] = avg * w;  // core.py:136
        sB[o] = c * w;    // core.py:142
        sU[o] = ssid | (cold ? (int32_t)0x80000000 : 0);
      }
      // validate_input_payload range check (core.py:59-60) on the ORIGINAL order
      const unsigned long long bad =
          ballot(valid[r] && (pv[r] < 0.0 || pv[r] > 1.0)) & segmask;
      if (t == 0) {
        sNU[mk] = __popcll(fm & segmask);
        sErr[mk] = bad ? (int)(__builtin_ctzll(bad) - seg_base) : -1;
      }
    }
    __syncthreads();

    // ---- serial phase: lane = market, exact left-to-right sums (core.py:107-144) ----
    // Fixed trip count with predication so every LDS read can be issued ahead of the
    // dependent adds; adding nothing for j >= u keeps the exact order.
    if (lane < TM) {
      const int u = sNU[lane];
      double total = 0.0, ws = 0.0, cs = 0.0;
      const int base = lane * RS;
      {
#pragma unroll
        for (int jj = 0; jj < G; ++jj) {
          if (jj < u) {
            total += sW[base + jj];
            ws += sA[base + jj];
            cs += sB[base + jj];
          }
        }
      }
      sTot[lane] = total;
      const int32_t m = sM[lane];
      if (m >= 0) {
        const bool null_ = (total == 0.0);
        a.consensus[m] = null_ ? 0.0 : ws / total;
        a.confidence[m] = null_ ? 0.0 : cs / total;
        a.total_weight[m] = total;
        a.n_unique[m] = u;
        if (a.err_idx) a.err_idx[m] = sErr[lane];
      }
    }
    __syncthreads();

    // ---- per-unique outputs (coalesced at CSR offsets) --------------------------------
    if ((a.usid || a.weight || a.nweight)) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int mk = r * SPR + seg;
        if (t < sNU[mk]) {
          const int64_t p = sOff[mk] + t;
          const double w = sW[mk * RS + t];
          const double tot = sTot[mk];
          if (a.usid) a.usid[p] = sU[mk * RS + t];
          if (a.weight) a.weight[p] = w;
          if (a.nweight) a.nweight[p] = (tot > 0.0) ? w / tot : 0.0;  // core.py:151
        }
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------
// long markets: workgroup per market
// ------------------------------------------------------------------------------------
constexpr int kLongThreads = 256;

// Fixed-order (deterministic) tree sum over the workgroup (BCE_MODE_FAST).
__device__ __forceinline__ double block_sum_tree(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = kLongThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// Pass structure per market (all arrays length P = next pow2 >= n):
//   0  keys[t] = sid<<32 | t, Pr[t] = prob (input order); first out-of-range index
//   1  bitonic sort of keys (ascending sid, then input index == core.py:103,115;
//      block_bitonic_sort_u64, consensus_sorted.hpp)
//   2  leaders (first position of each sid run) sum their run's probabilities in input
//      order (core.py:116), compact index j by block scan (block_compact_index) ->
//      Av[j] = avg, Sj[j] = sid
//   3  per unique j: w = rel, W[j] = w, A[j] = avg*w, C[j] = conf*w, per-unique outputs
//   4  ordered sums over j (exact: one lane per chain; fast: fixed tree)
//   5  normalizedWeight[j] = W[j] / total
template <bool IN_LDS>
__global__ __launch_bounds__(kLongThreads) void consensus_long_kernel(ConsArgs a) {
  constexpr int NT = kLongThreads;
  constexpr int NW = NT / kWave;
  constexpr int CAP = IN_LDS ? kLongMaxLds : 1;
  __shared__ unsigned long long lKeys[CAP];  // keys, then W (double)
  __shared__ double lP[CAP];                 // probabilities, then A
  __shared__ double lC[CAP];                 // avg, then C
  __shared__ int32_t lS[CAP];                // sid of unique j
  __shared__ double red[NT];
  __shared__ int32_t sInt[NW + 2];
  __shared__ double sTot[4];

  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wv = tid / kWave;

  for (int64_t li = blockIdx.x; li < a.n_list; li += gridDim.x) {
    const int32_t m = a.list ? a.list[li] : (int32_t)li;
    const int64_t off = a.offsets[m];
    const int32_t n = (int32_t)(a.offsets[m + 1] - off);
    int P = 1;
    while (P < n) P <<= 1;

    unsigned long long* keys;
    double* Pr;
    double* Cv;
    int32_t* Sj;
    if constexpr (IN_LDS) {
      keys = lKeys;
      Pr = lP;
      Cv = lC;
      Sj = lS;
    } else {
      unsigned long long* base = reinterpret_cast<unsigned long long*>(a.scratch) +
                                 (int64_t)blockIdx.x * 4 * a.scratch_stride;
      keys = base;
      Pr = reinterpret_cast<double*>(base + a.scratch_stride);
      Cv = reinterpret_cast<double*>(base + 2 * a.scratch_stride);
      Sj = reinterpret_cast<int32_t*>(base + 3 * a.scratch_stride);
    }
    double* Wv = reinterpret_cast<double*>(keys);

    // ---- pass 0 ------------------------------------------------------------------------
    if (tid == 0) sInt[0] = 0x7fffffff;
    __syncthreads();
    int myerr = 0x7fffffff;
    for (int i = tid; i < P; i += NT) {
      if (i < n) {
        const double p = a.prob[off + i];
        keys[i] = ((unsigned long long)(unsigned)a.sid[off + i] << 32) | (unsigned)i;
        Pr[i] = p;
        if ((p < 0.0 || p > 1.0) && i < myerr) myerr = i;  // core.py:59-60
      } else {
        keys[i] = kSent64;
      }
    }
    if (myerr != 0x7fffffff) atomicMin(&sInt[0], myerr);
    __syncthreads();
    const int errv = sInt[0];

    // ---- pass 1: bitonic sort ----------------------------------------------------------
    block_bitonic_sort_u64(keys, P, tid, NT);

    // ---- pass 2: leaders, run sums in input order, compact index ------------------------
    int u = 0;
    for (int c0 = 0; c0 < n; c0 += NT) {
      const int tpos = c0 + tid;
      bool first = false;
      int ssid = 0;
      double avg = 0.0;
      if (tpos < n) {
        ssid = (int)(keys[tpos] >> 32);
        first = (tpos == 0) || ((int)(keys[tpos - 1] >> 32) != ssid);
        if (first) {
          double s = 0.0;  // builtin sum() from 0 (core.py:116)
          int cnt = 0;
          for (int q = tpos; q < n; ++q) {
            const unsigned long long kq = keys[q];
            if ((int)(kq >> 32) != ssid) break;
            s += Pr[(int)(kq & 0xffffffffu)];
            ++cnt;
          }
          avg = (cnt > 1) ? s / (double)cnt : s;
        }
      }
      const int j = block_compact_index(first, sInt + 2, wv, NW, lane, u);
      if (first) {
        Cv[j] = avg;
        Sj[j] = ssid;
      }
      __syncthreads();
    }

    // ---- pass 3: gather + per-unique products (keys/probs are dead now) -----------------
    for (int j = tid; j < u; j += NT) {
      const int s = Sj[j];
      const double2 rc = a.relconf[s];
      const double w = rc.x;  // core.py:111,119
      const double c = rc.y;  // core.py:112
      const double avg = Cv[j];
      Wv[j] = w;
      Pr[j] = avg * w;  // core.py:136
      Cv[j] = c * w;    // core.py:142
      const int64_t p = off + j;
      if (a.usid) a.usid[p] = s | (int32_t)cold_flag(a.pbits[s >> 5], s);
      if (a.weight) a.weight[p] = w;
    }
    __syncthreads();

    // ---- pass 4: ordered sums ----------------------------------------------------------
    if (a.mode == BCE_MODE_EXACT) {
      if (tid < 3) {  // three independent chains on three lanes of wave 0
        const double* arr = (tid == 0) ? Wv : (tid == 1) ? Pr : Cv;
        double acc = 0.0;
        for (int j = 0; j < u; ++j) acc += arr[j];
        sTot[tid] = acc;
      }
      __syncthreads();
    } else {
      double pw = 0.0, pa = 0.0, pc = 0.0;
      for (int j = tid; j < u; j += NT) {
        pw += Wv[j];
        pa += Pr[j];
        pc += Cv[j];
      }
      const double tw = block_sum_tree(pw, red);
      const double ta = block_sum_tree(pa, red);
      const double tc = block_sum_tree(pc, red);
      if (tid == 0) {
        sTot[0] = tw;
        sTot[1] = ta;
        sTot[2] = tc;
      }
      __syncthreads();
    }
    const double total = sTot[0];
    if (tid == 0) {
      const bool null_ = (n == 0) || (total == 0.0);
      a.consensus[m] = null_ ? 0.0 : sTot[1] / total;
      a.confidence[m] = null_ ? 0.0 : sTot[2] / total;
      a.total_weight[m] = total;
      a.n_unique[m] = u;
      if (a.err_idx) a.err_idx[m] = (errv == 0x7fffffff) ? -1 : errv;
    }

    // ---- pass 5: normalizedWeight (core.py:151) ----------------------------------------
    if (a.nweight) {
      for (int j = tid; j < u; j += NT) a.nweight[off + j] = (total > 0.0) ? Wv[j] / total : 0.0;
    }
    __syncthreads();
  }
}


}  // namespace bce

// ======================================================================================
// host launchers
// ======================================================================================
namespace bce {

namespace {

template <int G, int TM>
int launch_seg(const ConsArgs& a, hipStream_t st) {
  return launch_persistent(consensus_seg_kernel<G, TM>, 64, 8, ceil_div(a.n_list, TM), "consensus_seg_kernel", a, st);
}

}  // namespace

// Markets with n <= 64 (a.list == NULL: contiguous CSR; else a planned market list).
//   contiguous, 16 < n <= 32, S <= kTabMaxSources   consensus_tab32_kernel (table in LDS)
//   ... S <= kTabHybMaxSources                       consensus_tab32_kernel<hybrid> (LDS rows + global rest)
//   contiguous, n <= 32, S < 2^25, all outputs       consensus_pipe_kernel<G> (loader + compute waves)
//   contiguous, n <= 32, otherwise                   consensus_flat_kernel<G>
//   market list, n <= 32                             consensus_lpm_kernel<G> (lane per market)
//   33 <= n <= 64                                    consensus_seg_kernel<64, 8>
int launch_seg_for_len(int max_len, const ConsArgs& a, hipStream_t st) {
  if (max_len > 32) return launch_seg<64, 8>(a, st);
  const int G = (max_len <= 8) ? 8 : (max_len <= 16) ? 16 : 32;  // lane kernels: keys per lane
  if (a.list != nullptr) return launch_lane(LaneKernel::Lpm, G, a, st);
  if (max_len > 16 && a.n_sources <= kTabHybMaxSources) return launch_tab32(a, st);
  const bool pipe = a.n_sources < (1 << 25) && a.n_signals >= 4 && a.usid && a.weight && a.nweight;
  return launch_lane(pipe ? LaneKernel::Pipe : LaneKernel::Flat, G, a, st);
}

int launch_long_lds(const ConsArgs& a, hipStream_t st) {
  if (a.n_list == 0) return BCE_OK;
  const int64_t cap = grid_cap(2);
  const int grid = (int)(a.n_list < cap ? a.n_list : cap);
  hipLaunchKernelGGL((consensus_long_kernel<true>), dim3(grid), dim3(kLongThreads), 0, st, a);
  return check_launch("consensus_long_kernel<lds>");
}

int launch_long_global(ConsArgs a, void* scratch, int64_t stride, hipStream_t st) {
  if (a.n_list == 0) return BCE_OK;
  a.scratch = scratch;
  a.scratch_stride = stride;
  // one scratch slice per workgroup of long_scratch_grid, whatever the device: only the debug
  // cap shrinks this grid, and a smaller grid only leaves slices unused
  int64_t grid = long_scratch_grid(a.n_list);
  const int64_t dbg = debug_grid_cap();
  if (dbg > 0 && grid > dbg) grid = dbg;
  hipLaunchKernelGGL((consensus_long_kernel<false>), dim3((int)grid), dim3(kLongThreads), 0, st, a);
  return check_launch("consensus_long_kernel<global>");
}

}  // namespace bce
