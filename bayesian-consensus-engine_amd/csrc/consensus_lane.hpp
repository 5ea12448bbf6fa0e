// consensus_lane.hpp -- the pieces the lane-per-market consensus kernels share
// (consensus_lane.hip: consensus_lpm_kernel, consensus_flat_kernel, consensus_pipe_kernel).
// The kernel idea: lane = market, (sid, slot) keys sorted in VGPRs by the odd-even merge
// network, a left-to-right walk in sorted order, per-unique results staged in place, coalesced
// copy-out.  Every piece below has this one definition (but lane_keys, whose text the flat
// kernel repeats inline for a measured reason); all of it inlines into its kernel.
#pragma once
#pragma clang fp contract(off)

#include "consensus_common.hpp"

namespace bce {

constexpr int kPackSlot = 25;  // staged per-unique word = sid | slot << 25 (sid < 2^25)

template <int G>
constexpr int lane_logg() {
  static_assert(G == 8 || G == 16 || G == 32, "lane-per-market widths");
  return (G == 8) ? 3 : (G == 16) ? 4 : 5;
}

// ---- a tile of consecutive markets: ONE contiguous signal range [B, E) -------------------
// The LDS images start at the 16-B chunk that holds B (Bs: 4 sids, Bp: 2 probabilities) and
// are filled by 16-B LDS-DMA up to es / ep, the end of the last chunk that lies inside the
// arrays; only the batch's last tile can have signals past them (copy_array_tail).
struct TileRange {
  int64_t B, E;
  int64_t Bs, Bp;   // image origins
  int64_t es, ep;   // DMA ends
  int nci, ncp;     // 16-B chunks of sids / probabilities
  __device__ __forceinline__ int dB() const { return (int)(B - Bs); }  // B inside the sid image
  __device__ __forceinline__ int dP() const { return (int)(B - Bp); }  // ... the prob image
};

__device__ __forceinline__ TileRange tile_range(int64_t B, int64_t E, int64_t n_signals) {
  TileRange r;
  r.B = B;
  r.E = E;
  r.Bs = B & ~3ll;
  r.Bp = B & ~1ll;
  const int64_t Nf4 = n_signals & ~3ll, Nf2 = n_signals & ~1ll;  // last full chunk ends
  r.es = (E < Nf4) ? ((E + 3) & ~3ll) : Nf4;
  r.ep = (E < Nf2) ? ((E + 1) & ~1ll) : Nf2;
  r.nci = (int)((r.es - r.Bs) >> 2);
  r.ncp = (int)((r.ep - r.Bp) >> 1);
  return r;
}

// tail of the arrays that does not fill a 16-B chunk (last tile only), after the DMA landed
__device__ __forceinline__ void copy_array_tail(const TileRange& r, const ConsArgs& a, uint32_t* iS, double* iP,
                                                int lane) {
  if (r.E > r.es && lane < (int)(r.E - r.es)) iS[r.es - r.Bs + lane] = (uint32_t)a.sid[r.es + lane];
  if (r.E > r.ep && lane < (int)(r.E - r.ep)) iP[r.ep - r.Bp + lane] = a.prob[r.ep + lane];
}

// ---- a lane's market -----------------------------------------------------------------------
// longer than the launch's max_len: report, skip
template <int G>
__device__ __forceinline__ void screen_len(int& n, int* fault) {
  if (ballot(n < 0 || n > G)) {
    raise_fault(fault, kFaultTooLong);
    if (n < 0 || n > G) n = 0;
  }
}

// The lane's row of the sid image (at rsi) as sorted keys sid << log2 G | slot, the sentinel
// past n.  16-B reads when every row of the tile starts on a 16-B chunk (rows may overrun into
// the image's slack), scalar reads otherwise.
// (The pipe kernel calls this; the flat kernel keeps the same text inline, where the call
// measured 4 % slower: measurements/consensus_lane_split_ab.txt.)
template <int G>
__device__ __forceinline__ void lane_keys(const uint32_t* iS, int rsi, int n, bool has, unsigned (&key)[G]) {
  constexpr int LOGG = lane_logg<G>();
  if (ballot(has && (rsi & 3) != 0) == 0) {
#pragma unroll
    for (int c = 0; c < G / 4; ++c) {
      const uint4 v = *reinterpret_cast<const uint4*>(iS + rsi + 4 * c);
      key[4 * c] = v.x; key[4 * c + 1] = v.y; key[4 * c + 2] = v.z; key[4 * c + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int t = 0; t < G; ++t) key[t] = iS[rsi + t];
  }
#pragma unroll
  for (int t = 0; t < G; ++t) key[t] = (t < n) ? ((key[t] << LOGG) | (unsigned)t) : kSent32;
  oem_sort<G>(key);
}

// Run structure of the sorted keys as bit masks in one VGPR each: bit t of fb / lb = position t
// is the first / last of its sid run, vb = valid (exactly t < n after the sort).  Bit t of nq =
// (sid_t != sid_t+1); sentinels sort last and never equal a sid, so lst = nq | top bit,
// fst = nq << 1 | 1, both masked to t < n.
template <int G>
__device__ __forceinline__ void run_masks(const unsigned (&key)[G], int n, unsigned& fb, unsigned& lb, unsigned& vb) {
  constexpr int LOGG = lane_logg<G>();
  unsigned nq = 0;
#pragma unroll
  for (int t = G - 2; t >= 0; --t) nq = (nq << 1) | (((key[t] ^ key[t + 1]) >> LOGG) != 0u ? 1u : 0u);
  vb = (n >= 32) ? 0xFFFFFFFFu : ((1u << n) - 1u);
  lb = (nq | (1u << (G - 1))) & vb;
  fb = ((nq << 1) | 1u) & vb;
  // opaque to the optimiser: otherwise it folds the bit tests back into the per-position
  // compare masks and keeps ~3*G of them alive in SGPRs across the walk (spills)
  asm volatile("" : "+v"(fb), "+v"(lb), "+v"(vb));
}

// ---- the walk (core.py:107-144 in sorted-source order) -------------------------------------
struct Walk {
  double total = 0.0, ws = 0.0, cs = 0.0;  // the reference's three left-to-right chains
  double psum = 0.0;                       // probability sum of the current run
  int cnt = 0, j = 0;                      // length of the current run, uniques so far
};

// One sorted position, general form (branch-free): duplicate runs summed in input order, the
// chains advanced at the last position of a run.  `stage(j)` stores the position's staged
// results for unique j (flat: to a sink when invalid; pipe: predicated).
template <class Stage>
__device__ __forceinline__ void walk_step(Walk& k, int t, unsigned fb, unsigned lb, double p, double2 rc,
                                          Stage&& stage) {
  const bool fst = __builtin_amdgcn_ubfe(fb, t, 1) != 0u;
  const bool lst = __builtin_amdgcn_ubfe(lb, t, 1) != 0u;
  k.psum = (fst ? 0.0 : k.psum) + p;   // builtin sum() from int 0 (core.py:116)
  k.cnt = fst ? 1 : k.cnt + 1;
  double avg = k.psum;
  if (ballot(lst && k.cnt > 1)) {       // duplicates: sum / len (core.py:116), rare
    if (lst && k.cnt > 1) avg = k.psum / (double)k.cnt;
  }
  const double wt = rc.x, cf = rc.y;
  // accumulate only at the last position of a run; +0.0 leaves every chain bit-exact
  // (the chains start at +0.0 and can never become -0.0)
  k.total += lst ? wt : 0.0;          // core.py:120
  k.ws += lst ? avg * wt : 0.0;       // core.py:135-137
  k.cs += lst ? cf * wt : 0.0;        // core.py:141-143
  stage(k.j);                         // j <= t: the row cell is dead
  k.j += lst ? 1 : 0;
}

// pin the chains at the end of a position: left alone the compiler sinks every add to the end
// of the walk and keeps all per-position operands and masks alive
__device__ __forceinline__ void walk_pin(Walk& k) {
  asm volatile("" : "+v"(k.total), "+v"(k.ws), "+v"(k.cs), "+v"(k.psum), "+v"(k.cnt), "+v"(k.j));
  __builtin_amdgcn_sched_barrier(0);
}

// ---- results (store_market, cold_flag, norm_weight: consensus_common.hpp) --------------------
struct Unique {
  unsigned sid;
  int slot;
};
template <int G>
__device__ __forceinline__ Unique unpack_unique(unsigned pk) {
  return {pk & ((1u << kPackSlot) - 1), (int)((pk >> kPackSlot) & (G - 1))};
}
// the present word of a source, from the staged copy or from global memory (two loads under a
// uniform branch: a select of the pointers would make them flat loads)
__device__ __forceinline__ uint32_t present_word(const uint32_t* sBits, const uint32_t* pbits, bool bits_in_lds,
                                                 unsigned sid) {
  return bits_in_lds ? sBits[sid >> 5] : pbits[sid >> 5];
}
// 8-B usid pairs and 16-B weight / nweight pairs can be stored: the arrays are aligned and
// every row of the tile starts at an even signal
__device__ __forceinline__ bool pair_store_ok(const ConsArgs& a, bool has, int64_t off, int64_t B) {
  const bool vec_ok = (((uintptr_t)a.usid & 7) | ((uintptr_t)a.weight & 15) | ((uintptr_t)a.nweight & 15)) == 0;
  return vec_ok && ballot(has && (off & 1) != 0) == 0 && (B & 1) == 0;
}

// Present bits staged in LDS up to 16384 sources (by the whole workgroup, before its barrier);
// larger tables read them from global memory (one 4-B gather per unique source, L2-resident:
// S/8 bytes).  Returns whether sBits holds them.
__device__ __forceinline__ bool stage_present_bits(uint32_t* sBits, const ConsArgs& a, int nthreads) {
  const int nwords = (a.n_sources + 31) >> 5;
  const bool bits_in_lds = nwords <= kBitsLds;
  if (bits_in_lds)
    for (int i = threadIdx.x; i < nwords; i += nthreads) sBits[i] = a.pbits[i];
  return bits_in_lds;
}

}  // namespace bce
