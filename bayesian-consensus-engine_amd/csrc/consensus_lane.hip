// consensus_lane.hip -- the lane-per-market consensus kernels (markets of n <= G signals,
// G in {8, 16, 32}) and their launchers; launch_seg_for_len (consensus.hip) picks among them:
//  consensus_pipe_kernel<G>    contiguous markets, all outputs: one loader wave streams tiles
//                              into an LDS ring (LDS-DMA), the compute waves (lane = market)
//                              sort keys in VGPRs and walk them with 16-B {rel, conf} gathers
//                              from global memory.
//  consensus_flat_kernel<G>    contiguous markets, compact outputs or huge tables: the same
//                              arithmetic, each wave loads its own tile.
//  consensus_lpm_kernel<G>     market lists (planned ragged batches): rows staged per market
//                              by LDS-DMA.
// The pieces they share are consensus_lane.hpp.  Every kernel sums in the reference's order
// (bit-exact outputs).  FP contraction is off for the whole file: every mul/add rounds like
// CPython.
#include "consensus_lane.hpp"

#pragma clang fp contract(off)

constexpr int kFlatTM = 64;   // flat kernel: markets per wave tile
constexpr int kFlatRing = 8;  // flat kernel: relconf gathers in flight per lane
constexpr int kFlatWPE = 1;   // flat kernel: min waves per SIMD (register budget)
constexpr int kFlatWPB = 2;   // flat kernel: waves per workgroup

namespace bce {

// ------------------------------------------------------------------------------------
// market lists: consensus_lpm_kernel<G>
// ------------------------------------------------------------------------------------
// Cross-lane LDS hand-off of the lpm kernel: a workgroup barrier, which in this single-wave
// workgroup only orders the wave's own LDS traffic.  (The wave's LDS instructions execute in
// order, so wave_sync_lds -- a compiler barrier + lgkmcnt drain -- would do; the kernel keeps
// the barrier it was measured with.)
__device__ __forceinline__ void wave_sync() {
  __syncthreads();
}

// One dword per lane by the builtin LDS-DMA, not dma_b32 (consensus_common.hpp): the compiler
// tracks the builtin in its wait counts and sets M0 itself; dma_b32 saves and restores M0 around
// every transfer: with it the lpm launches of a 200k-market ragged batch measured 2.5 % slower
// (measurements/consensus_lane_split_ab.txt).
__device__ __forceinline__ void dma4(const void* g, void* lds) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)lds, 4, 0, 0);
}

template <int G>
__global__ __launch_bounds__(64) void consensus_lpm_kernel(ConsArgs a) {
  dev_range(a);
  constexpr int LOGG = lane_logg<G>();
  constexpr int SST = G + 1;       // sid / usid row stride (dwords): conflict-free b32 reads
  constexpr int PST = 2 * G + 2;   // prob / weight row stride (dwords, even -> 8-B aligned)
  constexpr int RING = 8;          // gathers issued this many sorted positions ahead
  constexpr int MPI = kWave / G;   // markets per copy-out iteration

  __shared__ uint32_t sS[kWave * SST];  // sid rows; after the walk: usid rows
  __shared__ uint32_t sP[kWave * PST];  // prob rows; after the sorted read: weight rows
  __shared__ int64_t sOff[kWave];
  __shared__ int32_t sU[kWave];
  __shared__ double sTot[kWave];

  const int lane = lane_id();
  const int64_t n_tiles = (a.n_list + kWave - 1) / kWave;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    // ---- this lane's market ---------------------------------------------------------
    const int64_t li = tile * kWave + lane;
    int32_t mk = -1;
    int64_t off = 0;
    int n = 0;
    if (li < a.n_list) {
      mk = a.list ? a.list[li] : (int32_t)li;
      off = a.offsets[mk];
      n = (int)(a.offsets[mk + 1] - off);
    }
    screen_len<G>(n, a.fault);

    unsigned key[G];
    double sp[G];
    int err = -1;
    // ---- rows -> LDS by LDS-DMA: one dword per lane, market by market --------------
    for (int q = 0; q < kWave; ++q) {
      const int nq = __builtin_amdgcn_readlane(n, q);
      if (nq == 0) continue;
      const int64_t oq = readlane_i64(off, q);
      if (lane < nq) dma4(a.sid + oq + lane, sS + q * SST);
      if (lane < 2 * nq) dma4(reinterpret_cast<const uint32_t*>(a.prob + oq) + lane, sP + q * PST);
      if (2 * nq > kWave && lane < 2 * nq - kWave)
        dma4(reinterpret_cast<const uint32_t*>(a.prob + oq) + kWave + lane, sP + q * PST + kWave);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    const uint32_t* rowS = sS + lane * SST;
    const double* rowP = reinterpret_cast<const double*>(sP + lane * PST);
    // keys (sid, slot) and the validation scan in input order
#pragma unroll
    for (int t = 0; t < G; ++t) {
      const bool v = t < n;
      key[t] = v ? ((rowS[t] << LOGG) | (unsigned)t) : kSent32;
      const double p = rowP[t];
      if (v && err < 0 && (p < 0.0 || p > 1.0)) err = t;  // core.py:59-60 (NaN passes)
    }
    oem_sort<G>(key);
    // probabilities in sorted order (registers); the rows become output staging
#pragma unroll
    for (int t = 0; t < G; ++t) sp[t] = rowP[key[t] & (G - 1)];
    wave_sync();
    // ---- walk in sorted order: runs summed in input order (core.py:116), then the
    //      reference's left-to-right totals over unique sources (core.py:107-144) -----
    uint32_t* outS = sS + lane * SST;                         // usid of unique j
    double* outW = reinterpret_cast<double*>(sP + lane * PST);  // weight of unique j
    double2 rc[RING];
    uint32_t pw[RING];
#pragma unroll
    for (int t = 0; t < RING && t < G; ++t) {
      const bool kv = key[t] != kSent32;
      const int sid = (int)(key[t] >> LOGG);
      const bool fst = kv && (t == 0 || sid != (int)(key[t - 1 > 0 ? t - 1 : 0] >> LOGG));
      if (fst) {
        rc[t] = a.relconf[sid];
        pw[t] = a.pbits[sid >> 5];
      } else {
        rc[t] = make_double2(0.5, 0.25);
        pw[t] = 0xffffffffu;
      }
    }
    double total = 0.0, ws = 0.0, cs = 0.0;
    double psum = 0.0;
    int cnt = 0, j = 0, psid = 0;
    double2 prc = make_double2(0.0, 0.0);
    uint32_t ppw = 0;
    auto finalize = [&]() {
      double avg = psum;
      if (ballot(cnt > 1)) {  // duplicates: avg = sum / len (core.py:116), rare
        if (cnt > 1) avg = psum / (double)cnt;
      }
      const double w = prc.x, c = prc.y;
      total += w;          // core.py:120
      ws += avg * w;       // core.py:135-137
      cs += c * w;         // core.py:141-143
      const unsigned cold = cold_flag(ppw, psid);
      outS[j] = (uint32_t)psid | cold;
      outW[j] = w;
      ++j;
    };
#pragma unroll
    for (int t = 0; t < G; ++t) {
      const bool kv = key[t] != kSent32;
      const int sid = (int)(key[t] >> LOGG);
      const bool fst = kv && (t == 0 || sid != (int)(key[t > 0 ? t - 1 : 0] >> LOGG));
      if (fst) {
        if (cnt > 0) finalize();
        psid = sid;
        prc = rc[t % RING];
        ppw = pw[t % RING];
        psum = 0.0 + sp[t];  // builtin sum() starts from int 0
        cnt = 1;
      } else if (kv) {
        psum += sp[t];
        ++cnt;
      }
      if (t + RING < G) {  // refill the ring slot just consumed
        const int tt = t + RING;
        const bool kv2 = key[tt] != kSent32;
        const int sid2 = (int)(key[tt] >> LOGG);
        const bool fst2 = kv2 && sid2 != (int)(key[tt - 1] >> LOGG);
        if (fst2) {
          rc[tt % RING] = a.relconf[sid2];
          pw[tt % RING] = a.pbits[sid2 >> 5];
        }
      }
    }
    if (cnt > 0) finalize();

    // ---- per-market results (lane = market: coalesced) ------------------------------
    if (mk >= 0) {
      store_market(a, mk, total, ws, cs, j);
      if (a.err_idx) a.err_idx[mk] = err;
    }
    sOff[lane] = off;
    sU[lane] = (mk >= 0) ? j : 0;
    sTot[lane] = total;
    wave_sync();

    // ---- per-unique outputs: MPI markets per iteration, lane = slot (coalesced) ------
    if ((a.usid || a.weight || a.nweight)) {
      const int slot = lane & (G - 1);
#pragma unroll 4
      for (int it = 0; it < G; ++it) {
        const int q = it * MPI + lane / G;
        if (slot < sU[q]) {
          const int64_t p = sOff[q] + slot;
          const double w = reinterpret_cast<const double*>(sP + q * PST)[slot];
          const double tot = sTot[q];
          if (a.usid) a.usid[p] = (int32_t)sS[q * SST + slot];
          if (a.weight) a.weight[p] = w;
          if (a.nweight) a.nweight[p] = norm_weight(w, tot);
        }
      }
    }
    wave_sync();
  }
}

// ------------------------------------------------------------------------------------
// contiguous markets, each wave loads its own tile: consensus_flat_kernel<G, TM, WPB>
// ------------------------------------------------------------------------------------
// list == NULL, every n <= G.  WPB independent waves per workgroup share only the present
// bitmask; each wave owns a tile of TM consecutive markets whose signals form ONE contiguous
// range [B, E):
//   1. B, E by scalar loads; the range is streamed into the wave's LDS image with 16-B
//      LDS-DMA (global_load_lds_dwordx4): ceil(TM*G*12 / 1 KiB) wave-instructions, no
//      per-market loop, no VGPR staging.
//   2. lane = market: its sids -> 32-bit keys (sid << log2 G | slot), Batcher odd-even
//      merge network in VGPRs.
//   3. walk in sorted order (branch-free): probability of the sorted slot from LDS,
//      duplicate runs summed in input order (core.py:115-116), one 16-B relconf gather
//      per position (ring RING ahead), and the reference's left-to-right totals over
//      unique sources (core.py:120, 135-143) gated by "last of its run".  The range
//      check of core.py:59-60 is the minimum failing slot.  Per unique j the packed
//      (sid | slot << 25) goes to the (dead) sid image at j and the weight over the
//      (consumed) probability cell of that slot.
//   4. per-market scalars (lane = market, coalesced); per-unique outputs with G/2 lanes
//      per market, two slots per lane: 8-B usid pairs and 16-B weight/nweight pairs.

// Per-unique outputs of one tile, lane = (market q, NPL slots from k2): NPL = 2 stores 8-B usid
// and 16-B weight / nweight pairs (every row at an even signal), NPL = 1 single slots.
template <int G, int TM, int NPL>
__device__ __forceinline__ void flat_copy_out(const ConsArgs& a, const TileRange& r, const uint32_t* iS,
                                              const double* iP, const int32_t* sU, const int32_t* sRs,
                                              const double* sTot, const uint32_t* sBits, bool bits_in_lds,
                                              int lane) {
  constexpr int LPM = G / NPL;       // lanes per market
  constexpr int MPX = kWave / LPM;   // markets per iteration
  const int dB = r.dB(), dP = r.dP();
  const int k2 = NPL * (lane % LPM);
#pragma unroll 1
  for (int it = 0; it < TM / MPX; ++it) {
    const int q = it * MPX + lane / LPM;
    const int u = sU[q];
    if (k2 < u) {
      const int rq = sRs[q];
      const double tot = sTot[q];
      const int64_t pos = r.B + rq + k2;
      const bool two = NPL == 2 && k2 + 1 < u;
      const Unique q0 = unpack_unique<G>(iS[dB + rq + k2]);
      const Unique q1 = unpack_unique<G>(two ? iS[dB + rq + k2 + 1] : 0u);
      const double w0 = iP[dP + rq + q0.slot];
      const double w1 = iP[dP + rq + q1.slot];
      const unsigned u0 = q0.sid | cold_flag(present_word(sBits, a.pbits, bits_in_lds, q0.sid), q0.sid);
      const unsigned u1 = two ? q1.sid | cold_flag(present_word(sBits, a.pbits, bits_in_lds, q1.sid), q1.sid) : 0u;
      const double n0 = norm_weight(w0, tot), n1 = norm_weight(w1, tot);
      if (two) {
        if (a.usid) *reinterpret_cast<uint2*>(a.usid + pos) = make_uint2(u0, u1);
        if (a.weight) *reinterpret_cast<double2*>(a.weight + pos) = make_double2(w0, w1);
        if (a.nweight) *reinterpret_cast<double2*>(a.nweight + pos) = make_double2(n0, n1);
      } else {
        if (a.usid) a.usid[pos] = (int32_t)u0;
        if (a.weight) a.weight[pos] = w0;
        if (a.nweight) a.nweight[pos] = n0;
      }
    }
  }
}

template <int G, int TM, int WPB>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(kFlatWPE, 8)))
void consensus_flat_kernel(ConsArgs a) {
  static_assert(TM == 32 || TM == 64, "markets per wave tile");
  constexpr int LOGG = lane_logg<G>();
  constexpr int TS = TM * G;           // max signals per tile
  constexpr int SW = TS + 8 + G;       // sid image (dwords): alignment slack, row overrun, sink
  constexpr int PW = TS + 4 + G;       // prob image (doubles)
  constexpr int RING = kFlatRing;

  __shared__ uint32_t sBits[kBitsLds];
  __shared__ __attribute__((aligned(16))) uint32_t sSid[WPB][SW];
  __shared__ __attribute__((aligned(16))) double sProb[WPB][PW];
  __shared__ double sTot[WPB][TM];
  __shared__ int32_t sU[WPB][TM];
  __shared__ int32_t sRs[WPB][TM];

  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool bits_in_lds = stage_present_bits(sBits, a, 64 * WPB);
  __syncthreads();  // the only workgroup barrier: waves are independent from here on

  uint32_t* const iS = sSid[w];
  double* const iP = sProb[w];
  const int64_t M = a.n_list;
  const int64_t n_tiles = (M + TM - 1) / TM;
  for (int64_t tile = (int64_t)blockIdx.x * WPB + w; tile < n_tiles; tile += (int64_t)gridDim.x * WPB) {
    const int64_t m0 = tile * TM;
    const int64_t m1 = (m0 + TM < M) ? m0 + TM : M;
    // B, E are wave-uniform: scalar loads
    const TileRange r = tile_range(a.offsets[m0], a.offsets[m1], a.n_signals);

    // ---- this lane's market ------------------------------------------------------------
    const int64_t mk = m0 + lane;
    const bool has = lane < TM && mk < M;
    int64_t off = r.B;
    int n = 0;
    if (has) {
      off = a.offsets[mk];
      n = (int)(a.offsets[mk + 1] - off);
    }
    screen_len<G>(n, a.fault);

    // ---- 1. stream [B, E) into the LDS image (16-B LDS-DMA, full chunks in bounds) -------
    for (int i = 0; i * kWave < r.nci; ++i) {
      const int c = i * kWave + lane;
      if (c < r.nci)
        __builtin_amdgcn_global_load_lds(a.sid + r.Bs + 4 * c,
                                         (__attribute__((address_space(3))) void*)(iS + i * 256), 16, 0, 0);
    }
    for (int i = 0; i * kWave < r.ncp; ++i) {
      const int c = i * kWave + lane;
      if (c < r.ncp)
        __builtin_amdgcn_global_load_lds(a.prob + r.Bp + 2 * c,
                                         (__attribute__((address_space(3))) void*)(iP + i * 128), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    copy_array_tail(r, a, iS, iP, lane);
    wave_sync_lds();

    // ---- 2. keys + sort ------------------------------------------------------------------
    const int rs = (int)(off - r.B);   // row start relative to B
    const int rsi = rs + r.dB();       // ... in the sid image
    const int rsp = rs + r.dP();       // ... in the prob image
    // (lane_keys' text, inline: through the call flat<16> ran 3.6 % and flat<32> 4.1 % slower,
    // measurements/consensus_lane_split_ab.txt)
    unsigned key[G];
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
    unsigned fb, lb, vb;
    run_masks<G>(key, n, fb, lb, vb);
    // ---- 3. walk: every input of every position in registers before the ordered sums -----
    wave_sync_lds();  // every lane has read its sids: rows may be rewritten
    double sp[G];
#pragma unroll
    for (int t = 0; t < G; ++t) sp[t] = iP[rsp + (int)(key[t] & (G - 1))];  // sentinel: slot G-1, in the image
    // gathers: index clamped into the table (sentinels and out-of-range sids never fault;
    // their values are never used), no per-position branch
    const unsigned smax = (unsigned)(a.n_sources > 0 ? a.n_sources - 1 : 0);
    const bool have_tab = a.n_sources > 0;
    constexpr int NG = (G < RING) ? G : RING;  // gathers in flight
    double2 ring[NG];
#pragma unroll
    for (int t = 0; t < NG; ++t) {
      const unsigned ix = min(key[t] >> LOGG, smax);
      ring[t] = (have_tab) ? a.relconf[ix] : make_double2(0.5, 0.25);
    }
    const int dumS = SW - 1, dumP = PW - 1;  // write sinks for invalid positions
    Walk k;
    int err = G;
#pragma unroll
    for (int t = 0; t < G; ++t) {
      const bool kv = __builtin_amdgcn_ubfe(vb, t, 1) != 0u;
      const unsigned sid = key[t] >> LOGG;
      const int slot = (int)(key[t] & (G - 1));
      const double p = sp[t];
      const double2 rc = ring[t % NG];
      if (t + NG < G) {
        const unsigned ix = min(key[t + NG < G ? t + NG : t] >> LOGG, smax);
        if (have_tab) ring[t % NG] = a.relconf[ix];
      }
      if (kv && (p < 0.0 || p > 1.0)) err = (slot < err) ? slot : err;  // core.py:59-60
      walk_step(k, t, fb, lb, p, rc, [&](int j) {  // the slot's probability is already in registers
        iS[kv ? rsi + j : dumS] = sid | ((unsigned)slot << kPackSlot);
        iP[kv ? rsp + slot : dumP] = rc.x;
      });
      asm volatile("" : "+v"(err));
      walk_pin(k);
    }

    // ---- 4a. per-market results --------------------------------------------------------
    if (has) {
      store_market(a, mk, k.total, k.ws, k.cs, k.j);
      if (a.err_idx) a.err_idx[mk] = (err < G) ? err : -1;
    }
    if (lane < TM) {
      sTot[w][lane] = k.total;
      sU[w][lane] = has ? k.j : 0;
      sRs[w][lane] = rs;
    }
    wave_sync_lds();

    // ---- 4b. per-unique outputs ---------------------------------------------------------
    if ((a.usid || a.weight || a.nweight)) {
      if (pair_store_ok(a, has, off, r.B))
        flat_copy_out<G, TM, 2>(a, r, iS, iP, sU[w], sRs[w], sTot[w], sBits, bits_in_lds, lane);
      else
        flat_copy_out<G, TM, 1>(a, r, iS, iP, sU[w], sRs[w], sTot[w], sBits, bits_in_lds, lane);
    }
    wave_sync_lds();  // the next tile's DMA overwrites the images
  }
}

// ------------------------------------------------------------------------------------
// consensus_pipe_kernel<G>: one loader wave + C compute waves per workgroup
// ------------------------------------------------------------------------------------
// Per workgroup (one per CU) an LDS ring of R tile slots:
//   loader wave   streams tile after tile into free slots with LDS-DMA, a FIXED number
//                 of 16-B wave-instructions per tile (lanes past the tile's range re-read
//                 its first chunk into the slot's slack), so `s_waitcnt vmcnt(NDMA)`
//                 publishes tile i-1 while tile i is still in flight (two tiles deep);
//   compute waves grab tiles in sequence (LDS counter), wait for the slot's ready flag,
//                 and run the flat kernel's arithmetic on it: keys + odd-even merge sort
//                 in VGPRs, the walk with 16 relconf gathers in flight and the sorted-slot
//                 probabilities read from the slot just ahead of use, per-unique results
//                 staged in place (packed sid|slot over the dead sid row, the weight over
//                 the consumed probability cell), coalesced copy-out with 16-B pairs, then
//                 release the slot.
// A compute wave never issues an LDS-DMA, so none of its waits covers one; the loader
// never touches registers the compute waves need.  Flags live in LDS (one workgroup).
// Progress: the loader only waits for the release of sequence i-R, which a compute wave
// is processing or has released (sequences are grabbed in order and R > C).
constexpr int kPipeRing = 16;  // relconf gathers in flight per compute lane

constexpr int kPipeC32 = 4;  // compute waves at G = 32
constexpr int kPipeR32 = 6;  // slots at G = 32 (LDS: ~25 KB each)
// Slots R >= C + 2: with one spare slot the ring is load-latency bound (a released slot
// must be refilled within tile_time / C); two spares keep two tiles in flight.
template <int G>
struct PipeCfg {
  static constexpr int L = 1;  // one loader wave (two measured slower: TA contention)
  static constexpr int C = (G == 32) ? kPipeC32 : 6;
  static constexpr int R = (G == 32) ? kPipeR32 : C + 3;
};

// global (not constant) address space: selected against the relconf argument, a constant
// pointer would turn the gathers into flat loads (vmcnt + lgkmcnt, out of order)
__device__ double2 kColdRow[1] = {{0.5, 0.25}};  // DEFAULT_RELIABILITY / _CONFIDENCE

// The workgroup's LDS: its shapes, a view of the arrays (declared in the kernel), and the flag
// protocol between the loader and the compute waves.
template <int G>
struct PipeLds {
  static constexpr int C = PipeCfg<G>::C, R = PipeCfg<G>::R, NL = PipeCfg<G>::L;
  static constexpr int TM = kWave;
  static constexpr int TS = TM * G;
  // Fixed DMA shape per tile: body instructions cover chunks [64k, 64k + 64) of the
  // tile's range, one tail instruction covers its LAST 64 chunks [n - 64, n) (the same
  // bytes again where they overlap), so the image is only as long as the largest range
  // and the wave-instruction count never depends on the data.
  static constexpr int SCH = (TS + 6) / 4 + 1;   // max 16-B sid chunks of a tile (misaligned start)
  static constexpr int PCH = (TS + 2) / 2 + 1;   // max 16-B prob chunks
  static constexpr int OCH = 2 * (TM + 1);       // offsets block dwords
  static constexpr int NSI = SCH / kWave + 1;    // body + tail
  static constexpr int NPI = PCH / kWave + 1;
  static constexpr int NOI = OCH / kWave + 1;
  static constexpr int NDMA = NSI + NPI + NOI;
  static_assert(NDMA < 64, "vmcnt field");
  static constexpr int SW = (4 * SCH > TS + 4 + G) ? 4 * SCH : TS + 4 + G;  // sid image dwords (row overrun)
  static constexpr int PW = (2 * PCH > TS + 4 + G) ? 2 * PCH : TS + 4 + G;  // prob image doubles
  static constexpr int OW = OCH + 2;
  static constexpr int BW = TS / 32 + 2;
  static_assert(4 * kWave * (NSI - 1) <= SW && 2 * kWave * (NPI - 1) <= PW && kWave * (NOI - 1) <= OW,
                "every body-instruction lane lands inside its image");

  uint32_t* sBits;
  uint32_t (*sSid)[SW];
  double (*sProb)[PW];
  uint32_t (*sOffs)[OW];
  int64_t* sTile;
  int* sReady;          // sequence + 1 once the slot holds it
  int* sFree;           // sequence + 1 once the slot's tile has been released
  int* sNext;
  uint32_t (*sBad)[BW];  // bit i: prob of tile position i outside [0, 1]
  uint4 (*sInfo)[TM];    // per market: {rs, u | n << 8 | rot << 16, total (lo, hi)}

  // by the whole workgroup, before its barrier
  __device__ __forceinline__ void init() const {
    if (threadIdx.x < R) {
      sReady[threadIdx.x] = 0;
      sFree[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) *sNext = 0;
  }
  // loader: sequence `seq` (tile t, or -1 = end marker) is in its slot
  __device__ __forceinline__ void publish(int seq, int64_t t) const {
    const int s = seq % R;
    // every lane stores the same words: no lane-0-only region inside the loop (the
    // structurizer splits loops around such regions and breaks wave-uniform state)
    sTile[s] = t;
    __hip_atomic_store(&sReady[s], seq + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  // loader: has sequence need - 1 been released from slot s?
  __device__ __forceinline__ bool is_free(int s, int need) const { return ldsflag(&sFree[s]) >= need; }
  // ... wait for it; false: gave up after spin_cap polls
  __device__ __forceinline__ bool wait_free(int s, int need, int spin_cap) const {
    int spins = 0;
    while (!is_free(s, need)) {
      __builtin_amdgcn_s_sleep(2);
      if (++spins > spin_cap) return false;
    }
    return true;
  }
  // compute wave: every lane takes a ticket (one aggregated ds_add of 64 per wave): the
  // wave's sequence number is its first ticket / 64
  __device__ __forceinline__ int grab_ticket() const {
    const int tk = __hip_atomic_fetch_add(sNext, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(tk) >> 6;
  }
  // compute wave: wait until slot s holds sequence seq; false: gave up after spin_cap polls
  __device__ __forceinline__ bool wait_ready(int s, int seq, int spin_cap) const {
    int spins = 0;
    while (ldsflag(&sReady[s]) != seq + 1) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > spin_cap) return false;
    }
    return true;
  }
  // compute wave: done with slot s
  __device__ __forceinline__ void release(int s, int seq) const {
    __hip_atomic_store(&sFree[s], seq + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

// Loader, once a tile's DMA has landed in slot s: the tail of the arrays that no 16-B chunk
// covers is loaded here, then validation (core.py:59-60) for the compute waves: every
// position's range check becomes one bit of sBad (ballot per 64 positions, contiguous
// conflict-free reads); NaN passes.
template <int G>
__device__ __forceinline__ void pipe_finish(const ConsArgs& a, const PipeLds<G>& L, int s, int64_t B, int64_t E,
                                            int lane) {
  const TileRange r = tile_range(B, E, a.n_signals);
  copy_array_tail(r, a, L.sSid[s], L.sProb[s], lane);
  wave_sync_lds();
  const int nb = (int)(E - B), d = r.dP();
#pragma unroll 4
  for (int k = 0; k < PipeLds<G>::TS / kWave; ++k) {
    const int i = k * kWave + lane;
    const double p = L.sProb[s][d + ((i < nb) ? i : 0)];
    const unsigned long long m = ballot(i < nb && (p < 0.0 || p > 1.0));
    L.sBad[s][2 * k] = (uint32_t)m;
    L.sBad[s][2 * k + 1] = (uint32_t)(m >> 32);
  }
  wave_sync_lds();
}

// Loader: issue the NDMA wave-instructions of one tile (markets [m0, m1), range r) into slot s.
// Body instruction k covers chunks [64k, 64k + 64) (lanes past the range re-read the first
// chunk into slack the range never reaches); once the range is exhausted a body instruction
// repeats instruction 0 (same bytes to the same places); the tail instruction covers the
// range's last 64 chunks (from 0 if it is shorter).
template <int G>
__device__ __forceinline__ void pipe_dma_tile(const ConsArgs& a, const PipeLds<G>& L, int s, const TileRange& r,
                                              int64_t m0, int64_t m1, int lane) {
  using P = PipeLds<G>;
  const int64_t Nf4 = a.n_signals & ~3ll, Nf2 = a.n_signals & ~1ll;
  const int64_t clamp_s = (Nf4 - 4 > 0) ? Nf4 - 4 : 0;  // host: n_signals >= 4
  const int64_t clamp_p = (Nf2 - 2 > 0) ? Nf2 - 2 : 0;
  const int nci = r.nci, ncp = r.ncp;
  const int ndw = (int)(2 * (m1 - m0 + 1));
  const int64_t fs = (r.Bs < clamp_s) ? r.Bs : clamp_s, fp = (r.Bp < clamp_p) ? r.Bp : clamp_p;
#pragma unroll
  for (int k = 0; k < P::NSI - 1; ++k) {
    const int kk = (k * kWave < nci) ? k : 0;
    const int c = kk * kWave + lane;
    dma_b128(a.sid + ((c < nci) ? r.Bs + 4 * c : fs), &L.sSid[s][kk * 256]);
  }
  {
    const int tb = (nci > kWave) ? nci - kWave : 0;
    const int c = tb + lane;
    dma_b128(a.sid + ((c < nci) ? r.Bs + 4 * c : fs), &L.sSid[s][tb * 4]);
  }
#pragma unroll
  for (int k = 0; k < P::NPI - 1; ++k) {
    const int kk = (k * kWave < ncp) ? k : 0;
    const int c = kk * kWave + lane;
    dma_b128(a.prob + ((c < ncp) ? r.Bp + 2 * c : fp), &L.sProb[s][kk * 128]);
  }
  {
    const int tb = (ncp > kWave) ? ncp - kWave : 0;
    const int c = tb + lane;
    dma_b128(a.prob + ((c < ncp) ? r.Bp + 2 * c : fp), &L.sProb[s][tb * 2]);
  }
  const uint32_t* og = reinterpret_cast<const uint32_t*>(a.offsets + m0);
#pragma unroll
  for (int k = 0; k < P::NOI - 1; ++k) {
    const int kk = (k * kWave < ndw) ? k : 0;
    const int d = kk * kWave + lane;
    dma_b32(og + ((d < ndw) ? d : 0), &L.sOffs[s][kk * 64]);
  }
  {
    const int tb = (ndw > kWave) ? ndw - kWave : 0;
    const int d = tb + lane;
    dma_b32(og + ((d < ndw) ? d : 0), &L.sOffs[s][tb]);
  }
}

// ================================ loaders =========================================
// loader w owns sequences i = w, w + NL, ... (slot i % R); k counts its own tiles
template <int G>
__device__ __forceinline__ void pipe_loader(const ConsArgs& a, const PipeLds<G>& L, int w, int lane,
                                            int64_t n_tiles) {
  using P = PipeLds<G>;
  constexpr int C = P::C, R = P::R, NL = P::NL, TM = P::TM, NDMA = P::NDMA;
  const int64_t M = a.n_list;
  int64_t tbB = 0, tbE = 0;
  auto load_bounds = [&](int64_t kbase) {
    const int64_t t = (int64_t)blockIdx.x + (w + (kbase + lane) * NL) * gridDim.x;
    if (t < n_tiles) {
      const int64_t m0 = t * TM;
      tbB = a.offsets[m0];
      tbE = a.offsets[(m0 + TM < M) ? m0 + TM : M];
    }
  };
  const int64_t my_tiles = (n_tiles > (int64_t)blockIdx.x) ? (n_tiles - 1 - blockIdx.x) / gridDim.x + 1 : 0;
  int pending = -1;  // sequence whose DMA is in flight and not yet published
  int64_t pend_t = -1, pend_B = 0, pend_E = 0;
  auto land = [&]() {  // the pending tile's DMA has landed
    pipe_finish<G>(a, L, pending % R, pend_B, pend_E, lane);
    L.publish(pending, pend_t);
  };
  for (int64_t i = w, k = 0; i < my_tiles + C; i += NL, ++k) {
    const int s = (int)(i % R);
    // wait for the release of sequence i - R (publish what is in flight first)
    if (i >= R) {
      const int need = (int)(i - R) + 1;
      if (!L.is_free(s, need)) {
        if (pending >= 0) {
          __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
          land();
          pending = -1;
        }
        if (!L.wait_free(s, need, a.spin_cap)) {  // never expected: bounded so a bug cannot hang the
          raise_fault(a.fault, kFaultSpinLoader);  // GPU, and reported (bce_fault_check)
          return;
        }
      }
    }
    if (i >= my_tiles) {  // end markers: one per compute wave
      if (pending >= 0) {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        land();
        pending = -1;
      }
      L.publish((int)i, -1);
      continue;
    }
    if ((k & 63) == 0) {
      load_bounds(k);
      __builtin_amdgcn_s_waitcnt(0x0F70);  // (drains in-flight DMA too; once per 64 tiles)
      if (pending >= 0) {
        land();
        pending = -1;
      }
    }
    const int64_t t = (int64_t)blockIdx.x + i * gridDim.x;
    const int64_t B = readlane_i64(tbB, (int)(k & 63)), E = readlane_i64(tbE, (int)(k & 63));
    const int64_t m0 = t * TM, m1 = (m0 + TM < M) ? m0 + TM : M;
    pipe_dma_tile<G>(a, L, s, tile_range(B, E, a.n_signals), m0, m1, lane);
    if (pending >= 0) {  // the previous tile has landed once only this one is in flight
      __builtin_amdgcn_s_waitcnt((NDMA & 15) | (7 << 4) | (15 << 8) | ((NDMA >> 4) << 14));
      land();
    }
    pending = (int)i;
    pend_t = t;
    pend_B = B;
    pend_E = E;
  }
  if (pending >= 0) {
    __builtin_amdgcn_s_waitcnt(0x0F70);
    land();
  }
}

// Compute wave: the walk over the lane's sorted keys (core.py:107-144 in sorted-source order),
// 16 relconf gathers in flight and the sorted-slot probabilities read PA positions ahead.
// Unique j is staged at row cell (j + lane) mod n: rows of equal length sit at a stride of n
// dwords, so cell j alone would put every lane on one bank (32-way); rotating by the lane
// (rotn) spreads them (cells < n only: neighbours' rows untouched).
template <int G>
__device__ __forceinline__ void pipe_walk(Walk& k, const unsigned (&key)[G], unsigned fb, unsigned lb, unsigned vb,
                                          const double2* tab, unsigned smax, uint32_t* iS, double* iP, int rsi,
                                          int rsp, int n, int rotn) {
  constexpr int LOGG = lane_logg<G>();
  constexpr int NG = (G < kPipeRing) ? G : kPipeRing;
  constexpr int PA = 4;          // probabilities read this many positions ahead
  double2 ring[NG];
#pragma unroll
  for (int t = 0; t < NG; ++t) {
    const unsigned ix = min(key[t] >> LOGG, smax);
    ring[t] = tab[ix];
  }
  double pq[PA];
#pragma unroll
  for (int t = 0; t < PA; ++t) pq[t] = iP[rsp + (int)(key[t] & (G - 1))];

  // single positions: valid, first AND last of their run -- on random ids ~97 % of all
  // positions, and at ~83 % of positions every lane of the wave is single
  unsigned sb = fb & lb & vb;
  asm volatile("" : "+v"(sb));
  auto rot = [&](int jj) { const int x = jj + rotn; return (x >= n) ? x - n : x; };
#pragma unroll
  for (int t = 0; t < G; ++t) {
    const unsigned sid = key[t] >> LOGG;
    const int slot = (int)(key[t] & (G - 1));
    const double p = pq[t % PA];
    if (t + PA < G) pq[t % PA] = iP[rsp + (int)(key[t + PA < G ? t + PA : t] & (G - 1))];
    const double2 rc = ring[t % NG];
    if (t + NG < G) {
      const unsigned ix = min(key[t + NG < G ? t + NG : t] >> LOGG, smax);
      ring[t % NG] = tab[ix];
    }
    const double wt = rc.x, cf = rc.y;
    const bool kv = __builtin_amdgcn_ubfe(vb, t, 1) != 0u;
    if (ballot(__builtin_amdgcn_ubfe(sb, t, 1) == 0u) == 0) {
      // every lane: a source seen once (avg = 0 + p) -- plain left-to-right adds
      k.total += wt;                      // core.py:120
      k.ws += p * wt;                     // core.py:135-137 (0 + p == p bit for bit,
      k.cs += cf * wt;                    //   except -0.0 -> +0.0, which * w changes nothing)
      iS[rsi + rot(k.j)] = sid | ((unsigned)slot << kPackSlot);
      iP[rsp + slot] = wt;
      k.j += 1;
    } else {
      walk_step(k, t, fb, lb, p, rc, [&](int j) {  // the slot's probability has been read
        if (kv) {
          iS[rsi + rot(j)] = sid | ((unsigned)slot << kPackSlot);
          iP[rsp + slot] = wt;
        }
      });
    }
    walk_pin(k);
  }
}

// Compute wave: per-unique outputs from the in-place staging.  lane = (market q, NPL slots
// from k2: 2 = slot pairs with 16-B stores, 1 = single slots), batches of CB iterations: the
// three dependent LDS round trips (info -> packed usid -> weight cell / present bit) are issued
// for the whole batch before any result is used, and no load sits under a branch.
template <int G, int NPL>
__device__ __forceinline__ void pipe_copy_out(const ConsArgs& a, const TileRange& tr, const uint32_t* iS,
                                              const double* iP, const uint4* info, const uint32_t* sBits,
                                              bool bits_in_lds, unsigned smax, int ln) {
  constexpr int TM = PipeLds<G>::TM;
  constexpr int LPM = G / NPL;               // lanes per market
  constexpr int MPX = kWave / LPM;           // markets per iteration
  constexpr int NIT = TM / MPX;
  constexpr int CB = (NIT < 4) ? NIT : 4;
  const int dB = tr.dB(), dP = tr.dP();
  const int k2 = NPL * (ln % LPM), g = ln / LPM;
#pragma unroll 1
  for (int i0 = 0; i0 < NIT; i0 += CB) {
    uint4 inf[CB];
#pragma unroll
    for (int b = 0; b < CB; ++b) inf[b] = info[(i0 + b) * MPX + g];
    int r[CB], c0[CB], c1[CB];
    bool v0[CB], v1[CB];
#pragma unroll
    for (int b = 0; b < CB; ++b) {
      r[b] = (int)inf[b].x;
      const int u = (int)(inf[b].y & 255u), nq = (int)((inf[b].y >> 8) & 255u), rq = (int)(inf[b].y >> 16);
      v0[b] = k2 < u;
      v1[b] = NPL == 2 && k2 + 1 < u;
      int x0 = k2 + rq;
      x0 -= (x0 >= nq) ? nq : 0;
      int x1 = x0 + 1;
      x1 -= (x1 >= nq) ? nq : 0;
      c0[b] = v0[b] ? x0 : 0;
      c1[b] = v1[b] ? x1 : 0;
    }
    unsigned pk0[CB], pk1[CB];
#pragma unroll
    for (int b = 0; b < CB; ++b) {
      pk0[b] = iS[dB + r[b] + c0[b]];
      pk1[b] = (NPL == 2) ? iS[dB + r[b] + c1[b]] : 0u;
    }
    double w0[CB], w1[CB];
    unsigned u0[CB], u1[CB], bw0[CB], bw1[CB];
#pragma unroll
    for (int b = 0; b < CB; ++b) {
      const Unique q0 = unpack_unique<G>(pk0[b]), q1 = unpack_unique<G>(pk1[b]);
      u0[b] = q0.sid;
      u1[b] = q1.sid;
      w0[b] = iP[dP + r[b] + q0.slot];
      w1[b] = (NPL == 2) ? iP[dP + r[b] + q1.slot] : 0.0;
      bw0[b] = present_word(sBits, a.pbits, bits_in_lds, min(u0[b], smax));
      bw1[b] = (NPL == 2) ? present_word(sBits, a.pbits, bits_in_lds, min(u1[b], smax)) : 0u;
    }
    // materialise the batch here: left alone, loads used only under the store
    // branches are sunk into them and serialise again
#pragma unroll
    for (int b = 0; b < CB; ++b) asm volatile("" : "+v"(w0[b]), "+v"(w1[b]), "+v"(bw0[b]), "+v"(bw1[b]));
#pragma unroll
    for (int b = 0; b < CB; ++b) {
      const double tot = __hiloint2double((int)inf[b].w, (int)inf[b].z);
      const unsigned x0 = u0[b] | cold_flag(bw0[b], min(u0[b], smax));
      const unsigned x1 = u1[b] | cold_flag(bw1[b], min(u1[b], smax));
      const double n0 = norm_weight(w0[b], tot), n1 = norm_weight(w1[b], tot);
      const int64_t pos = tr.B + r[b] + k2;
      if (v1[b]) {
        *reinterpret_cast<uint2*>(a.usid + pos) = make_uint2(x0, x1);
        *reinterpret_cast<double2*>(a.weight + pos) = make_double2(w0[b], w1[b]);
        *reinterpret_cast<double2*>(a.nweight + pos) = make_double2(n0, n1);
      } else if (v0[b]) {
        a.usid[pos] = (int32_t)x0;
        a.weight[pos] = w0[b];
        a.nweight[pos] = n0;
      }
    }
  }
}

// ================================ compute waves =====================================
template <int G>
__device__ __forceinline__ void pipe_compute(const ConsArgs& a, const PipeLds<G>& L, int cw, bool bits_in_lds) {
  using P = PipeLds<G>;
  constexpr int R = P::R, TM = P::TM;
  const int64_t M = a.n_list;
  const unsigned smax = (unsigned)(a.n_sources > 0 ? a.n_sources - 1 : 0);
  const double2* const tab = (a.n_sources > 0) ? a.relconf : kColdRow;
  for (;;) {
    const int seq = L.grab_ticket();
    const int s = seq % R;
    if (!L.wait_ready(s, seq, a.spin_cap)) {  // never expected: bounded so a bug cannot hang the
      raise_fault(a.fault, kFaultSpinCompute);  // GPU, and reported (bce_fault_check)
      return;
    }
    const int64_t tile0 = L.sTile[s];
    const int64_t tile = readfirstlane_i64(tile0);  // uniform
    if (tile < 0) {
      L.release(s, seq);
      break;
    }
    uint32_t* const iS = L.sSid[s];
    double* const iP = L.sProb[s];
    const uint32_t* const iO = L.sOffs[s];
    int ln = lane_id();
    asm volatile("" : "+v"(ln));  // per-tile addresses (no loop-invariant hoisting)
    const int64_t m0 = tile * TM;
    const int64_t mlast = ((m0 + TM < M) ? m0 + TM : M) - m0;
    const TileRange r = tile_range(((int64_t)iO[1] << 32) | iO[0],
                                   ((int64_t)iO[2 * mlast + 1] << 32) | iO[2 * mlast], a.n_signals);
    const int64_t mk = m0 + ln;
    const bool has = mk < M;
    int64_t off = r.B;
    int n = 0;
    if (has) {
      off = ((int64_t)iO[2 * ln + 1] << 32) | iO[2 * ln];
      n = (int)((((int64_t)iO[2 * ln + 3] << 32) | iO[2 * ln + 2]) - off);
    }
    screen_len<G>(n, a.fault);
    const int rs = (int)(off - r.B);
    const int rsi = rs + r.dB();
    const int rsp = rs + r.dP();

    // ---- keys + sort, run masks, walk ------------------------------------------------------
    unsigned key[G];
    lane_keys<G>(iS, rsi, n, has, key);
    unsigned fb, lb, vb;
    run_masks<G>(key, n, fb, lb, vb);
    wave_sync_lds();  // every lane has its sids: rows become usid staging
    const int rotn = (n > 0) ? ln % n : 0;
    Walk k;
    pipe_walk<G>(k, key, fb, lb, vb, tab, smax, iS, iP, rsi, rsp, n, rotn);

    // ---- per-market results --------------------------------------------------------------
    if (has) {
      store_market(a, mk, k.total, k.ws, k.cs, k.j);
      if (a.err_idx) {  // first bad input index (the loader's range-check bits)
        const int w0 = rs >> 5, sh = rs & 31;
        const uint32_t lo = L.sBad[s][w0], hi = L.sBad[s][w0 + 1];
        const uint32_t bits = ((sh ? (hi << (32 - sh)) : 0u) | (lo >> sh)) & vb;
        a.err_idx[mk] = bits ? (int)__builtin_ctz(bits) : -1;
      }
    }
    {
      const uint2 tb = *reinterpret_cast<const uint2*>(&k.total);
      L.sInfo[cw][ln] = make_uint4((unsigned)rs, (unsigned)(has ? k.j : 0) | ((unsigned)((n > 0) ? n : 1) << 8) |
                                                     ((unsigned)rotn << 16), tb.x, tb.y);
    }
    wave_sync_lds();

    // ---- per-unique outputs from the in-place staging ------------------------------------
    if (pair_store_ok(a, has, off, r.B))
      pipe_copy_out<G, 2>(a, r, iS, iP, L.sInfo[cw], L.sBits, bits_in_lds, smax, ln);
    else
      pipe_copy_out<G, 1>(a, r, iS, iP, L.sInfo[cw], L.sBits, bits_in_lds, smax, ln);
    wave_sync_lds();  // every read of the slot has returned
    L.release(s, seq);
  }
}

template <int G>
__global__ __launch_bounds__(64 * (PipeCfg<G>::C + PipeCfg<G>::L))
void consensus_pipe_kernel(ConsArgs a) {
  using P = PipeLds<G>;
  __shared__ uint32_t sBits[kBitsLds];
  __shared__ __attribute__((aligned(16))) uint32_t sSid[P::R][P::SW];
  __shared__ __attribute__((aligned(16))) double sProb[P::R][P::PW];
  __shared__ __attribute__((aligned(16))) uint32_t sOffs[P::R][P::OW];
  __shared__ int64_t sTile[P::R];
  __shared__ int sReady[P::R];
  __shared__ int sFree[P::R];
  __shared__ int sNext;
  __shared__ uint32_t sBad[P::R][P::BW];
  __shared__ uint4 sInfo[P::C][P::TM];
  const P L{sBits, sSid, sProb, sOffs, sTile, sReady, sFree, &sNext, sBad, sInfo};

  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool bits_in_lds = stage_present_bits(sBits, a, 64 * (P::C + P::NL));
  L.init();
  __syncthreads();  // the only workgroup barrier

  const int64_t n_tiles = (a.n_list + P::TM - 1) / P::TM;
  if (w < P::NL)
    pipe_loader<G>(a, L, w, lane, n_tiles);
  else
    pipe_compute<G>(a, L, w - P::NL, bits_in_lds);
}

}  // namespace bce

// ======================================================================================
// host launchers
// ======================================================================================
namespace bce {
namespace {

template <int G>
int launch_lpm(const ConsArgs& a, hipStream_t st) {
  return launch_persistent(consensus_lpm_kernel<G>, 64, 4, ceil_div(a.n_list, kWave), "consensus_lpm_kernel", a, st);
}

template <int G>
int launch_pipe(const ConsArgs& a, hipStream_t st) {
  return launch_persistent(consensus_pipe_kernel<G>, 64 * (PipeCfg<G>::C + PipeCfg<G>::L), 1, ceil_div(a.n_list, 64),
                           "consensus_pipe_kernel", a, st);
}

template <int G>
int launch_flat(const ConsArgs& a, hipStream_t st) {
  constexpr int TM = kFlatTM, WPB = kFlatWPB;
  return launch_persistent(consensus_flat_kernel<G, TM, WPB>, 64 * WPB, 2, ceil_div(ceil_div(a.n_list, TM), WPB),
                           "consensus_flat_kernel", a, st);
}

template <int G>
int launch_lane_g(LaneKernel k, const ConsArgs& a, hipStream_t st) {
  return k == LaneKernel::Lpm ? launch_lpm<G>(a, st) : k == LaneKernel::Flat ? launch_flat<G>(a, st) : launch_pipe<G>(a, st);
}

}  // namespace

int launch_lane(LaneKernel k, int G, const ConsArgs& a, hipStream_t st) {
  return G == 8 ? launch_lane_g<8>(k, a, st) : G == 16 ? launch_lane_g<16>(k, a, st) : launch_lane_g<32>(k, a, st);
}

}  // namespace bce
