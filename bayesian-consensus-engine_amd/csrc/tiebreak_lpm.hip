// tiebreak_lpm.hip -- the tie-break's lane-per-market kernel (markets of <= kTbLpmMax agents)
// and its launcher.  tiebreak_lpm_kernel is a tile loop over named pieces:
//   TbMeta / TbTiles  a tile's metadata, the PART 1 prefetch of the next tile's, and the
//                     PART 1/2 split words
//   TbStage           the wave's LDS buffer: contiguous, FULL and gathered-row staging, their
//                     flushes, and a lane's reads and writes of its own row
//   tb_full_body      the five phases over a FULL tile (PART 1)
// and the general body, the five phases over any other tile, which stays in the kernel (lifted
// it cost the exotic-precision kernels time; the note is at the block).
// (tiebreak.hip: the wave and block kernels and the C entries.)
#include <atomic>

#include "tiebreak_common.hpp"

#pragma clang fp contract(off)

namespace bce {

// n <= 32, lane = market (64 markets per wave): every per-market step runs in one lane's
// registers, so none of the wave kernel's serial readlane loops exist and a wave's
// instructions serve 64 markets at once.
//
// Data movement (STAGED, contiguous markets): a wave's 64 markets are one contiguous CSR
// range [B, E) of <= 2048 agents.  Every input array is read ONCE with coalesced 16-B loads
// into a wave-private LDS buffer (one pad slot per 32, so lanes reading their own rows hit
// distinct bank pairs), and every per-agent / per-group output is assembled in such a buffer
// and leaves with coalesced 16-B stores (per-lane scattered stores wrote each line ~4 times:
// 5.3 GB of HBM writes for the 1.3 GB of outputs).  A group's outputs go to slot g of the
// market's row, overwriting the input of agent g in place: group g ends only after every
// group <= g, and agent g belongs to one of those (ordinals are assigned in first-seen
// order, so agent g's ordinal is <= g) -- its input has been consumed.  Slots g >= n_groups
// of a market's row receive unspecified values (include/bce.h).
// (The !STAGED path, for market lists, reads rows and writes outputs per lane.)
// Per lane:
//   1. keys round(pred, precision) (tiebreak.py:54) and each agent's group ordinal in
//      first-seen (dict insertion) order: O(n^2) key compares, == semantics (-0.0 == 0.0,
//      NaN never equal); keys (ordinal << 5 | agent) sorted by the odd-even merge network
//      with the rounded key as payload: every group becomes a run, groups in first-seen
//      order, members in input order;
//   2. walk (weight, reliability): the group's weight sum runs in input order from +0.0
//      (builtin sum from int 0), builtin max keeps the first maximum; at a run's end the
//      winner (lexicographic max of (density, max_rel, -key), tiebreak.py:113-117) and the
//      top-two tie flag (tiebreak.py:123-133) are updated;
//   3. variance (tiebreak.py:108-110; mean, then the squares -- libm pow restated,
//      glibc_pow.hpp -- summed in input order) and the per-group confidence sums.
constexpr int kTbLpmWaves = 4;
constexpr int kTbStage = 64 * kTbLpmMax + 64;  // doubles per wave buffer: a tile's agents + pads
constexpr int kTbStageIt = 64 * kTbLpmMax / 128;  // 16-B loads per lane for a full tile
constexpr int kTbStageBatch = 4;                  // of them in flight together (2 x 8 VGPRs each)
// A STAGED tile's arrays reach LDS as 16-B loads into registers, kTbStageBatch in flight, then
// ds_writes (two workgroups of four waves per CU).  LDS-DMA staging into the one buffer (1.070 vs
// 0.849-0.866 ms, profiles/archive/r04f/) and two DMA-filled buffers per wave (one workgroup per CU:
// 1.316 ms, profiles/archive/r04e/) were measured and removed.

__device__ __forceinline__ int tb_pad(int i) { return i + (i >> 5); }
constexpr bool kTbFullKeysInLds = true;  // FULL tiles: sort (ordinal, agent) alone, keys via LDS
// the staged general body likewise: tie-break over 1M ragged markets 0.7347-0.7364 -> 0.7201-0.7218
// ms, three interleaved reps (profiles/r06tb/)
constexpr bool kTbGeneralKeysInLds = true;
constexpr int kTbGatherBatch = 8;  // GATHER staging: passes whose row loads are in flight together
constexpr int kTbDump = 64;
// FULL tiles: 16-B loads per lane in flight while staging the predictions / confidences and the
// weights / reliabilities (8 for the latter spills ~10 VGPRs around those stages and still
// wins: 0.662 vs 0.688 ms with stage()'s 4, profiles/archive/r04q/)
constexpr int kTbFullBatchPC = 8;
constexpr int kTbFullBatchWR = 8;
constexpr bool kTbPrefetchMeta = true;
constexpr bool kTbFullKernel = true;  // FULL tiles get a launch of their own (PART 1, then PART 2)
// (FULL tiles, measured and removed: the next array's first batch issued before the phase's
// output flushes -- 36 spilled VGPRs, 0.712-0.716 vs 0.664 ms, profiles/archive/r04aa/; dword touches of
// the next phase's array -- -0.5% time for +27% FETCH_SIZE, profiles/archive/r04k/, archive/r04m/.)
// nontemporal hints on the staged input loads / the flushed output stores (both off: 0.727-0.730
// ms vs 0.712 for the 1M x 32 line, profiles/archive/r04j/)
constexpr bool kTbNtLoad = true;
constexpr bool kTbNtStore = true;
typedef double tb_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 tb_ld2(const double* p) {
  const tb_d2 v = kTbNtLoad ? __builtin_nontemporal_load(reinterpret_cast<const tb_d2*>(p))
                            : *reinterpret_cast<const tb_d2*>(p);
  return make_double2(v.x, v.y);
}
__device__ __forceinline__ void tb_st2(double* p, double x, double y) {
  tb_d2 v;
  v.x = x;
  v.y = y;
  if constexpr (kTbNtStore) __builtin_nontemporal_store(v, reinterpret_cast<tb_d2*>(p));
  else *reinterpret_cast<tb_d2*>(p) = v;
}  // per-lane sink slots after a wave buffer (FULL tiles' masked stores)

// A per-lane bit set hidden from the compiler: each phase re-derives its run-boundary
// compares from it instead of keeping 32 lane masks (64 SGPRs) alive across the tile.
__device__ __forceinline__ unsigned tb_bits(unsigned m) {
  asm volatile("" : "+v"(m));
  return m;
}

// The rare exact square (pow2_fast's near-midpoint cases) out of line: inlined, its log/exp
// polynomial constants were hoisted out of the tile loop and held in (spilled) registers.
__device__ __noinline__ double tb_pow2_full(double d) { return bce_pow::pow2_full(d); }

constexpr int kTbLpmWPE = 2;  // waves per SIMD (VGPR budget 256)
// GATHER kernels size their buffers for NP positions per lane; the 8-position body fits 128
// VGPRs, so four waves per SIMD (LDS: four workgroups of 4 x 4.2 KB per CU)
constexpr int tb_wpe(int np, bool gather) { return (gather && np == 8) ? 4 : kTbLpmWPE; }  // (EXOTIC: 2)
constexpr int tb_stage(int np, bool gather) { return gather ? 64 * np + 2 * np + 8 : kTbStage + kTbDump; }

// a tile's metadata: this lane's market and the tile's agent range [B, B + cnt)
struct TbMeta {
  int64_t m, off;
  int n;
  bool has;
  int64_t B;
  int cnt;
  int skip;  // 0 process, 1 every market empty, 2 a market longer than kTbLpmMax inside
  bool full;  // every lane holds a market of exactly kTbLpmMax agents
};

// A wave's walk over its tiles (64 list entries each): meta_of reads a tile's metadata,
// meta_pre loads the next tile's ahead of time, split_run / split_leave are the PART 1/2
// hand-over.
template <bool STAGED, int PART, int NP, bool GATHER>
struct TbTiles {
  static constexpr bool kFullBody = PART == 1;
  const TbArgs& a;
  const int32_t* list;
  int64_t n_list;
  int* fault;
  int lane;
  // PART 1: the next tile's two offsets per lane are loaded while this tile's confidences are
  // processed (kTbPrefetchMeta), so its meta costs no round trip of its own
  int64_t pre_o0 = 0, pre_o1 = 0;
  bool pre = false;
  __device__ __forceinline__ void meta_pre(int64_t tile) {
    const int64_t li = tile * 64 + lane;
    const bool h = tile * 64 < n_list && li < n_list;
    pre_o0 = h ? a.offsets[li] : 0;
    pre_o1 = h ? a.offsets[li + 1] : 0;
    pre = true;
  }
  __device__ __forceinline__ TbMeta meta_of(int64_t tile) {
    TbMeta t{};
    const int64_t li = tile * 64 + lane;
    t.has = tile * 64 < n_list && li < n_list;
    t.m = t.has ? (list ? (int64_t)list[li] : li) : 0;
    if (kFullBody && pre) {  // (STAGED: m = li)
      t.off = pre_o0;
      t.n = (int)(pre_o1 - pre_o0);
      pre = false;
    } else {
      t.off = t.has ? a.offsets[t.m] : 0;
      t.n = t.has ? (int)(a.offsets[t.m + 1] - t.off) : 0;
    }
    if (ballot(t.n > NP || t.n < 0)) {
      raise_fault(fault, kFaultTooLong);
      if (t.n > NP || t.n < 0) t.n = 0;
    }
    if (!ballot(t.n > 0)) {
      t.skip = 1;
      return t;
    }
    if constexpr (GATHER) return t;  // rows are copied one by one: no tile range
    // STAGED: the tile's agents [B, E) (lane 0's market starts it, the last lane's ends it)
    t.B = readfirstlane_i64(t.off);
    const int last_lane = 63 - __builtin_clzll(ballot(t.has));
    const int64_t E = readlane_i64(t.off + t.n, last_lane);
    t.cnt = (int)(E - t.B);  // <= 64 * 32 unless a market inside [B, E) was too long
    // (PART 1 launches only with 16-B aligned arrays, so an even B aligns every row load)
    t.full = ballot(t.has && t.n == kTbLpmMax) == ~0ull && (t.B & 1) == 0;
    // a market longer than kTbLpmMax (already faulted and zeroed above) still lies inside
    // [B, E): staging the range would run past this wave's buffer, so the tile is skipped
    // (every market gets the empty marker; the fault word reports the call as failed)
    if (STAGED && (E - t.B > 64 * kTbLpmMax || E < t.B)) {
      raise_fault(fault, kFaultTooLong);
      t.skip = 2;
    }
    return t;
  }
  // PART 2 has nothing to do when PART 1 found every tile full (the common uniform batch):
  // it then only counts itself out
  // (one word per wave: a single flag word took every skipping wave's store through the
  // device-coherent path to one address -- 0.55 ms of serialised stores on a ragged batch)
  // Words are shared round-robin by launch pairs (capi.hip split_slot), possibly on other
  // streams: PART 1 raises its word to its ticket with atomicMax, and PART 2 runs when the word
  // holds its own ticket or a NEWER pair's (then it may run for nothing -- it skips FULL tiles
  // itself -- but never skips a tile its own PART 1 left).  Tickets are positive and
  // increase; after a wrap split_slot clears the slot before the first pair that reuses it.
  __device__ __forceinline__ bool split_run(int64_t wave) const {
    if constexpr (PART == 2) return a.split[wave] >= a.ticket;
    return true;
  }
  // PART 1: this wave left a tile to PART 2
  __device__ __forceinline__ void split_leave(int64_t wave) const {
    if (lane == 0) atomicMax(&a.split[wave], a.ticket);
  }
};

// One tile in the wave's LDS buffer (STAGED), or this lane's row in global memory (!STAGED).
// stage / stage_full bring an input array in, the phases read it with at() and write a
// group's or an agent's output with put() / put_i32(), flush / flush_i32 send the buffer out.
template <bool STAGED, int NP, bool GATHER>
struct TbStage {
  double* const buf;      // the wave's buffer (padded: tb_pad)
  int32_t* const ibuf;
  int64_t* const rowOff;  // GATHER: every lane's row start and length, for the row-segment copies
  int* const rowN;
  const int lane;
  const int64_t off;  // this lane's market
  const int n;
  const int64_t B;  // the tile's agents [B, B + cnt_tile) (contiguous staging)
  const int cnt_tile;
  // this lane's row in the staged buffer (GATHER: a fixed row of NP slots per lane)
  const int lrow;
  // every lane reads inside its own row (positions past n re-read the last agent); a lane
  // with an empty market reads the tile's first agent (masked later)
  const int rbase;
  const int64_t gbase;
  __device__ __forceinline__ TbStage(double* buf_, int64_t* rowOff_, int* rowN_, int lane_, const TbMeta& t)
      : buf(buf_), ibuf(reinterpret_cast<int32_t*>(buf_)), rowOff(rowOff_), rowN(rowN_), lane(lane_),
        off(t.off), n(t.n), B(t.B), cnt_tile(t.cnt), lrow(GATHER ? NP * lane_ : (int)(t.off - t.B)),
        rbase(t.n > 0 ? lrow : 0), gbase(t.n > 0 ? t.off : t.B) {}
  // GATHER: publish this tile's rows to the wave
  __device__ __forceinline__ void rows_set() const {
    wave_sync_lds();  // the previous tile's row table readers are done
    rowOff[lane] = off;
    rowN[lane] = n;
    wave_sync_lds();
  }
  // GATHER: row r's agents [0, cnt) <-> global [off_r, off_r + cnt) as 16-B aligned pairs:
  // NP / 2 lanes per row, lane c of a row owns the pair starting at agent 2c - (off_r & 1)
  // (the row's aligned start), 64 / (NP / 2) rows per pass, NP / 2 passes -- one 16-B access
  // per lane and pass, as many as the contiguous staging of a full tile.  A 32-agent row
  // starting at an odd agent has one agent past its last pair (`tail`).  body(r, i, ro, rn)
  // gets the row's agent index i of the pair's first element (-1 .. NP - 1).
  static constexpr int kGL = NP / 2, kGR = 64 / kGL;
  template <class F>
  __device__ __forceinline__ void rows_copy(F&& body) const {
#pragma unroll 4
    for (int pass = 0; pass < kGL; ++pass) {
      const int r = pass * kGR + lane / kGL, c = lane % kGL;
      const int64_t ro = rowOff[r];
      body(r, 2 * c - (int)(ro & 1), ro, rowN[r]);
    }
  }
  template <class F>
  __device__ __forceinline__ void rows_tail(F&& body) const {  // agent NP of an odd-start NP-agent row, one lane each
    const int r = lane;
    const int64_t ro = rowOff[r];
    if ((ro & 1) && rowN[r] == NP) body(r, NP - 1, ro);
  }
  // global [B, E) -> LDS (padded), coalesced 16-B loads issued kTbStageBatch at a time
  // before any is written to LDS: one memory round trip per batch, not one per load (the
  // per-iteration loop paid ~16 serial HBM latencies per array and tile)
  __device__ __forceinline__ void stage(const double* src) const {
    wave_sync_lds();  // the buffer's previous readers (this wave) are done
    if constexpr (GATHER) {
      // kTbGatherBatch passes' loads issued before any is written to LDS: the loads are
      // unconditional (a pair outside its row reads agent 0 of the array, never used), so
      // they leave back to back -- one memory round trip per batch instead of one per pass
      constexpr int K = kGL < kTbGatherBatch ? kGL : kTbGatherBatch;
#pragma unroll 1
      for (int p0 = 0; p0 < kGL; p0 += K) {
        double2 v[K];
        int rr[K], ii[K], nn[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int r = (p0 + k) * kGR + lane / kGL, c = lane % kGL;
          const int64_t ro = rowOff[r];
          const int rn = rowN[r];
          const int i = 2 * c - (int)(ro & 1);
          const bool touch = i + 1 >= 0 && i < rn;  // the pair [i, i + 1] touches the row
          v[k] = tb_ld2(src + (touch ? ro + i : 0));  // 16-B aligned: ro + i is even
          rr[k] = r;
          ii[k] = i;
          nn[k] = touch ? rn : 0;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
          if (ii[k] >= 0 && ii[k] < nn[k]) buf[tb_pad(NP * rr[k] + ii[k])] = v[k].x;
          if (ii[k] + 1 >= 0 && ii[k] + 1 < nn[k]) buf[tb_pad(NP * rr[k] + ii[k] + 1)] = v[k].y;
        }
      }
      rows_tail([&](int r, int i, int64_t ro) { buf[tb_pad(NP * r + i)] = src[ro + i]; });
      wave_sync_lds();
      return;
    }
    if (((uintptr_t)(src + B) & 15) == 0) {
#pragma unroll 1
      for (int k0 = 0; k0 < kTbStageIt; k0 += kTbStageBatch) {
        if (k0 * 128 >= cnt_tile) break;  // wave-uniform
        double2 v[kTbStageBatch];
#pragma unroll
        for (int k = 0; k < kTbStageBatch; ++k) {
          const int e = 2 * lane + 128 * (k0 + k);
          v[k] = make_double2(0.0, 0.0);
          if (e + 1 < cnt_tile) v[k] = tb_ld2(src + B + e);
        }
#pragma unroll
        for (int k = 0; k < kTbStageBatch; ++k) {
          const int e = 2 * lane + 128 * (k0 + k);
          if (e + 1 < cnt_tile) {
            buf[tb_pad(e)] = v[k].x;
            buf[tb_pad(e + 1)] = v[k].y;
          }
        }
      }
      if ((cnt_tile & 1) && lane == 0) buf[tb_pad(cnt_tile - 1)] = src[B + cnt_tile - 1];  // odd tail
    } else {
#pragma unroll 1
      for (int k0 = 0; k0 < 2 * kTbStageIt; k0 += 2 * kTbStageBatch) {
        if (k0 * 64 >= cnt_tile) break;  // wave-uniform
        double v[2 * kTbStageBatch];
#pragma unroll
        for (int k = 0; k < 2 * kTbStageBatch; ++k) {
          const int e = lane + 64 * (k0 + k);
          v[k] = 0.0;
          if (e < cnt_tile) v[k] = src[B + e];
        }
#pragma unroll
        for (int k = 0; k < 2 * kTbStageBatch; ++k) {
          const int e = lane + 64 * (k0 + k);
          if (e < cnt_tile) buf[tb_pad(e)] = v[k];
        }
      }
    }
    wave_sync_lds();
  }
  // FULL tiles (2048 agents): no bounds checks, NB 16-B loads per lane in flight
  // (src + B is 16-B aligned: see TbMeta::full)
  template <int NB>
  __device__ __forceinline__ void stage_full(const double* src) const {
    wave_sync_lds();
#pragma unroll 1
    for (int k0 = 0; k0 < kTbStageIt; k0 += NB) {
      double2 v[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] = tb_ld2(src + B + 2 * lane + 128 * (k0 + k));
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const int e = 2 * lane + 128 * (k0 + k);
        buf[tb_pad(e)] = v[k].x;
        buf[tb_pad(e + 1)] = v[k].y;
      }
    }
    wave_sync_lds();
  }
  // LDS (padded) -> global [B, E), coalesced 16-B stores
  __device__ __forceinline__ void flush(double* dst) const {
    wave_sync_lds();
    if constexpr (GATHER) {
      // a pair wholly inside the row leaves as one 16-B store; a pair the row shares with
      // its neighbour writes only its own agent
      rows_copy([&](int r, int i, int64_t ro, int rn) {
        if (i >= 0 && i + 1 < rn) {
          tb_st2(dst + ro + i, buf[tb_pad(NP * r + i)], buf[tb_pad(NP * r + i + 1)]);
        } else {
          if (i >= 0 && i < rn) dst[ro + i] = buf[tb_pad(NP * r + i)];
          if (i + 1 >= 0 && i + 1 < rn) dst[ro + i + 1] = buf[tb_pad(NP * r + i + 1)];
        }
      });
      rows_tail([&](int r, int i, int64_t ro) { dst[ro + i] = buf[tb_pad(NP * r + i)]; });
      wave_sync_lds();
      return;
    }
    const bool al = ((uintptr_t)(dst + B) & 15) == 0;
    for (int e = 2 * lane; e < cnt_tile; e += 128) {
      if (al && e + 1 < cnt_tile) {
        tb_st2(dst + B + e, buf[tb_pad(e)], buf[tb_pad(e + 1)]);
      } else {
        dst[B + e] = buf[tb_pad(e)];
        if (e + 1 < cnt_tile) dst[B + e + 1] = buf[tb_pad(e + 1)];
      }
    }
    wave_sync_lds();  // the buffer's next writers (this wave) come after these reads
  }
  __device__ __forceinline__ void flush_i32(int32_t* dst) const {
    wave_sync_lds();
    if constexpr (GATHER) {
      rows_copy([&](int r, int i, int64_t ro, int rn) {
        if (i >= 0 && i < rn) dst[ro + i] = ibuf[tb_pad(NP * r + i)];
        if (i + 1 >= 0 && i + 1 < rn) dst[ro + i + 1] = ibuf[tb_pad(NP * r + i + 1)];
      });
      rows_tail([&](int r, int i, int64_t ro) { dst[ro + i] = ibuf[tb_pad(NP * r + i)]; });
      wave_sync_lds();
      return;
    }
    const bool al = ((uintptr_t)(dst + B) & 15) == 0;
    for (int e = 4 * lane; e < cnt_tile; e += 256) {
      if (al && e + 3 < cnt_tile) {
        *reinterpret_cast<int4*>(dst + B + e) =
            make_int4(ibuf[tb_pad(e)], ibuf[tb_pad(e + 1)], ibuf[tb_pad(e + 2)], ibuf[tb_pad(e + 3)]);
      } else {
        for (int q = 0; q < 4 && e + q < cnt_tile; ++q) dst[B + e + q] = ibuf[tb_pad(e + q)];
      }
    }
    wave_sync_lds();  // (as flush: the int32 reads are fenced before the next double writes)
  }
  // agent t of this lane's market
  __device__ __forceinline__ double at(const double* src, int t) const {
    if constexpr (STAGED) return buf[tb_pad(rbase + t)];
    else return src[gbase + t];
  }
  // this lane's slot g (an agent's or a group's output)
  __device__ __forceinline__ void put(double* dst, int g, double v) const {
    if constexpr (STAGED) buf[tb_pad(lrow + g)] = v;
    else dst[off + g] = v;
  }
  __device__ __forceinline__ void put_i32(int32_t* dst, int g, int v) const {
    if constexpr (STAGED) ibuf[tb_pad(lrow + g)] = v;
    else dst[off + g] = v;
  }
};

// ---- FULL tile: 64 markets of exactly kTbLpmMax agents, lane L's row at 33 L ------------
// The same four phases as below with n a compile-time 32: no per-position validity masks,
// row reads at immediate offsets (or one shift-add for a sorted position), and every
// conditional store a store to a selected address (the lane's sink slot when masked).
// m: this lane's market; next: the wave's next tile (its offsets are loaded in phase 5).
template <class Stage, class Tiles>
__device__ __forceinline__ void tb_full_body(const TbArgs& a, const Stage& s, Tiles& tiles, const double* sRc,
                                             int64_t m, int64_t next) {
  constexpr int N = kTbLpmMax;
  double* row = s.buf + 33 * s.lane;
  int32_t* irow = s.ibuf + 33 * s.lane;
  double* sink = s.buf + kTbStage + s.lane;
  int32_t* isink = s.ibuf + 2 * kTbStage + s.lane;
  auto put_sel = [&](unsigned bits, int p, unsigned g, double v) {
    *(((bits >> p) & 1u) ? row + g : sink) = v;
  };
  auto put_sel_i32 = [&](unsigned bits, int p, unsigned g, int v) {
    *(((bits >> p) & 1u) ? irow + g : isink) = v;
  };
  unsigned u[N];
  // each phase re-derives its row addresses from u (CSE across phases kept 64 address
  // registers alive through the tile and spilled)
  auto refresh_u = [&]() {
#pragma unroll
    for (int p = 0; p < N; ++p) u[p] = tb_bits(u[p]);
  };
  // 1. keys, first-seen ordinals, sort
  s.template stage_full<kTbFullBatchPC>(a.pred);
  double kp[N];  // (PART 1 runs only for round mode 0, see launch_tb_lpm)
#pragma unroll
  for (int t = 0; t < N; ++t) {
    bool slow;
    kp[t] = py_round_nd_fast(row[t], a.rscale, a.rinv, a.rthresh, slow);
    if (ballot(slow)) kp[t] = slow ? py_round_nd_sel(row[t], a.rscale, a.rinv, a.rthresh) : kp[t];
  }
  int ngf = 0;
  {
    int go[N];
#pragma unroll
    for (int t = 0; t < N; ++t) {
      int g = -1;
#pragma unroll
      for (int s2 = 0; s2 < t; ++s2) g = key_eq(kp[s2], kp[t]) ? go[s2] : g;
      go[t] = g < 0 ? ngf : g;
      ngf += g < 0 ? 1 : 0;
      u[t] = ((unsigned)go[t] << 5) | (unsigned)t;
    }
    if (a.g_of) {
      wave_sync_lds();
#pragma unroll
      for (int t = 0; t < N; ++t) irow[t] = go[t];
      s.flush_i32(a.g_of);
    }
  }
  // run boundaries: bit p of stm / enm = a run starts / ends at sorted position p
  unsigned stm = 1u, enm = 1u << (N - 1);
  if constexpr (kTbFullKeysInLds) {
    // the rounded keys wait in the lane's row while only the 32-bit (ordinal, agent)
    // keys go through the network; each sorted position then reads its run head's key
    wave_sync_lds();
#pragma unroll
    for (int t = 0; t < N; ++t) row[t] = kp[t];
    oem_sort(u);
#pragma unroll
    for (int p = 1; p < N; ++p) {
      const unsigned d = ((u[p] >> 5) != (u[p - 1] >> 5)) ? 1u : 0u;
      stm |= d << p;
      enm |= d << (p - 1);
    }
    unsigned ht = u[0] & 31u;
    kp[0] = row[ht];
#pragma unroll
    for (int p = 1; p < N; ++p) {
      ht = ((stm >> p) & 1u) ? (u[p] & 31u) : ht;
      kp[p] = row[ht];
    }
  } else {
    oem_sort_kv(u, kp);
#pragma unroll
    for (int p = 1; p < N; ++p) {
      const unsigned d = ((u[p] >> 5) != (u[p - 1] >> 5)) ? 1u : 0u;
      stm |= d << p;
      enm |= d << (p - 1);
    }
#pragma unroll
    for (int p = 1; p < N; ++p) kp[p] = ((stm >> p) & 1u) ? kp[p] : kp[p - 1];  // run head's key
  }
  // 2. group keys and counts
  if (a.g_key) {
    wave_sync_lds();
    const unsigned en_ = tb_bits(enm);
    refresh_u();
#pragma unroll
    for (int p = 0; p < N; ++p) put_sel(en_, p, u[p] >> 5, kp[p]);
    s.flush(a.g_key);
  }
  if (a.g_count) {
    wave_sync_lds();
    const unsigned st_ = tb_bits(stm), en_ = tb_bits(enm);
    refresh_u();
    int cnt = 0;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      cnt = (((st_ >> p) & 1u) ? 0 : cnt) + 1;
      put_sel_i32(en_, p, u[p] >> 5, cnt);
    }
    s.flush_i32(a.g_count);
  }
  // 3. densities
  double densp[N];
  s.template stage_full<kTbFullBatchWR>(a.weight);
  {
    const unsigned st_ = tb_bits(stm), en_ = tb_bits(enm);
    refresh_u();
    double tot = 0.0;
    int cnt = 0;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      const bool st = (st_ >> p) & 1u;
      tot = (st ? 0.0 : tot) + row[u[p] & 31u];  // tiebreak.py:60, sum from int 0
      cnt = (st ? 0 : cnt) + 1;
      densp[p] = tb_div_small(tot, cnt, sRc);
      put_sel(en_, p, u[p] >> 5, densp[p]);
    }
    if (a.g_density) s.flush(a.g_density);
  }
  // 4. max reliability per group, the winner and the tie flag
  double bd = 0.0, bm = 0.0, bk = 0.0;
  bool tie = false;
  s.template stage_full<kTbFullBatchWR>(a.rel);
  {
    const unsigned st_ = tb_bits(stm), en_ = tb_bits(enm);
    refresh_u();
    double mx = 0.0;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      const unsigned g = u[p] >> 5;
      const double r = row[u[p] & 31u];
      mx = ((st_ >> p) & 1u) ? r : ((r > mx) ? r : mx);  // tiebreak.py:62
      put_sel(en_, p, g, mx);
      const bool en = (en_ >> p) & 1u;
      const double dens = densp[p];
      const bool same = (dens == bd) && (mx == bm);
      const bool better = (g == 0) | tb_better_sel(dens, mx, kp[p], bd, bm, bk);  // tiebreak.py:113-117
      tie = en ? (better ? ((g != 0) && same) : (tie || same)) : tie;     // tiebreak.py:123-133
      const bool upd = en && better;
      bd = upd ? dens : bd;
      bm = upd ? mx : bm;
      bk = upd ? kp[p] : bk;
    }
    if (a.g_maxrel) s.flush(a.g_maxrel);
  }
  // 5. variance (input order), per-group mean confidences
  s.template stage_full<kTbFullBatchPC>(a.conf);
  if (kTbPrefetchMeta && next * 64 < tiles.n_list) tiles.meta_pre(next);
  double variance;
  {
    double cs = 0.0;
#pragma unroll
    for (int t = 0; t < N; ++t) cs += row[t];
    const double mean = cs / (double)N;
    // squares summed as they come (no array of 32): the fast square is exact unless
    // flagged; a lane with a flagged square redoes the ordered sum with exact ones
    wave_sync_lds();  // re-read the confidences instead of holding all 32
    double vs = 0.0;
    unsigned slow = 0;
#pragma unroll
    for (int t = 0; t < N; ++t) {
      bool ok;
      vs += bce_pow::pow2_fast(row[t] - mean, ok);
      slow |= ok ? 0u : (1u << t);
    }
    if (slow) {
      vs = 0.0;
#pragma unroll 1
      for (int t = 0; t < N; ++t) {
        const double d = row[t] - mean;
        bool ok;
        const double q = bce_pow::pow2_fast(d, ok);
        vs += ((slow >> t) & 1u) ? tb_pow2_full(d) : q;
      }
    }
    variance = vs / (double)N;
  }
  if (a.g_avgconf) {
    const unsigned st_ = tb_bits(stm), en_ = tb_bits(enm);
    refresh_u();
    double gcs = 0.0;
    int cnt = 0;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      const bool st = (st_ >> p) & 1u;
      gcs = (st ? 0.0 : gcs) + row[u[p] & 31u];  // tiebreak.py:61
      cnt = (st ? 0 : cnt) + 1;
      put_sel(en_, p, u[p] >> 5, tb_div_small(gcs, cnt, sRc));
    }
    s.flush(a.g_avgconf);
  }
  a.winner[m] = bk;
  a.label[m] = (ngf == 1) ? BCE_TB_UNANIMOUS : tie ? BCE_TB_PREDICTION_VALUE_SMALLEST : BCE_TB_WEIGHT_DENSITY;
  a.n_groups[m] = ngf;
  a.variance[m] = variance;
}

// a group mean: the reciprocal-table quotient where the table exists, else IEEE division
template <bool RC_TAB>
__device__ __forceinline__ double tb_div_cnt(double x, int c, const double* tab) {
  if constexpr (RC_TAB) return tb_div_small(x, c, tab);
  else return x / (double)c;
}

// PART (STAGED launches): 1 = only FULL tiles, 2 = every other tile; 0 = all tiles, one body.
// (Both bodies in one kernel: 21 spilled VGPRs and 190 SGPRs, so two launches.)
// GATHER (market lists, round 5): a tile is 64 list entries, each lane's market row is copied
// into the wave's LDS buffer at row NP * lane by groups of NP / 4 lanes (4 agents each, one
// contiguous row segment per group: coalesced like the contiguous staging) and the outputs
// leave the same way; the general body then runs over NP positions -- a length-bucketed plan
// (batch.tiebreak_plan: buckets of <= 8, 9..16, 17..32 agents) no longer walks 32 positions
// for a 5-agent market (verdict r04 item 5).
template <bool STAGED, bool EXOTIC, int PART = 0, int NP = kTbLpmMax, bool GATHER = false>
__global__ __launch_bounds__(64 * kTbLpmWaves) __attribute__((amdgpu_waves_per_eu(tb_wpe(NP, GATHER && !EXOTIC), tb_wpe(NP, GATHER && !EXOTIC)))) void tiebreak_lpm_kernel(TbArgs a, const int32_t* list,
                                                                         int64_t n_list, int* fault) {
  static_assert(PART == 0 || (STAGED && !EXOTIC), "FULL / rest split: staged kernels only");
  static_assert(!GATHER || (STAGED && PART == 0), "gather staging: staged general body only");
  static_assert(NP == kTbLpmMax || GATHER, "fewer positions: gathered rows only");
  static_assert(NP == 8 || NP == 16 || NP == 32, "positions per lane");
  // one buffer per wave (16.9 KB; two workgroups of four waves per CU)
  __shared__ double sBuf[STAGED ? kTbLpmWaves : 1][STAGED ? tb_stage(NP, GATHER) : 1];
  // GATHER: every lane's row start and length, for the row-segment copies
  __shared__ int64_t sRowOff[GATHER ? kTbLpmWaves : 1][GATHER ? 64 : 1];
  __shared__ int sRowN[GATHER ? kTbLpmWaves : 1][GATHER ? 64 : 1];
  // STAGED: RN(1 / c) for group sizes c = 1..32 (tb_div_small: group means via the table)
  __shared__ double sRc[STAGED ? kTbLpmMax + 1 : 1];
  if constexpr (STAGED) {
    if (threadIdx.x <= (unsigned)kTbLpmMax) sRc[threadIdx.x] = 1.0 / (double)(threadIdx.x ? threadIdx.x : 1);
    __syncthreads();
  }
  const int lane = lane_id();
  const int wv = STAGED ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;  // uniform: LDS bases in SGPRs
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  TbTiles<STAGED, PART, NP, GATHER> tiles{a, list, n_list, fault, lane};
  TbMeta cur{};
  const bool run = tiles.split_run(wave);
  bool left = false;  // PART 1: this wave left a tile to PART 2
  for (int64_t tile = wave; run && tile * 64 < n_list; tile += nwaves) {
    cur = tiles.meta_of(tile);
    if constexpr (PART == 1) {
      if (!cur.full) {  // (skipped tiles are never full)
        left = true;
        continue;
      }
    } else if constexpr (PART == 2) {
      if (cur.full) continue;
    }
    if (cur.skip) {
      const int64_t m = cur.m;
      if (cur.has) {
        a.winner[m] = 0.0; a.label[m] = -1; a.n_groups[m] = -1; a.variance[m] = 0.0;
      }
      continue;
    }
    const TbStage<STAGED, NP, GATHER> s(sBuf[wv], sRowOff[wv], sRowN[wv], lane, cur);
    if constexpr (GATHER) s.rows_set();
    if constexpr (PART == 1) {
      tb_full_body(a, s, tiles, sRc, cur.m, tile + nwaves);
    } else {
      // ---- the general body (any tile that is not FULL): NP positions per lane, of which this
      // lane's market fills n.  Kept here, not lifted like tb_full_body: as a function of its
      // own the two EXOTIC 32-position kernels ran 3-7% slower (the body is then optimised
      // twice, alone and after inlining; 445 -> 473 spilled SGPRs), see
      // measurements/tiebreak_split_ab.txt.
      const int64_t m = cur.m;
      const bool has = cur.has;
      const int n = cur.n;
      const int last = n > 0 ? n - 1 : 0;  // positions past n re-read the last agent (TbStage::at)
      const double nd = (double)(n > 0 ? n : 1);
      // ---- 1. keys, group ordinals (first-seen order), sort with the key as payload ---------
      // Per-lane validity is the bit set vm (bit t: t < n) and run boundaries are stm / enm
      // (bit p: a run starts / ends at sorted position p), each re-derived per phase through an
      // empty asm: kept as 32 lane masks they held 64 SGPRs through the tile and spilled.
      unsigned u[NP];
      double kp[NP];
      int ng = 0;
      const unsigned vm = (n >= NP) ? ~0u : ((1u << (n > 0 ? n : 0)) - 1u);
      auto vbit = [](unsigned bits, int p) { return ((bits >> p) & 1u) != 0u; };
      auto refresh_ug = [&]() {
#pragma unroll
        for (int p = 0; p < NP; ++p) u[p] = tb_bits(u[p]);
      };
      if constexpr (STAGED) s.stage(a.pred);
      const double praw0 = s.at(a.pred, 0);  // a single agent keeps its raw prediction (tiebreak.py:89-96)
      {
        if (!EXOTIC && a.rmode == 0) {  // the common precisions: rint fast path, exact redo if flagged
#pragma unroll
          for (int t = 0; t < NP; ++t) {
            const double x = s.at(a.pred, min(t, last));
            bool slow;
            kp[t] = py_round_nd_fast(x, a.rscale, a.rinv, a.rthresh, slow);
            if (ballot(slow)) kp[t] = slow ? py_round_nd_sel(x, a.rscale, a.rinv, a.rthresh) : kp[t];
          }
        } else {
#pragma unroll
          for (int t = 0; t < NP; ++t) kp[t] = tb_round<EXOTIC>(s.at(a.pred, min(t, last)), a, n >= 2);
        }
        const unsigned vm1 = tb_bits(vm);
        int go[NP];
#pragma unroll
        for (int t = 0; t < NP; ++t) {
          int g = -1;
#pragma unroll
          for (int s2 = 0; s2 < t; ++s2) g = key_eq(kp[s2], kp[t]) ? go[s2] : g;  // earlier equal key: its group
          const bool fresh = vbit(vm1, t) && g < 0;
          go[t] = fresh ? ng : g;
          ng += fresh ? 1 : 0;
          u[t] = vbit(vm1, t) ? (((unsigned)go[t] << 5) | (unsigned)t) : 0xFFFFFFFFu;
        }
        if (a.g_of) {  // agent t's prediction (slot t) is consumed: the ordinals go in place
          if constexpr (STAGED) wave_sync_lds();
          const unsigned vm2 = tb_bits(vm);
#pragma unroll
          for (int t = 0; t < NP; ++t)
            if (vbit(vm2, t)) s.put_i32(a.g_of, t, go[t]);
          if constexpr (STAGED) s.flush_i32(a.g_of);
        }
      }
      // STAGED (kTbGeneralKeysInLds): as the FULL body, only the 32-bit (ordinal, agent) keys go
      // through the network; the rounded keys wait in the lane's row (the predictions are
      // consumed) and each sorted position reads its run head's key back
      if constexpr (STAGED && kTbGeneralKeysInLds) {
        wave_sync_lds();  // the row's readers (keys, g_of flush) are done
        const unsigned vm3 = tb_bits(vm);
#pragma unroll
        for (int t = 0; t < NP; ++t)
          if (vbit(vm3, t)) s.buf[tb_pad(s.lrow + t)] = kp[t];
        wave_sync_lds();
        oem_sort(u);
      } else {
        oem_sort_kv(u, kp);
      }
      // run boundaries from the sorted keys alone (invalid positions hold 0xFFFFFFFF, sorted
      // last: the last valid position ends its run, no invalid position ends one)
      unsigned stm = 1u, enm = (u[NP - 1] != 0xFFFFFFFFu) ? (1u << (NP - 1)) : 0u;
#pragma unroll
      for (int p = 1; p < NP; ++p) {
        const unsigned d = ((u[p] >> 5) != (u[p - 1] >> 5)) ? 1u : 0u;
        stm |= d << p;
        enm |= d << (p - 1);
      }
      enm &= vm;
      // every member carries its run head's key: a group's dict key is its FIRST member's
      // rounded prediction (tiebreak.py:54-55), and -0.0 / 0.0 share a group with different bits
      if constexpr (STAGED && kTbGeneralKeysInLds) {
        // (an invalid position's head index is clamped into the lane's row: never used)
        unsigned ht = u[0] & (unsigned)(NP - 1);
        kp[0] = s.buf[tb_pad(s.lrow + (int)ht)];
#pragma unroll
        for (int p = 1; p < NP; ++p) {
          ht = vbit(stm, p) ? (u[p] & (unsigned)(NP - 1)) : ht;
          kp[p] = s.buf[tb_pad(s.lrow + (int)ht)];
        }
      } else {
#pragma unroll
        for (int p = 1; p < NP; ++p) kp[p] = vbit(stm, p) ? kp[p] : kp[p - 1];
      }

      // ---- 2. group keys and counts (registers only) ------------------------------------------
      if (a.g_key || a.g_count) {
        if (a.g_key) {
          const unsigned en_ = tb_bits(enm);
          refresh_ug();
#pragma unroll
          for (int p = 0; p < NP; ++p)
            if (vbit(en_, p)) s.put(a.g_key, (int)(u[p] >> 5), (n == 1) ? praw0 : kp[p]);
          if constexpr (STAGED) s.flush(a.g_key);
        }
        if (a.g_count) {
          if constexpr (STAGED) wave_sync_lds();
          const unsigned st_ = tb_bits(stm), en_ = tb_bits(enm);
          refresh_ug();
          int cnt = 0;
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            cnt = (vbit(st_, p) ? 0 : cnt) + 1;
            if (vbit(en_, p)) s.put_i32(a.g_count, (int)(u[p] >> 5), cnt);
          }
          if constexpr (STAGED) s.flush_i32(a.g_count);
        }
      }

      // ---- 3. weights: group densities, kept per run end for the winner -----------------------
      // A group's outputs overwrite slot g of its market's row in place: group g ends only after
      // every group <= g, and agent g (ordinal <= g) belongs to one of those -- consumed.
      // (Positions past n read slot min(31, ...) of the lane's row or the tile's slack: never used.)
      double densp[NP];
      if constexpr (STAGED) s.stage(a.weight);
      {
        const unsigned st_ = tb_bits(stm), en_ = tb_bits(enm);
        refresh_ug();
        double tot = 0.0;
        int cnt = 0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const int t = min((int)(u[p] & 31u), last);
          const bool st = vbit(st_, p);
          tot = (st ? 0.0 : tot) + s.at(a.weight, t);  // tiebreak.py:60, sum from int 0
          cnt = (st ? 0 : cnt) + 1;
          densp[p] = tb_div_cnt<STAGED>(tot, cnt, sRc);
          if (vbit(en_, p) && a.g_density) s.put(a.g_density, (int)(u[p] >> 5), densp[p]);
        }
        if constexpr (STAGED) {
          if (a.g_density) s.flush(a.g_density);
        }
      }

      // ---- 4. reliabilities: max per group (first maximum kept), the winner ------------------
      double bd = 0.0, bm = 0.0, bk = 0.0;
      bool tie = false;
      if constexpr (STAGED) s.stage(a.rel);
      {
        const unsigned st_ = tb_bits(stm), en_ = tb_bits(enm);
        refresh_ug();
        double mx = 0.0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const int t = min((int)(u[p] & 31u), last);
          const unsigned g = u[p] >> 5;
          const double r = s.at(a.rel, t);
          mx = vbit(st_, p) ? r : ((r > mx) ? r : mx);  // tiebreak.py:62
          if (vbit(en_, p)) {
            if (a.g_maxrel) s.put(a.g_maxrel, (int)g, mx);
            const double key = (n == 1) ? praw0 : kp[p], dens = densp[p];
            const bool same = (dens == bd) && (mx == bm);
            if (g == 0 || tb_better(dens, mx, key, bd, bm, bk)) {  // tiebreak.py:113-117
              tie = (g != 0) && same;
              bd = dens; bm = mx; bk = key;
            } else {
              tie = tie || same;  // tiebreak.py:123-133: does another group tie the winner?
            }
          }
        }
        if constexpr (STAGED) {
          if (a.g_maxrel) s.flush(a.g_maxrel);
        }
      }

      // ---- 5. confidences: variance (input order), then the per-group means -----------------
      if constexpr (STAGED) s.stage(a.conf);
      double variance;
      {
        const unsigned vm5 = tb_bits(vm);
        double cs = 0.0;
#pragma unroll
        for (int t = 0; t < NP; ++t) cs += vbit(vm5, t) ? s.at(a.conf, min(t, last)) : 0.0;
        const double mean = cs / nd;
        // squares: pow(d, 2.0) restated (glibc_pow.hpp), summed as they come; a lane with a
        // near-midpoint square (a bit in `slow`) redoes its ordered sum with the exact ones
        if constexpr (STAGED) wave_sync_lds();  // re-read the confidences instead of holding them
        const unsigned vm6 = tb_bits(vm);
        double vs = 0.0;
        unsigned slow = 0;
#pragma unroll
        for (int t = 0; t < NP; ++t) {
          bool ok;
          const double q = bce_pow::pow2_fast(s.at(a.conf, min(t, last)) - mean, ok);
          vs += vbit(vm6, t) ? q : 0.0;
          slow |= (vbit(vm6, t) && !ok) ? (1u << t) : 0u;
        }
        if (slow) {
          vs = 0.0;
#pragma unroll 1
          for (int t = 0; t < n; ++t) {
            const double d = s.at(a.conf, t) - mean;
            bool ok;
            const double q = bce_pow::pow2_fast(d, ok);
            vs += ((slow >> t) & 1u) ? tb_pow2_full(d) : q;
          }
        }
        variance = vs / nd;
      }
      if (a.g_avgconf) {
        const unsigned st_ = tb_bits(stm), en_ = tb_bits(enm);
        refresh_ug();
        double gcs = 0.0;
        int cnt = 0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const bool st = vbit(st_, p);
          gcs = (st ? 0.0 : gcs) + s.at(a.conf, min((int)(u[p] & 31u), last));  // tiebreak.py:61
          cnt = (st ? 0 : cnt) + 1;
          if (vbit(en_, p)) s.put(a.g_avgconf, (int)(u[p] >> 5), tb_div_cnt<STAGED>(gcs, cnt, sRc));
        }
        if constexpr (STAGED) s.flush(a.g_avgconf);
      }
      if (has) {
        if (n == 0) {  // tiebreak.py:86-87 (ValueError)
          a.winner[m] = 0.0; a.label[m] = -1; a.n_groups[m] = -1; a.variance[m] = 0.0;
        } else {
          a.winner[m] = bk;
          a.label[m] = (n == 1) ? BCE_TB_SINGLE_AGENT
                                : (ng == 1) ? BCE_TB_UNANIMOUS
                                            : tie ? BCE_TB_PREDICTION_VALUE_SMALLEST : BCE_TB_WEIGHT_DENSITY;
          a.n_groups[m] = ng;
          a.variance[m] = (n == 1) ? 0.0 : variance;
        }
      }
    }
  }
  if (PART == 1 && left) tiles.split_leave(wave);
}

using TbLpmFn = void (*)(TbArgs, const int32_t*, int64_t, int*);

// The one instantiation a call runs (the FULL / rest pair: its first), for the occupancy
// query and the launch alike.
template <bool EXOTIC>
static TbLpmFn tb_lpm_pick(bool listed, bool gather, int np, bool split) {
  if (listed && !gather) return tiebreak_lpm_kernel<false, EXOTIC>;
  if (listed)
    return np == 8    ? tiebreak_lpm_kernel<true, EXOTIC, 0, 8, true>
           : np == 16 ? tiebreak_lpm_kernel<true, EXOTIC, 0, 16, true>
                      : tiebreak_lpm_kernel<true, EXOTIC, 0, 32, true>;
  return split ? tiebreak_lpm_kernel<true, false, 1> : tiebreak_lpm_kernel<true, EXOTIC>;
}

// lane per market: 64 markets per wave, kTbLpmWaves per workgroup
template <bool EXOTIC>
int launch_tb_lpm(const TbArgs& a, const int32_t* market_list, int64_t nl, int32_t max_len, void* stream) {
  const int64_t tiles = (nl + 63) / 64;
  int64_t blocks = (tiles + kTbLpmWaves - 1) / kTbLpmWaves;
  // contiguous markets stage each wave's agent range in LDS; a market list gathers rows
  // contiguous markets, register-batch staging: the FULL tiles (64 markets of 32 agents)
  // run a kernel specialised for them, then a second launch takes every other tile (each
  // launch only reads the offsets of the tiles it leaves to the other)
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool listed = market_list != nullptr;
  bool split = !listed && kTbFullKernel && !EXOTIC && a.rmode == 0 && al16(a.pred) && al16(a.conf) &&
               al16(a.weight) && al16(a.rel);
  // market lists: rows gathered into LDS as 16-B aligned pairs (every array 16-B aligned;
  // else each lane reads and writes its own row in global memory), NP = the list's bound
  // rounded up to 8 / 16 / 32
  const int np = max_len <= 8 ? 8 : max_len <= 16 ? 16 : 32;
  const bool gather = al16(a.pred) && al16(a.conf) && al16(a.weight) && al16(a.rel) &&
                      (!a.g_key || al16(a.g_key)) && (!a.g_density || al16(a.g_density)) &&
                      (!a.g_avgconf || al16(a.g_avgconf)) && (!a.g_maxrel || al16(a.g_maxrel));
  TbLpmFn fn = tb_lpm_pick<EXOTIC>(listed, gather, np, split);
  const int per_cu = blocks_per_cu(reinterpret_cast<const void*>(fn), 64 * kTbLpmWaves, 0, 1, "tiebreak_lpm_kernel");
  const int64_t cap = grid_cap(per_cu);
  if (blocks > cap) blocks = cap;
  if (split && blocks * kTbLpmWaves > kSplitWords) {  // one split word per wave of the grid
    split = false;
    fn = tb_lpm_pick<EXOTIC>(listed, gather, np, split);
  }
  hipStream_t st = as_stream(stream);
  const dim3 grid((int)blocks), block(64 * kTbLpmWaves);
  if (!split) {
    hipLaunchKernelGGL(fn, grid, block, 0, st, a, market_list, nl, fault_word());
  } else {
    static std::atomic<int> tickets{0};
    TbArgs b = a;
    // positive; after a wrap split_slot clears the slot's stale (larger) tickets
    b.ticket = (tickets.fetch_add(1) & 0x3fffffff) + 1;
    b.split = split_slot(b.ticket, st);
    if (!b.split) {
      set_error("tiebreak: no device split words");
      return BCE_EHIP;
    }
    hipLaunchKernelGGL(fn, grid, block, 0, st, b, market_list, nl, fault_word());
    if (int rc = check_launch("tiebreak_lpm_kernel<full>")) return rc;
    hipLaunchKernelGGL((tiebreak_lpm_kernel<true, false, 2>), grid, block, 0, st, b, market_list, nl, fault_word());
  }
  return check_launch("tiebreak_lpm_kernel");
}

template int launch_tb_lpm<false>(const TbArgs&, const int32_t*, int64_t, int32_t, void*);
template int launch_tb_lpm<true>(const TbArgs&, const int32_t*, int64_t, int32_t, void*);

}  // namespace bce
