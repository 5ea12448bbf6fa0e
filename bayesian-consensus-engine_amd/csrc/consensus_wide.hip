// consensus_wide.hip -- core.compute_consensus (core.py:63-179) for markets with
// 64 < n <= 4096 signals: one workgroup of NW waves per market, P = 64*NW*R keys.
//
// Per market (core.py:103 sorted source ids, core.py:115-116 duplicates averaged in input
// order, core.py:111-112 table lookups, core.py:119-151 weights and ordered sums):
//   1. keys (sid << IB | input index, 32 bits; needs n_sources <= 2^(32-IB)) from the sid
//      registers loaded one market ahead, and the input-order probabilities (loaded during
//      the previous market) into region A with their range check (core.py:59-60)
//      [wide_stage_inputs]; the next market's sids and probabilities are issued right away.
//   2. register bitonic network (flip form, wide_sort.hpp): stages inside a thread are
//      min/max pairs, lane exchanges are VALU only (DPP in rows, v_permlane16/32_swap across
//      rows and halves), the few stages that cross waves go through LDS rows (region B, two
//      alternating buffers: one barrier per stage).
//   3. the probabilities are read back in sorted order into registers and written over
//      region A in place; run leaders get their unique index from a workgroup prefix count
//      and land in region B (sid << IB | first sorted position) [wide_leaders].
//   4. per unique j (thread t owns j = t + NT*i): one {rel, conf} row + present word
//      gathered [wide_gather], the run's probabilities summed in input order (builtin sum,
//      core.py:116 [run_sum]; FAST: runs longer than kWaveRun by the whole wave in a fixed
//      order [wide_long_runs]), products w, avg*w, conf*w (core.py:119,136,142)
//      [wide_products]; usid / weight written.
//        FAST  (BCE_MODE_FAST): per-thread partial sums in round order [wide_rounds], then a
//              fixed butterfly over the wave and a wave-ordered sum over the workgroup --
//              deterministic, within the north-star 1e-9 of the reference order.
//        EXACT: rounds of products staged through a two-slot LDS ring; wave 0 carries the
//              three left-to-right chains (core.py:120,136,142; ordered_chain.hpp) on lanes
//              0..2 -- with several waves it does only that [wide_chain_wave], fed by the
//              others [wide_produce] through LDS counters (no barriers), so the serial chains
//              overlap the next rounds' gathers; otherwise [wide_rounds] behind barriers.
//      normalizedWeight reads w[j] back from the weight output (or, without one, from the
//      dead sorted-probability slot j where it was parked).
//   5. per-market outputs [wide_totals] and normalizedWeight = w / total (core.py:151)
//      [wide_nweight].
// LDS: region A = P doubles (+ read-ahead pad), region B = max(sort exchange rows,
// leaders [+ the exact chain buffers]).  FAST at P = 4096 fits three workgroups per CU.
#include <stdio.h>
#include <stdlib.h>

#include "consensus_common.hpp"
#include "ordered_chain.hpp"
#include "wide_sort.hpp"

#pragma clang fp contract(off)

constexpr int kWideHR = 1;       // rounds of NT uniques whose gathers are in flight together (2: C3 fast +6%)
constexpr int kWideWPE = 4;      // min waves per SIMD (register budget; 4 vs 2: exact -1.3%, fast unchanged)
constexpr int kWideNWBF = 4;     // FAST nweight read-backs per batch (1: 1.645, 2: 1.634, 4: 1.587 ms C3)
constexpr bool kWideChainDeep = true;  // EXACT piped chain wave: chain_add_deep (16-term steps)
constexpr bool kWideChain3 = true;     // EXACT chains run on lanes 0..2 only (exec = 3 lanes)
// FAST: run averages and normalizedWeight by reciprocal products instead of IEEE divisions
// (a few ulps; FAST's contract is 1e-9 relative)
constexpr bool kWideFastRecip = true;

namespace bce {
namespace {

constexpr int kWaveRun = 48;  // FAST: duplicate runs longer than this are summed wave-wide

// NW waves (threads = 64*NW) hold P = 64*NW*R keys; the sort network spans NN >= NW waves
// (PN = 64*NN*R, a power of two): NN > NW is a non-power-of-two bin -- the network's
// missing waves hold +inf keys, so every exchange with them leaves the key in place and
// they are never materialised (6 waves for 2049..3072 signals, 3 for 1025..1536).
// KT: the sort key, (sid << IB) | input index -- 32 bits while n_sources <= 2^(32 - IB), else
// 64 bits (large tables, DESIGN.md §4.2 "Large source tables").
template <int NW, int R, bool FAST, int NN = NW, class KT = unsigned>
struct WideCfg {
  static constexpr int NT = 64 * NW;
  static constexpr int P = NT * R;
  static constexpr int PN = 64 * NN * R;
  static constexpr int IB = ilog2c(PN);
  static constexpr int LW = (int)(sizeof(KT) / 4);  // u32 words per key
  static constexpr int HR = (R < kWideHR) ? R : kWideHR;
  // register budget: workgroups of >= 4 waves get 4 waves per SIMD (<= 128 VGPRs), so two
  // LDS-sized workgroups share a CU
  // (the 6-wave FAST kernel at 5 waves per SIMD, <= 102 VGPRs, so three workgroups share a
  // CU: C3 fast 1.55 -> 1.72 ms from its spills, profiles/r03g/wide_ab.txt)
  static constexpr int WPE = kWideWPE;
  static constexpr int A_DBL = P + 64;  // + the run sums' read-ahead
  // region B (u32): sort exchange rows (32-bit keys: two alternating buffers of P words;
  // 64-bit keys: one buffer of P keys), then leaders [P] keys (+ exact: chain buffers
  // [2][3][NT] doubles + the chain's read-ahead)
  static constexpr int X_U32 = 2 * P;
  static constexpr int LEAD_U32 = LW * P + (FAST ? 0 : 2 * (6 * NT + 32));
  static constexpr int B_U32 = (X_U32 > LEAD_U32) ? X_U32 : LEAD_U32;
};

// One fixed-order sum over the wave, returned in every lane: DPP rotations inside each
// 16-lane row and quad swaps (no LDS round trips), then the four row sums in row order.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)__double_as_longlong(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)((uint64_t)__double_as_longlong(v) >> 32), CTRL, 0xF, 0xF,
                                          false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_fixed(double v) {
  v = v + dpp_f64<0x128>(v);  // row_ror:8
  v = v + dpp_f64<0x124>(v);  // row_ror:4
  v = v + dpp_f64<0x4E>(v);   // quad_perm 2,3,0,1
  v = v + dpp_f64<0xB1>(v);   // quad_perm 1,0,3,2
  return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

// builtin sum() from 0 over a run of len sorted probabilities in input order (core.py:116);
// terms past the run add +0.0, exact since the sum starts at +0.0 and is never -0.0.
// APPROX (FAST): the average as sum * (1/len) -- v_rcp_f64 refined by one Newton step.
template <int R, bool APPROX = false>
__device__ __forceinline__ double run_sum(const double* sA, int q0, int len) {
  double x[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = sA[q0 + e];
  double sum = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) sum += (e < len) ? x[e] : 0.0;
  if (len > 4) {  // long (hot-source) run: 8 terms per step, the next 8 in flight
    int e0 = 4;
    double xa[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) xa[e] = sA[q0 + e0 + e];
    for (; e0 + 8 <= len; e0 += 8) {
      double xb[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) xb[e] = sA[q0 + e0 + 8 + e];
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += xa[e];
#pragma unroll
      for (int e = 0; e < 8; ++e) xa[e] = xb[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += (e0 + e < len) ? xa[e] : 0.0;
  }
  if constexpr (APPROX) {
    const double c = (double)len;
    double y = __builtin_amdgcn_rcp(c);
    y = __builtin_fma(__builtin_fma(-c, y, 1.0), y, y);
    return (len > 1) ? sum * y : sum;
  } else {
    return (len > 1) ? sum / (double)len : sum;
  }
}

// The piped EXACT path's dedicated chain wave (kWideChainDeep): ordered_chain.hpp's 16-term
// steps in v[96:127], then masked 8-term tail steps.  Reads may run 16 past ce (the chain ring
// holds 6 (NT - NP) = 384 doubles of slack past its last chain).
// (six batches -- 24-term steps, 48 fixed VGPRs -- spilled 22 VGPRs in the 8-wave kernel and
// ran C3 exact 2.00 vs 1.90 ms, profiles/archive/r05r/)
__device__ __forceinline__ void chain_add_deep(double& acc, const double* src, int ce) {
  for (int from = chain16_v96(acc, src, ce); from < ce; from += 8) chain_tail(acc, src, from, ce);
}

// LDS of one market's workgroup of NW waves, carved from a byte buffer.
//   region A  P doubles (+ read-ahead pad): input-order probs, then sorted probs in place
//   region B  sort exchange rows, then leaders [P] (+ exact: chain buffers [2][3][NT])
//   small     per-wave last keys / counts, totals, error index, exact hand-off counters
template <int NW, int R, bool FAST, int NN, class KT = unsigned>
struct WideLds {
  using Cfg = WideCfg<NW, R, FAST, NN, KT>;
  static constexpr int A_BYTES = Cfg::A_DBL * 8;
  static constexpr int B_BYTES = ((Cfg::B_U32 * 4 + 15) / 16) * 16;
  static constexpr int TOT_OFF = A_BYTES + B_BYTES;          // sTot [3*NW] doubles
  static constexpr int LAST_OFF = TOT_OFF + 24 * NW;          // sLast [NW] keys
  static constexpr int CNT_OFF = LAST_OFF + (int)sizeof(KT) * NW;  // sCnt [NW]
  static constexpr int MISC_OFF = CNT_OFF + 4 * NW;           // sErr, sRdy[2], sDone
  static constexpr int BYTES = ((MISC_OFF + 16 + 15) / 16) * 16;
  double* sA;
  unsigned* sB;
  double* sTot;
  KT* sLast;
  int* sCnt;
  int* sErr;
  int* sRdy;
  int* sDone;
  __device__ __forceinline__ explicit WideLds(unsigned char* base)
      : sA(reinterpret_cast<double*>(base)),
        sB(reinterpret_cast<unsigned*>(base + A_BYTES)),
        sTot(reinterpret_cast<double*>(base + TOT_OFF)),
        sLast(reinterpret_cast<KT*>(base + LAST_OFF)),
        sCnt(reinterpret_cast<int*>(base + CNT_OFF)),
        sErr(reinterpret_cast<int*>(base + MISC_OFF)),
        sRdy(reinterpret_cast<int*>(base + MISC_OFF + 4)),
        sDone(reinterpret_cast<int*>(base + MISC_OFF + 12)) {}
};

// The buffer loads of a market's sids
// and probabilities into registers (records = n signals, so i >= n reads 0).
template <int NW, int R>
__device__ __forceinline__ void wide_load(const ConsArgs& a, int64_t off, int n, int t, unsigned (&ps)[R],
                                          double (&pp)[R]) {
  constexpr int NT = 64 * NW, P = NT * R;
  const int cnt = n < P ? n : P;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.sid + off), 0, cnt * 4, 0x00020000);
#pragma unroll
  for (int c = 0; c < R; ++c) ps[c] = __builtin_amdgcn_raw_buffer_load_b32(rs, t * 4, c * NT * 4, 0);
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)(a.prob + off), 0, cnt * 8, 0x00020000);
#pragma unroll
  for (int c = 0; c < R; ++c)
    pp[c] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rp, t * 8, c * NT * 8, 0));
}

constexpr int kWideNoErr = 0x7fffffff;  // no probability out of range (so far)

// What every phase of one market knows: the launch, the workgroup's LDS, the thread, the market.
template <int NW, int R, bool FAST, int NN, class KT>
struct WideCtx {
  using Cfg = WideCfg<NW, R, FAST, NN, KT>;
  static constexpr int NT = Cfg::NT, P = Cfg::P, IB = Cfg::IB, HR = Cfg::HR, LW = Cfg::LW;
  static constexpr KT QMASK = (KT)Cfg::PN - 1u;  // the input-index bits of a key
  // FAST: the region past the leaders (the dead exchange rows) parks w[j] for normalizedWeight
  // when the market's uniques fit -- C3's Zipf markets have u <= 0.55 n, which fits in ~all
  // of them -- instead of reading the weight output back (each load there waits for this
  // thread's earlier stores to retire: vmcnt is in order)
  // (race-free: the next market's first wave-crossing stage writes exchange buffer 0 =
  // sB[0, P); buffer 1 = sB[P, 2P) is written only after that stage's barrier, which every
  // thread reaches after its own tail)
  // (64-bit keys: the leaders fill region B, nothing is parked)
  static constexpr int WFREE = FAST ? (Cfg::B_U32 - LW * P) / 2 : 0;

  const ConsArgs& a;
  const WideLds<NW, R, FAST, NN, KT>& L;
  const int t, lane;
  const int wv;       // wave within the workgroup (uniform)
  const int64_t off;  // the market's first signal
  const int n;        // ... and its length
  const unsigned smax;
  // normalizedWeight reads w[j] back from the weight output (this thread's own stores)
  // in workgroups of several waves (it saves their barriers); a single wave parks w[j] in
  // region A (dead sorted-prob slot j), which is faster than the global round trip.
  const bool wback;

  __device__ __forceinline__ KT* sLead() const { return reinterpret_cast<KT*>(L.sB); }  // [u] sid<<IB | q0
  __device__ __forceinline__ double* sWAC() const {  // exact: [2][3][NT]
    return reinterpret_cast<double*>(L.sB + LW * P);
  }
  __device__ __forceinline__ double* sW() const { return reinterpret_cast<double*>(L.sB + LW * P); }  // fast: parked w[j]
};

// ---- 1. keys from the sid registers (the bad-sid ballot raises kFaultSid), then the
// input-order probabilities into region A with their range check.  Returns the first bad input
// index this thread saw, or kWideNoErr.
template <int NW, int R, bool FAST, int NN, class KT>
__device__ __forceinline__ int wide_stage_inputs(const WideCtx<NW, R, FAST, NN, KT>& c, const unsigned (&ps)[R],
                                                 const double (&pp)[R], KT (&key)[R]) {
  constexpr int NT = 64 * NW, IB = WideCfg<NW, R, FAST, NN, KT>::IB;
  bool badsid = false;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int i = k * NT + c.t;
    const unsigned s = ps[k];
    badsid |= (i < c.n) && (s > c.smax);
    key[k] = (i < c.n) ? ((KT)(s < c.smax ? s : c.smax) << IB) | (KT)i : ~(KT)0;
  }
  if (ballot(badsid)) raise_fault(c.a.fault, kFaultSid);
  int myerr = kWideNoErr;
  // input-order probs into region A before the next loads; region A's last readers are
  // the previous market's run sums (before its final barrier) unless normalizedWeight
  // reads w[j] from it
  if (NW > 1 && !c.wback) __syncthreads();
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int i = k * NT + c.t;
    const double p = pp[k];
    c.L.sA[i] = p;
    if ((i < c.n) && (p < 0.0 || p > 1.0) && myerr == kWideNoErr) myerr = i;  // core.py:59-60
  }
  return myerr;
}

// ---- 3. sorted probs in place, leaders.  The sorted keys pick the probabilities out of
// region A (input order) into registers, which then overwrite region A in sorted order; a key
// whose sid differs from its predecessor's leads a run and gets its unique index from the wave
// and workgroup prefix counts; sLead[j] = sid << IB | first sorted position.  Returns u, the
// number of unique sources.
template <int NW, int R, bool FAST, int NN, class KT>
__device__ __forceinline__ int wide_leaders(const WideCtx<NW, R, FAST, NN, KT>& c, const KT (&key)[R], int myerr) {
  using Ctx = WideCtx<NW, R, FAST, NN, KT>;
  constexpr int IB = Ctx::IB, LW = Ctx::LW;
  constexpr KT QMASK = Ctx::QMASK;
  const auto& L = c.L;
  double* const sA = L.sA;
  KT* const sLead = c.sLead();
  const int t = c.t, lane = c.lane, wv = c.wv, n = c.n;
  if (lane == 63) L.sLast[wv] = key[R - 1];
  __syncthreads();  // (a) input-order probs + sLast visible; exchange rows dead
  if (myerr != kWideNoErr) atomicMin(L.sErr, myerr);
  double x[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int q = t * R + r;
    x[r] = (q < n) ? sA[key[r] & QMASK] : 0.0;
  }
  KT prev_in_wave;  // wave_shr:1
  if constexpr (LW == 2)
    prev_in_wave = k_make((unsigned)__builtin_amdgcn_update_dpp(0, (int)k_hi(key[R - 1]), 0x138, 0xF, 0xF, false),
                          (unsigned)__builtin_amdgcn_update_dpp(0, (int)k_lo(key[R - 1]), 0x138, 0xF, 0xF, false));
  else
    prev_in_wave = (unsigned)__builtin_amdgcn_update_dpp(0, (int)key[R - 1], 0x138, 0xF, 0xF, false);
  const KT prev_key = (lane > 0) ? prev_in_wave : (wv > 0 ? L.sLast[wv - 1] : (KT)0);
  unsigned lead = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int q = t * R + r;
    const KT ps0 = ((r == 0) ? prev_key : key[r - 1]) >> IB;
    const bool is = (q < n) && (q == 0 || (key[r] >> IB) != ps0);
    lead |= is ? (1u << r) : 0u;
  }
  const int cnt = __popc(lead);
  const int incl = wave_incl_scan(cnt);
  if (lane == 63) L.sCnt[wv] = incl;
  __syncthreads();  // (b) every read of the input-order probs done; counts visible
#pragma unroll
  for (int r = 0; r < R; r += 2) *reinterpret_cast<double2*>(sA + t * R + r) = make_double2(x[r], x[r + 1]);
  int base = incl - cnt, u = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const int cw = L.sCnt[w];
    if (w < wv) base += cw;
    u += cw;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (lead & (1u << r)) {
      const int jj = base + __popc(lead & ((1u << r) - 1u));
      sLead[jj] = (key[r] & ~QMASK) | (KT)(t * R + r);
    }
  }
  if (t == 0) {
    L.sRdy[0] = L.sRdy[1] = 0;
    *L.sDone = 0;
  }
  __syncthreads();  // (c) sorted probs + leaders visible
  return u;
}

// ---- 4. per-unique pieces ---------------------------------------------------------------------
// Unique jj of the market: its run [q0, q1) of sorted positions, its sid, its {rel, conf} row
// and present word (the gathers are issued here and awaited where first used).  jj >= u: an
// empty run and the cold default row, DEFAULT_RELIABILITY / _CONFIDENCE, as with an empty table.
struct WideUnique {
  double2 rc;
  int q0, q1;
  unsigned sid, pwd;
};
template <int NW, int R, bool FAST, int NN, class KT>
__device__ __forceinline__ WideUnique wide_gather(const WideCtx<NW, R, FAST, NN, KT>& c, int jj, int u) {
  using Ctx = WideCtx<NW, R, FAST, NN, KT>;
  const KT* const sLead = c.sLead();
  WideUnique g;
  g.q0 = g.q1 = 0;
  g.sid = g.pwd = 0;
  g.rc = make_double2(0.5, 0.25);
  if (jj < u) {
    const KT lv = sLead[jj];
    g.q0 = (int)(lv & Ctx::QMASK);
    g.sid = (unsigned)min(lv >> Ctx::IB, (KT)c.smax);  // <= smax by construction of the key; clamped anyway
    g.q1 = (jj + 1 < u) ? (int)(sLead[jj + 1] & Ctx::QMASK) : c.n;
    if (c.a.n_sources > 0) {
      g.rc = c.a.relconf[g.sid];
      g.pwd = c.a.pbits[g.sid >> 5];
    }
  }
  return g;
}

// w, avg * w, conf * w of a unique (core.py:111,119 / 136 / 142); zeros past the last one
struct WideProducts {
  double w, aw, cw;
};
__device__ __forceinline__ WideProducts wide_products(const WideUnique& g, double avg, bool live) {
  WideProducts p{0.0, 0.0, 0.0};
  if (live) {
    const double w = g.rc.x;
    p.w = w;
    p.aw = avg * w;
    p.cw = g.rc.y * w;
  }
  return p;
}

// the usid output word: the sid, bit 31 set for a cold source
__device__ __forceinline__ int32_t wide_usid(const WideUnique& g) {
  return (int32_t)(g.sid | cold_flag(g.pwd, (int)g.sid));
}

// Wait until the LDS counter *flag reaches `need` (the piped path's hand-offs); a wave that polls
// spin_cap times gives up and raises kFaultSpinChain.
__device__ __forceinline__ void wide_wait(int* flag, int need, const ConsArgs& a) {
  int spins = 0;
  while (ldsflag(flag) < need) {
    if (++spins > a.spin_cap) {
      raise_fault(a.fault, kFaultSpinChain);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

// EXACT with several waves (and the weight output, so region A is not needed for w):
// wave 0 only carries the chains while waves 1.. produce rounds of NP = NT - 64
// uniques into a two-slot LDS ring, handed over with LDS counters instead of barriers,
// so the serial chains overlap the gathers and run sums of the next rounds.
// The consumer, wave 0: lanes 0..2 add round r's three chains once all NW - 1 producers
// have signed the slot (sRdy), then release it (sDone).
template <int NW, int R, bool FAST, int NN, class KT>
__device__ __forceinline__ void wide_chain_wave(const WideCtx<NW, R, FAST, NN, KT>& c, int u, double& acc) {
  constexpr int NP = (NW > 1) ? 64 * NW - 64 : 64 * NW;
  const auto& L = c.L;
  const int lane = c.lane;
  const int nrp = (u + NP - 1) / NP;
  __builtin_amdgcn_s_setprio(2);  // the chain is the critical path
  for (int r = 0; r < nrp; ++r) {
    const int slot = r & 1;
    wide_wait(&L.sRdy[slot], (NW - 1) * ((r >> 1) + 1), c.a);
    const int ce = (u - r * NP < NP) ? u - r * NP : NP;
    if (!kWideChain3 || lane < 3) {  // kWideChain3: only the three chain lanes read LDS
      if constexpr (kWideChainDeep) chain_add_deep(acc, c.sWAC() + slot * 3 * NP + (lane % 3) * NP, ce);
      else chain_add(acc, c.sWAC() + slot * 3 * NP + (lane % 3) * NP, ce);
    }
    if (lane == 0) __hip_atomic_store(L.sDone, r + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __builtin_amdgcn_s_setprio(0);
}

// The producers, waves 1..: thread pt = t - 64 owns unique r * NP + pt of round r; a round's
// products go into ring slot r & 1 once the chain wave has consumed round r - 2, then usid and
// weight are stored.
template <int NW, int R, bool FAST, int NN, class KT>
__device__ __forceinline__ void wide_produce(const WideCtx<NW, R, FAST, NN, KT>& c, int u) {
  using Ctx = WideCtx<NW, R, FAST, NN, KT>;
  constexpr int HR = Ctx::HR;
  constexpr int NP = (NW > 1) ? 64 * NW - 64 : 64 * NW;
  const auto& L = c.L;
  const ConsArgs& a = c.a;
  const int nrp = (u + NP - 1) / NP;
  const int pt = c.t - 64;
  for (int h = 0; h < nrp; h += HR) {
    WideUnique g[HR];
#pragma unroll
    for (int i = 0; i < HR; ++i) g[i] = wide_gather(c, (h + i) * NP + pt, u);  // every gather of the group in flight together
    WideProducts v[HR];
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      const bool live = (h + i) * NP + pt < u;
      double avg = 0.0;
      if (live) avg = run_sum<R>(L.sA, g[i].q0, g[i].q1 - g[i].q0);  // core.py:116
      v[i] = wide_products(g[i], avg, live);
    }
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      const int r = h + i;
      if (r < nrp) {
        const int slot = r & 1;
        if (r >= 2) wide_wait(L.sDone, r - 1, a);  // the slot's previous round is consumed
        double* const buf = c.sWAC() + slot * 3 * NP;
        buf[pt] = v[i].w;
        buf[NP + pt] = v[i].aw;
        buf[2 * NP + pt] = v[i].cw;
        wave_sync_lds();  // this wave's part of the round is in LDS
        if (c.lane == 0) __hip_atomic_fetch_add(&L.sRdy[slot], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      const int jj = (h + i) * NP + pt;
      if (jj < u) {
        const int64_t p = c.off + jj;
        if (a.usid) a.usid[p] = wide_usid(g[i]);
        a.weight[p] = v[i].w;
      }
    }
  }
}

// FAST: runs longer than kWaveRun (hot sources) are summed by the whole wave in a fixed
// order instead of by their own lane, so one hot source does not hold the wave.  `mine`: this
// lane's unique has such a run [q0, q0 + len); its average lands in avg.
__device__ __forceinline__ void wide_long_runs(const double* sA, int lane, bool mine, int q0, int len, double& avg) {
  unsigned long long lm = ballot(mine);
  while (lm) {
    const int LL = __builtin_ctzll(lm);
    lm &= lm - 1;
    const int lq0 = __builtin_amdgcn_readlane(q0, LL), llen = __builtin_amdgcn_readlane(len, LL);
    double part = 0.0;
    for (int e = lane; e < llen; e += 64) part += sA[lq0 + e];
    part = wave_sum_fixed(part);
    if (lane == LL) avg = part / (double)llen;
  }
}

// What the rounds leave for the totals.
struct WideSums {
  double acc = 0.0;                     // exact: wave 0 lanes 0..2 carry the chains
  double pw = 0.0, pa = 0.0, pc = 0.0;  // fast: this thread's partial sums
};

// The plain rounds (every path but the piped one): thread t owns unique r * NT + t of round r.
// FAST adds its products to the thread's partial sums; EXACT stages each round in the two-slot
// buffer behind a barrier and wave 0 adds the chains (8-term steps).  Without the weight
// read-back (!wback) w[j] is parked in region A for normalizedWeight; `park`: FAST parks it
// past the leaders.
template <int NW, int R, bool FAST, int NN, class KT>
__device__ __forceinline__ void wide_rounds(const WideCtx<NW, R, FAST, NN, KT>& c, int u, bool park, WideSums& s) {
  using Ctx = WideCtx<NW, R, FAST, NN, KT>;
  constexpr int NT = Ctx::NT, HR = Ctx::HR;
  const ConsArgs& a = c.a;
  double* const sA = c.L.sA;
  const int t = c.t, lane = c.lane;
  const bool wback = c.wback;
  const int nr = (u + NT - 1) / NT;
  for (int h = 0; h < nr; h += HR) {
    WideUnique g[HR];
#pragma unroll
    for (int i = 0; i < HR; ++i) g[i] = wide_gather(c, (h + i) * NT + t, u);  // every gather of the group in flight together
    WideProducts v[HR];
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      const bool live = (h + i) * NT + t < u;
      const int len = g[i].q1 - g[i].q0;
      double avg = 0.0;
      if constexpr (FAST) {
        avg = (live && len <= kWaveRun) ? run_sum<R, kWideFastRecip>(sA, g[i].q0, len) : 0.0;
        wide_long_runs(sA, lane, live && len > kWaveRun, g[i].q0, len, avg);
      } else if (live) {
        avg = run_sum<R>(sA, g[i].q0, len);
      }
      v[i] = wide_products(g[i], avg, live);
    }
    if constexpr (FAST) {
#pragma unroll
      for (int i = 0; i < HR; ++i) {  // round order: fixed per thread
        s.pw += v[i].w;
        s.pa += v[i].aw;
        s.pc += v[i].cw;
      }
      if (!wback) {
        __syncthreads();  // every sorted-prob read of this group done
#pragma unroll
        for (int i = 0; i < HR; ++i) {
          const int jj = (h + i) * NT + t;
          if (jj < u) sA[jj] = v[i].w;  // later groups read only positions > jj
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < HR; ++i) {
        if (h + i < nr) {
          double* const buf = c.sWAC() + ((h + i) & 1) * 3 * NT;
          buf[t] = v[i].w;
          buf[NT + t] = v[i].aw;
          buf[2 * NT + t] = v[i].cw;
          __syncthreads();  // round staged; every sorted-prob read of this group is done
          const int jj = (h + i) * NT + t;
          if (jj < u && !wback) sA[jj] = v[i].w;  // position jj is only read by uniques <= jj
          if (c.wv == 0) {
            __builtin_amdgcn_s_setprio(2);  // the chain is the critical path
            const int ce = (u - (h + i) * NT < NT) ? u - (h + i) * NT : NT;
            if (!kWideChain3 || lane < 3) chain_add(s.acc, buf + (lane % 3) * NT, ce);
            __builtin_amdgcn_s_setprio(0);
          }
        }
      }
    }
    // per-unique outputs after the group's LDS work, so no store is pending under it;
    // nontemporal (FAST -0.5..1%, profiles/r03k/wide_r03u_ab.txt)
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      const int jj = (h + i) * NT + t;
      if (jj < u) {
        const int64_t p = c.off + jj;
        if (a.usid) __builtin_nontemporal_store(wide_usid(g[i]), &a.usid[p]);
        if (a.weight) __builtin_nontemporal_store(v[i].w, &a.weight[p]);
        if (park) c.sW()[jj] = v[i].w;
      }
    }
  }
}

// ---- 5. the three totals over the workgroup (FAST: each wave's fixed-order sum, the waves in
// order; EXACT: the chains of wave 0's lanes 0..2), the barrier that also makes the parked w[j]
// visible, and the per-market outputs.  Returns the total weight.
template <int NW, int R, bool FAST, int NN, class KT>
__device__ __forceinline__ double wide_totals(const WideCtx<NW, R, FAST, NN, KT>& c, int32_t m, int u, WideSums s) {
  const auto& L = c.L;
  const ConsArgs& a = c.a;
  if constexpr (FAST) {
    s.pw = wave_sum_fixed(s.pw);
    s.pa = wave_sum_fixed(s.pa);
    s.pc = wave_sum_fixed(s.pc);
    if (c.lane == 0) {
      L.sTot[3 * c.wv] = s.pw;
      L.sTot[3 * c.wv + 1] = s.pa;
      L.sTot[3 * c.wv + 2] = s.pc;
    }
  } else {
    if (c.wv == 0 && c.lane < 3) L.sTot[c.lane] = s.acc;
  }
  __syncthreads();  // totals + w[j] visible
  double tw = L.sTot[0], ta = L.sTot[1], tc = L.sTot[2];
  if constexpr (FAST) {
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      tw += L.sTot[3 * w];
      ta += L.sTot[3 * w + 1];
      tc += L.sTot[3 * w + 2];
    }
  }
  if (c.t == 0 && m >= 0) {
    // store_market's null test is tw == 0.0 alone: an empty market (n == 0) has u == 0, so
    // nothing was added and tw is +0.0 -- the same markets as (n == 0) || (tw == 0.0)
    store_market(a, m, tw, ta, tc, u);
    if (a.err_idx) a.err_idx[m] = (*L.sErr == kWideNoErr) ? -1 : *L.sErr;
  }
  return tw;
}

// normalizedWeight = w[j] / total (core.py:151), if requested, for the thread's uniques
// j = t + NT*k; w[j] from where it was left: the weight output (wback), region A, or (FAST,
// `park`) past the leaders.
// (The test of a.nweight sits in here: in front of the call, the EXACT kernels of several waves
// spilled 12 to 22 more VGPRs, measurements/consensus_wide_split_ab.txt.)
template <int NW, int R, bool FAST, int NN, class KT>
__device__ __forceinline__ void wide_nweight(const WideCtx<NW, R, FAST, NN, KT>& c, int u, double tw, bool park) {
  constexpr int NT = 64 * NW;
  const ConsArgs& a = c.a;
  const double* const sA = c.L.sA;
  const int t = c.t;
  const int64_t off = c.off;
  const bool wback = c.wback;
  if (!a.nweight) return;  // not requested
  if constexpr (!FAST) {
    // every read-back issued before any nweight store: loads retire behind earlier
    // stores (vmcnt is in order), so a load/store per iteration waits out each store
    // (C3 exact -2.6%; FAST: batches of kWideNWBF, a full batch costs it spills)
    double wj[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int jj = t + NT * k;
      wj[k] = (jj < u) ? (wback ? a.weight[off + jj] : sA[jj]) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int jj = t + NT * k;
      if (jj < u) a.nweight[off + jj] = norm_weight(wj[k], tw);
    }
  } else {
    constexpr int NB = (kWideNWBF < R) ? kWideNWBF : R;  // read-backs per batch
    const double* const sW = c.sW();
    const double rtw = (tw > 0.0) ? 1.0 / tw : 0.0;
    for (int j0 = t; j0 < u; j0 += NB * NT) {
      double wj[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const int jj = j0 + NT * k;
        wj[k] = (jj < u) ? (park ? sW[jj] : wback ? a.weight[off + jj] : sA[jj]) : 0.0;
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const int jj = j0 + NT * k;
        const double nw = kWideFastRecip ? ((tw > 0.0) ? wj[k] * rtw : 0.0) : norm_weight(wj[k], tw);
        if (jj < u) __builtin_nontemporal_store(nw, &a.nweight[off + jj]);
      }
    }
  }
}

// One market (m, off, n) on a workgroup of NW waves; t = thread.  ps / pp hold
// its sids and probabilities (loaded by the caller); issue_next() is called once the keys are
// built, to start the workgroup's next market's loads into ps / pp.  The steps are the file
// header's.
template <int NW, int R, bool FAST, int NN, class KT, class NextFn>
__device__ __forceinline__ void wide_market(const ConsArgs& a, const WideLds<NW, R, FAST, NN, KT>& L, const int t,
                                            const int32_t m, const int64_t off, int n, unsigned (&ps)[R],
                                            double (&pp)[R], NextFn&& issue_next) {
  using Ctx = WideCtx<NW, R, FAST, NN, KT>;
  unsigned* const sX = L.sB;  // sort exchange rows
  const int lane = lane_id();
  const Ctx c{a,
              L,
              t,
              lane,
              __builtin_amdgcn_readfirstlane(t >> 6),
              off,
              n,
              (unsigned)(a.n_sources > 0 ? a.n_sources - 1 : 0),
              (NW > 1) && a.weight != nullptr};

  // ---- 1. keys, input-order probs into region A; next market's metadata + sids + probs ----
  KT key[R];
  const int myerr = wide_stage_inputs(c, ps, pp, key);
  issue_next();
  if (n > Ctx::P) {  // longer than this launch's max_len: left unprocessed, reported
    raise_fault(a.fault, kFaultTooLong);
    return;  // uniform over the workgroup
  }
  if (t == 0) *L.sErr = kWideNoErr;

  // ---- 2. sort (core.py:103 order; ties in input order by the index bits) ----------
  wide_sort<NN, NW, R>(key, sX, t, lane);

  // ---- 3. range check reported, sorted probs in place, leaders ----------------------
  const int u = wide_leaders(c, key, myerr);

  // ---- 4. per-unique products: the piped ring (EXACT, several waves, weight read-back:
  // wave 0 adds the chains, the others produce) or the plain rounds ----------------------
  WideSums s;
  const bool piped = !FAST && NW > 1 && c.wback;
  const bool park = FAST && c.wback && u <= Ctx::WFREE;
  if (piped) {
    if (c.wv == 0) wide_chain_wave(c, u, s.acc);
    else wide_produce(c, u);
  } else {
    wide_rounds(c, u, park, s);
  }

  // ---- 5. totals, per-market outputs, nweight ------------------------------------------
  const double tw = wide_totals(c, m, u, s);
  wide_nweight(c, u, tw, park);
}

// One bin per launch: a persistent grid of NW-wave workgroups strides over the bin's market
// list (one market per workgroup at a time, the next one's loads issued during this one).
template <int NW, int R, bool FAST, int NN = NW, class KT = unsigned>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(WideCfg<NW, R, FAST, NN, KT>::WPE, 8))) void consensus_wide_kernel(ConsArgs a) {
  dev_range(a);
  using LD = WideLds<NW, R, FAST, NN, KT>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[LD::BYTES];
  const LD L(smem);
  const int t = threadIdx.x;
  const int lane = lane_id();

  // Market metadata for this workgroup's next 64 markets (li = base + G*k on lane k) is
  // loaded in one vector batch, so picking a market is a readlane, never a scalar-load
  // stall.  A market's sids are loaded one market ahead, its probabilities while the
  // previous market finishes (buffer loads: records = n signals, so i >= n reads 0).
  const int64_t G = gridDim.x;
  int32_t vm = 0;
  int64_t voff = 0;
  int vn = 0;
  auto refill = [&](int64_t base) {
    const int64_t li = base + G * lane;
    vm = (li < a.n_list) ? (a.list ? (li < a.n_hi ? a.list_hi[li] : a.list[li - a.n_hi]) : (int32_t)li) : 0;
    voff = (li < a.n_list) ? a.offsets[vm] : 0;
    vn = (li < a.n_list) ? (int)(a.offsets[vm + 1] - voff) : 0;
  };
  int32_t nm = 0;
  int64_t noff = 0;
  int nn = 0;
  auto meta = [&](int64_t li) {
    const int k = (int)(((li - blockIdx.x) / G) & 63);
    if (k == 0) refill(li);
    nm = __builtin_amdgcn_readlane(vm, k);
    noff = ((int64_t)__builtin_amdgcn_readlane((int)(voff >> 32), k) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)voff, k);
    nn = __builtin_amdgcn_readlane(vn, k);
  };
  unsigned ps[R];
  double pp[R];
  if (blockIdx.x < a.n_list) {
    meta(blockIdx.x);
    wide_load<NW, R>(a, noff, nn, t, ps, pp);
  }
  for (int64_t li = blockIdx.x; li < a.n_list; li += G) {
    const int32_t m = nm;
    const int64_t off = noff;
    const int n = nn;
    wide_market<NW, R, FAST, NN, KT>(a, L, t, m, off, n, ps, pp, [&]() {
      if (li + G < a.n_list) {
        meta(li + G);
        wide_load<NW, R>(a, noff, nn, t, ps, pp);
      }
    });
  }
}

// The kernel of a wide launch and its workgroup size.
struct WideKernel {
  void (*fn)(ConsArgs);
  int threads;
};

// 32-bit keys while the sid fits beside the IB index bits, 64-bit keys for larger tables
template <int NW, int R, bool FAST, int NN = NW>
WideKernel wide_kernel(int32_t n_sources) {
  constexpr int IB = WideCfg<NW, R, FAST, NN>::IB;
  if ((int64_t)n_sources <= (1ll << (32 - IB))) return {consensus_wide_kernel<NW, R, FAST, NN, unsigned>, 64 * NW};
  return {consensus_wide_kernel<NW, R, FAST, NN, uint64_t>, 64 * NW};
}

// (NW, R[, NN]) per length bin: P = 64*NW*R >= max_len; the 1536 and 3072 bins run the
// 2048 / 4096-key network on 3 / 6 waves
// (Round 5: a market shard's 513..1024 / 1025..2048 bins on 4 / 8 waves with R = 4 -- half the
// latency per market, more rounds -- made one 8th of C3 slower, 0.2069-0.2072 -> 0.2274-0.2300
// ms, profiles/archive/r05g/; removed.)
template <bool FAST>
WideKernel wide_kernel_for(int64_t max_len, int32_t n_sources) {
  if (max_len <= 128) return wide_kernel<1, 2, FAST>(n_sources);
  if (max_len <= 256) return wide_kernel<1, 4, FAST>(n_sources);
  if (max_len <= 512) return wide_kernel<1, 8, FAST>(n_sources);
  if (max_len <= 1024) return wide_kernel<2, 8, FAST>(n_sources);
  if (max_len <= 1536) return wide_kernel<3, 8, FAST, 4>(n_sources);
  if (max_len <= 2048) return wide_kernel<4, 8, FAST>(n_sources);
  if (max_len <= 3072) return wide_kernel<6, 8, FAST, 8>(n_sources);
  return wide_kernel<8, 8, FAST>(n_sources);
}

WideKernel wide_kernel_for(int64_t max_len, int32_t mode, int32_t n_sources) {
  return (mode == BCE_MODE_FAST) ? wide_kernel_for<true>(max_len, n_sources) : wide_kernel_for<false>(max_len, n_sources);
}

int64_t resident(const WideKernel& k) {
  return grid_cap(blocks_per_cu(reinterpret_cast<const void*>(k.fn), k.threads, 0, 1, "consensus_wide_kernel"));
}

}  // namespace


namespace {
__global__ void lane_xor_selftest_kernel(unsigned* out) {
  const unsigned l = (unsigned)lane_id();
  out[0 * 64 + l] = lane_xor<1>(l);
  out[1 * 64 + l] = lane_xor<2>(l);
  out[2 * 64 + l] = lane_xor<3>(l);
  out[3 * 64 + l] = lane_xor<4>(l);
  out[4 * 64 + l] = lane_xor<7>(l);
  out[5 * 64 + l] = lane_xor<8>(l);
  out[6 * 64 + l] = lane_xor<15>(l);
  out[7 * 64 + l] = lane_xor<16>(l);
  out[8 * 64 + l] = lane_xor<31>(l);
  out[9 * 64 + l] = lane_xor<32>(l);
  out[10 * 64 + l] = lane_xor<63>(l);
  out[11 * 64 + l] = (unsigned)wave_incl_scan((int)l + 1);
  out[12 * 64 + l] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)l + 100, 0x138, 0xF, 0xF, false);  // wave_shr:1
}
}  // namespace

// Self-test of the sort's lane exchanges and the wave scan (one wave, touches only `out`):
// out[q*64 + l] must equal l ^ {1,2,3,4,7,8,15,16,31,32,63}[q], out[11*64 + l] = (l+1)(l+2)/2,
// out[12*64 + l] = l + 99 (lane l-1's l+100; 0 in lane 0).  `out` holds 13*64 words.
extern "C" int bce_debug_lane_selftest(unsigned* out, void* stream) {
  BCE_REQUIRE(out, "lane_selftest: NULL");
  hipLaunchKernelGGL(lane_xor_selftest_kernel, dim3(1), dim3(64), 0, as_stream(stream), out);
  return check_launch("lane_xor_selftest_kernel");
}


int64_t wide_resident(int64_t max_len, int32_t mode, int32_t n_sources) {
  return resident(wide_kernel_for(max_len, mode, n_sources));
}

// One bin per launch: a persistent grid (every workgroup resident) strides over the market list.
int launch_wide_len(int64_t max_len, const ConsArgs& a, hipStream_t st) {
  if (a.n_list == 0) return BCE_OK;
  const WideKernel k = wide_kernel_for(max_len, a.mode, a.n_sources);
  const int64_t cap = resident(k);
  const int grid = (int)(a.n_list < cap ? a.n_list : cap);
  hipLaunchKernelGGL(k.fn, dim3(grid), dim3(k.threads), 0, st, a);
  return check_launch("consensus_wide_kernel");
}

}  // namespace bce
