// wide_sort.hpp -- the register sort network of the wide consensus kernel (consensus_wide.hip):
// a flip-form bitonic network over PN = 64*NN*R keys held R per thread in VGPRs.  Stages
// inside a thread are min/max pairs, lane exchanges are VALU only (DPP in rows,
// v_permlane16/32_swap across rows and halves), the few stages that cross waves go through LDS
// rows.  Nothing here knows about consensus arithmetic: keys are 32- or 64-bit unsigned words
// (tools/sort_ab.hip times the network on its own).  Also the wave prefix sum the kernel's
// leader scan uses.
#pragma once

#include "bce_device.hpp"

namespace bce {

constexpr int ilog2c(int x) { return x <= 1 ? 0 : 1 + ilog2c(x >> 1); }

// 64-bit key halves through the 32-bit lane primitives
__device__ __forceinline__ unsigned k_lo(uint64_t v) { return (unsigned)v; }
__device__ __forceinline__ unsigned k_hi(uint64_t v) { return (unsigned)(v >> 32); }
__device__ __forceinline__ uint64_t k_make(unsigned hi, unsigned lo) { return ((uint64_t)hi << 32) | lo; }

// v from lane ^ M (whole wave) for the masks the flip-form sort uses -- all VALU, no LDS
// round trip: DPP for the in-row patterns, the CDNA4 half-exchanges v_permlane16_swap /
// v_permlane32_swap (plus a lane select) across rows and halves.
template <int M>
__device__ __forceinline__ unsigned lane_xor(unsigned v) {
  const int lane = lane_id();
  if constexpr (M == 1) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);   // quad_perm 1,0,3,2
  else if constexpr (M == 2) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);  // 2,3,0,1
  else if constexpr (M == 3) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x1B, 0xF, 0xF, false);  // 3,2,1,0
  else if constexpr (M == 4) {  // row_ror:N reads lane (l - N) mod 16: bit 2 set -> ror 4, clear -> ror 12
    const unsigned a = (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false);
    const unsigned b = (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x12C, 0xF, 0xF, false);
    return (lane & 4) ? a : b;
  } else if constexpr (M == 7) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
  else if constexpr (M == 8) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false);    // row_ror:8
  else if constexpr (M == 15) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, false);   // row_mirror
  else if constexpr (M == 16) {  // odd rows <-> even rows
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return (lane & 16) ? r[0] : r[1];
  } else if constexpr (M == 32) {  // upper half <-> lower half
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (lane & 32) ? r[0] : r[1];
  } else if constexpr (M == 31) {  // l ^ 31 = (l ^ 16) ^ 15
    return (unsigned)__builtin_amdgcn_mov_dpp((int)lane_xor<16>(v), 0x140, 0xF, 0xF, false);
  } else if constexpr (M == 63) {  // l ^ 63 = (l ^ 32) ^ 31
    return lane_xor<31>(lane_xor<32>(v));
  } else {
    static_assert(M == 1, "unsupported lane distance");
    return v;
  }
}

template <int M>
__device__ __forceinline__ uint64_t lane_xor(uint64_t v) {
  return k_make(lane_xor<M>(k_hi(v)), lane_xor<M>(k_lo(v)));
}

// Inclusive prefix sum over the wave with DPP (GFX9 row shifts + row broadcasts).
__device__ __forceinline__ int wave_incl_scan(int x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);  // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
  return x;
}

// Index of wave-crossing stage (K, J) among the network's wave-crossing stages (they
// alternate between two exchange buffers, so each needs one barrier, not two).
constexpr int xw_index(int K, int J, int R) {
  int idx = 0;
  for (int k = 2; k < K; k <<= 1)
    for (int j = k / 2; j >= 1; j >>= 1)
      if ((j == k / 2) ? (k > 64 * R) : (j >= 64 * R)) ++idx;
  for (int j = K / 2; j > J; j >>= 1)
    if ((j == K / 2) ? (K > 64 * R) : (j >= 64 * R)) ++idx;
  return idx;
}

// One lane stage over 8 keys with the partner's key read through DPP inside the
// instructions that use it: per key v_sub_co_u32_dpp (borrow = partner < key, into VCC),
// s_xor_b64 with the stage's lower-lane mask, v_cndmask_b32_dpp (keep the key or take the
// partner's) -- two VALU per key instead of a v_mov_b32_dpp, a v_cmp and a v_cndmask (the
// compiler neither folds DPP into a compare nor into a select whose DPP operand is src1,
// and gfx950 has no VOPC DPP).  FLIP: key r's partner is key R-1-r of the partner lane.
// The outputs are early-clobber, so no instruction in the block reads a register written
// in it; `s_nop 1` covers the VALU-write -> DPP-read hazard on the inputs; the s_xor writes
// SCC, so the block clobbers it (a scalar branch condition computed before it is dead).
#define BCE_DPP_CAS(O, A, B, C)                                                  \
  "v_sub_co_u32_dpp %[j], vcc, %[" B "], %[" A "] " C " row_mask:0xf bank_mask:0xf\n" \
  "s_xor_b64 vcc, vcc, %[lm]\n"                                                  \
  "v_cndmask_b32_dpp %[" O "], %[" B "], %[" A "], vcc " C " row_mask:0xf bank_mask:0xf\n"
#define BCE_DPP_STAGE8(C, B0, B1, B2, B3, B4, B5, B6, B7)                                                       \
  asm("s_nop 1\n" BCE_DPP_CAS("o0", "k0", B0, C) BCE_DPP_CAS("o1", "k1", B1, C) BCE_DPP_CAS("o2", "k2", B2, C)    \
          BCE_DPP_CAS("o3", "k3", B3, C) BCE_DPP_CAS("o4", "k4", B4, C) BCE_DPP_CAS("o5", "k5", B5, C)           \
              BCE_DPP_CAS("o6", "k6", B6, C) BCE_DPP_CAS("o7", "k7", B7, C)                                      \
      : [o0] "=&v"(o[0]), [o1] "=&v"(o[1]), [o2] "=&v"(o[2]), [o3] "=&v"(o[3]), [o4] "=&v"(o[4]),              \
        [o5] "=&v"(o[5]), [o6] "=&v"(o[6]), [o7] "=&v"(o[7]), [j] "=&v"(junk)                                  \
      : [k0] "v"(s[0]), [k1] "v"(s[1]), [k2] "v"(s[2]), [k3] "v"(s[3]), [k4] "v"(s[4]), [k5] "v"(s[5]),        \
        [k6] "v"(s[6]), [k7] "v"(s[7]), [lm] "s"(lower)                                                        \
      : "vcc", "scc")
#define BCE_DPP_STAGE8_ANY(C, FLIP)                                                   \
  do {                                                                                \
    if (FLIP)                                                                         \
      BCE_DPP_STAGE8(C, "k7", "k6", "k5", "k4", "k3", "k2", "k1", "k0");              \
    else                                                                              \
      BCE_DPP_STAGE8(C, "k0", "k1", "k2", "k3", "k4", "k5", "k6", "k7");              \
  } while (0)

// Lane bits 2 and 3 separate the two lanes of a pair by DPP bank (bank = lane bits 3..2
// of the row), so the stage needs no select at all: v_min_u32_dpp writes the lower lanes'
// banks, v_max_u32_dpp the upper lanes' (bank_mask), each reading the partner through its
// own row pattern -- two VALU per key, no compare in VCC.  CLO/BLO: the lower lanes' DPP
// pattern and banks, CHI/BHI the upper lanes'.
#define BCE_BANK_CAS(O, A, B, CLO, BLO, CHI, BHI)                                            \
  "v_min_u32_dpp %[" O "], %[" B "], %[" A "] " CLO " row_mask:0xf bank_mask:" BLO "\n"     \
  "v_max_u32_dpp %[" O "], %[" B "], %[" A "] " CHI " row_mask:0xf bank_mask:" BHI "\n"
#define BCE_BANK_STAGE8(CLO, BLO, CHI, BHI, B0, B1, B2, B3, B4, B5, B6, B7)                                   \
  asm("s_nop 1\n" BCE_BANK_CAS("o0", "k0", B0, CLO, BLO, CHI, BHI) BCE_BANK_CAS("o1", "k1", B1, CLO, BLO, CHI, BHI) \
          BCE_BANK_CAS("o2", "k2", B2, CLO, BLO, CHI, BHI) BCE_BANK_CAS("o3", "k3", B3, CLO, BLO, CHI, BHI)          \
              BCE_BANK_CAS("o4", "k4", B4, CLO, BLO, CHI, BHI) BCE_BANK_CAS("o5", "k5", B5, CLO, BLO, CHI, BHI)      \
                  BCE_BANK_CAS("o6", "k6", B6, CLO, BLO, CHI, BHI) BCE_BANK_CAS("o7", "k7", B7, CLO, BLO, CHI, BHI)  \
      : [o0] "=&v"(o[0]), [o1] "=&v"(o[1]), [o2] "=&v"(o[2]), [o3] "=&v"(o[3]), [o4] "=&v"(o[4]),               \
        [o5] "=&v"(o[5]), [o6] "=&v"(o[6]), [o7] "=&v"(o[7])                                                    \
      : [k0] "v"(s[0]), [k1] "v"(s[1]), [k2] "v"(s[2]), [k3] "v"(s[3]), [k4] "v"(s[4]), [k5] "v"(s[5]),         \
        [k6] "v"(s[6]), [k7] "v"(s[7]))
#define BCE_BANK_STAGE8_ANY(CLO, BLO, CHI, BHI, FLIP)                                          \
  do {                                                                                         \
    if (FLIP)                                                                                  \
      BCE_BANK_STAGE8(CLO, BLO, CHI, BHI, "k7", "k6", "k5", "k4", "k3", "k2", "k1", "k0");     \
    else                                                                                       \
      BCE_BANK_STAGE8(CLO, BLO, CHI, BHI, "k0", "k1", "k2", "k3", "k4", "k5", "k6", "k7");     \
  } while (0)

// Lane distances the fused 8-key stage serves: lane bits 0..1 through one DPP pattern
// (quad_perm) with the compare in VCC, lane bits 2..3 (row_ror:4/12, row_ror:8,
// row_half_mirror, row_mirror) by bank.
constexpr bool dpp_fusable(int M) { return M == 1 || M == 2 || M == 3 || M == 4 || M == 7 || M == 8 || M == 15; }

template <int M, bool FLIP>
__device__ __forceinline__ void dpp_stage8(unsigned (&key)[8], uint64_t lower) {
  unsigned o[8], junk;
  const unsigned (&s)[8] = key;
  // row_ror:N reads lane (l - N) mod 16: the l ^ 4 partner is ror 12 for bit 2 clear
  // (banks 0, 2), ror 4 for bit 2 set (banks 1, 3)
  if constexpr (M == 4) BCE_BANK_STAGE8_ANY("row_ror:12", "0x5", "row_ror:4", "0xa", FLIP);
  else if constexpr (M == 8) BCE_BANK_STAGE8_ANY("row_ror:8", "0x3", "row_ror:8", "0xc", FLIP);
  else if constexpr (M == 7) BCE_BANK_STAGE8_ANY("row_half_mirror", "0x5", "row_half_mirror", "0xa", FLIP);
  else if constexpr (M == 15) BCE_BANK_STAGE8_ANY("row_mirror", "0x3", "row_mirror", "0xc", FLIP);
  else if constexpr (M == 1) BCE_DPP_STAGE8_ANY("quad_perm:[1,0,3,2]", FLIP);
  else if constexpr (M == 2) BCE_DPP_STAGE8_ANY("quad_perm:[2,3,0,1]", FLIP);
  else if constexpr (M == 3) BCE_DPP_STAGE8_ANY("quad_perm:[3,2,1,0]", FLIP);
  (void)junk;
  (void)lower;
#pragma unroll
  for (int r = 0; r < 8; ++r) key[r] = o[r];
}

// v_permlane32_swap (M == 32) or v_permlane16_swap (M == 16) of one register pair
template <int M>
__device__ __forceinline__ auto permlane_swap(unsigned a, unsigned b) {
  static_assert(M == 16 || M == 32, "the half-exchange distances");
  if constexpr (M == 32) return __builtin_amdgcn_permlane32_swap(a, b, false, false);
  else return __builtin_amdgcn_permlane16_swap(a, b, false, false);
}

// Half-cleaner across lane bit 4 or 5 (l ^ 16, l ^ 32) on pairs of keys: v_permlane16/32_swap
// of keys (a, b) leaves each lane holding both members of one pair -- a[l] and a[l ^ M] in
// the lanes with the bit clear, b[l ^ M] and b[l] in the others, the lower position always
// in the first register -- so one min/max pair does the stage for both keys, and a second
// swap puts them back.  Four VALU per two keys, no lane masks.
template <int M, int R>
__device__ __forceinline__ void swap_stage(uint64_t (&key)[R]) {  // 64-bit keys: both halves swapped
#pragma unroll
  for (int r = 0; r < R; r += 2) {
    const auto h1 = permlane_swap<M>(k_hi(key[r]), k_hi(key[r + 1]));
    const auto l1 = permlane_swap<M>(k_lo(key[r]), k_lo(key[r + 1]));
    const uint64_t a = k_make(h1[0], l1[0]), b = k_make(h1[1], l1[1]);
    const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
    const auto h2 = permlane_swap<M>(k_hi(lo), k_hi(hi));
    const auto l2 = permlane_swap<M>(k_lo(lo), k_lo(hi));
    key[r] = k_make(h2[0], l2[0]);
    key[r + 1] = k_make(h2[1], l2[1]);
  }
}

template <int M, int R>
__device__ __forceinline__ void swap_stage(unsigned (&key)[R]) {
#pragma unroll
  for (int r = 0; r < R; r += 2) {
    const auto s1 = permlane_swap<M>(key[r], key[r + 1]);
    const unsigned lo = min(s1[0], s1[1]), hi = max(s1[0], s1[1]);
    const auto s2 = permlane_swap<M>(lo, hi);
    key[r] = s2[0];
    key[r + 1] = s2[1];
  }
}

// One stage of the flip-form bitonic network over PN = 64*NN*R keys, position q = t*R + r:
// the first stage of merge K pairs q with q ^ (K-1), the others pair q with q ^ J, and the
// lower position always keeps the minimum -- no direction bits anywhere.  Threads t >= 64*NW
// (a non-power-of-two bin's missing waves) hold +inf: their partners keep their own keys.
// sX: the LDS exchange rows of the wave-crossing stages (32-bit keys: two alternating buffers
// of 64*NW*R words; 64-bit keys: one buffer of 64*NW*R keys).
template <int NN, int NW, int R, int K, int J, class KT>
__device__ __forceinline__ void wide_stage(KT (&key)[R], unsigned* sX, int t, int lane) {
  constexpr bool flip = (J == K / 2);
  constexpr bool K64 = sizeof(KT) == 8;
  if constexpr (flip ? (K <= R) : (J < R)) {  // inside a thread: min/max pairs
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int r2 = flip ? (r ^ (K - 1)) : (r | J);
      if (flip ? (r < r2) : ((r & J) == 0)) {
        const KT x = key[r], y = key[r2];
        key[r] = x < y ? x : y;
        key[r2] = x < y ? y : x;
      }
    }
  } else if constexpr (flip ? (K <= 64 * R) : (J < 64 * R)) {  // across lanes (never crosses a wave)
    constexpr int MK = flip ? (K / R - 1) : (J / R);
    const bool lower = (lane & (flip ? (K / R / 2) : MK)) == 0;
    if constexpr (!K64 && R == 8 && dpp_fusable(MK)) {
      dpp_stage8<MK, flip>(key, (uint64_t)ballot(lower));
      if constexpr (J > 1) wide_stage<NN, NW, R, K, J / 2>(key, sX, t, lane);
      return;
    }
    if constexpr (!flip && (MK == 16 || MK == 32)) {
      swap_stage<MK, R>(key);
      if constexpr (J > 1) wide_stage<NN, NW, R, K, J / 2>(key, sX, t, lane);
      return;
    }
    if constexpr (flip && MK == 31) {
      // the flip of merge K = 32R as a reversal of each K-block's upper half (q ^ (K/2 - 1):
      // row_mirror of key R-1-r, written in rows 1 and 3 only) and a half-cleaner on lane
      // bit 4 -- the pairs are the same; the upper half then holds its bitonic sequence
      // reversed, which the following half-cleaners sort as well (a reversed bitonic
      // sequence is bitonic), so the merge's output is the same sorted sequence
      KT nk[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if constexpr (K64) {
          nk[r] = k_make((unsigned)__builtin_amdgcn_update_dpp((int)k_hi(key[r]), (int)k_hi(key[R - 1 - r]), 0x140, 0xA,
                                                               0xF, false),
                         (unsigned)__builtin_amdgcn_update_dpp((int)k_lo(key[r]), (int)k_lo(key[R - 1 - r]), 0x140, 0xA,
                                                               0xF, false));
        } else {
          nk[r] = (unsigned)__builtin_amdgcn_update_dpp((int)key[r], (int)key[R - 1 - r], 0x140, 0xA, 0xF, false);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) key[r] = nk[r];
      swap_stage<16, R>(key);
      if constexpr (J > 1) wide_stage<NN, NW, R, K, J / 2>(key, sX, t, lane);
      return;
    }
    KT y[R];
#pragma unroll
    for (int r = 0; r < R; ++r) y[r] = lane_xor<MK>(key[flip ? R - 1 - r : r]);
#pragma unroll
    for (int r = 0; r < R; ++r) key[r] = ((key[r] < y[r]) == lower) ? key[r] : y[r];
  } else if constexpr (K64) {  // across waves, 64-bit keys: one LDS buffer, two barriers
    constexpr int MT = flip ? (K / R - 1) : (J / R);
    const bool lower = (t & (flip ? (K / R / 2) : MT)) == 0;
    // planes of 2 keys: key r of thread t at (r/2)*NT*2 + t*2 + r%2 (16-B accesses, a wave's
    // 64 accesses consecutive)
    uint64_t* const buf = reinterpret_cast<uint64_t*>(sX);
    constexpr int PL = 2 * 64 * NW;  // keys per plane
#pragma unroll
    for (int r = 0; r < R; r += 2) {
      uint4 v;
      v.x = k_lo(key[r]); v.y = k_hi(key[r]); v.z = k_lo(key[r + 1]); v.w = k_hi(key[r + 1]);
      *reinterpret_cast<uint4*>(buf + (r >> 1) * PL + t * 2) = v;
    }
    __syncthreads();
    uint64_t y[R];
    const bool real = NN == NW || (t ^ MT) < 64 * NW;  // partner in a missing wave: +inf
#pragma unroll
    for (int r = 0; r < R; r += 2) {
      const uint4 v = real ? *reinterpret_cast<const uint4*>(buf + (r >> 1) * PL + (t ^ MT) * 2)
                           : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
      y[r] = k_make(v.y, v.x);
      y[r + 1] = k_make(v.w, v.z);
    }
    __syncthreads();  // every read done before the next stage rewrites the buffer
    if (__builtin_amdgcn_readfirstlane((int)lower)) {
#pragma unroll
      for (int r = 0; r < R; ++r) key[r] = key[r] < y[flip ? R - 1 - r : r] ? key[r] : y[flip ? R - 1 - r : r];
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) key[r] = key[r] < y[flip ? R - 1 - r : r] ? y[flip ? R - 1 - r : r] : key[r];
    }
  } else {  // across waves, through LDS rows; buffers alternate, so the previous reads
            // of this buffer finished before the last stage's barrier
    constexpr int MT = flip ? (K / R - 1) : (J / R);
    unsigned* const buf = sX + (xw_index(K, J, R) & 1) * (64 * NW * R);
    const bool lower = (t & (flip ? (K / R / 2) : MT)) == 0;
    // planes of 4 keys: key r of thread t at (r/4)*NT*4 + t*4 + r%4, so every 16-B access
    // of a wave covers 1 KB of consecutive words (a thread-major row of R keys put lanes 32 B
    // apart: two lanes per bank group, a 2-way conflict on every exchange)
    constexpr int PL = 4 * 64 * NW;  // words per plane
#pragma unroll
    for (int r = 0; r < R; r += 4)
      *reinterpret_cast<uint4*>(buf + (r >> 2) * PL + t * 4) = make_uint4(key[r], key[r + 1], key[r + 2], key[r + 3]);
    __syncthreads();
    unsigned y[R];
    const bool real = NN == NW || (t ^ MT) < 64 * NW;  // partner in a missing wave: +inf
#pragma unroll
    for (int r = 0; r < R; r += 4) {
      const uint4 y4 = real ? *reinterpret_cast<const uint4*>(buf + (r >> 2) * PL + (t ^ MT) * 4)
                            : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
      y[r] = y4.x;
      y[r + 1] = y4.y;
      y[r + 2] = y4.z;
      y[r + 3] = y4.w;
    }
    // `lower` is uniform over the wave here (the partner is a whole wave away): one min or
    // one max per key under a scalar branch, no compare in VCC
    if (__builtin_amdgcn_readfirstlane((int)lower)) {
#pragma unroll
      for (int r = 0; r < R; ++r) key[r] = min(key[r], y[flip ? R - 1 - r : r]);
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) key[r] = max(key[r], y[flip ? R - 1 - r : r]);
    }
  }
  if constexpr (J > 1) wide_stage<NN, NW, R, K, J / 2>(key, sX, t, lane);
}

// The whole network: merges K = 2, 4, .. 64*NN*R; the keys end sorted by position q = t*R + r.
template <int NN, int NW, int R, int K = 2, class KT>
__device__ __forceinline__ void wide_sort(KT (&key)[R], unsigned* sX, int t, int lane) {
  wide_stage<NN, NW, R, K, K / 2>(key, sX, t, lane);
  if constexpr (K < 64 * NN * R) wide_sort<NN, NW, R, 2 * K>(key, sX, t, lane);
}

#undef BCE_DPP_CAS
#undef BCE_DPP_STAGE8
#undef BCE_DPP_STAGE8_ANY
#undef BCE_BANK_CAS
#undef BCE_BANK_STAGE8
#undef BCE_BANK_STAGE8_ANY

}  // namespace bce
