// ordered_chain.hpp -- acc += src[0] + src[1] + ... left to right over doubles in LDS: the
// reference's ordered sums (core.py:120,136,142 in consensus_wide.hip; market.py:386-407 in
// aggregate.hip), one chain per lane, on the kernel's critical path.
//
// Why the full steps are asm: the terms come in 4-term batches (ds_read_b128 pairs) held in
// FIXED registers, each batch reloaded right after its adds, so one batch's LDS latency hides
// under the other batches' dependent adds.  The same pipelining in C++ makes the compiler copy
// the loop-carried batch registers behind an lgkmcnt(0), i.e. wait on every batch.  The fixed
// registers are a block the surrounding kernel's VGPR budget leaves free; the block is named
// in the clobber list, so the compiler keeps nothing live in it across the loop.
//
// Each loop consumes whole steps only and says how many terms that was; the tail is the
// caller's (masked chain_tail steps in the wide kernel, a scalar loop in the aggregation).
// src is 16-B aligned; the loops read one step past the terms they add (never added).
#pragma once
#pragma clang fp contract(off)

#include "bce_device.hpp"

namespace bce {

// up to 8 terms from src[from], those at or past ce masked to +0.0 -- exact, because these
// chains start at +0.0 and never hold -0.0.  Reads 8 doubles whatever ce is.
__device__ __forceinline__ void chain_tail(double& acc, const double* src, int from, int ce) {
  double xt[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) xt[e] = src[from + e];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc += (from + e < ce) ? xt[e] : 0.0;
}

// 8-term steps: two 4-term batches in v[112:127], 4 terms ahead of the adds; then the < 8-term
// tail.  Reads may run 8 past ce.
__device__ __forceinline__ void chain_add(double& acc, const double* src, int ce) {
  const int nfull = ce & ~7;
  if (nfull) {
    unsigned addr = (unsigned)(uintptr_t)src;
    int steps = nfull >> 3;
    asm volatile(
        "ds_read_b128 v[112:115], %[ad] offset:0\n"
        "ds_read_b128 v[116:119], %[ad] offset:16\n"
        "ds_read_b128 v[120:123], %[ad] offset:32\n"
        "ds_read_b128 v[124:127], %[ad] offset:48\n"
        "1:\n"
        "s_waitcnt lgkmcnt(3)\n"
        "v_add_f64 %[acc], %[acc], v[112:113]\n"
        "v_add_f64 %[acc], %[acc], v[114:115]\n"
        "s_waitcnt lgkmcnt(2)\n"
        "v_add_f64 %[acc], %[acc], v[116:117]\n"
        "v_add_f64 %[acc], %[acc], v[118:119]\n"
        "ds_read_b128 v[112:115], %[ad] offset:64\n"
        "ds_read_b128 v[116:119], %[ad] offset:80\n"
        "s_waitcnt lgkmcnt(3)\n"
        "v_add_f64 %[acc], %[acc], v[120:121]\n"
        "v_add_f64 %[acc], %[acc], v[122:123]\n"
        "s_waitcnt lgkmcnt(2)\n"
        "v_add_f64 %[acc], %[acc], v[124:125]\n"
        "v_add_f64 %[acc], %[acc], v[126:127]\n"
        "ds_read_b128 v[120:123], %[ad] offset:96\n"
        "ds_read_b128 v[124:127], %[ad] offset:112\n"
        "v_add_u32 %[ad], 64, %[ad]\n"
        "s_sub_u32 %[st], %[st], 1\n"
        "s_cmp_lg_u32 %[st], 0\n"
        "s_cbranch_scc1 1b\n"
        "s_waitcnt lgkmcnt(0)\n"
        : [acc] "+v"(acc), [ad] "+v"(addr), [st] "+s"(steps)
        :
        : "memory", "scc", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121",
          "v122", "v123", "v124", "v125", "v126", "v127");
  }
  if (nfull < ce) chain_tail(acc, src, nfull, ce);
}

// 16-term steps: four 4-term batches in the 32 VGPRs from v[b], each reloaded 16 terms ahead
// right after its adds (12 terms ahead of the adds instead of chain_add's 4).  The register
// block is the immediate operand b: the assembler takes constant expressions in register
// ranges, v[%[b]+4:%[b]+7] is v[100:103] at b = 96.  Reads may run 16 past the terms added.
// BATCH(o, d0, d1): the 4-term batch in v[b + o .. b + o + 7] added, then reloaded from byte
// offsets d0 and d1 (16 terms further on).
#define BCE_CHAIN16_BATCH(O, D0, D1)                                    \
  "s_waitcnt lgkmcnt(6)\n"                                              \
  "v_add_f64 %[acc], %[acc], v[%[b]+" O ":%[b]+" O "+1]\n"              \
  "v_add_f64 %[acc], %[acc], v[%[b]+" O "+2:%[b]+" O "+3]\n"            \
  "v_add_f64 %[acc], %[acc], v[%[b]+" O "+4:%[b]+" O "+5]\n"            \
  "v_add_f64 %[acc], %[acc], v[%[b]+" O "+6:%[b]+" O "+7]\n"            \
  "ds_read_b128 v[%[b]+" O ":%[b]+" O "+3], %[ad] offset:" D0 "\n"      \
  "ds_read_b128 v[%[b]+" O "+4:%[b]+" O "+7], %[ad] offset:" D1 "\n"
// NAME(acc, src, ce): the whole 16-term steps of ce terms; returns the terms consumed.  The
// variadic part is the clobber list, "v<b>" .. "v<b + 31>" as literals.
#define BCE_DEFINE_CHAIN16(NAME, BASE, ...)                                               \
  __device__ __forceinline__ int NAME(double& acc, const double* src, int ce) {           \
    const int steps = ce / 16;                                                            \
    if (steps) {                                                                          \
      unsigned addr = (unsigned)(uintptr_t)src;                                           \
      int st = steps;                                                                     \
      asm volatile(                                                                       \
          "ds_read_b128 v[%[b]:%[b]+3], %[ad] offset:0\n"                                 \
          "ds_read_b128 v[%[b]+4:%[b]+7], %[ad] offset:16\n"                              \
          "ds_read_b128 v[%[b]+8:%[b]+11], %[ad] offset:32\n"                             \
          "ds_read_b128 v[%[b]+12:%[b]+15], %[ad] offset:48\n"                            \
          "ds_read_b128 v[%[b]+16:%[b]+19], %[ad] offset:64\n"                            \
          "ds_read_b128 v[%[b]+20:%[b]+23], %[ad] offset:80\n"                            \
          "ds_read_b128 v[%[b]+24:%[b]+27], %[ad] offset:96\n"                            \
          "ds_read_b128 v[%[b]+28:%[b]+31], %[ad] offset:112\n"                           \
          "1:\n"                                                                          \
          BCE_CHAIN16_BATCH("0", "128", "144")                                            \
          BCE_CHAIN16_BATCH("8", "160", "176")                                            \
          BCE_CHAIN16_BATCH("16", "192", "208")                                           \
          BCE_CHAIN16_BATCH("24", "224", "240")                                           \
          "v_add_u32 %[ad], 128, %[ad]\n"                                                 \
          "s_sub_u32 %[st], %[st], 1\n"                                                   \
          "s_cmp_lg_u32 %[st], 0\n"                                                       \
          "s_cbranch_scc1 1b\n"                                                           \
          "s_waitcnt lgkmcnt(0)\n"                                                        \
          : [acc] "+v"(acc), [ad] "+v"(addr), [st] "+s"(st)                               \
          : [b] "n"(BASE)                                                                 \
          : "memory", "scc", __VA_ARGS__);                                                \
    }                                                                                     \
    return steps * 16;                                                                    \
  }

// the wide kernel's chain wave (v[96:127]) and the aggregation kernel's (v[48:79])
BCE_DEFINE_CHAIN16(chain16_v96, 96, "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105",
                   "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117",
                   "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127")
BCE_DEFINE_CHAIN16(chain16_v48, 48, "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58",
                   "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72",
                   "v73", "v74", "v75", "v76", "v77", "v78", "v79")

#undef BCE_DEFINE_CHAIN16
#undef BCE_CHAIN16_BATCH

}  // namespace bce
