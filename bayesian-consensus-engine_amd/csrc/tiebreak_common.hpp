// tiebreak_common.hpp -- what the tie-break translation units share: the kernels' argument
// block, the rounding of the grouping key, the winner order and the group-mean quotient
// (device), and the host's choice of rounding mode.
//   tiebreak.hip      wave and block kernels, the C entries
//   tiebreak_lpm.hip  lane-per-market kernel (n <= kTbLpmMax) and its launcher
#pragma once

#include "bce_device.hpp"
#include "bce_internal.hpp"
#include "consensus_common.hpp"
#include "glibc_pow.hpp"
#include "py_round_big.hpp"

#pragma clang fp contract(off)

namespace bce {

struct TbArgs {
  const int64_t* offsets;
  int64_t n_markets;
  const double* pred;
  const double* conf;
  const double* weight;
  const double* rel;
  double* winner;
  int32_t* label;
  int32_t* n_groups;
  double* variance;
  double* g_key;
  int32_t* g_count;
  double* g_density;
  double* g_avgconf;
  double* g_maxrel;
  int32_t* g_of;   // nullable: per agent, the ordinal of its group (dict insertion order)
  double rscale;   // 10^ndigits (ndigits >= 0) or 10^-ndigits (ndigits < 0)
  double rthresh;  // see py_round_nd
  double rinv;     // RN(1 / rscale) (mode 0)
  int rmode;       // 0: py_round_nd, 1: py_round_neg, 2: identity (nd > 323), 3: signed zero (nd < -308),
                   // 4: big-integer path 23 <= nd <= 323, 5: big-integer path -308 <= nd <= -16
  int rnd;         // ndigits (modes 4, 5)
  int* fault;      // device fault word: kFaultRoundOverflow (CPython's OverflowError)
  int* split;      // PART 1/2 launches: one word per wave of the (shared) grid; a PART 1 wave
                   // that leaves a tile to PART 2 writes `ticket` into its word
  int ticket;      // this launch pair's number (host counter, never 0): no reset needed
};

constexpr int kFaultRoundOverflow = 6;  // round(x, nd) too large to represent (mode 5)

// round(prediction, precision) of tiebreak.py:54 for every precision CPython accepts (see
// tb_round_mode on the host).  EXOTIC kernels (modes 4, 5: 10^|nd| not an exact double) run
// the exact big-integer restatement of py_round_big.hpp; the others never contain it.
// report: this lane's value is really rounded by the reference -- an agent of a market with
// >= 2 agents (a single agent keeps its raw prediction, tiebreak.py:89-96, and lanes without a
// market round a placeholder) -- so its OverflowError is raised.
template <bool EXOTIC>
__device__ __forceinline__ double tb_round(double x, const TbArgs& a, bool report = true) {
  if constexpr (EXOTIC) {
    if (a.rmode == 4) return bce_round::round_pos(x, a.rnd);
    bool ovf = false;
    const double r = bce_round::round_neg(x, -a.rnd, &ovf);
    if (ovf && report && a.fault) atomicCAS(a.fault, 0, kFaultRoundOverflow);
    return r;
  } else {
    switch (a.rmode) {
      case 0: return py_round_nd(x, a.rscale, a.rthresh);
      case 1: return py_round_neg(x, a.rscale);
      case 2: return x;
      default: return (x != x || fabs(x) == __builtin_inf()) ? x : copysign(0.0, x);
    }
  }
}

__device__ __forceinline__ bool key_eq(double a, double b) { return a == b; }  // -0.0 == 0.0

// (d1, m1, k1) strictly better than (d2, m2, k2) under Python tuple order of
// (density, max_reliability, -key).
__device__ __forceinline__ bool tb_better(double d1, double m1, double k1, double d2, double m2,
                                          double k2) {
  if (d1 != d2) return d1 > d2;
  if (m1 != m2) return m1 > m2;
  return (-k1) > (-k2);
}

// tb_better without short-circuit returns
__device__ __forceinline__ bool tb_better_sel(double d1, double m1, double k1, double d2, double m2,
                                              double k2) {
  const bool nd = d1 != d2, nm = m1 != m2;
  return nd ? (d1 > d2) : (nm ? (m1 > m2) : ((-k1) > (-k2)));
}

// x / c for a group size c in 1..32: RN(x * rc) with one FMA correction, rc = RN(1 / c)
// (Markstein; tools/check_markstein.c checks 3e9 quotients against IEEE division), exact
// for |x| in [2^-1000, 2^1000]; a wave with any other x (0, subnormal, huge, inf, NaN)
// divides those lanes.
__device__ __forceinline__ double tb_div_small(double x, int c, const double* rc_tab) {
  const double rc = rc_tab[c];
  const double b = (double)c;
  const double q0 = x * rc;
  const double q = __builtin_fma(__builtin_fma(-q0, b, x), rc, q0);
  const bool ok = ((int)(fabs(x) >= 0x1p-1000) & (int)(fabs(x) <= 0x1p1000)) != 0;
  return ballot(!ok) ? (ok ? q : x / b) : q;
}

// Markets of at most kTbLpmMax agents go to the lane-per-market kernel (tiebreak_lpm.hip):
// launch_tb_lpm picks its instantiation, sizes the grid and launches.
constexpr int kTbLpmMax = 32;
template <bool EXOTIC>
int launch_tb_lpm(const TbArgs& a, const int32_t* market_list, int64_t nl, int32_t max_len, void* stream);

static inline double pow10_exact(int nd) {
  double s = 1.0;
  for (int i = 0; i < nd; ++i) s *= 10.0;  // exact for nd <= 22
  return s;
}
// 2^E with E = floor(52 - nd*log2(10)) + 1: the smallest power of two whose ulp exceeds 10^-nd
static inline double round_thresh(int nd) {
  const double y = nd * 3.321928094887362;
  const int E = (int)floor(52.0 - y) + 1;
  return ldexp(1.0, E);
}
// CPython float.__round__(x, nd): nd > 323 returns x, nd < -308 returns 0.0 * x
// (NDIGITS_MAX / NDIGITS_MIN of floatobject.c); in between the correctly rounded decimal.
// Restated with doubles for -15 <= nd <= 22 (10^|nd| exact, remainders exact) and with
// exact big integers (py_round_big.hpp, EXOTIC kernels) for the rest.
static inline int tb_round_mode(int nd, double* scale, double* thresh) {
  *scale = 1.0;
  *thresh = 0.0;
  if (nd > 323) return 2;
  if (nd < -308) return 3;
  if (nd >= 0 && nd <= 22) {
    *scale = pow10_exact(nd);
    *thresh = round_thresh(nd);
    return 0;
  }
  if (nd < 0 && nd >= -15) {
    *scale = pow10_exact(-nd);
    return 1;
  }
  return nd > 0 ? 4 : 5;
}

}  // namespace bce
