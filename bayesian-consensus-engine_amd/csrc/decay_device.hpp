// decay_device.hpp -- the decayed reliability of one stored row, shared by the elementwise
// kernels (elementwise.hip) and the market-scope lookup (pair_scope.hip).
#pragma once
#include "bce_device.hpp"
#include "bce_internal.hpp"
#include "glibc_pow.hpp"

#pragma clang fp contract(off)

namespace bce {

struct DecayConst {
  int64_t now_us;
  double half_life;
  double min_rel;
  double default_rel;
  double default_conf;
};

// n / 10**6 correctly rounded for n >= 2^53, where (double)n already rounds and the division
// would round a second time.  10^6 = 2^6 * 15625: with n = a * 15625 + b the quotient is
// (a + b / 15625) / 64, its exponent e is that of floor(n / 10^6) = a >> 6 (33..43 here), and
// the 53-bit significand is (a << s) + (b << s) / 15625 rounded to nearest with
// s = 46 - e >= 3.  15625 is odd, so the fraction is never a tie.  a << s < 2^53 and
// b << s < 2^27: everything is exact in 64-bit integers.
__device__ __forceinline__ double secs_wide(int64_t n) {
  const uint64_t a = (uint64_t)n / 15625u, b = (uint64_t)n % 15625u;
  const int s = 46 - (63 - __builtin_clzll(a >> 6));
  const uint64_t bs = b << s, rem = bs % 15625u;
  const uint64_t m = (a << s) + bs / 15625u + (2 * rem > 15625u);  // <= 2^53: converts exactly
  return (double)m * bce_pow::asd((uint64_t)(1023 - 6 - s) << 52);   // * 2^-(s+6), exact
}

// timedelta.total_seconds() of n microseconds: CPython's int / int, one rounding.  Below 2^53
// (285 years) the conversion is exact and the division is that one rounding; a negative n ends
// as max(0.0, .) = 0.0 days whichever way it rounds.
__device__ __forceinline__ double total_seconds(int64_t n) {
  if (__builtin_expect(n >= ((int64_t)1 << 53), 0)) return secs_wide(n);
  return (double)n / 1e6;
}

// decay.py:52-58 and 90-100, with days from decay.py:140-145.
__device__ __forceinline__ double decayed(double r, int64_t t_us, const DecayConst& k,
                                          const unsigned long long* tab = kExpTab) {
  if (t_us == BCE_NO_TIMESTAMP) return r;
  const double secs = total_seconds(k.now_us - t_us);
  const double days = py_max(0.0, secs / 86400.0);
  if (!(days > 0.0)) return r;
  const double f = bce_pow::pow_base2(-days / k.half_life, tab);  // 2.0 ** x as libm pow (glibc_pow.hpp)
  const double d = k.min_rel + (r - k.min_rel) * f;
  return py_max(k.min_rel, py_min(1.0, d));
}

}  // namespace bce
