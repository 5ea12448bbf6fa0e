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

// decay.py:52-58 and 90-100, with days from decay.py:140-145.
__device__ __forceinline__ double decayed(double r, int64_t t_us, const DecayConst& k,
                                          const unsigned long long* tab = kExpTab) {
  if (t_us == BCE_NO_TIMESTAMP) return r;
  const double secs = (double)(k.now_us - t_us) / 1e6;  // timedelta.total_seconds()
  const double days = py_max(0.0, secs / 86400.0);
  if (!(days > 0.0)) return r;
  const double f = bce_pow::pow_base2(-days / k.half_life, tab);  // 2.0 ** x as libm pow (glibc_pow.hpp)
  const double d = k.min_rel + (r - k.min_rel) * f;
  return py_max(k.min_rel, py_min(1.0, d));
}

}  // namespace bce
