// boot_weights.hpp -- the Poisson(1) bootstrap weight of a (replicate, unit) pair, integer only
// (include/bce.h: the bootstrap block states the function in full).  The same code
// runs on the host (bce_boot_weights_host) and in the kernel (score_boot.hip), so a weight is a
// function of (seed, replicate, unit) alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BCE_BOOT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BCE_BOOT_HD inline
#endif

namespace bce {

constexpr uint64_t kBootGold = 0x9E3779B97F4A7C15ull;
constexpr int kBootThresholds = 21;  // a weight is in 0 .. 21

// splitmix64's finaliser (wrapping uint64 arithmetic).
BCE_BOOT_HD uint64_t boot_mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// key(r): one per replicate.
BCE_BOOT_HD uint64_t boot_key(uint64_t seed, int64_t r) { return boot_mix(seed + (uint64_t)r * kBootGold); }

// The unit's half of h(r, u): one per item, any int64 hashed as its bit pattern.
BCE_BOOT_HD uint64_t boot_unit_hash(int64_t u) { return boot_mix((uint64_t)u + kBootGold); }

// #{k : h >= T[k]}, T[k] = min(floor(2^64 * sum_{j <= k} e^-1 / j!), 2^64 - 1): the Poisson(1)
// quantile of h / 2^64.  The table is derived with `decimal` at 80 digits (tests/boot_ref.py
// repeats the derivation).  h >= T[6] has probability 8.3e-5: the tail is a branch that a whole
// wave almost never takes.
BCE_BOOT_HD int boot_count(uint64_t h) {
  constexpr uint64_t T[kBootThresholds] = {
      0x5e2d58d8b3bcdf1aull, 0xbc5ab1b16779be35ull, 0xeb715e1dc1582dc2ull, 0xfb23979734a252f1ull,
      0xff1025f59174dc3dull, 0xffd90f3ba4055e19ull, 0xfffa8b71fc72c913ull, 0xffff540c0914b3c9ull,
      0xffffed1f4aa8f120ull, 0xfffffe216e641462ull, 0xffffffd4d85d3183ull, 0xfffffffc6da262b4ull,
      0xffffffffba12d178ull, 0xfffffffffb07c64cull, 0xffffffffffab8ea5ull, 0xfffffffffffabe22ull,
      0xffffffffffffb11aull, 0xfffffffffffffba1ull, 0xffffffffffffffc5ull, 0xfffffffffffffffdull,
      0xffffffffffffffffull};
  int w = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) w += h >= T[k];
  if (h >= T[6]) {
#pragma unroll
    for (int k = 6; k < kBootThresholds; ++k) w += h >= T[k];
  }
  return w;
}

// w(r, u) from key(r) and the unit's hash: replicate 0 is the sample itself.
BCE_BOOT_HD int boot_weight(uint64_t key, uint64_t unit_hash, int64_t r) {
  return r == 0 ? 1 : boot_count(boot_mix(key ^ unit_hash));
}

}  // namespace bce
