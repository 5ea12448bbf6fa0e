// glob_match.hpp -- fnmatch.fnmatchcase(name, pattern) for one compiled pattern and one name,
// shared by the device kernel (glob.hip), the host entry bce_glob_match_host and the CPU
// sanitizer harness (tests/native/glob_fuzz.cpp).  Plain C++: BCE_HD is empty under g++.
//
// A pattern is compiled on the host (batch.GlobSet.compile, a restatement of CPython 3.10's
// fnmatch.translate) into 32-bit ops, kind in bits 31..29:
//   kGlobLit   bits 20..0 = the code point that must come next
//   kGlobAny   any one code point ('?', '[!]'-like sets that translate() turns into '.')
//   kGlobStar  any run of code points, newline included; runs of '*' arrive as one op
//   kGlobCls   bits 27..0 = class index, bit 28 = negate; the class is a CSR row of inclusive
//              [lo, hi] code-point ranges (an empty row never matches, negated: always)
// translate() anchors every "STAR fixed" piece at its leftmost match and never backtracks over
// it; with '*' the only op of variable width that gives the same boolean as the classic
// iterative matcher below: one saved (op, byte) position, retried one code point later on a
// mismatch.  The matcher only ever decodes forward, so it walks UTF-8 directly; lone surrogates
// are the 3-byte sequences of 'surrogatepass'.
//
// Bounds: name bytes are read through name(i) with 0 <= i < len only, ops through prog(i) with
// 0 <= i < n_ops only, class rows only after their offsets were checked against the tables.
// Bytes that are not UTF-8 decode to some code point of 1..4 bytes clipped to the name.
#pragma once
#include <stdint.h>

#ifndef BCE_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BCE_HD __host__ __device__
#else
#define BCE_HD
#endif
#endif

namespace bce {

constexpr uint32_t kGlobLit = 0, kGlobAny = 1, kGlobStar = 2, kGlobCls = 3;
constexpr int kGlobKindShift = 29;
constexpr uint32_t kGlobNegate = 1u << 28;
constexpr uint32_t kGlobIndexMask = kGlobNegate - 1;
constexpr uint32_t kGlobCpMask = 0x1FFFFFu;

// The class side table: row c is rng[2 * off[c] .. 2 * off[c + 1]) as (lo, hi) pairs.
struct GlobClasses {
  const uint32_t* rng;
  int64_t n_rng;
  const int32_t* off;  // [n_cls + 1], or NULL when n_cls == 0
  int64_t n_cls;
};

struct GlobBytes {  // a name in ordinary memory
  const uint8_t* p;
  BCE_HD uint32_t operator()(int32_t i) const { return p[i]; }
};
struct GlobOps {  // a program in ordinary memory
  const uint32_t* p;
  BCE_HD uint32_t operator()(int32_t i) const { return p[i]; }
};

// Bytes of the code point that starts at i (1..4 by its lead byte), clipped to the name.
template <class Name>
BCE_HD inline int32_t glob_width(const Name& name, int32_t i, int32_t len) {
  const uint32_t b = name(i);
  const int32_t w = b < 0xC0u ? 1 : b < 0xE0u ? 2 : b < 0xF0u ? 3 : 4;
  return w < len - i ? w : len - i;
}

template <class Name>
BCE_HD inline uint32_t glob_decode(const Name& name, int32_t i, int32_t len, int32_t* width) {
  const uint32_t b = name(i);
  int32_t w = b < 0xC0u ? 1 : b < 0xE0u ? 2 : b < 0xF0u ? 3 : 4;
  uint32_t cp = w == 1 ? b : w == 2 ? (b & 0x1Fu) : w == 3 ? (b & 0x0Fu) : (b & 0x07u);
  if (w > len - i) w = len - i;
  for (int32_t k = 1; k < w; ++k) cp = (cp << 6) | (name(i + k) & 0x3Fu);
  *width = w;
  return cp;
}

// 1: the program matches the whole name; 0: it does not; -1: the program is malformed (an op
// kind or a class index outside its table, a class row outside the range table) -- no match.
template <class Prog, class Name>
BCE_HD inline int glob_match(const Prog& prog, int32_t n_ops, const GlobClasses& cls, const Name& name,
                             int32_t len) {
  int32_t pi = 0, ni = 0;     // next op, next name byte
  int32_t spi = -1, sni = 0;  // the op after the last star, and where its current try began
  for (;;) {
    if (pi < n_ops) {
      const uint32_t op = prog(pi);
      const uint32_t kind = op >> kGlobKindShift;
      if (kind == kGlobStar) {
        if (pi + 1 == n_ops) return 1;  // a trailing star takes whatever is left
        spi = ++pi;
        sni = ni;
        continue;
      }
      if (kind > kGlobCls) return -1;
      if (ni < len) {
        int32_t w;
        const uint32_t cp = glob_decode(name, ni, len, &w);
        bool ok;
        if (kind == kGlobLit) {
          ok = cp == (op & kGlobCpMask);
        } else if (kind == kGlobAny) {
          ok = true;
        } else {
          const int64_t c = (int64_t)(op & kGlobIndexMask);
          if (c >= cls.n_cls) return -1;
          const int64_t a = cls.off[c], b = cls.off[c + 1];
          if (a < 0 || b < a || b > cls.n_rng) return -1;
          bool in = false;
          for (int64_t r = a; r < b; ++r) in = in || (cls.rng[2 * r] <= cp && cp <= cls.rng[2 * r + 1]);
          ok = in != ((op & kGlobNegate) != 0);
        }
        if (ok) {
          ++pi;
          ni += w;
          continue;
        }
      }
    } else if (ni == len) {
      return 1;
    }
    // mismatch: let the last star take one more code point
    if (spi < 0 || sni >= len) return 0;
    sni += glob_width(name, sni, len);
    ni = sni;
    pi = spi;
  }
}

}  // namespace bce
