// glob_fuzz.cpp -- csrc/glob_match.hpp as plain C++ under AddressSanitizer + UBSan (CPU only):
// seeded random programs, well-formed and malformed (op kinds 0..7, class indices and class rows
// outside their tables, negative and decreasing class offsets), over random byte strings (ASCII,
// valid multi-byte UTF-8, truncated sequences, stray continuation bytes).  Every array is an
// exactly sized heap allocation, so one byte or op read outside a name, a program or a table is
// a sanitizer report.  Well-formed star/literal/any programs over ASCII are also compared with a
// recursive matcher.  usage: glob_fuzz [rounds]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "glob_match.hpp"

using namespace bce;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (uint32_t)(g_state >> 16);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

// exponential-time reference for ops of kind literal / any / star over single-byte names
static bool ref_match(const uint32_t* op, int n, const uint8_t* s, int len) {
  if (n == 0) return len == 0;
  const uint32_t kind = op[0] >> kGlobKindShift;
  if (kind == kGlobStar) {
    for (int k = 0; k <= len; ++k)
      if (ref_match(op + 1, n - 1, s + k, len - k)) return true;
    return false;
  }
  if (len == 0) return false;
  if (kind == kGlobLit && (op[0] & kGlobCpMask) != s[0]) return false;
  return ref_match(op + 1, n - 1, s + 1, len - 1);
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 20000;
  long matched = 0, faulted = 0, compared = 0;
  for (int it = 0; it < rounds; ++it) {
    const bool wild = below(4) == 0;  // malformed tables
    // the class table
    const int n_cls = (int)below(4);
    std::vector<int32_t> off((size_t)n_cls + 1);
    std::vector<uint32_t> rng;
    off[0] = 0;
    for (int c = 0; c < n_cls; ++c) {
      const int k = (int)below(4);
      for (int r = 0; r < k; ++r) {
        const uint32_t lo = below(2) ? below(0x80) : below(0x110000);
        rng.push_back(lo);
        rng.push_back(lo + below(3));
      }
      off[(size_t)c + 1] = (int32_t)(rng.size() / 2);
    }
    int64_t n_rng = (int64_t)(rng.size() / 2);
    if (wild && n_cls) {
      const int c = (int)below((uint32_t)n_cls + 1);
      const uint32_t how = below(4);
      off[(size_t)c] = how == 0 ? -1 : how == 1 ? (int32_t)n_rng + 1 + (int32_t)below(100) : how == 2 ? INT32_MAX : 0;
    }
    uint32_t* rng_heap = (uint32_t*)malloc(rng.size() * 4 + 1);  // exactly sized (the + 1: malloc(0))
    for (size_t i = 0; i < rng.size(); ++i) rng_heap[i] = rng[i];
    int32_t* off_heap = (int32_t*)malloc(off.size() * 4);
    for (size_t i = 0; i < off.size(); ++i) off_heap[i] = off[i];
    const GlobClasses cls{rng_heap, n_rng, n_cls ? off_heap : nullptr, n_cls};
    // the program
    const int n_ops = (int)below(9);
    uint32_t* prog = (uint32_t*)malloc((size_t)n_ops * 4 + 1);
    bool simple = true;
    for (int i = 0; i < n_ops; ++i) {
      uint32_t kind = below(wild ? 8 : 4);
      if (kind == kGlobCls && !wild && n_cls == 0) kind = kGlobAny;
      uint32_t payload = 0;
      if (kind == kGlobLit) payload = below(3) ? 'a' + below(3) : below(0x110000);
      if (kind == kGlobCls) payload = (wild ? below(6) : below((uint32_t)n_cls)) | (below(2) ? kGlobNegate : 0);
      if (wild && below(8) == 0) payload = rnd() & ((1u << kGlobKindShift) - 1);
      if (kind > kGlobStar || payload >= 0x80) simple = false;
      prog[i] = (kind << kGlobKindShift) | payload;
    }
    // the name
    const int len = (int)below(below(8) ? 14 : 300);
    uint8_t* name = (uint8_t*)malloc((size_t)len + 1);
    const uint32_t flavour = below(3);
    bool ascii = true;
    for (int i = 0; i < len; ++i) {
      if (flavour == 0) {
        name[i] = (uint8_t)('a' + below(3));
      } else if (flavour == 1) {
        name[i] = (uint8_t)rnd();
      } else {
        static const uint8_t lead[] = {'a', 'b', 0xC3, 0xE2, 0xF0, 0x82, 0xED, 0xFF};
        name[i] = below(2) ? lead[below(8)] : (uint8_t)(0x80 + below(0x40));
      }
      if (name[i] >= 0x80) ascii = false;
    }
    const int r = glob_match(GlobOps{prog}, n_ops, cls, GlobBytes{name}, len);
    if (r < -1 || r > 1) {
      fprintf(stderr, "glob_fuzz: result %d\n", r);
      return 1;
    }
    if (!wild && r < 0) {
      fprintf(stderr, "glob_fuzz: a well-formed program was reported malformed (round %d)\n", it);
      return 1;
    }
    matched += r > 0;
    faulted += r < 0;
    if (!wild && simple && ascii && len <= 14) {
      ++compared;
      if ((r > 0) != ref_match(prog, n_ops, name, len)) {
        fprintf(stderr, "glob_fuzz: differs from the recursive matcher (round %d)\n", it);
        return 1;
      }
    }
    free(name);
    free(prog);
    free(off_heap);
    free(rng_heap);
  }
  if (matched == 0 || faulted == 0 || compared == 0) {
    fprintf(stderr, "glob_fuzz: the corpus is one-sided (%ld matched, %ld malformed, %ld compared)\n", matched,
            faulted, compared);
    return 1;
  }
  printf("glob_fuzz ok: %d rounds, %ld matched, %ld malformed, %ld compared\n", rounds, matched, faulted, compared);
  return 0;
}
