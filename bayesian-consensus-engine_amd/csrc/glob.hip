// glob.hip -- market-id glob patterns against all ids at once, and the member lists of the
// matches: MarketId.matches (market.py:74-82) under MarketStore.list_markets(pattern=...)
// (:184-198) for every (pattern, market) pair, and the member loop of
// CrossMarketAggregator.aggregate_consensus (:352-357) for many pattern lists.
//
//   glob_match_kernel  bits[p][m / 64] bit (m % 64) = fnmatchcase(name m, pattern p).  One lane
//     per name, one wave per 64 consecutive names: an output word is one 64-bit ballot, written
//     by lane 0 with an ordinary store, exactly once (grid = name tiles x pattern-tile stripes).
//     A workgroup stages its 256 names once in LDS -- 64 bytes per lane, dword-transposed
//     (dword d of lane l at [d][l], bank l % 32 whatever d: lanes at different byte positions
//     never conflict, where a 64-byte slot per lane would be a 16-way conflict) -- and reuses
//     them over every pattern tile of its stripe; a tile's programs are staged in LDS too (each
//     lane is at its own op).  A longer name is matched from global memory by the same matcher.
//   glob_count_kernel  cnt[r] = popcount of row rows[r]; one wave per slot.
//   glob_fill_kernel   the same walk; a wave-level exclusive scan of the popcounts gives every
//     lane the position of its word's first set bit, and it expands its own word.
#include "bce_device.hpp"
#include "bce_internal.hpp"
#include "consensus_common.hpp"
#include "glob_match.hpp"

namespace bce {

constexpr int kGlobT = 256;                   // threads = names per workgroup
constexpr int kGlobSlot = 64;                 // bytes of a name staged in LDS
constexpr int kGlobSlotW = kGlobSlot / 4;
// Patterns per tile.  16 and 64 measured the same as 32 (260.7-261.3 / 259.9-260.9 against
// 260.5-261.1 ms on the 1M x 5777 shape, three interleaved repetitions); so did a literal-prefix
// prefilter on the name's first byte held in a register (261.4-262.1 ms, and 7.19-7.23 against
// 6.83-6.87 ms on the prefix patterns alone): the matcher's first step is the same test.  Neither
// is kept (measurements/glob_match.txt).
constexpr int kGlobPT = 32;
constexpr int kGlobProgLds = 2048;            // ops of a pattern tile staged in LDS (else global)
static_assert(kGlobPT <= kGlobT, "one thread per pattern of a tile reads its offsets");

struct GlobArgs {
  const uint8_t* name_bytes;
  int64_t n_bytes;
  const int64_t* name_off;
  int64_t M;
  const uint32_t* prog;
  int64_t n_ops;
  const int64_t* prog_off;
  int64_t P;
  GlobClasses cls;
  uint64_t* bits;
  int* fault;
};

struct GlobLdsName {  // this lane's column of the transposed tile
  const uint32_t* col;
  __device__ uint32_t operator()(int32_t i) const { return (col[(i >> 2) * kWave] >> ((i & 3) * 8)) & 0xFFu; }
};

__global__ __launch_bounds__(kGlobT) void glob_match_kernel(GlobArgs a) {
  __shared__ uint32_t sName[kGlobT / kWave][kGlobSlotW][kWave];
  __shared__ uint32_t sProg[kGlobProgLds];
  __shared__ int64_t sPb[kGlobPT];
  __shared__ int32_t sPn[kGlobPT];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t m = (int64_t)blockIdx.x * kGlobT + t;
  const int64_t n_words = (a.M + 63) / 64;
  const int64_t wi = (int64_t)blockIdx.x * (kGlobT / kWave) + w;
  bool live = m < a.M;
  int64_t nb = 0;
  int32_t len = 0;
  if (live) {
    nb = a.name_off[m];
    const int64_t ne = a.name_off[m + 1];
    if (nb < 0 || ne < nb || ne > a.n_bytes || ne - nb > (int64_t)INT32_MAX) {
      live = false;
      if (a.fault) atomicCAS(a.fault, 0, kFaultOffsets);
    } else {
      len = (int32_t)(ne - nb);
    }
  }
  const uint8_t* src = a.name_bytes + nb;
  const bool in_lds = len <= kGlobSlot;
  if (live && in_lds) {
    for (int d = 0; d * 4 < len; ++d) {
      uint32_t v = 0;
      if (d * 4 + 4 <= len) {
        __builtin_memcpy(&v, src + d * 4, 4);
      } else {
        for (int k = 0; d * 4 + k < len; ++k) v |= (uint32_t)src[d * 4 + k] << (8 * k);
      }
      sName[w][d][lane] = v;
    }
  }
  const GlobLdsName lds_name{&sName[w][0][lane]};
  const GlobBytes mem_name{src};
  const int64_t n_tiles = (a.P + kGlobPT - 1) / kGlobPT;
  for (int64_t pt = blockIdx.y; pt < n_tiles; pt += gridDim.y) {
    const int64_t p0 = pt * kGlobPT;
    const int np = (int)((a.P - p0) < kGlobPT ? (a.P - p0) : kGlobPT);
    __syncthreads();  // the names are staged; the last tile's programs are no longer read
    int badp = 0;
    if (t < np) {
      const int64_t ob = a.prog_off[p0 + t], oe = a.prog_off[p0 + t + 1];
      badp = ob < 0 || oe < ob || oe > a.n_ops || oe - ob > (int64_t)INT32_MAX;
      sPb[t] = ob;
      sPn[t] = badp ? -1 : (int32_t)(oe - ob);
    }
    const int any_bad = __syncthreads_or(badp);
    if (any_bad && t == 0 && a.fault) atomicCAS(a.fault, 0, kFaultOffsets);
    // every range valid => the tile is the contiguous run [first begin, last end)
    const int64_t tb = sPb[0];
    const int64_t total = any_bad ? 0 : sPb[np - 1] + sPn[np - 1] - tb;
    const bool prog_lds = !any_bad && total <= kGlobProgLds;
    if (prog_lds)
      for (int i = t; i < (int)total; i += kGlobT) sProg[i] = a.prog[tb + i];
    __syncthreads();
    for (int j = 0; j < np; ++j) {
      const int32_t n = sPn[j];
      int r = 0;
      if (live && n >= 0) {
        if (prog_lds) {
          const GlobOps ops{sProg + (sPb[j] - tb)};
          r = in_lds ? glob_match(ops, n, a.cls, lds_name, len) : glob_match(ops, n, a.cls, mem_name, len);
        } else {
          const GlobOps ops{a.prog + sPb[j]};
          r = in_lds ? glob_match(ops, n, a.cls, lds_name, len) : glob_match(ops, n, a.cls, mem_name, len);
        }
      }
      if (ballot(r < 0)) raise_fault(a.fault, kFaultOffsets);
      const unsigned long long word = ballot(r > 0);
      if (lane == 0 && wi < n_words) a.bits[(p0 + j) * n_words + wi] = word;
    }
  }
}

// One wave per slot; 4 slots per workgroup.
__global__ __launch_bounds__(kGlobT) void glob_count_kernel(const uint64_t* bits, int64_t n_words, int64_t P,
                                                            const int64_t* rows, int64_t R, int64_t* cnt,
                                                            int* fault) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (kGlobT / kWave) + (threadIdx.x >> 6);
  if (r >= R) return;
  const int64_t row = rows[r];
  int64_t c = 0;
  if (row < 0 || row >= P) {
    raise_fault(fault, kFaultOffsets);
  } else {
    const uint64_t* b = bits + row * n_words;
    for (int64_t i = lane; i < n_words; i += kWave) c += __popcll(b[i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) cnt[r] = c;
}

__global__ __launch_bounds__(kGlobT) void glob_fill_kernel(const uint64_t* bits, int64_t n_words, int64_t P,
                                                           const int64_t* rows, int64_t R, const int64_t* slot_off,
                                                           int64_t n_members, int64_t* members, int* fault) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (kGlobT / kWave) + (threadIdx.x >> 6);
  if (r >= R) return;
  const int64_t row = rows[r];
  const int64_t base = slot_off[r], end = slot_off[r + 1];
  if (row < 0 || row >= P || base < 0 || end < base || end > n_members) {
    raise_fault(fault, kFaultOffsets);
    return;
  }
  const uint64_t* b = bits + row * n_words;
  int64_t run = base;  // where the next chunk's first member goes
  for (int64_t i0 = 0; i0 < n_words; i0 += kWave) {
    const int64_t i = i0 + lane;
    uint64_t v = i < n_words ? b[i] : 0;
    if (!ballot(v != 0)) continue;
    const int c = __popcll(v);
    int inc = c;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int y = __shfl_up(inc, o);
      if (lane >= o) inc += y;
    }
    int64_t pos = run + (inc - c);
    while (v) {
      const int bit = __ffsll((unsigned long long)v) - 1;
      v &= v - 1;
      if (pos < end) members[pos] = i * 64 + bit;  // a slot sized for another bitmap is not overrun
      ++pos;
    }
    run += __shfl(inc, kWave - 1);
  }
  if (run != end) raise_fault(fault, kFaultOffsets);  // the slot was not sized by bce_glob_count
}

static int glob_check_host(const int64_t* off, int64_t n, int64_t limit) {
  for (int64_t i = 0; i < n; ++i)
    if (off[i] < 0 || off[i + 1] < off[i] || off[i + 1] > limit || off[i + 1] - off[i] > (int64_t)INT32_MAX) return 0;
  return 1;
}

}  // namespace bce

using namespace bce;

#define BCE_GLOB_REQUIRE_TABLES(fn)                                                                     \
  BCE_REQUIRE(M >= 0 && P >= 0 && n_bytes >= 0 && n_ops >= 0 && n_rng >= 0 && n_cls >= 0,               \
              fn ": negative size");                                                                    \
  BCE_REQUIRE(n_cls <= (int64_t)kGlobIndexMask, fn ": more than 2^28 - 1 classes");                     \
  if (M == 0 || P == 0) return BCE_OK;                                                                  \
  BCE_REQUIRE(name_off && prog_off && bits, fn ": NULL offsets or output");                             \
  BCE_REQUIRE(name_bytes || n_bytes == 0, fn ": NULL name bytes");                                      \
  BCE_REQUIRE(prog || n_ops == 0, fn ": NULL program");                                                 \
  BCE_REQUIRE((cls_rng || n_rng == 0) && (cls_off || n_cls == 0), fn ": NULL class table")

extern "C" int bce_glob_match(const uint8_t* name_bytes, int64_t n_bytes, const int64_t* name_off, int64_t M,
                              const uint32_t* prog, int64_t n_ops, const int64_t* prog_off, int64_t P,
                              const uint32_t* cls_rng, int64_t n_rng, const int32_t* cls_off, int64_t n_cls,
                              uint64_t* bits, void* stream) {
  BCE_GLOB_REQUIRE_TABLES("glob_match");
  const int64_t name_tiles = (M + kGlobT - 1) / kGlobT;
  BCE_REQUIRE(name_tiles <= (int64_t)INT32_MAX, "glob_match: more than 2^31 - 1 name tiles");
  // pattern stripes: enough workgroups to fill the device, as few restagings of the names as that allows
  const int64_t n_tiles = (P + kGlobPT - 1) / kGlobPT;
  int64_t stripes = (grid_cap(16) + name_tiles - 1) / name_tiles;
  if (stripes > n_tiles) stripes = n_tiles;
  if (stripes > 65535) stripes = 65535;
  if (stripes < 1) stripes = 1;
  GlobArgs a{name_bytes, n_bytes, name_off, M, prog, n_ops, prog_off, P, GlobClasses{cls_rng, n_rng, cls_off, n_cls},
             bits, fault_word()};
  hipLaunchKernelGGL(glob_match_kernel, dim3((unsigned)name_tiles, (unsigned)stripes), dim3(kGlobT), 0,
                     as_stream(stream), a);
  return check_launch("glob_match_kernel");
}

extern "C" int bce_glob_match_host(const uint8_t* name_bytes, int64_t n_bytes, const int64_t* name_off, int64_t M,
                                   const uint32_t* prog, int64_t n_ops, const int64_t* prog_off, int64_t P,
                                   const uint32_t* cls_rng, int64_t n_rng, const int32_t* cls_off, int64_t n_cls,
                                   uint64_t* bits) {
  BCE_GLOB_REQUIRE_TABLES("glob_match_host");
  BCE_REQUIRE(glob_check_host(name_off, M, n_bytes), "glob_match_host: name offsets decrease or leave the bytes");
  BCE_REQUIRE(glob_check_host(prog_off, P, n_ops), "glob_match_host: program offsets decrease or leave the ops");
  const GlobClasses cls{cls_rng, n_rng, cls_off, n_cls};
  const int64_t n_words = (M + 63) / 64;
  for (int64_t p = 0; p < P; ++p) {
    const GlobOps ops{prog + prog_off[p]};
    const int32_t n = (int32_t)(prog_off[p + 1] - prog_off[p]);
    for (int64_t wd = 0; wd < n_words; ++wd) {
      uint64_t word = 0;
      for (int64_t m = wd * 64; m < M && m < wd * 64 + 64; ++m) {
        const GlobBytes name{name_bytes + name_off[m]};
        const int r = glob_match(ops, n, cls, name, (int32_t)(name_off[m + 1] - name_off[m]));
        BCE_REQUIRE(r >= 0, "glob_match_host: pattern %lld has an op or class index outside its table",
                    (long long)p);
        word |= (uint64_t)(r > 0) << (m & 63);
      }
      bits[p * n_words + wd] = word;
    }
  }
  return BCE_OK;
}

extern "C" int bce_glob_count(const uint64_t* bits, int64_t M, int64_t P, const int64_t* rows, int64_t R,
                              int64_t* cnt, void* stream) {
  BCE_REQUIRE(M >= 0 && P >= 0 && R >= 0, "glob_count: negative size");
  if (R == 0) return BCE_OK;
  BCE_REQUIRE(rows && cnt, "glob_count: NULL rows or output");
  BCE_REQUIRE(bits || M == 0 || P == 0, "glob_count: NULL bitmap");
  const int64_t grid = (R + kGlobT / kWave - 1) / (kGlobT / kWave);
  BCE_REQUIRE(grid <= (int64_t)INT32_MAX, "glob_count: too many slots");
  hipLaunchKernelGGL(glob_count_kernel, dim3((unsigned)grid), dim3(kGlobT), 0, as_stream(stream), bits,
                     (M + 63) / 64, P, rows, R, cnt, fault_word());
  return check_launch("glob_count_kernel");
}

extern "C" int bce_glob_fill(const uint64_t* bits, int64_t M, int64_t P, const int64_t* rows, int64_t R,
                             const int64_t* slot_off, int64_t n_members, int64_t* members, void* stream) {
  BCE_REQUIRE(M >= 0 && P >= 0 && R >= 0 && n_members >= 0, "glob_fill: negative size");
  if (R == 0) return BCE_OK;
  BCE_REQUIRE(rows && slot_off, "glob_fill: NULL rows or slot offsets");
  BCE_REQUIRE(members || n_members == 0, "glob_fill: NULL members");
  BCE_REQUIRE(bits || M == 0 || P == 0, "glob_fill: NULL bitmap");
  const int64_t grid = (R + kGlobT / kWave - 1) / (kGlobT / kWave);
  BCE_REQUIRE(grid <= (int64_t)INT32_MAX, "glob_fill: too many slots");
  hipLaunchKernelGGL(glob_fill_kernel, dim3((unsigned)grid), dim3(kGlobT), 0, as_stream(stream), bits,
                     (M + 63) / 64, P, rows, R, slot_off, n_members, members, fault_word());
  return check_launch("glob_fill_kernel");
}
