// score_boot.hip -- the paired Poisson bootstrap of back-test scores (include/bce.h):
// the sums of bce_score_groups under n_rep resamples of the markets, for up to BCE_BOOT_MAX_SETS
// forecast sets that share every resample.
//
// Every output depends on the arguments alone: a weight is an integer function of (seed,
// replicate, unit) (boot_weights.hpp), the summation shape is fixed by the group lengths, and
// there are no floating-point atomics.
//   boot_segment_kernel<K>  one 256-thread workgroup per (segment, 256 replicates): lane t owns
//     replicate blockIdx.y * 256 + t.  The workgroup walks the segment's items in tiles of
//     kBootTile: thread t classifies item t of the tile once per set (score_item.hpp: the item
//     rule of bce_score_groups) and stages the unit's hash, the scored / hit bits and the 3 K
//     terms in LDS; then every lane walks the tile, all lanes reading the same LDS address (a
//     broadcast: no bank conflict), computes ONE hash per item and adds (double)w * term, the
//     product then the add, into its 3 K fp64 and 2 K integer accumulators, which live in
//     registers (K is a template parameter: no dynamically indexed array).  The items are added
//     left to right from 0.0; an item that is not scored is the term 0.0 (w * 0.0 == 0.0 and
//     x + 0.0 == x for these non-negative sums), so no cross-lane reduction exists at all.  The
//     lane's row goes to the scratch table [segment][column][replicate] with ordinary stores,
//     coalesced over the replicates.
//   boot_finish_kernel  one thread per (group, column, replicate): the rows of the group's
//     segments added left to right from 0.0 (integers: plain sums), 8 loads in flight.
#include "boot_weights.hpp"
#include "score_item.hpp"

#pragma clang fp contract(off)

namespace bce {

constexpr int kBootTile = BCE_BOOT_TILE;  // items staged at a time: one per thread
constexpr int kBootCols = 5;              // W, W_hit, brier, logloss, brier_base: 8 bytes each
static_assert(kBootTile == kScoreT && kScoreSeg % kBootTile == 0, "a segment is a whole number of tiles");
static_assert(BCE_BOOT_MAX_SETS == 8, "boot_launch is instantiated for 1 .. 8 sets");
static_assert(BCE_BOOT_MAX_SETS <= 16, "the scored / hit bits of a tile item share one 32-bit word");

struct BootArgs {
  const int64_t* goff;       // [G + 1]
  int64_t G;
  const int64_t* seg_start;  // [G + 1]
  const int64_t* seg_group;  // [n_seg]
  int64_t n_seg;
  const int64_t* pidx;       // [n_items]
  const int64_t* oidx;       // [n_items], nullable: pidx
  int64_t n_items;
  const double* value;       // set k at value + k * value_stride, n_values entries
  int64_t n_values;
  int64_t value_stride;
  const int8_t* outcome;     // [n_markets]
  const uint8_t* valid;      // nullable; set k at valid + k * valid_stride
  int64_t valid_stride;
  const double* base;        // [n_markets] nullable
  const int64_t* unit;       // [n_markets] nullable: the market itself
  int64_t n_markets;
  double eps;
  uint64_t seed;
  int64_t rep0, n_rep;
  unsigned long long* rows;  // [n_seg][K * kBootCols][n_rep]
  int* fault;
};

__host__ __device__ constexpr int boot_lds_bytes(int K) { return kBootTile * (3 * K * 8 + 8 + 4); }

template <int K>
__global__ __launch_bounds__(kScoreT) void boot_segment_kernel(BootArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sBoot[];
  double* sTerm = reinterpret_cast<double*>(sBoot);                        // [tile][K][3]
  uint64_t* sHash = reinterpret_cast<uint64_t*>(sTerm + kBootTile * 3 * K);  // [tile] the unit's hash
  uint32_t* sBits = reinterpret_cast<uint32_t*>(sHash + kBootTile);        // [tile] bit k: scored in set k; 16 + k: hit
  const int t = threadIdx.x;
  const int64_t seg = blockIdx.x;
  int64_t i0, i1;
  int code = score_segment_items(a.goff, a.G, a.seg_start, a.seg_group, a.n_items, seg, &i0, &i1);
  const int64_t j = (int64_t)blockIdx.y * kScoreT + t;  // the lane's row
  const bool live = j < a.n_rep;
  const int64_t r = a.rep0 + j;
  const uint64_t key = boot_key(a.seed, r);
  const bool has_base = a.base != nullptr;

  double acc[K][3];
  int cnt[K][2];  // a segment holds at most kScoreSeg * 21 < 2^31
#pragma unroll
  for (int k = 0; k < K; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
    cnt[k][0] = cnt[k][1] = 0;
  }

  for (int64_t t0 = i0; t0 < i1; t0 += kBootTile) {
    const int n = (int)(i1 - t0 < kBootTile ? i1 - t0 : kBootTile);
    __syncthreads();  // every lane has left the previous tile
    if (t < n) {
      const int64_t i = t0 + t;
      const int64_t p = a.pidx[i];
      const int64_t m = a.oidx ? a.oidx[i] : p;
      const bool in = p >= 0 && p < a.n_values && m >= 0 && m < a.n_markets;
      uint32_t bits = 0;
      uint64_t hu = 0;
      int o = 0;
      double bs = 0.0;
      if (in) {
        o = (int)a.outcome[m];
        if (has_base) bs = a.base[m];
        hu = boot_unit_hash(a.unit ? a.unit[m] : m);
      } else {
        code = kFaultOffsets;  // an index outside its array: the item contributes nothing
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        double tb = 0.0, tl = 0.0, tbase = 0.0;
        if (in) {
          const double v = a.value[k * a.value_stride + p];
          const int ok = a.valid ? (int)a.valid[k * a.valid_stride + m] : 1;
          if (score_class(v, o, ok, has_base, bs) == kScScored) {
            const ScoreTerms it = score_terms(v, o, has_base, bs, a.eps);
            tb = it.brier;
            tl = it.logloss;
            tbase = it.brier_base;
            bits |= 1u << k;
            if (it.hit) bits |= 1u << (16 + k);
          }
        }
        sTerm[(t * K + k) * 3 + 0] = tb;
        sTerm[(t * K + k) * 3 + 1] = tl;
        sTerm[(t * K + k) * 3 + 2] = tbase;
      }
      sHash[t] = hu;
      sBits[t] = bits;
    }
    __syncthreads();
    if (!live) continue;
    for (int x = 0; x < n; ++x) {
      const uint32_t bits = sBits[x];
      if (bits == 0) continue;  // scored in no set: every term is 0.0 (the same word in every lane)
      const int w = boot_weight(key, sHash[x], r);
      const double wd = (double)w;
      const double* term = sTerm + x * 3 * K;
#pragma unroll
      for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double prod = wd * term[k * 3 + c];
          acc[k][c] = acc[k][c] + prod;
        }
        cnt[k][0] += (bits >> k) & 1u ? w : 0;
        cnt[k][1] += (bits >> (16 + k)) & 1u ? w : 0;
      }
    }
  }
  if (code && a.fault) atomicCAS(a.fault, 0, code);
  if (!live) return;
  unsigned long long* row = a.rows + seg * (K * kBootCols) * a.n_rep + j;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    row[(k * kBootCols + 0) * a.n_rep] = (unsigned long long)(long long)cnt[k][0];
    row[(k * kBootCols + 1) * a.n_rep] = (unsigned long long)(long long)cnt[k][1];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      row[(k * kBootCols + 2 + c) * a.n_rep] = (unsigned long long)__double_as_longlong(acc[k][c]);
  }
}

__global__ __launch_bounds__(kScoreT) void boot_finish_kernel(BootArgs a, int K, int64_t* counts, double* sums) {
  const int C = K * kBootCols;
  const int64_t id = (int64_t)blockIdx.x * kScoreT + threadIdx.x;
  if (id >= a.G * C * a.n_rep) return;
  const int64_t j = id % a.n_rep;
  const int64_t gc = id / a.n_rep;
  const int c = (int)(gc % C);
  const int64_t g = gc / C;
  int64_t s0 = a.seg_start[g], s1 = a.seg_start[g + 1];
  const int64_t b = a.goff[g], e = a.goff[g + 1];
  const bool range = b >= 0 && e >= b && e <= a.n_items;
  // every item is in exactly one segment only if the table holds the group's own segment count
  if (s0 < 0 || s1 < s0 || s1 > a.n_seg || s1 - s0 != score_segments(range ? e - b : 0)) {
    if (a.fault) atomicCAS(a.fault, 0, kFaultOffsets);
    s0 = s1 = 0;  // the group's outputs are zeros
  }
  const int k = c / kBootCols, cc = c % kBootCols;
  const bool is_f = cc >= 2;
  const int64_t step = (int64_t)C * a.n_rep;
  const unsigned long long* col = a.rows + (int64_t)c * a.n_rep + j;
  long long isum = 0;
  double fsum = 0.0;
  int64_t s = s0;
  for (; s + 8 <= s1; s += 8) {  // 8 loads in flight, then the ordered adds
    unsigned long long x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = col[(s + q) * step];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (is_f) fsum = fsum + __longlong_as_double((long long)x[q]); else isum += (long long)x[q];
    }
  }
  for (; s < s1; ++s) {
    const unsigned long long x = col[s * step];
    if (is_f) fsum = fsum + __longlong_as_double((long long)x); else isum += (long long)x;
  }
  const int64_t at = (j * a.G + g) * K + k;
  if (is_f) sums[at * 3 + (cc - 2)] = fsum; else counts[at * 2 + cc] = isum;
}

template <int K>
static int boot_launch(const BootArgs& a, int64_t* counts, double* sums, hipStream_t st) {
  const dim3 grid((unsigned)a.n_seg, (unsigned)((a.n_rep + kScoreT - 1) / kScoreT));
  hipLaunchKernelGGL(boot_segment_kernel<K>, grid, dim3(kScoreT), boot_lds_bytes(K), st, a);
  const int rs = check_launch("boot_segment_kernel");
  if (rs != BCE_OK) return rs;
  const int64_t fblocks = (a.G * K * kBootCols * a.n_rep + kScoreT - 1) / kScoreT;
  hipLaunchKernelGGL(boot_finish_kernel, dim3((unsigned)fblocks), dim3(kScoreT), 0, st, a, K, counts, sums);
  return check_launch("boot_finish_kernel");
}

}  // namespace bce

using namespace bce;

extern "C" int bce_boot_weights_host(int64_t seed, const int64_t* replicates, int64_t R, const int64_t* units,
                                     int64_t U, int32_t* w) {
  BCE_REQUIRE(R >= 0 && U >= 0, "boot_weights_host: negative size");
  BCE_REQUIRE((replicates || R == 0) && (units || U == 0) && (w || R == 0 || U == 0),
              "boot_weights_host: NULL replicates, units or weights");
  for (int64_t i = 0; i < R; ++i) BCE_REQUIRE(replicates[i] >= 0, "boot_weights_host: a replicate is negative");
  for (int64_t i = 0; i < R; ++i) {
    const uint64_t key = boot_key((uint64_t)seed, replicates[i]);
    for (int64_t u = 0; u < U; ++u) w[i * U + u] = boot_weight(key, boot_unit_hash(units[u]), replicates[i]);
  }
  return BCE_OK;
}

extern "C" int64_t bce_boot_scratch_bytes(int64_t n_segments, int64_t n_rep, int32_t n_sets) {
  if (n_segments < 0 || n_rep < 0 || n_sets < 1 || n_sets > BCE_BOOT_MAX_SETS) return 0;
  if (n_rep > 0 && n_segments > (INT64_MAX / (8 * kBootCols * BCE_BOOT_MAX_SETS)) / n_rep) return 0;
  return n_segments * n_rep * n_sets * kBootCols * 8;
}

extern "C" int bce_score_bootstrap(const int64_t* group_offsets, int64_t n_groups, const int64_t* seg_start,
                                   const int64_t* seg_group, int64_t n_segments, const int64_t* pidx,
                                   const int64_t* oidx, int64_t n_items, const double* value, int64_t n_values,
                                   int64_t value_stride, int32_t n_sets, const int8_t* outcome, const uint8_t* valid,
                                   int64_t valid_stride, const double* base, const int64_t* unit, int64_t n_markets,
                                   double eps, int64_t seed, int64_t rep0, int64_t n_rep, void* scratch,
                                   int64_t scratch_bytes, int64_t* counts, double* sums, void* stream) {
  BCE_REQUIRE(n_groups >= 0 && n_segments >= 0 && n_items >= 0 && n_values >= 0 && n_markets >= 0 && n_rep >= 0 &&
                  value_stride >= 0 && valid_stride >= 0,
              "score_bootstrap: negative size or stride");
  BCE_REQUIRE(n_sets >= 1 && n_sets <= BCE_BOOT_MAX_SETS, "score_bootstrap: n_sets must be in [1, %d] (got %d)",
              BCE_BOOT_MAX_SETS, (int)n_sets);
  BCE_REQUIRE(rep0 >= 0 && rep0 <= INT64_MAX - n_rep, "score_bootstrap: rep0 must be >= 0");
  BCE_REQUIRE(eps >= 0.0, "score_bootstrap: eps must be >= 0");  // NaN fails too
  if (n_groups == 0 || n_rep == 0) return BCE_OK;
  BCE_REQUIRE(group_offsets && seg_start && seg_group && counts && sums,
              "score_bootstrap: NULL offsets, segment table, counts or sums");
  BCE_REQUIRE(pidx || n_items == 0, "score_bootstrap: NULL item list");
  BCE_REQUIRE((value || n_values == 0) && (outcome || n_markets == 0), "score_bootstrap: NULL value or outcome");
  BCE_REQUIRE(n_segments >= n_groups && n_segments < (1ll << 31),
              "score_bootstrap: the segment table must hold 1 .. 2^31 - 1 segments, one or more per group");
  BCE_REQUIRE(n_rep <= 65535ll * kScoreT, "score_bootstrap: at most %lld replicates per call", 65535ll * kScoreT);
  BCE_REQUIRE(n_groups <= (1ll << 40), "score_bootstrap: too many groups");
  const int64_t need = bce_boot_scratch_bytes(n_segments, n_rep, n_sets);
  BCE_REQUIRE(need > 0 && scratch && scratch_bytes >= need && (uintptr_t)scratch % 8 == 0,
              "score_bootstrap: scratch must be 8-byte aligned and hold bce_boot_scratch_bytes()");
  const int64_t cells = n_groups * n_sets * kBootCols;
  BCE_REQUIRE(cells <= (((1ll << 31) - 1) * kScoreT) / n_rep, "score_bootstrap: too many groups times replicates");
  BootArgs a{group_offsets, n_groups,     seg_start, seg_group, n_segments, pidx,           oidx, n_items,
             value,         n_values,     value_stride, outcome, valid,      valid_stride,   base, unit,
             n_markets,     eps,          (uint64_t)seed, rep0,  n_rep,      reinterpret_cast<unsigned long long*>(scratch),
             fault_word()};
  hipStream_t st = as_stream(stream);
  switch (n_sets) {
    case 1: return boot_launch<1>(a, counts, sums, st);
    case 2: return boot_launch<2>(a, counts, sums, st);
    case 3: return boot_launch<3>(a, counts, sums, st);
    case 4: return boot_launch<4>(a, counts, sums, st);
    case 5: return boot_launch<5>(a, counts, sums, st);
    case 6: return boot_launch<6>(a, counts, sums, st);
    case 7: return boot_launch<7>(a, counts, sums, st);
    default: return boot_launch<8>(a, counts, sums, st);
  }
}
