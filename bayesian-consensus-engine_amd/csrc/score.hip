// score.hip -- proper scoring of forecasts against resolved outcomes: Brier score, log loss, hit
// count and a calibration histogram per group of items (include/bce.h).
//
// A group is a CSR list of items; item i reads its forecast value[pidx[i]] and its market
// m = oidx[i] (outcome, valid, base by market).  The same kernel scores market groups (value =
// the consensus, pidx = oidx = the members bce_glob_fill emits) and sources (value = the signal
// probabilities, pidx = the signals sorted by source, oidx = their markets).
//
// Every fp64 output depends on the arguments alone: no floating-point atomics, and the
// summation shape is fixed by the group lengths.
//   score_segment_kernel  one 256-thread workgroup per segment of kScoreSeg consecutive items of
//     one group.  Lane t adds the terms of items t, t + 256, t + 512 ... of the segment left to
//     right from 0.0 (a term that is not scored is 0.0: x + 0.0 == x for these non-negative
//     terms); the 256 lane partials are folded by the halving tree p[l] += p[l + o], o = 128 .. 1.
//     The calibration sums are the same tree over the masked terms (bin == b ? v : 0.0): a lane
//     keeps its B bin sums in a private LDS column (a dynamically indexed register array would go
//     to scratch memory), so no lane ever adds into another lane's sum.  Integer counters are LDS
//     integer atomics (exact).  The segment's row goes to the scratch table with ordinary stores.
//     The segment's group comes from seg_group[] (one load; the caller's table).
//   score_finish_kernel   one thread per (group, column): the rows of the group's segments added
//     left to right from 0.0 (integers: plain sums), 16 loads in flight ahead of the ordered adds.
#include "bce_device.hpp"
#include "bce_internal.hpp"
#include "consensus_common.hpp"
#include "score_item.hpp"

#pragma clang fp contract(off)

namespace bce {

constexpr int kScorePer = kScoreSeg / kScoreT;  // items per lane and segment
static_assert(kScoreSeg % kScoreT == 0, "a segment is a whole number of lane strides");

// Columns of a scratch row / of the outputs, 8 bytes each:
//   [0, 5) counts  [5, 8) sums  [8, 8 + B) bin_n  [8 + B, 8 + 2B) bin_pos  [8 + 2B, 8 + 3B) bin_psum
constexpr int kScoreFixed = 8;
__host__ __device__ constexpr int score_cols(int B) { return kScoreFixed + 3 * B; }

struct ScoreArgs {
  const int64_t* goff;       // [G + 1]
  int64_t G;
  const int64_t* seg_start;  // [G + 1]
  const int64_t* seg_group;  // [n_seg] the group of every segment
  int64_t n_seg;
  const int64_t* pidx;       // [n_items]
  const int64_t* oidx;       // [n_items], nullable: pidx
  int64_t n_items;
  const double* value;       // [n_values]
  int64_t n_values;
  const int8_t* outcome;     // [n_markets]
  const uint8_t* valid;      // [n_markets] nullable
  const double* base;        // [n_markets] nullable
  int64_t n_markets;
  int B;
  double eps;
  unsigned long long* rows;  // [n_seg][score_cols(B)]
  int* fault;
};

// Fold the 256 lane partials of column c by the halving tree; valid in lane 0 of the wave.
__device__ __forceinline__ double score_tree(const double* col, int lane) {
  double v0 = col[lane], v1 = col[lane + 64];
  const double v2 = col[lane + 128], v3 = col[lane + 192];
  v0 = v0 + v2;  // o = 128
  v1 = v1 + v3;
  v0 = v0 + v1;  // o = 64
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v0 = v0 + __shfl_down(v0, o);  // lanes < o hold p[l] + p[l + o]
  return v0;
}

__global__ __launch_bounds__(kScoreT) void score_segment_kernel(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sCol[];  // [3 + B][256], lane-private columns
  __shared__ int sInt[5 + 2 * BCE_SCORE_MAX_BINS];               // counts, bin_n, bin_pos
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int B = a.B;
  const int64_t seg = blockIdx.x;
  int64_t i0, i1;  // the segment's items
  int code = score_segment_items(a.goff, a.G, a.seg_start, a.seg_group, a.n_items, seg, &i0, &i1);
  for (int c = t; c < 5 + 2 * B; c += kScoreT) sInt[c] = 0;
  for (int b = 0; b < B; ++b) sCol[(3 + b) * kScoreT + t] = 0.0;
  __syncthreads();

  int64_t p[kScorePer], m[kScorePer];
#pragma unroll
  for (int k = 0; k < kScorePer; ++k) {
    const int64_t i = i0 + k * kScoreT + t;
    p[k] = -1;
    m[k] = -1;
    if (i < i1) {
      p[k] = a.pidx[i];
      m[k] = a.oidx ? a.oidx[i] : p[k];
    }
  }
  double v[kScorePer], bs[kScorePer];
  int o[kScorePer], ok[kScorePer], cls[kScorePer];  // cls: -1 = no item
#pragma unroll
  for (int k = 0; k < kScorePer; ++k) {
    const bool item = i0 + k * kScoreT + t < i1;
    const bool in = item && p[k] >= 0 && p[k] < a.n_values && m[k] >= 0 && m[k] < a.n_markets;
    v[k] = in ? a.value[p[k]] : 0.0;
    o[k] = in ? (int)a.outcome[m[k]] : 0;
    ok[k] = in ? (a.valid ? (int)a.valid[m[k]] : 1) : 0;
    bs[k] = (in && a.base) ? a.base[m[k]] : 0.0;
    cls[k] = !item ? -1 : in ? 0 : kScBad;
    if (item && !in) code = kFaultOffsets;  // an index outside its array: counted as bad
  }
  double brier = 0.0, ll = 0.0, bbase = 0.0;
#pragma unroll
  for (int k = 0; k < kScorePer; ++k) {
    if (cls[k] < 0) continue;
    if (cls[k] == 0) cls[k] = score_class(v[k], o[k], ok[k], a.base != nullptr, bs[k]);
    atomicAdd(&sInt[cls[k]], 1);
    if (cls[k] != kScScored) continue;
    const ScoreTerms it = score_terms(v[k], o[k], a.base != nullptr, bs[k], a.eps);
    brier = brier + it.brier;
    ll = ll + it.logloss;
    if (a.base) bbase = bbase + it.brier_base;
    if (it.hit) atomicAdd(&sInt[kScHit], 1);
    int bin = (int)(v[k] * (double)B);
    if (bin > B - 1) bin = B - 1;
    atomicAdd(&sInt[5 + bin], 1);
    if (o[k] == 1) atomicAdd(&sInt[5 + B + bin], 1);
    double* mine = &sCol[(3 + bin) * kScoreT + t];
    *mine = *mine + v[k];
  }
  sCol[0 * kScoreT + t] = brier;
  sCol[1 * kScoreT + t] = ll;
  sCol[2 * kScoreT + t] = bbase;
  if (code && a.fault) atomicCAS(a.fault, 0, code);
  __syncthreads();

  unsigned long long* row = a.rows + seg * score_cols(B);
  for (int c = w; c < 3 + B; c += kScoreT / kWave) {
    const double s = score_tree(sCol + c * kScoreT, lane);
    if (lane == 0) row[c < 3 ? 5 + c : kScoreFixed + 2 * B + (c - 3)] = (unsigned long long)__double_as_longlong(s);
  }
  for (int c = t; c < 5 + 2 * B; c += kScoreT)
    row[c < 5 ? c : kScoreFixed + (c - 5)] = (unsigned long long)(long long)sInt[c];
}

struct ScoreOut {
  int64_t* counts;   // [G][5]
  double* sums;      // [G][3] nullable
  int64_t* bin_n;    // [G][B] nullable
  int64_t* bin_pos;  // [G][B] nullable
  double* bin_psum;  // [G][B] nullable
};

__global__ __launch_bounds__(kScoreT) void score_finish_kernel(ScoreArgs a, ScoreOut out) {
  const int B = a.B, C = score_cols(B);
  const int64_t id = (int64_t)blockIdx.x * kScoreT + threadIdx.x;
  if (id >= a.G * C) return;
  const int64_t g = id / C;
  const int c = (int)(id - g * C);
  int64_t s0 = a.seg_start[g], s1 = a.seg_start[g + 1];
  const int64_t b = a.goff[g], e = a.goff[g + 1];
  const bool range = b >= 0 && e >= b && e <= a.n_items;
  // every item is in exactly one segment only if the table holds the group's own segment count
  if (s0 < 0 || s1 < s0 || s1 > a.n_seg || s1 - s0 != score_segments(range ? e - b : 0)) {
    if (a.fault) atomicCAS(a.fault, 0, kFaultOffsets);
    s0 = s1 = 0;  // the group's outputs are zeros
  }
  const bool is_f = (c >= 5 && c < kScoreFixed) || c >= kScoreFixed + 2 * B;
  long long isum = 0;
  double fsum = 0.0;
  int64_t s = s0;
  for (; s + 16 <= s1; s += 16) {  // 16 loads in flight, then the ordered adds
    unsigned long long x[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = a.rows[(s + k) * C + c];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (is_f) fsum = fsum + __longlong_as_double((long long)x[k]); else isum += (long long)x[k];
    }
  }
  for (; s < s1; ++s) {
    const unsigned long long x = a.rows[s * C + c];
    if (is_f) fsum = fsum + __longlong_as_double((long long)x); else isum += (long long)x;
  }
  if (c < 5) {
    out.counts[g * 5 + c] = isum;
  } else if (c < kScoreFixed) {
    if (out.sums) out.sums[g * 3 + (c - 5)] = fsum;
  } else if (c < kScoreFixed + B) {
    if (out.bin_n) out.bin_n[g * B + (c - kScoreFixed)] = isum;
  } else if (c < kScoreFixed + 2 * B) {
    if (out.bin_pos) out.bin_pos[g * B + (c - kScoreFixed - B)] = isum;
  } else {
    if (out.bin_psum) out.bin_psum[g * B + (c - kScoreFixed - 2 * B)] = fsum;
  }
}

}  // namespace bce

using namespace bce;

extern "C" int64_t bce_score_scratch_bytes(int64_t n_segments, int32_t n_bins) {
  if (n_segments < 0 || n_bins < 1 || n_bins > BCE_SCORE_MAX_BINS) return 0;
  return n_segments * (int64_t)score_cols(n_bins) * 8;
}

extern "C" int bce_score_groups(const int64_t* group_offsets, int64_t n_groups, const int64_t* seg_start,
                                const int64_t* seg_group, int64_t n_segments, const int64_t* pidx, const int64_t* oidx, int64_t n_items,
                                const double* value, int64_t n_values, const int8_t* outcome, const uint8_t* valid,
                                const double* base, int64_t n_markets, int32_t n_bins, double eps, void* scratch,
                                int64_t scratch_bytes, int64_t* counts, double* sums, int64_t* bin_n,
                                int64_t* bin_pos, double* bin_psum, void* stream) {
  BCE_REQUIRE(n_groups >= 0 && n_segments >= 0 && n_items >= 0 && n_values >= 0 && n_markets >= 0,
              "score_groups: negative size");
  BCE_REQUIRE(n_bins >= 1 && n_bins <= BCE_SCORE_MAX_BINS, "score_groups: n_bins must be in [1, %d] (got %d)",
              BCE_SCORE_MAX_BINS, (int)n_bins);
  BCE_REQUIRE(eps >= 0.0, "score_groups: eps must be >= 0");  // NaN fails too
  if (n_groups == 0) return BCE_OK;
  BCE_REQUIRE(group_offsets && seg_start && seg_group && counts, "score_groups: NULL offsets, segment table or counts");
  BCE_REQUIRE(pidx || n_items == 0, "score_groups: NULL item list");
  BCE_REQUIRE((value || n_values == 0) && (outcome || n_markets == 0), "score_groups: NULL value or outcome");
  BCE_REQUIRE(n_segments >= n_groups && n_segments < (1ll << 31), "score_groups: the segment table must hold 1 .. 2^31 - 1 segments, one or more per group");
  BCE_REQUIRE(n_groups <= (1ll << 40), "score_groups: too many groups");
  BCE_REQUIRE(scratch && scratch_bytes >= bce_score_scratch_bytes(n_segments, n_bins) && (uintptr_t)scratch % 8 == 0,
              "score_groups: scratch must be 8-byte aligned and hold bce_score_scratch_bytes()");
  const int C = score_cols(n_bins);
  const int64_t fblocks = (n_groups * C + kScoreT - 1) / kScoreT;
  BCE_REQUIRE(fblocks < (1ll << 31), "score_groups: too many groups");
  ScoreArgs a{group_offsets, n_groups, seg_start, seg_group, n_segments, pidx,   oidx, n_items,
              value,         n_values, outcome,   valid,      base,   n_markets, (int)n_bins,
              eps,           reinterpret_cast<unsigned long long*>(scratch), fault_word()};
  const int lds = (3 + (int)n_bins) * kScoreT * 8;
  const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(score_segment_kernel), (3 + BCE_SCORE_MAX_BINS) * kScoreT * 8);
  if (rc != BCE_OK) return rc;
  hipLaunchKernelGGL(score_segment_kernel, dim3((unsigned)n_segments), dim3(kScoreT), lds, as_stream(stream), a);
  const int rs = check_launch("score_segment_kernel");
  if (rs != BCE_OK) return rs;
  ScoreOut out{counts, sums, bin_n, bin_pos, bin_psum};
  hipLaunchKernelGGL(score_finish_kernel, dim3((unsigned)fblocks), dim3(kScoreT), 0, as_stream(stream), a, out);
  return check_launch("score_finish_kernel");
}
