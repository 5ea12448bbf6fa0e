// settle.hip -- commit a batch of resolved markets to one scope of the reliability table.
//
// The reference settles one signal at a time: update_reliability(source, correct) for every
// signal of every resolved market (reliability.py:142-233, reliability_abstraction.py:190-240),
// correct = (probability >= 0.5) == outcome (market.py:298-301).  A source that signals in many
// markets therefore receives a CHAIN of updates whose result depends on their order (the [0, 1]
// clamp of the reliability, the rounding of the confidence at every step).  A batch is compiled
// once into one correctness bit per participating signal, the bits of a source contiguous and in
// the reference's loop order; applying it walks every source's bits through update_rel /
// update_conf (reliability_update.hpp), bit-exact.
//
//   settle_compile_kernel  one lane per sorted signal: gathers prob and outcome[market] through
//                          the permutation, 64 consecutive bits -> one u64 by a ballot; the
//                          popcount per source by int64 atomics on the plan's `correct`
//   settle_chain_kernel    one lane per touched source, longest chain first: the whole chain,
//                          for the first n_long sources only a snapshot of the start state
//   settle_long_kernel     one lane per chunk of a long chain.  After 11 equal bits in a row the
//                          reliability is exactly 1.0 or 0.0 whatever came before (ten steps of
//                          0.10 from 0.0 give 0.9999999999999999, the eleventh clamps to 1.0; the
//                          mirror from 1.0; every step is monotone and the state is inside [0, 1]
//                          after its first step), so the worker of chunk j >= 1 starts after the
//                          first such run that lies inside its chunk and every worker walks on
//                          until the next chunk's first run ends.  No communication, no atomics:
//                          exactly one worker reaches the chain's end and stores the result.
#include "bce_device.hpp"
#include "bce_internal.hpp"
#include "consensus_common.hpp"
#include "reliability_update.hpp"
#include "settle_walk.hpp"

#pragma clang fp contract(off)

namespace bce {

__global__ __launch_bounds__(256) void settle_compile_kernel(
    const int64_t* __restrict__ perm, int64_t Np, const int32_t* __restrict__ key,
    const int32_t* __restrict__ sid, const double* __restrict__ prob, const int32_t* __restrict__ market,
    int64_t N, const int8_t* __restrict__ outcome, int64_t M, int32_t S, unsigned long long* __restrict__ bits,
    unsigned long long* __restrict__ correct, int* fault) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;  // a wave holds 64 consecutive sorted signals
  const bool in = j < Np;
  bool bit = false;
  int code = 0;
  int32_t s = 0;
  if (in) {
    int64_t i = perm[j];
    if (i < 0 || i >= N) {  // not a signal of the batch: nothing is read through it
      code = kFaultOffsets;
      i = 0;
    }
    int32_t m = market[i];
    if (m < 0 || m >= M) {
      code = kFaultOffsets;
      m = 0;
    }
    const int32_t raw = sid[i];
    s = key[j];  // the sort key: the sid clamped by the caller
    if (raw < 0 || raw >= S || s < 0 || s >= S) {
      code = code ? code : kFaultSid;
      s = s < 0 ? 0 : (s >= S ? S - 1 : s);
    }
    const int8_t o = outcome[m];
    const double p = prob[i];
    // market.py:298-301; NaN >= 0.5 is false, a probability outside [0, 1] is not screened
    bit = code != kFaultOffsets && o >= 0 && ((p >= 0.5) == (o != 0));
  }
  const unsigned long long word = ballot(bit);
  if (ballot(in) == 0) return;
  const int lane = lane_id();
  if (lane == 0) bits[j >> 6] = word;  // lane 0 is inside whenever any lane of the wave is
  const int32_t s0 = __builtin_amdgcn_readfirstlane(s);
  if (ballot(in && s != s0) == 0) {  // one source fills the wave (the hot sources): one atomic
    if (lane == 0 && word) atomicAdd(&correct[s0], (unsigned long long)__popcll(word));
  } else if (bit) {
    atomicAdd(&correct[s], 1ull);
  }
  if (code && fault) atomicCAS(fault, 0, code);
}

__global__ __launch_bounds__(64) void settle_chain_kernel(SettleArgs a) {
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= a.T) return;
  int32_t s;
  int64_t b0, b1;
  if (!settle_range(a, q, s, b0, b1)) return;
  const bool pres = a.present ? a.present[s] != 0 : true;
  double r = pres ? a.rel[s] : a.default_rel;  // reliability.py:133-140 cold start
  double c = pres ? a.conf[s] : a.default_conf;
  if (q < a.n_long) {  // settle_long_kernel walks it; it must not read a row it may have written
    a.snap[q] = make_double2(r, c);
    return;
  }
  int run = 0;
  bool prev = false;
  settle_span<true, false>(a.bits, b0, 0, b1 - b0, r, run, prev);
  a.rel[s] = r;
  a.conf[s] = settle_conf(c, b1 - b0);
  a.t_us[s] = a.now_us;  // reliability.py:175
  if (a.present) a.present[s] = 1;
}

__global__ __launch_bounds__(64) void settle_long_kernel(SettleArgs a, const int64_t* __restrict__ chunk_start,
                                                         int64_t n_chunks, int64_t C) {
  const int64_t wk = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (wk >= n_chunks) return;
  // the long source this chunk belongs to: the last q with chunk_start[q] <= wk
  int64_t lo = 0, hi = a.n_long;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (chunk_start[mid] <= wk) lo = mid; else hi = mid;
  }
  const int64_t q = lo, j = wk - chunk_start[q];
  int32_t s;
  int64_t b0, b1;
  if (j < 0 || !settle_range(a, q, s, b0, b1)) return;
  const int64_t L = b1 - b0;
  if (j > (L - 1) / C) return;  // more chunks than the chain has: nothing to do
  const int64_t home_end = (j + 1) * C < L ? (j + 1) * C : L;
  double r = 0.0;
  int run = 0;
  bool prev = false;
  int64_t pos = j * C;
  if (j == 0) {  // the head worker: the stored state, and everything that is not the rel chain
    const double2 st = a.snap[q];
    r = st.x;
    a.conf[s] = settle_conf(st.y, L);
    a.t_us[s] = a.now_us;
    if (a.present) a.present[s] = 1;
  } else {  // the first run of kSyncRun equal bits that lies inside the home chunk
    const int64_t p = settle_span<false, true>(a.bits, b0, pos, home_end, r, run, prev);
    if (p < 0) return;    // none: the worker before walks through this chunk
    r = prev ? 1.0 : 0.0; // exact whatever came before
    pos = p + 1;
  }
  settle_span<true, false>(a.bits, b0, pos, home_end, r, run, prev);  // the rest of the home chunk
  for (int64_t c = home_end; c < L; c += C) {  // later chunks, until one has a sync run of its own
    const int64_t cend = c + C < L ? c + C : L;
    run = 0;  // a run counts from its chunk's first bit
    if (settle_span<true, true>(a.bits, b0, c, cend, r, run, prev) >= 0) return;  // that chunk's worker goes on
  }
  a.rel[s] = r;  // the one worker that reaches the chain's end
}

}  // namespace bce

using namespace bce;

extern "C" int bce_settle_compile(const int64_t* perm, int64_t n_part, const int32_t* key, const int32_t* sid,
                                  const double* prob, const int32_t* market, int64_t n_signals,
                                  const int8_t* outcome, int64_t n_markets, int32_t n_sources, uint64_t* bits,
                                  int64_t* correct, void* stream) {
  BCE_REQUIRE(n_part >= 0 && n_signals >= 0 && n_markets >= 0 && n_sources > 0, "settle_compile: bad shape");
  BCE_REQUIRE(n_markets < (1ll << 31), "settle_compile: n_markets >= 2^31");
  BCE_REQUIRE(n_part <= n_signals, "settle_compile: more participating signals than signals");
  if (n_part == 0) return BCE_OK;
  BCE_REQUIRE(n_markets > 0, "settle_compile: signals without markets");
  BCE_REQUIRE(perm && key && sid && prob && market && outcome && bits && correct, "settle_compile: NULL argument");
  const int64_t blocks = (n_part + 255) / 256;
  BCE_REQUIRE(blocks < (1ll << 31), "settle_compile: grid too large");
  hipLaunchKernelGGL(settle_compile_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), perm, n_part,
                     key, sid, prob, market, n_signals, outcome, n_markets, n_sources,
                     reinterpret_cast<unsigned long long*>(bits), reinterpret_cast<unsigned long long*>(correct),
                     fault_word());
  return check_launch("settle_compile_kernel");
}

extern "C" int bce_settle_apply(const uint64_t* bits, int64_t n_bits, const int64_t* start, const int32_t* order,
                                int64_t n_touched, int64_t n_long, const int64_t* chunk_start, int64_t n_chunks,
                                int64_t chunk_bits, int32_t n_sources, double* rel, double* conf, int64_t* t_us,
                                uint8_t* present, int64_t now_us, double default_rel, double default_conf,
                                double* snap, void* stream) {
  BCE_REQUIRE(n_bits >= 0 && n_touched >= 0 && n_sources > 0 && n_touched <= n_sources, "settle_apply: bad shape");
  BCE_REQUIRE(n_long >= 0 && n_long <= n_touched && n_chunks >= 0, "settle_apply: bad long-chain split");
  if (n_touched == 0) return BCE_OK;
  BCE_REQUIRE(bits && start && order && rel && conf && t_us, "settle_apply: NULL argument");
  if (n_long > 0) {
    BCE_REQUIRE(chunk_start && snap && (uintptr_t)snap % 16 == 0, "settle_apply: long chains need chunk_start and snap");
    BCE_REQUIRE(chunk_bits >= 64, "settle_apply: chunk_bits < 64");
    BCE_REQUIRE(n_chunks >= n_long, "settle_apply: fewer chunks than long chains");
  }
  const int64_t blocks = (n_touched + 63) / 64, lblocks = (n_chunks + 63) / 64;
  BCE_REQUIRE(blocks < (1ll << 31) && lblocks < (1ll << 31), "settle_apply: grid too large");
  SettleArgs a{reinterpret_cast<const unsigned long long*>(bits), n_bits, start, order, n_touched, n_long, n_sources,
               rel, conf, t_us, present, now_us, default_rel, default_conf, reinterpret_cast<double2*>(snap),
               fault_word()};
  hipLaunchKernelGGL(settle_chain_kernel, dim3((unsigned)blocks), dim3(64), 0, as_stream(stream), a);
  int rc = check_launch("settle_chain_kernel");
  if (rc != BCE_OK || n_long == 0) return rc;
  hipLaunchKernelGGL(settle_long_kernel, dim3((unsigned)lblocks), dim3(64), 0, as_stream(stream), a, chunk_start,
                     n_chunks, chunk_bits);
  return check_launch("settle_long_kernel");
}
