// trace_all.hip -- every prefix state of every settlement chain: the raw {rel, conf} of a source
// after EACH of its chain bits, states[g] for chain bit g (the global bit index start[s] + k), one
// 16-byte vector store per bit.  What bce_settle_trace stores at the query positions of a walk,
// stored at all of them: the live consensus history (consensus_history_live.hip) reads the state a
// source stood in at any arrival as states[start[s] + pos - 1].
//
//   trace_all_chain_kernel  one lane per short chain of `order`, the walk of trace_chain_kernel
//   trace_all_long_kernel   one lane per chunk of a long chain, the workers of trace_long_kernel
//
// The ownership rule is bce_settle_trace's: the worker that applies bit k stores
// the state behind it.  Worker 0 walks from the start row; worker j > 0 finds the first run of
// kSyncRun equal bits inside its home chunk, which pins the reliability to exactly 1.0 / 0.0 behind
// the run's last bit p, and walks from p + 1 -- bit p itself is applied, and stored, by the worker
// before, which walks on through every chunk until it meets such a run (counted from the chunk's
// first bit, as the owner counts it).  Every position has one writer, there are no atomics, and
// the result does not depend on long_min / chunk_bits.  The confidence does not depend on the bits
// (reliability.py:172-173): a worker that starts at position p starts from settle_conf(c0, p).
// Neither kernel writes the table.
#include "reliability_update.hpp"
#include "settle_walk.hpp"
#include "trace_walk.hpp"

#pragma clang fp contract(off)

namespace bce {
namespace {

struct TraceAllArgs {
  SettleArgs s;     // the chains and the start table (read only; t_us / now_us / snap unused)
  double2* states;  // [n_bits]
};

// settle_span<true, TRACK> over chain positions [p0, p1) of the chain at bit b0, the state stored
// behind every bit; c steps with it.  TRACK: the position whose bit completed a sync run (already
// applied and stored; the walk ends there), else -1.  The caller has checked b0 + p1 <= n_bits.
template <bool TRACK>
__device__ __forceinline__ int64_t trace_all_span(const TraceAllArgs& a, int64_t b0, int64_t p0, int64_t p1,
                                                  double& r, double& c, int& run, bool& prev) {
  int64_t g = b0 + p0;
  const int64_t gend = b0 + p1;
  while (g < gend) {
    const int sh = (int)(g & 63);
    unsigned long long w = a.s.bits[g >> 6] >> sh;
    const int64_t left = gend - g;
    const int n = left < 64 - sh ? (int)left : 64 - sh;
    for (int k = 0; k < n; ++k) {
      const bool bit = (w & 1ull) != 0;
      w >>= 1;
      update_one(r, c, bit);
      a.states[g + k] = make_double2(r, c);
      if (TRACK) {
        run = (run > 0 && bit == prev) ? run + 1 : 1;
        prev = bit;
        if (run >= kSyncRun) return g + k - b0;
      }
    }
    g += n;
  }
  return -1;
}

__global__ __launch_bounds__(64) void trace_all_chain_kernel(TraceAllArgs a) {
  const int64_t q = a.s.n_long + (int64_t)blockIdx.x * 64 + threadIdx.x;  // the long chains: trace_all_long_kernel
  if (q >= a.s.T) return;
  int32_t s;
  int64_t b0, b1;
  if (!settle_range(a.s, q, s, b0, b1)) return;
  double r, c;
  trace_start_row(a.s, s, r, c);
  int run = 0;
  bool prev = false;
  trace_all_span<false>(a, b0, 0, b1 - b0, r, c, run, prev);
}

__global__ __launch_bounds__(64) void trace_all_long_kernel(TraceAllArgs a, const int64_t* __restrict__ chunk_start,
                                                            int64_t n_chunks, int64_t C) {
  const int64_t wk = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (wk >= n_chunks) return;
  // the long source this chunk belongs to: the last q with chunk_start[q] <= wk
  int64_t lo = 0, hi = a.s.n_long;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (chunk_start[mid] <= wk) lo = mid; else hi = mid;
  }
  const int64_t q = lo, j = wk - chunk_start[q];
  int32_t s;
  int64_t b0, b1;
  if (j < 0 || !settle_range(a.s, q, s, b0, b1)) return;
  const int64_t L = b1 - b0;
  if (j > (L - 1) / C) return;  // more chunks than the chain has: nothing to do
  const int64_t home_end = (j + 1) * C < L ? (j + 1) * C : L;
  double r, c;
  trace_start_row(a.s, s, r, c);
  int run = 0;
  bool prev = false;
  int64_t pos = j * C;
  if (j > 0) {  // the first run of kSyncRun equal bits that lies inside the home chunk
    const int64_t p = settle_span<false, true>(a.s.bits, b0, pos, home_end, r, run, prev);
    if (p < 0) return;     // none: the worker before walks through this chunk and owns its states
    r = prev ? 1.0 : 0.0;  // exact whatever came before
    pos = p + 1;           // bit p was applied by the worker before: the state behind it is theirs
    c = settle_conf(c, pos);
  }
  trace_all_span<false>(a, b0, pos, home_end, r, c, run, prev);  // the rest of the home chunk
  for (int64_t cb = home_end; cb < L; cb += C) {  // later chunks, until one has a sync run of its own
    const int64_t cend = cb + C < L ? cb + C : L;
    run = 0;  // a run counts from its chunk's first bit
    if (trace_all_span<true>(a, b0, cb, cend, r, c, run, prev) >= 0) return;  // that chunk's worker goes on
  }
}

}  // namespace
}  // namespace bce

using namespace bce;

extern "C" int bce_settle_trace_all(const uint64_t* bits, int64_t n_bits, const int64_t* start, const int32_t* order,
                                    int64_t n_touched, int64_t n_long, const int64_t* chunk_start, int64_t n_chunks,
                                    int64_t chunk_bits, int32_t n_sources, const double* rel, const double* conf,
                                    const uint8_t* present, double default_rel, double default_conf, double* states,
                                    void* stream) {
  BCE_REQUIRE(n_bits >= 0 && n_touched >= 0 && n_sources > 0 && n_touched <= n_sources, "settle_trace_all: bad shape");
  BCE_REQUIRE(n_long >= 0 && n_long <= n_touched && n_chunks >= 0, "settle_trace_all: bad long-chain split");
  if (n_touched == 0 || n_bits == 0) return BCE_OK;
  BCE_REQUIRE(bits && start && order && rel && conf && states, "settle_trace_all: NULL argument");
  BCE_REQUIRE((uintptr_t)states % 16 == 0, "settle_trace_all: states must be 16-byte aligned");
  if (n_long > 0) {
    BCE_REQUIRE(chunk_start, "settle_trace_all: long chains need chunk_start");
    BCE_REQUIRE(chunk_bits >= 64, "settle_trace_all: chunk_bits < 64");
    BCE_REQUIRE(n_chunks >= n_long, "settle_trace_all: fewer chunks than long chains");
  }
  const int64_t blocks = (n_touched - n_long + 63) / 64, lblocks = (n_chunks + 63) / 64;
  BCE_REQUIRE(blocks < (1ll << 31) && lblocks < (1ll << 31), "settle_trace_all: grid too large");
  TraceAllArgs a{};
  // the kernels only read the table: the shared argument block is settle's, which writes it
  a.s = SettleArgs{reinterpret_cast<const unsigned long long*>(bits), n_bits, start, order, n_touched, n_long,
                   n_sources, const_cast<double*>(rel), const_cast<double*>(conf), nullptr,
                   const_cast<uint8_t*>(present), 0, default_rel, default_conf, nullptr, fault_word()};
  a.states = reinterpret_cast<double2*>(states);
  if (blocks > 0) {
    hipLaunchKernelGGL(trace_all_chain_kernel, dim3((unsigned)blocks), dim3(64), 0, as_stream(stream), a);
    const int rc = check_launch("trace_all_chain_kernel");
    if (rc != BCE_OK) return rc;
  }
  if (n_long == 0) return BCE_OK;
  hipLaunchKernelGGL(trace_all_long_kernel, dim3((unsigned)lblocks), dim3(64), 0, as_stream(stream), a, chunk_start,
                     n_chunks, chunk_bits);
  return check_launch("trace_all_long_kernel");
}
