// reestimate_csr.hip -- iterated consensus <-> reliability over a ragged CSR batch.
//
// Everything that depends on (offsets, sid, prob) alone is compiled once per batch into one
// entry per unique (market, source) pair, in (market, ascending sid) order -- the order
// compute_consensus sums in (core.py:103-137).  A round then reads only the entries:
//
//   reestimate_csr_compile    one thread per entry: avg = (0.0 + p1 + p2 ...) / count over the
//                             source's signals in input order (core.py:115-116), the raw votes
//                             (p >= 0.5, market.py:298-299) as two 16-bit counts, and the
//                             market's out-of-range flag (core.py:59-60)
//   reestimate_csr_consensus  a wave per 64 consecutive markets: their entries are one
//                             contiguous range, staged into LDS as {avg * w[usid], w[usid]} with
//                             coalesced loads; each lane then walks its own market's segment in
//                             order (core.py:120,135-137) -> consensus, null, outcome
//   reestimate_csr_agreement  one lane per entry: correct / total += the entry's vote counts
//                             against outcome[market] (market.py:293-304); int64 atomics, exact
//                             and order-free, accumulated (market shards share one count vector)
//   reestimate_csr_weights    w[s] = correct / total, 0.5 where total == 0 (market.py:309-310)
#include "bce_device.hpp"
#include "bce_internal.hpp"
#include "consensus_common.hpp"

#pragma clang fp contract(off)

namespace bce {

constexpr int kRcMaxVotes = 65535;  // per entry: n_ge and n_lt are 16 bits each

__global__ __launch_bounds__(256) void reestimate_csr_compile_kernel(
    const int64_t* __restrict__ group_start, int64_t E, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ key, int64_t N, const int32_t* __restrict__ sid, const double* __restrict__ prob,
    int64_t S, int64_t M, int32_t* __restrict__ usid, double* __restrict__ avg, int32_t* __restrict__ votes,
    int32_t* __restrict__ emarket, uint8_t* __restrict__ bad, int* fault) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= E) return;
  int64_t a = group_start[e], b = group_start[e + 1];
  int code = 0;
  if (a < 0 || b > N || a >= b) {  // not a run of the sorted signals: nothing to read
    code = kFaultOffsets;
    a = b = 0;
  }
  const int64_t k = (a < b) ? key[a] : 0;
  int64_t mk = k / S, s = k - mk * S;  // key = market * S + clamped sid
  if (k < 0 || mk >= M) {
    code = kFaultOffsets;
    mk = 0;
    s = 0;
  }
  double psum = 0.0;  // builtin sum() starts from 0 (core.py:116)
  int64_t n_ge = 0, n_lt = 0;
  bool oor = false;
  for (int64_t j = a; j < b; ++j) {  // the stable sort kept the source's signals in input order
    int64_t i = perm[j];
    if (i < 0 || i >= N) {
      code = kFaultOffsets;
      i = 0;
    }
    const int32_t raw = sid[i];
    if (raw < 0 || raw >= S) code = code ? code : kFaultSid;  // the key holds it clamped
    const double p = prob[i];
    psum += p;
    oor = oor || p < 0 || p > 1;  // NaN passes (core.py:59)
    if (p >= 0.5) ++n_ge; else ++n_lt;  // market.py:298-299
  }
  if (n_ge > kRcMaxVotes || n_lt > kRcMaxVotes) {
    code = code ? code : kFaultTooLong;
    n_ge = n_ge > kRcMaxVotes ? kRcMaxVotes : n_ge;
    n_lt = n_lt > kRcMaxVotes ? kRcMaxVotes : n_lt;
  }
  usid[e] = (int32_t)s;
  avg[e] = psum / (double)(b - a);
  votes[e] = (int32_t)(((uint32_t)n_ge << 16) | (uint32_t)n_lt);
  emarket[e] = (int32_t)mk;
  if (oor) bad[mk] = 1;  // every writer of the byte stores the same value
  if (code && fault) atomicCAS(fault, 0, code);
}

// LDS budget of one wave: kRcChunk staged entries of {avg * w, w}.  A tile's entry range is cut
// into chunks of this size, so a market of any length works; a lane carries its two running
// sums from chunk to chunk.
constexpr int kRcChunk = 512;
constexpr int kRcWalk = 8;  // LDS reads in flight per lane while it walks its segment

__global__ __launch_bounds__(64) void reestimate_csr_consensus_kernel(
    const int64_t* __restrict__ uoffsets, int64_t M, const int32_t* __restrict__ usid,
    const double* __restrict__ avg, const uint8_t* __restrict__ bad, const int8_t* __restrict__ known,
    const double* __restrict__ w, int32_t S, double* __restrict__ cons, uint8_t* __restrict__ null_out,
    int8_t* __restrict__ outcome, int* fault) {
  __shared__ double2 stage[kRcChunk];
  const int lane = threadIdx.x;
  const int64_t m0 = (int64_t)blockIdx.x * 64;
  const int64_t m = m0 + lane;
  const bool in = m < M;
  const int64_t mend = (m0 + 64 < M) ? m0 + 64 : M;
  const int64_t lo = uoffsets[m0], hi = uoffsets[mend];  // the tile's entries
  const int64_t sa = in ? uoffsets[m] : hi, sb = in ? uoffsets[m + 1] : hi;
  double total = 0.0, ws = 0.0;  // core.py:107 and builtin sum() from 0 (core.py:135)
  bool badsid = false;
  for (int64_t c0 = lo; c0 < hi; c0 += kRcChunk) {
    const int64_t c1 = (c0 + kRcChunk < hi) ? c0 + kRcChunk : hi;
    const int n = (int)(c1 - c0);
#pragma unroll
    for (int q = 0; q < kRcChunk / 64; ++q) {
      const int i = q * 64 + lane;
      if (i < n) {
        int32_t s = usid[c0 + i];
        if (s < 0 || s >= S) {  // never from a compiled plan; the read stays in bounds
          badsid = true;
          s = 0;
        }
        const double wv = w[s];
        stage[i] = make_double2(avg[c0 + i] * wv, wv);  // core.py:136: avg * weight, rounded once
      }
    }
    __syncthreads();  // one wave per workgroup: orders the LDS writes before the reads
    const int64_t a = sa > c0 ? sa : c0, b = sb < c1 ? sb : c1;
    // ascending sid, left to right: total += w (core.py:120), ws += avg * w (core.py:135-137).
    // kRcWalk LDS reads are issued ahead of the two add chains they feed (same order of adds).
    int i = (int)(a - c0 < kRcChunk ? a - c0 : kRcChunk);  // a >= c0
    const int iend = (int)(b > c0 ? b - c0 : 0);           // <= i when the segment misses this chunk
    for (; i + kRcWalk <= iend; i += kRcWalk) {
      double2 v[kRcWalk];
#pragma unroll
      for (int q = 0; q < kRcWalk; ++q) v[q] = stage[i + q];
#pragma unroll
      for (int q = 0; q < kRcWalk; ++q) {
        total += v[q].y;
        ws += v[q].x;
      }
    }
    for (; i < iend; ++i) {
      const double2 v = stage[i];
      total += v.y;
      ws += v.x;
    }
    __syncthreads();
  }
  if (ballot(badsid)) raise_fault(fault, kFaultSid);
  if (!in) return;
  const bool isnull = (sa >= sb) || (total == 0.0);  // core.py:88 / core.py:131
  const double c = isnull ? 0.0 : ws / total;
  cons[m] = c;
  null_out[m] = isnull ? 1 : 0;
  const int8_t kn = known ? known[m] : (int8_t)-1;
  int8_t o;
  if (kn >= 0) o = kn ? 1 : 0;                  // a resolved outcome (market.py:280,301)
  else if (isnull || bad[m]) o = -1;            // no consensus / ValidationError: skipped
  else o = (c >= 0.5) ? 1 : 0;                  // the consensus vote
  outcome[m] = o;
}

__global__ __launch_bounds__(256) void reestimate_csr_agreement_kernel(
    int64_t E, const int32_t* __restrict__ usid, const int32_t* __restrict__ votes,
    const int32_t* __restrict__ emarket, const int8_t* __restrict__ outcome, int64_t M, int32_t S,
    unsigned long long* __restrict__ correct, unsigned long long* __restrict__ total, int* fault) {
  bool badidx = false;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t s = usid[e], mk = emarket[e];
    const uint32_t v = (uint32_t)votes[e];
    if (s < 0 || s >= S || mk < 0 || mk >= M) {  // never from a compiled plan
      badidx = true;
      continue;
    }
    const int8_t o = outcome[mk];
    if (o < 0) continue;
    const unsigned n_ge = v >> 16, n_lt = v & 0xffffu;
    atomicAdd(&total[s], (unsigned long long)(n_ge + n_lt));  // market.py:293
    const unsigned hit = o ? n_ge : n_lt;                     // market.py:299-302
    if (hit) atomicAdd(&correct[s], (unsigned long long)hit);
  }
  if (badidx && fault) atomicCAS(fault, 0, kFaultSid);
}

__global__ __launch_bounds__(256) void reestimate_csr_weights_kernel(int64_t S, const long long* __restrict__ correct,
                                                                     const long long* __restrict__ total,
                                                                     double* __restrict__ w) {
  const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s >= S) return;
  const long long t = total[s];
  w[s] = t > 0 ? (double)correct[s] / (double)t : 0.5;  // market.py:309-310
}

}  // namespace bce

using namespace bce;

extern "C" int bce_reestimate_csr_compile(const int64_t* group_start, int64_t n_entries, const int64_t* perm,
                                          const int64_t* key, int64_t n_signals, const int32_t* sid,
                                          const double* prob, int32_t n_sources, int64_t n_markets,
                                          int32_t* usid, double* avg, int32_t* votes, int32_t* emarket,
                                          uint8_t* bad, void* stream) {
  BCE_REQUIRE(n_entries >= 0 && n_signals >= 0 && n_markets >= 0 && n_sources > 0, "reestimate_csr_compile: bad shape");
  BCE_REQUIRE(n_markets < (1ll << 31), "reestimate_csr_compile: n_markets >= 2^31");
  BCE_REQUIRE(n_entries <= n_signals, "reestimate_csr_compile: more entries than signals");
  if (n_entries == 0) return BCE_OK;
  BCE_REQUIRE(group_start && perm && key && sid && prob && usid && avg && votes && emarket && bad,
              "reestimate_csr_compile: NULL argument");
  const int64_t blocks = (n_entries + 255) / 256;
  BCE_REQUIRE(blocks < (1ll << 31), "reestimate_csr_compile: grid too large");
  hipLaunchKernelGGL(reestimate_csr_compile_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     group_start, n_entries, perm, key, n_signals, sid, prob, (int64_t)n_sources, n_markets, usid,
                     avg, votes, emarket, bad, fault_word());
  return check_launch("reestimate_csr_compile_kernel");
}

extern "C" int bce_reestimate_csr_consensus(const int64_t* uoffsets, int64_t n_markets, const int32_t* usid,
                                            const double* avg, const uint8_t* bad, const int8_t* known,
                                            const double* w, int32_t n_sources, double* consensus,
                                            uint8_t* null_out, int8_t* outcome, void* stream) {
  BCE_REQUIRE(n_markets >= 0 && n_markets < (1ll << 31) && n_sources > 0, "reestimate_csr_consensus: bad shape");
  if (n_markets == 0) return BCE_OK;
  BCE_REQUIRE(uoffsets && usid && avg && bad && w && consensus && null_out && outcome,
              "reestimate_csr_consensus: NULL argument");
  hipLaunchKernelGGL(reestimate_csr_consensus_kernel, dim3((unsigned)((n_markets + 63) / 64)), dim3(64), 0,
                     as_stream(stream), uoffsets, n_markets, usid, avg, bad, known, w, n_sources, consensus,
                     null_out, outcome, fault_word());
  return check_launch("reestimate_csr_consensus_kernel");
}

extern "C" int bce_reestimate_csr_agreement(int64_t n_entries, const int32_t* usid, const int32_t* votes,
                                            const int32_t* emarket, const int8_t* outcome, int64_t n_markets,
                                            int32_t n_sources, int64_t* correct, int64_t* total, void* stream) {
  BCE_REQUIRE(n_entries >= 0 && n_markets >= 0 && n_sources > 0, "reestimate_csr_agreement: bad shape");
  if (n_entries == 0) return BCE_OK;
  BCE_REQUIRE(usid && votes && emarket && outcome && correct && total, "reestimate_csr_agreement: NULL argument");
  int64_t blocks = (n_entries + 255) / 256;
  const int64_t cap = grid_cap(8);
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(reestimate_csr_agreement_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     n_entries, usid, votes, emarket, outcome, n_markets, n_sources,
                     reinterpret_cast<unsigned long long*>(correct), reinterpret_cast<unsigned long long*>(total),
                     fault_word());
  return check_launch("reestimate_csr_agreement_kernel");
}

extern "C" int bce_reestimate_csr_weights(int64_t n_sources, const int64_t* correct, const int64_t* total,
                                          double* w, void* stream) {
  BCE_REQUIRE(n_sources > 0 && correct && total && w, "reestimate_csr_weights: bad argument");
  const int64_t blocks = (n_sources + 255) / 256;
  BCE_REQUIRE(blocks < (1ll << 31), "reestimate_csr_weights: grid too large");
  hipLaunchKernelGGL(reestimate_csr_weights_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     n_sources, reinterpret_cast<const long long*>(correct), reinterpret_cast<const long long*>(total),
                     w);
  return check_launch("reestimate_csr_weights_kernel");
}
