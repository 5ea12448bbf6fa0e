// plan.hip -- the planners of the planned consensus launch (consensus_api.hip
// bce_consensus_planned / bce_consensus_planned_device): markets grouped by length bin
// (plan_host.hpp), longest first inside the wide bins, built from host offsets (bce_plan_bins)
// or on the GPU from device offsets (bce_plan_bins_device, bce_plan_bins_device_async); and
// bce_plan_schedule, the launches plan_schedule lists for a plan.
#include <algorithm>

#include "consensus_common.hpp"
#include "plan_host.hpp"

using namespace bce;

extern "C" int bce_plan_bins(const int64_t* offsets_host, int64_t n_markets, int32_t* order_host,
                             int64_t* bin_start_host, int32_t* max_len_host) {
  BCE_REQUIRE(n_markets >= 0 && offsets_host && order_host && bin_start_host,
              "plan_bins: NULL argument");
  int64_t cnt[BCE_NBINS] = {0};
  int64_t mx = 0;
  for (int64_t m = 0; m < n_markets; ++m) {
    const int64_t n = offsets_host[m + 1] - offsets_host[m];
    BCE_REQUIRE(n >= 0, "plan_bins: offsets not monotone at market %lld", (long long)m);
    cnt[bin_of(n)]++;
    mx = n > mx ? n : mx;
  }
  bin_start_host[0] = 0;
  for (int b = 0; b < BCE_NBINS; ++b) bin_start_host[b + 1] = bin_start_host[b] + cnt[b];
  int64_t pos[BCE_NBINS];
  for (int b = 0; b < BCE_NBINS; ++b) pos[b] = bin_start_host[b];
  for (int64_t m = 0; m < n_markets; ++m) {
    const int64_t n = offsets_host[m + 1] - offsets_host[m];
    order_host[pos[bin_of(n)]++] = (int32_t)m;
  }
  // Wide bins (65..4096) longest market first (LPT order, ties by market index): a
  // persistent workgroup takes its next market as it finishes one, so the last round of
  // workgroups gets the short ones and the launch's tail shrinks (C3 fast -0.7%, exact
  // -0.6%, one of 8 market shards -1.3%: profiles/r03ae/).
  for (int b = kPlanSideLast + 1; b < BCE_NBINS - 1; ++b)
    std::stable_sort(order_host + bin_start_host[b], order_host + bin_start_host[b + 1], [&](int32_t x, int32_t y) {
      return offsets_host[x + 1] - offsets_host[x] > offsets_host[y + 1] - offsets_host[y];
    });
  if (max_len_host) *max_len_host = (int32_t)(mx > 0x7fffffff ? 0x7fffffff : mx);
  return BCE_OK;
}

extern "C" int64_t bce_consensus_scratch_bytes(const int64_t* offsets_host, const int32_t* order_host,
                                               const int64_t* bin_start_host) {
  const int64_t b0 = bin_start_host[BCE_NBINS - 1], b1 = bin_start_host[BCE_NBINS];
  if (b1 <= b0) return 0;
  int64_t mx = 0;
  for (int64_t i = b0; i < b1; ++i) {
    const int32_t m = order_host[i];
    const int64_t n = offsets_host[m + 1] - offsets_host[m];
    mx = n > mx ? n : mx;
  }
  return long_scratch_bytes(b1 - b0, mx);
}

extern "C" int bce_plan_schedule(const int64_t* bin_start_host, int32_t mode, const int64_t* resident,
                                 int32_t* launches, int32_t* n_launches, int32_t* fork) {
  BCE_REQUIRE(resident && launches && n_launches && fork, "plan_schedule: NULL argument");
  BCE_REQUIRE(mode == BCE_MODE_EXACT || mode == BCE_MODE_FAST, "plan_schedule: bad mode %d", mode);
  const PlanSchedule s = plan_schedule(bin_start_host, mode, [&](int b) { return resident[b]; });
  for (int i = 0; i < s.n; ++i) {
    launches[3 * i] = s.launch[i].b0;
    launches[3 * i + 1] = s.launch[i].b1;
    launches[3 * i + 2] = s.launch[i].side;
  }
  *n_launches = s.n;
  *fork = s.fork;
  return BCE_OK;
}

// ======================================================================================
// The device planner (bce_plan_bins_device): the plan of bce_plan_bins built from device
// offsets, no D2H copy of the CSR.  A market's bin and its LPT position are one 12-bit key
//   bins 0..3 (n <= 64)           key = bin                (market order inside the bin)
//   wide bin b, lengths lo..hi    key = 4 + (lo - 65) + (hi - n)   (bins ascending, longest first)
//   n > 4096                      key = kPlanKeys - 1
// so the plan is a STABLE sort of the market indices by key: two LSD passes of 6-bit digits,
// each a per-chunk digit count, one exclusive scan of the [digit][chunk] counts and a stable
// scatter (the rank inside a chunk from a [thread][digit] count matrix in LDS).  Stable at
// every pass, hence market order inside equal keys: exactly bce_plan_bins' order.
// ======================================================================================
namespace bce {
constexpr int kPlanKeys = 4 + (4096 - 65 + 1) + 1;  // 4037 < 2^12
constexpr int kPlanThreads = 256;
constexpr int kPlanPer = 4;                          // markets per thread
constexpr int kPlanChunk = kPlanThreads * kPlanPer;  // markets per workgroup
constexpr int kPlanDigits = 64;                      // 6-bit digits, two passes
constexpr int kPlanScanThreads = 1024;
static_assert(kPlanKeys <= kPlanDigits * kPlanDigits, "two 6-bit passes");

struct PlanInfo {
  unsigned long long bins[BCE_NBINS];
  unsigned long long max_len;
  unsigned long long long_max;  // longest market of the > 4096 bin (scratch sizing)
  unsigned long long badrev;    // M - (first market whose offsets decrease), 0 = none
};

__device__ __forceinline__ int plan_bin(int64_t n) {
  return n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : n <= 64 ? 3 : n <= 128 ? 4 : n <= 256 ? 5 : n <= 512 ? 6
       : n <= 1024 ? 7 : n <= 1536 ? 8 : n <= 2048 ? 9 : n <= 3072 ? 10 : n <= 4096 ? 11 : 12;
}

__device__ __forceinline__ int plan_key(int64_t n, int b) {
  if (b <= 3) return b;
  if (b == 12) return kPlanKeys - 1;
  const int lo = b == 4 ? 65 : b == 5 ? 129 : b == 6 ? 257 : b == 7 ? 513 : b == 8 ? 1025 : b == 9 ? 1537
               : b == 10 ? 2049 : 3073;
  const int hi = b == 4 ? 128 : b == 5 ? 256 : b == 6 ? 512 : b == 7 ? 1024 : b == 8 ? 1536 : b == 9 ? 2048
               : b == 10 ? 3072 : 4096;
  return 4 + (lo - 65) + (hi - (int)n);
}

template <typename T>
__device__ __forceinline__ T wave_max_u64(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const T o = (T)__shfl_xor((unsigned long long)v, m);
    v = o > v ? o : v;
  }
  return v;
}

// Pass PASS digit counts of chunk blockIdx.x -> counts[digit * nchunks + chunk].  Pass 0 reads
// the offsets (striped: coalesced) and also writes the chunk's record for PlanInfo (bin counts,
// longest market, longest > 4096 market, first decreasing offset) -- no global atomics: the
// pass-0 scan reduces the records (800 same-address atomicMax per call cost ~10 us).
constexpr int kPlanRec = 16;  // int64 per chunk record: bins[13], max_len, long_max, badrev
template <int PASS, bool CM>
__global__ __launch_bounds__(kPlanThreads) void plan_count_kernel(const int64_t* __restrict__ offsets, int64_t M,
                                                                  const uint16_t* __restrict__ keys_in,
                                                                  int32_t* __restrict__ counts, int64_t nchunks,
                                                                  int64_t* __restrict__ crec) {
  __shared__ int cnt[kPlanDigits];
  __shared__ int bincnt[BCE_NBINS];
  __shared__ unsigned long long wmax[kPlanThreads / kWave][3];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x;
  if (t < kPlanDigits) cnt[t] = 0;
  if (PASS == 0 && t < BCE_NBINS) bincnt[t] = 0;
  __syncthreads();
  unsigned long long mx = 0, lmx = 0, badrev = 0;
#pragma unroll
  for (int k = 0; k < kPlanPer; ++k) {
    const int64_t i = c * kPlanChunk + k * kPlanThreads + t;
    if (i < M) {
      int key;
      if constexpr (PASS == 0) {
        const int64_t n = offsets[i + 1] - offsets[i];
        if (n < 0) badrev = (unsigned long long)(M - i) > badrev ? (unsigned long long)(M - i) : badrev;
        const int b = plan_bin(n);
        key = plan_key(n < 0 ? 0 : n, n < 0 ? 0 : b);
        atomicAdd(&bincnt[n < 0 ? 0 : b], 1);
        const unsigned long long un = n < 0 ? 0ull : (unsigned long long)n;
        mx = un > mx ? un : mx;
        if (b == 12) lmx = un > lmx ? un : lmx;
      } else {
        key = keys_in[i];
      }
      atomicAdd(&cnt[(key >> (6 * PASS)) & (kPlanDigits - 1)], 1);
    }
  }
  if constexpr (PASS == 0) {
    mx = wave_max_u64(mx);
    lmx = wave_max_u64(lmx);
    badrev = wave_max_u64(badrev);
    if (lane_id() == 0) {
      wmax[t / kWave][0] = mx;
      wmax[t / kWave][1] = lmx;
      wmax[t / kWave][2] = badrev;
    }
  }
  __syncthreads();
  if (t < kPlanDigits) counts[CM ? c * kPlanDigits + t : (int64_t)t * nchunks + c] = cnt[t];
  if constexpr (PASS == 0) {
    int64_t* r = crec + c * kPlanRec;
    if (t < BCE_NBINS) r[t] = bincnt[t];
    if (t >= BCE_NBINS && t < BCE_NBINS + 3) {
      unsigned long long v = 0;
      for (int w = 0; w < kPlanThreads / kWave; ++w) v = wmax[w][t - BCE_NBINS] > v ? wmax[w][t - BCE_NBINS] : v;
      r[t] = (int64_t)v;
    }
  }
}

// Reduce the count pass's chunk records into PlanInfo; with bin_start_dev also the device bin
// boundaries and the device-driven faults (decreasing offsets: every bin empty + kFaultOffsets;
// raise_long: a market > 4096 raises kFaultTooLong).  Called by one whole workgroup.
__device__ __forceinline__ void plan_reduce_info(const int64_t* __restrict__ crec, int64_t nchunks, PlanInfo* info,
                                                 int64_t* bin_start_dev, int* fault, int raise_long,
                                                 unsigned long long* sacc, int t, int nthreads) {
  if (t < BCE_NBINS + 3) sacc[t] = 0;
  __syncthreads();
  unsigned long long b[BCE_NBINS] = {}, m0 = 0, m1 = 0, m2 = 0;
  for (int64_t c = t; c < nchunks; c += nthreads) {
    const int64_t* r = crec + c * kPlanRec;
#pragma unroll
    for (int k = 0; k < BCE_NBINS; ++k) b[k] += (unsigned long long)r[k];
    m0 = (unsigned long long)r[BCE_NBINS] > m0 ? (unsigned long long)r[BCE_NBINS] : m0;
    m1 = (unsigned long long)r[BCE_NBINS + 1] > m1 ? (unsigned long long)r[BCE_NBINS + 1] : m1;
    m2 = (unsigned long long)r[BCE_NBINS + 2] > m2 ? (unsigned long long)r[BCE_NBINS + 2] : m2;
  }
  // wave reductions first: one LDS atomic per wave and counter
#pragma unroll
  for (int k = 0; k < BCE_NBINS; ++k) {
    unsigned long long v = b[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
    b[k] = v;
  }
  m0 = wave_max_u64(m0);
  m1 = wave_max_u64(m1);
  m2 = wave_max_u64(m2);
  if (lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < BCE_NBINS; ++k)
      if (b[k]) atomicAdd(&sacc[k], b[k]);
    if (m0) atomicMax(&sacc[BCE_NBINS], m0);
    if (m1) atomicMax(&sacc[BCE_NBINS + 1], m1);
    if (m2) atomicMax(&sacc[BCE_NBINS + 2], m2);
  }
  __syncthreads();
  if (t == 0) {
    for (int k = 0; k < BCE_NBINS; ++k) info->bins[k] = sacc[k];
    info->max_len = sacc[BCE_NBINS];
    info->long_max = sacc[BCE_NBINS + 1];
    info->badrev = sacc[BCE_NBINS + 2];
    if (bin_start_dev) {
      const bool bad = sacc[BCE_NBINS + 2] != 0;
      int64_t run = 0;
      bin_start_dev[0] = 0;
      for (int k = 0; k < BCE_NBINS; ++k) {
        run += bad ? 0 : (int64_t)sacc[k];
        bin_start_dev[k + 1] = run;
      }
      if (fault && bad) atomicCAS(fault, 0, kFaultOffsets);
      if (fault && !bad && raise_long && sacc[BCE_NBINS - 1]) atomicCAS(fault, 0, kFaultTooLong);
    }
  }
}

// In-place exclusive scan of counts[0..E) by one workgroup (E = 64 x chunks), in tiles of 8
// consecutive counts per thread (the loads of a tile in flight together).  INFO (pass 0): also
// reduces the chunk records into PlanInfo and, with bin_start_dev, writes the device bin
// boundaries (decreasing offsets: every bin empty + kFaultOffsets; raise_long: a market > 4096
// raises kFaultTooLong -- the device-driven launch does not compute those).
template <bool INFO>
__global__ __launch_bounds__(kPlanScanThreads) void plan_scan_kernel(int32_t* __restrict__ counts, int64_t E,
                                                                     const int64_t* __restrict__ crec, int64_t nchunks,
                                                                     PlanInfo* info, int64_t* bin_start_dev, int* fault,
                                                                     int raise_long) {
  constexpr int V = 8;
  constexpr int NW = kPlanScanThreads / kWave;
  __shared__ int64_t wsum[NW];
  __shared__ int64_t tile_total;
  __shared__ unsigned long long sacc[BCE_NBINS + 3];
  const int t = threadIdx.x;
  const int w = t / kWave;
  if constexpr (INFO) plan_reduce_info(crec, nchunks, info, bin_start_dev, fault, raise_long, sacc, t, kPlanScanThreads);
  int64_t carry = 0;
  for (int64_t base = 0; base < E; base += (int64_t)kPlanScanThreads * V) {
    const int64_t i0 = base + (int64_t)t * V;
    int v[V];
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      v[k] = (i0 + k < E) ? counts[i0 + k] : 0;
      s += v[k];
    }
    int64_t inc = s;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int64_t o = __shfl_up(inc, d);
      if (lane_id() >= d) inc += o;
    }
    if (lane_id() == kWave - 1) wsum[w] = inc;
    __syncthreads();
    if (t == 0) {
      int64_t run = 0;
      for (int k = 0; k < NW; ++k) {
        const int64_t x = wsum[k];
        wsum[k] = run;
        run += x;
      }
      tile_total = run;
    }
    __syncthreads();
    int64_t run = carry + wsum[w] + inc - s;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (i0 + k < E) counts[i0 + k] = (int32_t)run;
      run += v[k];
    }
    carry += tile_total;
    __syncthreads();  // wsum / tile_total are rewritten by the next tile
  }
}

// Stable scatter of chunk blockIdx.x by its pass-PASS digit.  Thread t holds markets
// 4t..4t+3 of the chunk (blocked: thread order == input order); mat[t][d] counts thread t's
// items of digit d, and its exclusive scan in (d, t) order gives every item its rank among the
// chunk's items of smaller digit or equal digit and earlier position.
// INKB (<= kPlanInkbMax chunks): the counts are chunk-major [chunk][digit] and every workgroup
// derives its own 64 bases from all of them (a wave reads one 256-B chunk row per step), so no
// scan launch sits between the passes; PASS 0 runs one extra workgroup that reduces the chunk
// records (plan_reduce_info) alongside.  Otherwise `base` is the digit-major exclusive scan of plan_scan_kernel.
constexpr int64_t kPlanInkbMax = 1024;
template <int PASS, bool INKB>
__global__ __launch_bounds__(kPlanThreads) void plan_scatter_kernel(const int64_t* __restrict__ offsets, int64_t M,
                                                                    const uint16_t* __restrict__ keys_in,
                                                                    const int32_t* __restrict__ idx_in,
                                                                    const int32_t* __restrict__ base, int64_t nchunks,
                                                                    uint16_t* __restrict__ keys_out,
                                                                    int32_t* __restrict__ idx_out,
                                                                    const int64_t* __restrict__ crec, PlanInfo* info,
                                                                    int64_t* bin_start_dev, int* fault, int raise_long) {
  __shared__ int mat[kPlanThreads * kPlanDigits];  // [t][d], 64 KB
  __shared__ int part[kPlanThreads];
  __shared__ int sTot[kPlanDigits], sPre[kPlanDigits];
  __shared__ unsigned long long sacc[BCE_NBINS + 3];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x;
  if constexpr (INKB) {
    if (PASS == 0 && c == nchunks) {  // the extra workgroup of pass 0: PlanInfo, in parallel with the scatter
      plan_reduce_info(crec, nchunks, info, bin_start_dev, fault, raise_long, sacc, t, kPlanThreads);
      return;
    }
    if (t < kPlanDigits) {
      sTot[t] = 0;
      sPre[t] = 0;
    }
    __syncthreads();
    const int dd = t & (kPlanDigits - 1), qq = t / kPlanDigits;
    int tot = 0, pre = 0;
#pragma unroll 4
    for (int64_t c2 = qq; c2 < nchunks; c2 += kPlanThreads / kPlanDigits) {
      const int v = base[c2 * kPlanDigits + dd];
      tot += v;
      pre += (c2 < c) ? v : 0;
    }
    atomicAdd(&sTot[dd], tot);
    atomicAdd(&sPre[dd], pre);
    __syncthreads();
    if (t < kWave) {  // exclusive scan of the digit totals (one wave, lane = digit), + this chunk's prefix
      const int v = sTot[t];
      int inc = v;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const int y = __shfl_up(inc, o);
        if (lane_id() >= o) inc += y;
      }
      sPre[t] += inc - v;
    }
  }
#pragma unroll 8
  for (int j = 0; j < kPlanDigits; ++j) mat[j * kPlanThreads + t] = 0;
  int key[kPlanPer], idx[kPlanPer], before[kPlanPer];
  const int64_t i0 = c * kPlanChunk + (int64_t)t * kPlanPer;
#pragma unroll
  for (int k = 0; k < kPlanPer; ++k) {
    const int64_t i = i0 + k;
    key[k] = -1;
    idx[k] = 0;
    if (i < M) {
      if constexpr (PASS == 0) {
        int64_t n = offsets[i + 1] - offsets[i];
        n = n < 0 ? 0 : n;
        key[k] = plan_key(n, plan_bin(n));
        idx[k] = (int)i;
      } else {
        key[k] = keys_in[i];
        idx[k] = idx_in[i];
      }
    }
  }
  __syncthreads();
  int* row = mat + t * kPlanDigits;
#pragma unroll
  for (int k = 0; k < kPlanPer; ++k) {
    if (key[k] >= 0) {
      const int d = (key[k] >> (6 * PASS)) & (kPlanDigits - 1);
      before[k] = row[d];
      row[d] = before[k] + 1;
    }
  }
  __syncthreads();
  // column sums: thread j = (q, d) sums mat[64q .. 64q+63][d] (a wave reads consecutive words)
  const int d = t & (kPlanDigits - 1), q = t / kPlanDigits;
  int s = 0;
#pragma unroll 8
  for (int r = 0; r < kPlanDigits; ++r) s += mat[(q * kPlanDigits + r) * kPlanDigits + d];
  part[d * (kPlanThreads / kPlanDigits) + q] = s;
  __syncthreads();
  if (t < kWave) {  // exclusive scan of part[] (256 values, 4 per lane) by one wave
    int v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = part[4 * t + k]; sum += v[k]; }
    int inc = sum;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int y = __shfl_up(inc, o);
      if (lane_id() >= o) inc += y;
    }
    int run = inc - sum;
#pragma unroll
    for (int k = 0; k < 4; ++k) { part[4 * t + k] = run; run += v[k]; }
  }
  __syncthreads();
  int run = part[d * (kPlanThreads / kPlanDigits) + q];
#pragma unroll 8
  for (int r = 0; r < kPlanDigits; ++r) {
    int* p = &mat[(q * kPlanDigits + r) * kPlanDigits + d];
    const int v = *p;
    *p = run;
    run += v;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPlanPer; ++k) {
    if (key[k] >= 0) {
      const int dg = (key[k] >> (6 * PASS)) & (kPlanDigits - 1);
      const int64_t pos = (INKB ? (int64_t)sPre[dg] : (int64_t)base[(int64_t)dg * nchunks + c]) + (row[dg] - mat[dg]) +
                          before[k];
      if constexpr (PASS == 0) keys_out[pos] = (uint16_t)key[k];
      idx_out[pos] = idx[k];
    }
  }
}
}  // namespace bce

static int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
static int plan_device_launch(const int64_t* offsets, int64_t n_markets, int32_t* order, void* scratch,
                              hipStream_t st, PlanInfo** info_out, int64_t* bin_start_dev, int raise_long);

extern "C" int64_t bce_plan_device_scratch_bytes(int64_t n_markets) {
  if (n_markets <= 0) return 0;
  const int64_t chunks = (n_markets + kPlanChunk - 1) / kPlanChunk;
  return align256(sizeof(PlanInfo)) + align256(2 * n_markets) + align256(4 * n_markets) +
         align256(4 * kPlanDigits * chunks) + align256(8 * kPlanRec * chunks);
}

extern "C" int bce_plan_bins_device(const int64_t* offsets, int64_t n_markets, int32_t* order,
                                    int64_t* bin_start_host, int32_t* max_len_host,
                                    int64_t* long_scratch_bytes_host, void* scratch, int64_t scratch_bytes,
                                    void* stream) {
  BCE_REQUIRE(n_markets >= 0 && n_markets < ((int64_t)1 << 31), "plan_bins_device: bad n_markets %lld",
              (long long)n_markets);
  BCE_REQUIRE(bin_start_host, "plan_bins_device: bin_start_host NULL");
  if (long_scratch_bytes_host) *long_scratch_bytes_host = 0;
  if (max_len_host) *max_len_host = 0;
  for (int b = 0; b <= BCE_NBINS; ++b) bin_start_host[b] = 0;
  if (n_markets == 0) return BCE_OK;
  BCE_REQUIRE(offsets && order && scratch, "plan_bins_device: NULL argument");
  BCE_REQUIRE(scratch_bytes >= bce_plan_device_scratch_bytes(n_markets), "plan_bins_device: scratch too small");
  hipStream_t st = as_stream(stream);
  PlanInfo* info = nullptr;
  int rc = plan_device_launch(offsets, n_markets, order, scratch, st, &info, nullptr, 0);
  if (rc) return rc;
  PlanInfo h{};
  BCE_HIP(hipMemcpyAsync(&h, info, sizeof h, hipMemcpyDeviceToHost, st));
  BCE_HIP(hipStreamSynchronize(st));
  BCE_REQUIRE(h.badrev == 0, "plan_bins: offsets not monotone at market %lld",
              (long long)(n_markets - (int64_t)h.badrev));
  for (int b = 0; b < BCE_NBINS; ++b) bin_start_host[b + 1] = bin_start_host[b] + (int64_t)h.bins[b];
  if (max_len_host) *max_len_host = (int32_t)(h.max_len > 0x7fffffffull ? 0x7fffffff : h.max_len);
  const int64_t n_long = (int64_t)h.bins[BCE_NBINS - 1];
  if (long_scratch_bytes_host && n_long > 0) *long_scratch_bytes_host = long_scratch_bytes(n_long, (int64_t)h.long_max);
  return BCE_OK;
}


static int plan_device_launch(const int64_t* offsets, int64_t n_markets, int32_t* order, void* scratch,
                              hipStream_t st, PlanInfo** info_out, int64_t* bin_start_dev, int raise_long) {
  const int64_t chunks = (n_markets + kPlanChunk - 1) / kPlanChunk;
  char* p = static_cast<char*>(scratch);
  PlanInfo* info = reinterpret_cast<PlanInfo*>(p);
  p += align256(sizeof(PlanInfo));
  uint16_t* keys = reinterpret_cast<uint16_t*>(p);
  p += align256(2 * n_markets);
  int32_t* idx = reinterpret_cast<int32_t*>(p);
  p += align256(4 * n_markets);
  int32_t* counts = reinterpret_cast<int32_t*>(p);
  p += align256(4 * kPlanDigits * chunks);
  int64_t* crec = reinterpret_cast<int64_t*>(p);
  const dim3 g((unsigned)chunks), blk(kPlanThreads), sg(1), sblk(kPlanScanThreads);
  int* fw = fault_word();
  if (chunks <= kPlanInkbMax) {  // 4 launches: bases derived inside the scatter kernels
    hipLaunchKernelGGL((plan_count_kernel<0, true>), g, blk, 0, st, offsets, n_markets, nullptr, counts, chunks, crec);
    hipLaunchKernelGGL((plan_scatter_kernel<0, true>), dim3((unsigned)chunks + 1), blk, 0, st, offsets, n_markets,
                       nullptr, nullptr, counts, chunks, keys, idx, crec, info, bin_start_dev, fw, raise_long);
    hipLaunchKernelGGL((plan_count_kernel<1, true>), g, blk, 0, st, offsets, n_markets, keys, counts, chunks, nullptr);
    hipLaunchKernelGGL((plan_scatter_kernel<1, true>), g, blk, 0, st, offsets, n_markets, keys, idx, counts, chunks,
                       nullptr, order, nullptr, nullptr, nullptr, nullptr, 0);
  } else {  // huge batches: one digit-major scan launch per pass
    hipLaunchKernelGGL((plan_count_kernel<0, false>), g, blk, 0, st, offsets, n_markets, nullptr, counts, chunks, crec);
    hipLaunchKernelGGL((plan_scan_kernel<true>), sg, sblk, 0, st, counts, kPlanDigits * chunks, crec, chunks, info,
                       bin_start_dev, fw, raise_long);
    hipLaunchKernelGGL((plan_scatter_kernel<0, false>), g, blk, 0, st, offsets, n_markets, nullptr, nullptr, counts,
                       chunks, keys, idx, nullptr, nullptr, nullptr, nullptr, 0);
    hipLaunchKernelGGL((plan_count_kernel<1, false>), g, blk, 0, st, offsets, n_markets, keys, counts, chunks, nullptr);
    hipLaunchKernelGGL((plan_scan_kernel<false>), sg, sblk, 0, st, counts, kPlanDigits * chunks, nullptr, (int64_t)0,
                       nullptr, nullptr, nullptr, 0);
    hipLaunchKernelGGL((plan_scatter_kernel<1, false>), g, blk, 0, st, offsets, n_markets, keys, idx, counts, chunks,
                       nullptr, order, nullptr, nullptr, nullptr, nullptr, 0);
  }
  *info_out = info;
  return check_launch("plan_bins_device");
}

extern "C" int bce_plan_bins_device_async(const int64_t* offsets, int64_t n_markets, int32_t* order,
                                          int64_t* bin_start_dev, void* scratch, int64_t scratch_bytes,
                                          void* stream) {
  BCE_REQUIRE(n_markets >= 0 && n_markets < ((int64_t)1 << 31), "plan_bins_device_async: bad n_markets %lld",
              (long long)n_markets);
  BCE_REQUIRE(bin_start_dev, "plan_bins_device_async: bin_start_dev NULL");
  hipStream_t st = as_stream(stream);
  if (n_markets == 0) {
    BCE_HIP(hipMemsetAsync(bin_start_dev, 0, (BCE_NBINS + 1) * sizeof(int64_t), st));
    return BCE_OK;
  }
  BCE_REQUIRE(offsets && order && scratch, "plan_bins_device_async: NULL argument");
  BCE_REQUIRE(scratch_bytes >= bce_plan_device_scratch_bytes(n_markets), "plan_bins_device_async: scratch too small");
  PlanInfo* info = nullptr;
  return plan_device_launch(offsets, n_markets, order, scratch, st, &info, bin_start_dev, 1);
}
