// consensus_api.hip -- the C entries of the batched consensus: bce_consensus_csr (one launch
// picked by the longest market), bce_consensus_planned / bce_consensus_planned_device (the
// launches plan_schedule lists for a length-binned plan, plan_host.hpp), and the two small
// kernels that go with them, bce_validate_csr and bce_table_pack.  The consensus kernels and
// their launchers are consensus.hip, consensus_lane.hip, consensus_tab.hip and consensus_wide.hip
// (with wide_sort.hpp and ordered_chain.hpp).
#include "consensus_common.hpp"
#include "plan_host.hpp"

namespace bce {
namespace {

__global__ void max_len_kernel(const int64_t* offsets, int64_t n, const int32_t* list, int64_t n_list,
                               unsigned long long* out) {
  int64_t best = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_list;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = list ? list[i] : i;
    const int64_t len = offsets[m + 1] - offsets[m];
    best = len > best ? len : best;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t x = __shfl_xor(best, o);
    best = x > best ? x : best;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(out, (unsigned long long)best);
}

// The argument checks of the three consensus entries, in two steps because an entry's check of
// its plan has always come between them: the batch and the source table ...
int check_tables(const int64_t* offsets, int64_t n_markets, const double* relconf, const uint32_t* present_bits,
                 int32_t n_sources, double* consensus, double* confidence, double* total_weight,
                 int32_t* n_unique) {
  BCE_REQUIRE(n_markets >= 0, "consensus: n_markets < 0");
  BCE_REQUIRE(n_markets == 0 || offsets, "consensus: offsets is NULL");
  BCE_REQUIRE(n_markets == 0 || (consensus && confidence && total_weight && n_unique),
              "consensus: per-market outputs must be non-NULL");
  BCE_REQUIRE(n_sources >= 0 && (n_sources == 0 || (relconf && present_bits)),
              "consensus: source table is NULL");
  BCE_REQUIRE((uintptr_t)relconf % 16 == 0, "consensus: relconf must be 16-byte aligned");
  return BCE_OK;
}

// ... then the mode and the signal arrays (messages under the entry's prefix `who`), and the
// ConsArgs every launch of the entry starts from: everything but the market list.
int make_args(const char* who, const int64_t* offsets, const int32_t* sid, const double* prob, int64_t n_signals,
              const double* relconf, const uint32_t* present_bits, int32_t n_sources, int32_t mode,
              double* consensus, double* confidence, double* total_weight, int32_t* n_unique, int32_t* err_idx,
              int32_t* usid, double* weight, double* nweight, ConsArgs* out) {
  BCE_REQUIRE(mode == BCE_MODE_EXACT || mode == BCE_MODE_FAST, "%s: bad mode %d", who, mode);
  BCE_REQUIRE(n_signals == 0 || (sid && prob), "%s: sid/prob NULL", who);
  ConsArgs a{};
  a.offsets = offsets; a.sid = sid; a.prob = prob;
  a.relconf = reinterpret_cast<const double2*>(relconf); a.pbits = present_bits;
  a.n_sources = n_sources; a.n_signals = n_signals;
  a.consensus = consensus; a.confidence = confidence; a.total_weight = total_weight;
  a.n_unique = n_unique; a.err_idx = err_idx; a.usid = usid; a.weight = weight; a.nweight = nweight;
  a.mode = mode;
  a.fault = fault_word();
  a.spin_cap = spin_cap();
  *out = a;
  return BCE_OK;
}

// the 32-bit (sid, index) key of the segment kernel needs sid < 2^(31 - log2 G)
constexpr int kSegMaxSources = 1 << 25;

}  // namespace
}  // namespace bce

using namespace bce;

extern "C" int bce_consensus_csr(const int64_t* offsets, int64_t n_markets, const int32_t* sid,
                                 const double* prob, int64_t n_signals, const double* relconf,
                                 const uint32_t* present_bits, int32_t n_sources,
                                 const int32_t* market_list, int64_t n_list, int32_t max_len,
                                 int32_t mode, double* consensus, double* confidence,
                                 double* total_weight, int32_t* n_unique, int32_t* err_idx,
                                 int32_t* usid, double* weight, double* nweight, void* stream) {
  int rc = check_tables(offsets, n_markets, relconf, present_bits, n_sources, consensus, confidence, total_weight,
                        n_unique);
  if (rc) return rc;
  ConsArgs a;
  rc = make_args("consensus", offsets, sid, prob, n_signals, relconf, present_bits, n_sources, mode, consensus,
                 confidence, total_weight, n_unique, err_idx, usid, weight, nweight, &a);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  a.list = market_list;
  a.n_list = market_list ? n_list : n_markets;
  if (a.n_list == 0) return BCE_OK;
  int64_t L = max_len;
  if (L <= 0) {  // unknown: measure on device (synchronises)
    unsigned long long* d = nullptr;
    BCE_HIP(hipMallocAsync((void**)&d, sizeof(unsigned long long), st));
    BCE_HIP(hipMemsetAsync(d, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(max_len_kernel, dim3(256), dim3(256), 0, st, offsets, n_markets, market_list,
                       a.n_list, d);
    unsigned long long h = 0;
    BCE_HIP(hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, st));
    BCE_HIP(hipFreeAsync(d, st));
    BCE_HIP(hipStreamSynchronize(st));
    L = (int64_t)h;
  }
  if (L <= 64 && n_sources <= kSegMaxSources) return launch_seg_for_len((int)(L < 1 ? 1 : L), a, st);
  if (L <= kLongMaxLds) return launch_wide_len(L, a, st);
  const int64_t bytes = long_scratch_bytes(a.n_list, L);
  void* scratch = nullptr;
  BCE_HIP(hipMallocAsync(&scratch, (size_t)bytes, st));
  rc = launch_long_global(a, scratch, long_scratch_stride(a.n_list, bytes), st);
  BCE_HIP(hipFreeAsync(scratch, st));
  return rc;
}

// The host-planned launch: what plan_schedule lists for the plan's bin counts, each launch over
// its range of the plan order (a merged launch: bin b1's markets first, then the shorter bins').
extern "C" int bce_consensus_planned(const int64_t* offsets, int64_t n_markets, const int32_t* sid,
                                     const double* prob, int64_t n_signals, const double* relconf,
                                     const uint32_t* present_bits, int32_t n_sources,
                                     const int32_t* order, const int64_t* bin_start_host,
                                     int32_t mode, double* consensus, double* confidence,
                                     double* total_weight, int32_t* n_unique, int32_t* err_idx,
                                     int32_t* usid, double* weight, double* nweight, void* scratch,
                                     int64_t scratch_bytes, void* stream) {
  int rc = check_tables(offsets, n_markets, relconf, present_bits, n_sources, consensus, confidence, total_weight,
                        n_unique);
  if (rc) return rc;
  BCE_REQUIRE(bin_start_host && (order || n_markets == 0), "planned: missing plan");
  ConsArgs base;
  rc = make_args("planned", offsets, sid, prob, n_signals, relconf, present_bits, n_sources, mode, consensus,
                 confidence, total_weight, n_unique, err_idx, usid, weight, nweight, &base);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const bool seg_ok = n_sources <= kSegMaxSources;
  const PlanSchedule s =
      plan_schedule(bin_start_host, mode, [&](int b) { return wide_resident(kBinMax[b], mode, n_sources); });
  hipStream_t side = st;
  std::unique_lock<std::mutex> fork_lock;
  rc = side_fork(st, s.fork, &side, &fork_lock);
  if (rc) return rc;
  for (int i = 0; i < s.n && !rc; ++i) {
    const PlanLaunch& l = s.launch[i];
    ConsArgs a = base;
    a.list = order + bin_start_host[l.b0];
    a.n_list = bin_start_host[l.b1 + 1] - bin_start_host[l.b0];
    if (l.b0 != l.b1) {  // merged: this bin's (longer) markets first, then the bins below
      a.list_hi = order + bin_start_host[l.b1];
      a.n_hi = bin_start_host[l.b1 + 1] - bin_start_host[l.b1];
    }
    hipStream_t sb = l.side ? side : st;
    if (l.b1 <= kPlanSideLast) {
      rc = seg_ok ? launch_seg_for_len((int)kBinMax[l.b1], a, sb) : launch_long_lds(a, sb);
    } else if (l.b1 < BCE_NBINS - 1) {
      rc = launch_wide_len(kBinMax[l.b1], a, sb);
    } else {
      // scratch stride from the caller's sizing (bce_consensus_scratch_bytes)
      const int64_t P = long_scratch_stride(a.n_list, scratch_bytes);
      if (P <= kLongMaxLds) {  // not BCE_REQUIRE: the side stream must still be joined
        set_error("planned: scratch too small for the >4096 bin");
        rc = BCE_EINVAL;
      } else {
        rc = launch_long_global(a, scratch, P, sb);
      }
    }
  }
  const int rj = side_join(st, s.fork);  // join even after a failed launch: st must not run ahead
  if (!rc) rc = rj;
  return rc;
}

// The planned launch driven by device bin boundaries (bce_plan_bins_device_async): no host
// sync between planning and consensus.  Every launch of the schedule gets its kernel's resident
// grid (its market count is not known on the host) and reads its range of the plan order at
// entry (dev_range); an empty bin's launch exits at once.  Markets longer than 4096 are not
// computed: they raise the device fault word (a caller with such markets uses the
// host-synchronised plan).
extern "C" int bce_consensus_planned_device(const int64_t* offsets, int64_t n_markets, const int32_t* sid,
                                            const double* prob, int64_t n_signals, const double* relconf,
                                            const uint32_t* present_bits, int32_t n_sources, const int32_t* order,
                                            const int64_t* bin_start_dev, int32_t mode, double* consensus,
                                            double* confidence, double* total_weight, int32_t* n_unique,
                                            int32_t* err_idx, int32_t* usid, double* weight, double* nweight,
                                            void* stream) {
  int rc = check_tables(offsets, n_markets, relconf, present_bits, n_sources, consensus, confidence, total_weight,
                        n_unique);
  if (rc) return rc;
  if (n_markets == 0) return BCE_OK;
  BCE_REQUIRE(bin_start_dev && order, "planned_device: missing plan");
  ConsArgs base;
  rc = make_args("planned_device", offsets, sid, prob, n_signals, relconf, present_bits, n_sources, mode, consensus,
                 confidence, total_weight, n_unique, err_idx, usid, weight, nweight, &base);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  base.list = order;           // the whole plan order: each launch's range is read on the device
  base.n_list = n_markets;     // upper bound: sizes the launch grids
  base.dev_bins = bin_start_dev;
  const bool seg_ok = n_sources <= kSegMaxSources;
  const PlanSchedule s = plan_schedule(nullptr, mode, [](int) { return (int64_t)0; });
  hipStream_t side = st;
  std::unique_lock<std::mutex> fork_lock;
  rc = side_fork(st, s.fork, &side, &fork_lock);
  if (rc) return rc;
  for (int i = 0; i < s.n && !rc; ++i) {
    const PlanLaunch& l = s.launch[i];
    ConsArgs a = base;
    a.dev_b0 = l.b0;
    a.dev_b1 = l.b1;
    hipStream_t sb = l.side ? side : st;
    if (l.b1 > kPlanSideLast) {
      rc = launch_wide_len(kBinMax[l.b1], a, sb);
    } else if (seg_ok) {
      rc = launch_seg_for_len((int)kBinMax[l.b1], a, sb);
    } else {
      rc = BCE_EUNSUPPORTED;  // (n_sources > 2^25: the long-LDS kernel has no device range)
      set_error("planned_device: more than 2^25 sources -- use bce_consensus_planned");
    }
  }
  const int rj = side_join(st, s.fork);
  if (!rc) rc = rj;
  return rc;
}

// ======================================================================================
// validation only: core.validate_input_payload range check (core.py:59-60)
// ======================================================================================
namespace bce {
__global__ __launch_bounds__(256) void validate_kernel(const int64_t* offsets, int64_t n_markets,
                                                       const double* prob, int32_t* err_idx) {
  const int lane = lane_id();
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t m = wave; m < n_markets; m += nwaves) {
    const int64_t a = offsets[m], b = offsets[m + 1];
    int32_t e = -1;
    for (int64_t base = a; base < b; base += 64) {
      const int64_t i = base + lane;
      const double p = (i < b) ? prob[i] : 0.5;
      const unsigned long long bad = ballot(p < 0.0 || p > 1.0);  // NaN passes
      if (bad) {
        e = (int32_t)(base - a) + __builtin_ctzll(bad);
        break;
      }
    }
    if (lane == 0) err_idx[m] = e;
  }
}
}  // namespace bce


extern "C" int bce_validate_csr(const int64_t* offsets, int64_t n_markets, const double* prob,
                                int32_t* err_idx, void* stream) {
  BCE_REQUIRE(n_markets >= 0, "validate: n_markets < 0");
  if (n_markets == 0) return BCE_OK;
  BCE_REQUIRE(offsets && prob && err_idx, "validate: NULL argument");
  int64_t blocks = (n_markets + 3) / 4;
  const int64_t cap = grid_cap(16);
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(validate_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), offsets,
                     n_markets, prob, err_idx);
  return check_launch("validate_kernel");
}

// ======================================================================================
// source-table packing: separate (rel, conf, present) -> the consensus layout
// ======================================================================================
namespace bce {
__global__ __launch_bounds__(256) void table_pack_kernel(int64_t n, const double* rel, const double* conf,
                                                         const uint8_t* present, double2* relconf,
                                                         uint32_t* bits) {
  const int lane = lane_id();
  for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < ((n + 63) & ~63ll);
       s += (int64_t)gridDim.x * blockDim.x) {
    const bool in = s < n;
    if (in) relconf[s] = make_double2(rel[s], conf[s]);
    const unsigned long long b = ballot(in && (present == nullptr || present[s] != 0));
    if (lane == 0 && s < n) bits[s >> 5] = (uint32_t)b;
    if (lane == 32 && s < n) bits[s >> 5] = (uint32_t)(b >> 32);
  }
}
}  // namespace bce

extern "C" int bce_table_pack(int64_t n, const double* rel, const double* conf, const uint8_t* present,
                              double* relconf, uint32_t* present_bits, void* stream) {
  BCE_REQUIRE(n >= 0, "table_pack: n < 0");
  if (n == 0) return BCE_OK;
  BCE_REQUIRE(rel && conf && relconf && present_bits, "table_pack: NULL argument");
  BCE_REQUIRE((uintptr_t)relconf % 16 == 0, "table_pack: relconf must be 16-byte aligned");
  int64_t blocks = (n + 255) / 256;
  const int64_t cap = grid_cap(16);
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(table_pack_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), n, rel, conf,
                     present, reinterpret_cast<double2*>(relconf), present_bits);
  return check_launch("table_pack_kernel");
}
