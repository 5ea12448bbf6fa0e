/*
 * bce.h -- C ABI of the MI355X-native batched consensus engine (libbce_hip.so).
 *
 * This is the drop-in boundary for the reference's hot path
 * (consensus-nexus/bayesian-consensus-engine, src/bayesian_engine/).  The reference is
 * pure Python and exposes no plugin registry, so the boundary is
 * this C ABI, bound from Python with ctypes (see INTEGRATION.md for the binding a
 * maintainer of the reference would add).  Every entry point names the reference
 * function it replaces.
 *
 * Conventions
 *  - All arrays are DEVICE pointers (hipMalloc / torch tensors on cuda:N) unless the
 *    name ends in _host.  Work is enqueued on `stream` (a hipStream_t; NULL = the
 *    legacy default stream).  Nothing synchronises unless stated.
 *  - Every entry point returns an int status: BCE_OK (0) or a negative BCE_E*; the
 *    library keeps no global mutable state besides the last-error string
 *    (bce_last_error(), thread-local).  The caller owns every buffer; the library never
 *    frees caller memory.
 *  - Markets are CSR: offsets[M+1] int64 (offsets[0] may be non-zero: a shard view),
 *    sid[N] int32 = interned source rank ids whose integer order equals Python's
 *    sorted() order of the sourceId strings (code-point order), prob[N] fp64.
 *  - The consensus source table is dense over rank ids and laid out for the gather:
 *    relconf[2*S] fp64 = interleaved {reliability, confidence} pairs (16-byte aligned, one
 *    16-B load per unique source) with the cold-start defaults (config.py:17-18) baked in
 *    for absent keys, and present_bits[ceil(S/32)] u32 = bit s%32 of word s/32 set iff
 *    the sourceId is a key of source_reliability (core.py:167-170).  bce_table_pack
 *    builds it from separate rel/conf/present arrays.
 *  - Per-unique-source outputs are written at the market's CSR offsets: slot
 *    offsets[m]+j for j < n_unique[m].  Slots n_unique[m] <= j < n (the market's length)
 *    are scratch: a kernel may leave them untouched or write unspecified values there
 *    (the short-market kernel stores whole 16-byte chunks).  Nothing outside the
 *    market's own [offsets[m], offsets[m+1]) range is ever written.  usid carries the
 *    cold-start bit in bit 31 (value = rank | cold << 31).
 *  - Floating point follows CPython: no fused multiply-add anywhere on the parity path,
 *    sums in the reference's order in BCE_MODE_EXACT (bit-exact vs the reference).
 */
#ifndef BCE_H
#define BCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCE_ABI_VERSION 3  /* 3: BCE_NBINS 13 (1536 and 3072 length bins), tie-break per-group scratch slots */

enum bce_status {
    BCE_OK = 0,
    BCE_EINVAL = -1,      /* bad argument (null pointer, size, sid out of range) */
    BCE_EHIP = -2,        /* a HIP runtime call failed (message in bce_last_error) */
    BCE_EUNSUPPORTED = -3 /* shape outside what this build handles */
};

enum bce_mode {
    BCE_MODE_EXACT = 0, /* reference summation order: bit-exact outputs */
    BCE_MODE_FAST = 1   /* tree reductions for long markets (<= 1e-9 abs vs reference) */
};
/* BCE_MODE_FAST reproducibility: deterministic for a given call (the same launch reproduces
 * every bit), but NOT invariant to batch composition.  bce_consensus_planned merges a small
 * call's non-power-of-two bins (1025..1536, 2049..3072) into the launch of the bin above when a
 * launch would fill fewer than 6 rounds of its resident grid (which depends on the market count
 * and the GPU's CU count); the wider workgroup sums the partial totals over 8 instead of 6 (4
 * instead of 3) waves.  So one market's consensus / confidence / total weight / normalizedWeight
 * can differ in the last bits between a full batch, a shard of it, or another GPU model -- always
 * within the 1e-9 bound.  Integer outputs, usid and weight are bit-exact in both modes, and
 * BCE_MODE_EXACT is bit-identical in every launch shape. */

/* Tie-break labels (tiebreak.py:123-133, 89-96). */
enum bce_tb_label {
    BCE_TB_UNANIMOUS = 0,
    BCE_TB_WEIGHT_DENSITY = 1,
    BCE_TB_PREDICTION_VALUE_SMALLEST = 2,
    BCE_TB_SINGLE_AGENT = 3
};

#define BCE_NO_TIMESTAMP INT64_MIN /* falsy / unparseable updated_at (decay.py:125-131) */

/* ---- library ------------------------------------------------------------------ */
int bce_abi_version(void);
const char* bce_last_error(void);
/* Number of visible devices (0 on a machine without a GPU; never fails). */
int bce_device_count(void);
/* Synchronise `stream` and report (then clear) the current device's fault word: a kernel
 * that had to give up -- a persistent wave whose bounded wait expired, a sid >= n_sources,
 * a market longer than the max_len it was launched with -- records a code there instead
 * of failing silently.  BCE_OK when clean, else BCE_EHIP with the reason in
 * bce_last_error(). */
int bce_fault_check(void* stream);
/* Test hook: polls a persistent wave makes before giving up (<= 0 restores the default,
 * 2^22).  A tiny cap makes the pipe kernel's waves give up at once, which exercises the
 * fault path above; results of such a launch are garbage. */
int bce_debug_set_spin_cap(int cap);
/* Test hook: caps every persistent grid at `blocks` workgroups (<= 0 restores the default, CUs x
 * resident workgroups); it is for tests, a smaller grid is always fully resident, and results
 * must not depend on it. */
int bce_debug_set_grid_cap(int blocks);
/* Self-test of the wide kernel's VALU lane exchanges (DPP / permlane swaps) and wave scan:
 * one wave writes 13*64 words to `out` (see consensus_wide.hip); tests run it first. */
int bce_debug_lane_selftest(unsigned* out, void* stream);
/* Host run of the exact big-integer round(x, ndigits) the tie-break kernels use for
 * 23 <= ndigits <= 323 and -308 <= ndigits <= -16 (valid for any 1 <= |ndigits| in range):
 * for the CPU tests against Python round().  *overflow = 1 where CPython raises
 * OverflowError.  No GPU needed. */
double bce_debug_py_round(double x, int32_t ndigits, int32_t* overflow);

/* ---- consensus: core.compute_consensus (core.py:63-179) + validation -------------
 *
 * Replaces: core.compute_consensus(signals, source_reliability) for every market of
 * the batch, and the numeric part of core.validate_input_payload (core.py:59-60):
 * err_idx[m] = first signal index whose probability is < 0 or > 1 (NaN passes), -1 if
 * none.  Also the batch loop MarketStore.compute_all_consensus (market.py:200-221).
 *
 * Outputs per market: consensus (0.0 where null), confidence, total_weight,
 * n_unique, err_idx (may be NULL to skip).  null <=> total_weight == 0 (core.py:131)
 * or the market is empty (core.py:88-96).  Per unique source (sorted by rank):
 * usid (rank | cold<<31), weight (= reliability, core.py:119), nweight
 * (core.py:151).  Any of usid/weight/nweight may be NULL ("compact" mode).
 *
 * market_list (nullable): process only markets market_list[0..n_list) (ascending
 * market indices recommended).  NULL = all markets 0..n_markets.  max_len is an
 * upper bound on the market lengths processed (0 = unknown: the library computes it,
 * which synchronises the stream).  n_sources bounds sid.
 */
int bce_consensus_csr(const int64_t* offsets, int64_t n_markets, const int32_t* sid,
                      const double* prob, int64_t n_signals, const double* relconf,
                      const uint32_t* present_bits, int32_t n_sources,
                      const int32_t* market_list, int64_t n_list, int32_t max_len, int32_t mode,
                      double* consensus, double* confidence, double* total_weight,
                      int32_t* n_unique, int32_t* err_idx, int32_t* usid, double* weight,
                      double* nweight, void* stream);

/* Pack separate rel[S], conf[S], present[S] (u8, nullable = all present) into the
 * consensus table layout: relconf[2*S] interleaved, present_bits[ceil(S/32)]. */
int bce_table_pack(int64_t n, const double* rel, const double* conf, const uint8_t* present,
                   double* relconf, uint32_t* present_bits, void* stream);

/* Validation only (core.validate_input_payload's numeric check, core.py:59-60):
 * err_idx[m] = first signal index with probability < 0 or > 1 (NaN passes), -1 if none.
 * The structural/type checks (core.py:34-58) are done where the Python objects live. */
int bce_validate_csr(const int64_t* offsets, int64_t n_markets, const double* prob,
                     int32_t* err_idx, void* stream);

/* Host-planned variant for ragged batches: the caller bins markets by length once
 * (bce_plan_bins on HOST offsets) and passes the device copy of the ordered market
 * list plus the bin boundaries.  bin_start has BCE_NBINS+1 entries (host array).  Inside
 * a bin markets keep their index order, except the wide bins (65..4096 signals), which
 * are ordered longest first (ties by index) so each launch ends on its short markets.
 * bce_consensus_planned runs the n <= 64 bins on a library-owned side stream (one per
 * device) forked from `stream` by an event and joined back into it before it returns, so
 * the caller sees ordinary stream order; concurrent callers are serialised over the fork. */
#define BCE_NBINS 13 /* n<=8, <=16, <=32, <=64, <=128, <=256, <=512, <=1024, <=1536, <=2048, <=3072, <=4096, >4096 */
int bce_plan_bins(const int64_t* offsets_host, int64_t n_markets, int32_t* order_host,
                  int64_t* bin_start_host, int32_t* max_len_host);
/* The same plan built on the GPU from DEVICE offsets (no D2H copy of the CSR, no host sort):
 * a stable two-pass LSD radix sort of the market indices by a 12-bit key (bin, then longest
 * first inside the wide bins), so `order` (device int32[n_markets]) is bit-identical to
 * bce_plan_bins'.  Enqueued on `stream`; the call then SYNCHRONISES that stream to return the
 * bin boundaries (host int64[BCE_NBINS+1]), the longest market (host, nullable) and the >4096
 * bin's scratch bytes for bce_consensus_planned (host, nullable).  scratch: device buffer of
 * bce_plan_device_scratch_bytes(n_markets) bytes (256-byte aligned).  Decreasing offsets ->
 * BCE_EINVAL (as bce_plan_bins).  Replaces the per-call host planning of a fresh batch
 * (the reference sorts each market's sources, core.py:103, inside its market loop,
 * market.py:200-221). */
int bce_plan_bins_device(const int64_t* offsets, int64_t n_markets, int32_t* order, int64_t* bin_start_host,
                         int32_t* max_len_host, int64_t* long_scratch_bytes_host, void* scratch,
                         int64_t scratch_bytes, void* stream);
int64_t bce_plan_device_scratch_bytes(int64_t n_markets);
/* The same plan without any host synchronisation: the bin boundaries stay on the device
 * (bin_start_dev, device int64[BCE_NBINS+1]); decreasing offsets raise the device fault word
 * (bce_fault_check) and leave every bin empty.  Pair with bce_consensus_planned_device. */
int bce_plan_bins_device_async(const int64_t* offsets, int64_t n_markets, int32_t* order, int64_t* bin_start_dev,
                               void* scratch, int64_t scratch_bytes, void* stream);
/* bce_consensus_planned over a device-resident plan: every bin's kernel reads its range of the
 * plan order on the device, so planning + consensus of a fresh batch enqueue with no host sync.
 * Launch structure of a full batch (no small-call merges).  Markets longer than 4096 signals are
 * not computed and raise the device fault word (use bce_plan_bins_device + bce_consensus_planned
 * for them); n_sources must be <= 2^25. */
int bce_consensus_planned_device(const int64_t* offsets, int64_t n_markets, const int32_t* sid, const double* prob,
                                 int64_t n_signals, const double* relconf, const uint32_t* present_bits,
                                 int32_t n_sources, const int32_t* order, const int64_t* bin_start_dev,
                                 int32_t mode, double* consensus, double* confidence, double* total_weight,
                                 int32_t* n_unique, int32_t* err_idx, int32_t* usid, double* weight,
                                 double* nweight, void* stream);
/* The launches bce_consensus_planned makes for a plan (bin_start_host, host int64[BCE_NBINS+1]),
 * or bce_consensus_planned_device makes (bin_start_host NULL), in issue order.  Host code only:
 * no GPU, and the resident workgroups of each wide bin's kernel come from the caller
 * (resident, host int64[BCE_NBINS], entries 4..11 read) -- a cost model prices a rank's markets
 * with it (sharding._rank_main_us).  launches: host int32[BCE_NBINS][3], rows {b0, b1, side}:
 * the markets of bins b0..b1 in one kernel sized for bin b1, side != 0 on the side stream;
 * *n_launches rows are written.  *fork: whether the side stream is forked and joined. */
int bce_plan_schedule(const int64_t* bin_start_host, int32_t mode, const int64_t* resident, int32_t* launches,
                      int32_t* n_launches, int32_t* fork);
/* Bytes of device scratch bce_consensus_planned needs for the >4096 bin. */
int64_t bce_consensus_scratch_bytes(const int64_t* offsets_host, const int32_t* order_host,
                                    const int64_t* bin_start_host);
int bce_consensus_planned(const int64_t* offsets, int64_t n_markets, const int32_t* sid,
                          const double* prob, int64_t n_signals, const double* relconf,
                          const uint32_t* present_bits, int32_t n_sources,
                          const int32_t* order, const int64_t* bin_start_host, int32_t mode,
                          double* consensus, double* confidence, double* total_weight,
                          int32_t* n_unique, int32_t* err_idx, int32_t* usid, double* weight,
                          double* nweight, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- consensus history: every market's consensus after each signal arrived --------
 *
 * Replaces: the online use of a Market (market.py: add_signal, compute_consensus, add_signal
 * again): point k of market m, stored at CSR position offsets[m] + k, is
 * core.compute_consensus (core.py:63-180) of the market's first k + 1 signals in arrival
 * (CSR) order.  Per point: consensus (0.0 where the reference returns None, core.py:131-133),
 * confidence (0.0 there too), total_weight, n_unique; null <=> total_weight == 0.  All four
 * outputs have n_signals elements.  Probabilities outside [0, 1] are computed, not rejected
 * (bce_validate_csr is the range check).  Exact order only; no per-unique outputs.
 *
 * Every signal is read once (the expansion into prefix markets reads (n + 1) / 2 times as
 * many); the arithmetic is quadratic in a market's length by construction (each prefix is
 * its own ordered sum).  Markets of up to 4096 signals; a longer one (or one longer than a
 * max_len <= 64 launch takes) is left untouched and raises the device fault word, as does a
 * sid outside [0, n_sources), whose row read is clamped (bce_fault_check).  present_bits is
 * not read (cold sources carry their defaults in relconf) and may be NULL.
 *
 * Which markets, and how they are launched:
 *   bin_start_host and bin_start_dev NULL: markets market_list[0..n_list) (NULL: all) in ONE
 *     launch sized by max_len, an upper bound on their lengths (0 = unknown: as 4096); no host
 *     synchronisation.
 *   bin_start_host (host int64[BCE_NBINS+1], bce_plan_bins / bce_plan_bins_device): market_list
 *     is the plan's order (device); one launch per non-empty length bin, longest first.
 *   bin_start_dev (device int64[BCE_NBINS+1], bce_plan_bins_device_async): the same with the
 *     bin boundaries read on the device; no host synchronisation.
 * Positions of markets outside the list or the plan are left untouched.  A NULL required
 * pointer, a negative size or max_len outside [0, 4096] returns BCE_EINVAL before anything
 * touches the GPU. */
int bce_consensus_history(const int64_t* offsets, int64_t n_markets, const int32_t* sid, const double* prob,
                          int64_t n_signals, const double* relconf, const uint32_t* present_bits,
                          int32_t n_sources, const int32_t* market_list, int64_t n_list,
                          const int64_t* bin_start_host, const int64_t* bin_start_dev, int32_t max_len,
                          double* consensus, double* confidence, double* total_weight, int32_t* n_unique,
                          void* stream);

/* ---- leave-one-source-out consensus: every source's marginal effect on its market ----
 *
 * Replaces: compute_consensus([s for s in signals if s["sourceId"] != x], table) for every
 * source x of every market (core.py:63-180).  The signal at CSR position p, of source x in
 * market m, gets the consensus of m's signals whose source is not x: consensus (0.0 where the
 * reference returns None, core.py:131-133), confidence (0.0 there too), total_weight, n_unique
 * (the market's unique sources less one); null <=> total_weight == 0, which includes "nothing is
 * left".  All four outputs have n_signals elements; all signals of one source in one market hold
 * the same values.  full_* (each [n_markets]; all four NULL or all four non-NULL) receive the
 * market's own consensus, bit-identical to bce_consensus_csr in exact mode; the row of an empty
 * market is zeros.  Exact order only; no per-unique outputs.
 *
 * Every signal is read once (the expansion into one reduced market per signal reads about U - 1
 * times as many, U the market's unique sources).  A market is sorted once, every source's
 * average and products are formed once, and leave-out j is the ordered sum of the three columns
 * over the other sources: O(n + U^2) per market.
 *
 * The arguments before the outputs, the three launch routes, the fault word (a market over 4096
 * signals or over the bound of a max_len <= 64 launch is left untouched; a sid outside
 * [0, n_sources) has its row read clamped) and the BCE_EINVAL checks are those of
 * bce_consensus_history.  Positions and full_* rows of markets outside the list or the plan are
 * left untouched. */
int bce_consensus_leave_one_out(const int64_t* offsets, int64_t n_markets, const int32_t* sid, const double* prob,
                                int64_t n_signals, const double* relconf, const uint32_t* present_bits,
                                int32_t n_sources, const int32_t* market_list, int64_t n_list,
                                const int64_t* bin_start_host, const int64_t* bin_start_dev, int32_t max_len,
                                double* consensus, double* confidence, double* total_weight, int32_t* n_unique,
                                double* full_consensus, double* full_confidence, double* full_total_weight,
                                int32_t* full_n_unique, void* stream);

/* ---- decay: get_reliability(apply_decay=True) over a table ----------------------
 * Replaces: decay.apply_reliability_decay (decay.py:61-100) composed with
 * decay.days_since_update (decay.py:103-145) as used by
 * SQLiteReliabilityStore.get_reliability (reliability.py:110-131).
 * view[s] = present[s] ? decay(rel[s], days(now_us - t_us[s])) : default_rel.
 * present may be NULL (all present).  t_us[s] == BCE_NO_TIMESTAMP means no decay. */
int bce_decay_view(int64_t n, const double* rel, const int64_t* t_us, const uint8_t* present,
                   int64_t now_us, double half_life_days, double min_rel, double default_rel,
                   double* view, void* stream);

/* ---- decay on elapsed days: decay.compute_decay_factor (decay.py:31-58) and
 * decay.apply_reliability_decay (decay.py:61-100), elementwise.  factor (nullable) gets
 * 2^(-days/h) (1.0 where days <= 0); out (nullable) gets the decayed reliability. */
int bce_decay_apply(int64_t n, const double* rel, const double* elapsed_days,
                    double half_life_days, double min_rel, double* out, double* factor,
                    void* stream);

/* ---- outcome update: compute_update / update_reliability (reliability.py:142-233) --
 * One outcome per source per call: flags[s] bit0 = participates, bit1 = correct.
 * Participants: rel = clamp(rel +- MAX_UPDATE_STEP) (reliability.py:163-169),
 * conf = min(1, conf + (1-conf)*0.1) (:172-173), t_us = now_us (:175), present = 1.
 * Absent rows start from (default_rel, default_conf) (reliability.py:133-140). */
int bce_outcome_update(int64_t n, double* rel, double* conf, int64_t* t_us, uint8_t* present,
                       const uint8_t* flags, int64_t now_us, double default_rel,
                       double default_conf, void* stream);

/* ---- replay step (config 4): decayed view at now_us, then the outcome update --------
 * flags2 is 2-bit packed: source s uses bits 2*(s%4)..+1 of byte s/4 (bit0 participates,
 * bit1 correct).  Equivalent to bce_decay_view followed by bce_outcome_update. */
int bce_replay_step(int64_t n, double* rel, double* conf, int64_t* t_us, uint8_t* present,
                    const uint8_t* flags2, int64_t now_us, double half_life_days,
                    double min_rel, double default_rel, double default_conf, double* view,
                    void* stream);

/* ---- namespaced fallback: NamespacedReliabilityStore.get_reliability ----------------
 * Replaces reliability_abstraction.py:119-188 for every source of a rank space at once.
 * Up to three scope tables in precedence order: scope 0 = market (the row keyed by
 * market_id), 1 = domain ("__domain__:<domain>"), 2 = global ("__global__"); a NULL rel
 * skips the scope, as a falsy market_id / domain does (:136, :150).  has[s] != 0 iff the
 * scope holds a row with a truthy updated_at (the `if record.updated_at:` tests).  The
 * first scope with has[s] supplies (reliability, confidence); the reliability is decayed
 * at now_us when apply_decay, as SQLiteReliabilityStore.get_reliability does
 * (reliability.py:114-123; t_us == BCE_NO_TIMESTAMP = unparseable = no decay).  No scope
 * => the cold-start defaults (:177-186).  Outputs (each nullable, at least one given):
 * relconf[2*n] = the packed consensus table, present_bits = bit set for every source
 * (mark_cold = 0: callers put every sourceId in the dict) or only for sources that
 * resolved to a stored row (mark_cold = 1), scope[s] = 0/1/2, or 3 for cold start. */
int bce_namespace_resolve(int64_t n, const double* rel0, const double* conf0, const int64_t* t0,
                          const uint8_t* has0, const double* rel1, const double* conf1,
                          const int64_t* t1, const uint8_t* has1, const double* rel2,
                          const double* conf2, const int64_t* t2, const uint8_t* has2,
                          int apply_decay, int64_t now_us, double half_life_days, double min_rel,
                          double default_rel, double default_conf, int mark_cold, double* relconf,
                          uint32_t* present_bits, uint8_t* scope, void* stream);

/* ---- tie-break: DeterministicTieBreaker.resolve (tiebreak.py:73-152) per market -----
 * Per signal: pred (AgentSignal.prediction), conf, weight, rel (reliability_score).
 * Per market: winner (rounded group key, or the raw prediction for a single agent),
 * label (enum bce_tb_label; -1 for an empty market = the reference's ValueError),
 * n_groups, variance (unrounded population variance of conf, tiebreak.py:108-110).
 * Per group, first-seen order, at CSR offsets: key, count, weight density, avg conf,
 * max reliability (tiebreak.py:58-71); per signal (nullable g_of) the ordinal of its group,
 * which lets a caller rebuild the reference's dict keys with their Python types (an int
 * prediction keys its group with an int).  Group pointers may be NULL.  ndigits is the
 * DeterministicTieBreaker precision: CPython round(x, ndigits) restated exactly for every
 * int (tiebreak.py:46-47,54): -15 <= ndigits <= 22 with doubles, ndigits < -308 (signed
 * zero), ndigits > 323 (x itself), the rest with exact big integers (py_round_big.hpp).  A
 * rounded key too large for a double (ndigits <= -16, |x| near DBL_MAX: CPython raises
 * OverflowError) sets device fault 6, which bce_fault_check reports.
 * Slots n_groups <= j < n of a market's per-group outputs are scratch (unspecified values).
 * bce_tiebreak_csr: markets market_list[0..n_list) (NULL = all), every length <= max_len
 * <= 64 (one lane per market up to 32 agents, one wave per market beyond).  bce_tiebreak_csr_long: markets of any length >= 1, max_len
 * >= every listed market's length (one workgroup per market; sorted in LDS up to 4096
 * agents, beyond that in a global scratch slice the library allocates on `stream`). */
int bce_tiebreak_csr(const int64_t* offsets, int64_t n_markets, const int32_t* market_list,
                     int64_t n_list, const double* pred, const double* conf, const double* weight,
                     const double* rel, int32_t max_len, int32_t ndigits, double* winner,
                     int32_t* label, int32_t* n_groups, double* variance, double* g_key,
                     int32_t* g_count, double* g_density, double* g_avgconf, double* g_maxrel,
                     int32_t* g_of, void* stream);
int bce_tiebreak_csr_long(const int64_t* offsets, int64_t n_markets, const int32_t* list,
                          int64_t n_list, int32_t ndigits, const double* pred, const double* conf,
                          const double* weight, const double* rel, int64_t max_len, double* winner,
                          int32_t* label, int32_t* n_groups, double* variance, double* g_key,
                          int32_t* g_count, double* g_density, double* g_avgconf, double* g_maxrel,
                          int32_t* g_of, void* stream);

/* ---- agreement statistics: CrossMarketAggregator.summarize_sources counts -----------
 * (market.py:279-304).  outcome[m]: -1 skip (unresolved), 0 false, 1 true.
 * correct[sid] / total[sid] are ACCUMULATED (zero them first); int32 atomics, exact.
 * sid is not range-checked and must lie in [0, len(correct)). */
int bce_agreement_stats(const int64_t* offsets, int64_t n_markets, const int32_t* sid,
                        const double* prob, const int8_t* outcome, int32_t* correct,
                        int32_t* total, void* stream);

/* ---- cross-market aggregation: CrossMarketAggregator.aggregate_consensus ------------
 * (market.py:340-408) for n_groups groups at once.  Group g is the ordered member list
 * members[group_offsets[g] .. group_offsets[g+1]) of market indices (< n_markets; the
 * markets matched by the patterns in list_markets order, duplicates kept, :355-357).
 * has_consensus[m] != 0 iff market m has a consensus result whose consensus is not None
 * (:369-375).  Per group (outputs nullable): wavg = weighted_average (:386-393), median
 * = sorted(consensus)[k // 2] (:394-397), majority (:398-401), mean_conf = the result's
 * confidence (:407), n_included = k.  k == 0 => the float outputs are NaN (the reference
 * returns consensus None).  Sums are left to right in list order: bit-exact.  A member index
 * outside [0, n_markets) counts as a market without a consensus (skipped, nothing is read).  The
 * median is the element sorted() would return -- sorted() is stable and compares 0.0 == -0.0, so
 * a zero median keeps the sign of the zero at that list position.  The median of a group holding
 * a NaN consensus is unspecified. */
int bce_aggregate_groups(const int64_t* group_offsets, int64_t n_groups, const int64_t* members,
                         int64_t n_markets, const double* consensus, const double* confidence,
                         const uint8_t* has_consensus, double* wavg, double* median,
                         double* majority, double* mean_conf, int64_t* n_included, void* stream);

/* ---- re-estimation (config 5): consensus <-> reliability over a dense matrix --------
 * P is agent-major [A][ld] fp64 (column m of market m; ld >= M).  One pass:
 *   consensus[m] = sum_a P[a][m]*w[a] / sum_a w[a]  (agent order, core.py:130-144),
 *   null[m] = (sum_a w[a] == 0);
 * then agreement[a] += #{m not null : (P[a][m] >= 0.5) == (consensus[m] >= 0.5)}
 * (market.py:298-304) and resolved += #{m not null}.  w_new[a] = agree/resolved
 * (0.5 if resolved == 0, market.py:310) is bce_reestimate_weights. */
int bce_reestimate_consensus(const double* P, int64_t A, int64_t M, int64_t ld, const double* w,
                             double* consensus, uint8_t* null_out, void* stream);
int bce_reestimate_agreement(const double* P, int64_t A, int64_t M, int64_t ld,
                             const double* consensus, const uint8_t* null_in,
                             int64_t* agreement, int64_t* resolved, void* stream);
int bce_reestimate_weights(int64_t A, const int64_t* agreement, const int64_t* resolved,
                           double* w, void* stream);
/* Single-read iteration (what batch.reestimate runs): the consensus pass above that also
 * records the votes, then agreement from the votes alone, so P is read once per iteration.
 * vote_bits [K][A] uint64 with K = ceil(M/64): bit j of vote_bits[k][a] = (P[a][64k+j] >= 0.5);
 * cvote_words[k] bit j = market 64k+j is resolved and its consensus >= 0.5; ok_words[k] bit
 * j = market 64k+j exists and is resolved.  Counts identical to bce_reestimate_agreement. */
int bce_reestimate_consensus_votes(const double* P, int64_t A, int64_t M, int64_t ld, const double* w,
                                   double* consensus, uint8_t* null_out, uint64_t* vote_bits,
                                   uint64_t* cvote_words, uint64_t* ok_words, void* stream);
int bce_reestimate_agreement_votes(const uint64_t* vote_bits, int64_t A, int64_t M, const uint64_t* cvote_words,
                                   const uint64_t* ok_words, int64_t* agreement, int64_t* resolved,
                                   void* stream);
/* Pass 1 of the single-read iteration on the matrix cores: w^T P with
 * v_mfma_f64_16x16x4_f64 (the north star's "MFMA contraction"; batch.reestimate
 * mode="mfma" -- mode="fast" runs bce_reestimate_consensus_votes, which streams P at the same
 * HBM rate and measured faster), same outputs as
 * bce_reestimate_consensus_votes.  consensus within 4*A*2^-53 of the agent-order value;
 * markets within 8*A*2^-53 of 0.5 (or with a finite cell outside [0, 1]) are redone in agent
 * order, so vote_bits / cvote_words / ok_words -- and the agreement counts -- are identical
 * to the exact pass (a column with a NaN cell is NaN in every order and is not redone).
 * PRECONDITION of the MFMA order: every w[a] finite and >= 0.  It is checked on the device;
 * when any weight breaks it, this call computes the iteration with the exact kernel instead
 * (results identical to bce_reestimate_consensus_votes, at exact-mode speed).  scratch:
 * device buffer of bce_reestimate_mfma_scratch_bytes(M) bytes (8-byte aligned). */
int bce_reestimate_consensus_votes_mfma(const double* P, int64_t A, int64_t M, int64_t ld, const double* w,
                                        double* consensus, uint8_t* null_out, uint64_t* vote_bits,
                                        uint64_t* cvote_words, uint64_t* ok_words, void* scratch,
                                        int64_t scratch_bytes, void* stream);
int64_t bce_reestimate_mfma_scratch_bytes(int64_t M);

/* ---- re-estimation over a ragged CSR batch: compile once, then iterate --------------
 * The same composition as above -- compute_consensus with source_reliability = w
 * (core.py:103-144), then the summarize_sources counts (market.py:293-304) and
 * w_new = correct / total (market.py:309-310) -- for CSR markets with any number of signals
 * per source, duplicates included.  Everything that depends on (offsets, sid, prob) alone is
 * compiled into one entry per unique (market, source) pair, in (market, ascending sid)
 * order (core.py:103); a round reads the entries only, each array at most once per kernel.
 *
 * bce_reestimate_csr_compile: the caller sorts the n_signals keys market * n_sources + sid
 * (sid clamped to [0, n_sources)) with a STABLE sort -> key (sorted) and perm (signal index
 * of each sorted position), and marks the n_entries runs of equal keys in
 * group_start[n_entries + 1] (group_start[n_entries] = n_signals).  Per entry e the kernel
 * writes usid[e], emarket[e], avg[e] = (0.0 + p1 + p2 ...) / count over the run's signals in
 * input order (core.py:115-116), votes[e] = n_ge << 16 | n_lt with n_ge = #{p >= 0.5}
 * (market.py:298-299; each count <= 65535, n_markets < 2^31), and sets bad[market] = 1 when
 * a signal of the run has p < 0 or p > 1 (core.py:59-60; NaN passes).  bad must be zeroed
 * first.  A raw sid outside [0, n_sources) raises the device fault word (bce_fault_check).
 *
 * bce_reestimate_csr_consensus: uoffsets[n_markets + 1] = the entry range of every market.
 * consensus[m] = sum avg * w[usid] / sum w[usid], both left to right (core.py:120,135-138);
 * null[m] = the market is empty or its weights sum to 0 (core.py:88,131; consensus 0.0);
 * outcome[m] = known[m] where known (nullable) is >= 0 (a resolved market, market.py:280),
 * else -1 (skip) for a null or bad market, else consensus >= 0.5.
 *
 * bce_reestimate_csr_agreement: for every entry of a market with outcome >= 0,
 * total[usid] += n_ge + n_lt and correct[usid] += (outcome ? n_ge : n_lt)
 * (market.py:293-302).  int64 atomics, exact and order-free; ACCUMULATED (zero them first),
 * so the shards of a batch can add into one pair of count vectors.
 *
 * bce_reestimate_csr_weights: w[s] = correct[s] / total[s], 0.5 where total[s] == 0
 * (market.py:309-310). */
int bce_reestimate_csr_compile(const int64_t* group_start, int64_t n_entries, const int64_t* perm,
                               const int64_t* key, int64_t n_signals, const int32_t* sid, const double* prob,
                               int32_t n_sources, int64_t n_markets, int32_t* usid, double* avg,
                               int32_t* votes, int32_t* emarket, uint8_t* bad, void* stream);
int bce_reestimate_csr_consensus(const int64_t* uoffsets, int64_t n_markets, const int32_t* usid,
                                 const double* avg, const uint8_t* bad, const int8_t* known, const double* w,
                                 int32_t n_sources, double* consensus, uint8_t* null_out, int8_t* outcome,
                                 void* stream);
int bce_reestimate_csr_agreement(int64_t n_entries, const int32_t* usid, const int32_t* votes,
                                 const int32_t* emarket, const int8_t* outcome, int64_t n_markets,
                                 int32_t n_sources, int64_t* correct, int64_t* total, void* stream);
int bce_reestimate_csr_weights(int64_t n_sources, const int64_t* correct, const int64_t* total, double* w,
                               void* stream);

/* ---- settlement: a batch of resolved markets into one scope of the reliability table ------
 * Replaces the per-signal loop update_reliability(source, correct) over every signal of every
 * resolved market (reliability.py:142-233, reliability_abstraction.py:190-240) with
 * correct = (probability >= 0.5) == outcome (market.py:298-301), bit for bit: a source's updates
 * are applied as one chain in the reference's loop order (market ascending, then position).
 *
 * bce_settle_compile: the caller lists the n_part signals of markets with outcome >= 0 in CSR
 * order, sorts them by sid (clamped to [0, n_sources)) with a STABLE sort -> key (sorted sids)
 * and perm (signal index of each sorted position), and gives market[n_signals] (the market of
 * every signal).  The kernel packs one correctness bit per sorted position into
 * bits[ceil(n_part / 64)] (bit j % 64 of word j / 64; NaN >= 0.5 is false, a probability outside
 * [0, 1] is not screened) and ADDS every source's set bits into correct[n_sources] (zero it
 * first).  A raw sid outside [0, n_sources), or a perm / market entry outside the batch, raises
 * the device fault word (bce_fault_check).
 *
 * bce_settle_apply: in place on rel / conf / t_us / present (nullable: every row exists) of one
 * scope.  start[n_sources + 1] = the bit offset of every source's chain, order[n_touched] = the
 * sources with a chain, longest first.  Every such source starts from its row, or from
 * (default_rel, default_conf) where present is 0 (reliability.py:133-140), takes one update per
 * bit (reliability.py:163-173), and gets t_us = now_us, present = 1; other rows are not
 * written.  The first n_long sources of order are cut into chunks of chunk_bits (>= 64) bits,
 * chunk_start[n_long + 1] = the running chunk count, n_chunks = its last entry; they run one
 * worker per chunk (a run of 11 equal bits pins the reliability to exactly 1.0 or 0.0, so a
 * worker can start behind one) from snap[2 * n_long] (16-byte aligned scratch).  n_long = 0
 * walks every chain by one lane. */
int bce_settle_compile(const int64_t* perm, int64_t n_part, const int32_t* key, const int32_t* sid,
                       const double* prob, const int32_t* market, int64_t n_signals, const int8_t* outcome,
                       int64_t n_markets, int32_t n_sources, uint64_t* bits, int64_t* correct, void* stream);
int bce_settle_apply(const uint64_t* bits, int64_t n_bits, const int64_t* start, const int32_t* order,
                     int64_t n_touched, int64_t n_long, const int64_t* chunk_start, int64_t n_chunks,
                     int64_t chunk_bits, int32_t n_sources, double* rel, double* conf, int64_t* t_us,
                     uint8_t* present, int64_t now_us, double default_rel, double default_conf, double* snap,
                     void* stream);

/* ---- walk-forward consensus: every market reads the table as of its turn ---------------------
 * A chronological batch run as the reference runs online: market m reads
 * get_reliability(s, scope, apply_decay=True) with the clock at market_time_us[m]
 * (reliability.py:104-140), after the resolved markets before it were settled with
 * update_reliability, each stamping updated_at with its own time (reliability.py:142-233).  The
 * state an entry -- a unique (market, source) pair, in (market, ascending sid) order -- reads is
 * the state of its source's settlement chain after the qpos bits of earlier markets.
 *
 * bce_settle_trace: the plan of bce_settle_apply (bits .. chunk_bits; the same workers) plus the
 * queries regrouped by source: qstart[n_sources + 1], qpos[n_entries] (0 <= qpos <= chain length,
 * ascending inside a source) and qentry[n_entries] (the entry a query answers).  Every query with
 * qpos > 0 gets {rel, conf} after qpos updates from the source's row (or the cold defaults), raw,
 * as one 16-byte store into trace[2 * qentry]; each exactly once, by the worker that applied bit
 * qpos - 1.  Queries with qpos == 0 are not written (bce_walk_read serves them from the row) and
 * the table is only read.  A qstart that is no range, a qpos that is not ascending or lies
 * outside the chain, a qentry outside [0, n_entries) raise the fault word and that query is not
 * answered.  The result does not depend on n_long / chunk_bits.
 *
 * bce_walk_read: per entry, the traced state stamped with market_time_us[qlast] where qlast >= 0
 * (the market of chain bit qpos - 1), else the row of usid (present nullable: every row exists)
 * or the cold defaults; a state that exists is decayed to market_time_us[emarket] (decay.py:90-145;
 * equal or earlier times: no decay).  Writes the consensus table over the entry index: relconf
 * [2 * n_entries] (16-byte aligned; may be `trace` itself), present_bits[ceil(n_entries / 32)]
 * (all set, or with mark_cold only where a row existed) and exists[n_entries] (nullable).  A
 * usid outside [0, n_sources) is clamped, an emarket or qlast outside the batch read as 0 / -1,
 * and the fault word is raised; sid_clamped != 0 (the caller clamped a sid while building the
 * entries) raises it as a raw sid does elsewhere. */
int bce_settle_trace(const uint64_t* bits, int64_t n_bits, const int64_t* start, const int32_t* order,
                     int64_t n_touched, int64_t n_long, const int64_t* chunk_start, int64_t n_chunks,
                     int64_t chunk_bits, int32_t n_sources, const double* rel, const double* conf,
                     const uint8_t* present, double default_rel, double default_conf, const int64_t* qstart,
                     const int64_t* qpos, const int32_t* qentry, int64_t n_entries, double* trace,
                     void* stream);
int bce_walk_read(int64_t n_entries, const int32_t* usid, const int32_t* emarket, const int32_t* qlast,
                  const double* trace, const int64_t* market_time_us, int64_t n_markets, const double* rel,
                  const double* conf, const int64_t* t_us, const uint8_t* present, int32_t n_sources,
                  double half_life_days, double min_rel, double default_rel, double default_conf,
                  int mark_cold, int sid_clamped, double* relconf, uint32_t* present_bits, uint8_t* exists,
                  void* stream);

/* ---- the settlement trace under a grid of update rules ----------------------------------------
 * update_reliability's step is max(-MAX_UPDATE_STEP, min(MAX_UPDATE_STEP, _BASE_LEARNING_RATE *
 * direction)) with direction = +-1.0 (reliability.py:163-169): for a rate >= 0 and a cap >= 0
 * exactly +-delta with delta = min(cap, rate).  bce_settle_trace_grid is bce_settle_trace (the
 * same arguments up to n_entries, the same workers and faults) for n_points rules at once, over
 * one read of the bits and the queries: rule k walks every chain with step[k] = delta_k and
 * stores its states into trace[2 * (k * n_entries + qentry)] -- n_points traces back to back,
 * each as bce_settle_trace writes it, so bce_walk_read / bce_walk_read_lag take slice k
 * unchanged.  The confidence chain does not depend on the rule.
 *
 * sync_run[k]: the number of equal bits in a row that pin the reliability to exactly 1.0 / 0.0
 * under delta_k, whatever it was before -- the caller's bound, ceil(1 / delta) + 1 for delta >=
 * 2^-20 (11 for 0.1) -- or <= 0: no run does (delta == 0, or a delta too small to bound: the
 * chain's first worker then walks all of it).  It matters on the long path only, and a value that
 * is no bound gives wrong states there, not a fault.
 *
 * final (nullable, 16-byte aligned, [n_points * n_sources * 2]): {rel, conf} after the whole
 * chain of every touched source under rule k at final[2 * (k * n_sources + s)]; the other
 * sources are not written.  A step that is negative or NaN raises the fault word and its rule is
 * not traced.  n_points outside [1, BCE_UPDATE_MAX_POINTS], a NULL step or sync_run, a trace or
 * final that is not 16-byte aligned, chunk_bits >= 2^31: BCE_EINVAL. */
#define BCE_UPDATE_MAX_POINTS 64
int bce_settle_trace_grid(const uint64_t* bits, int64_t n_bits, const int64_t* start, const int32_t* order,
                          int64_t n_touched, int64_t n_long, const int64_t* chunk_start, int64_t n_chunks,
                          int64_t chunk_bits, int32_t n_sources, const double* rel, const double* conf,
                          const uint8_t* present, double default_rel, double default_conf, const int64_t* qstart,
                          const int64_t* qpos, const int32_t* qentry, int64_t n_entries, const double* step,
                          const int64_t* sync_run, int32_t n_points, double* trace, double* final, void* stream);

/* ---- walk-forward with resolution lag: a forecast time and a resolve time per market ----------
 * The reference as an event loop, the events sorted by (time, market, kind): F_m = (forecast_time_us
 * [m], m, 0) scores market m with every source read at that time, R_m = (resolve_time_us[m], m, 1)
 * runs update_reliability for every signal of a resolved market m and stamps updated_at with the
 * resolve time.  Markets are given in forecast order (forecast times do not decrease) and
 * resolve_time_us[m] >= forecast_time_us[m]; resolve times of unresolved markets are not read.  A
 * source's chain then holds its bits in (resolve time, market, position) order, and entry (j, s)
 * reads the state after the chain bits whose market m has resolve_time_us[m] < forecast_time_us[j],
 * or the same time and m < j: a prefix of the chain.  bce_settle_compile, bce_settle_trace and
 * bce_settle_apply run unchanged on that bit order.
 *
 * bce_walk_lag_queries: one lane per query q, e = qentry[q], s = usid[e], j = emarket[e]: the
 * length of that prefix by bisection of [start[s], start[s + 1]) over bit_market[n_bits] (the
 * market of every chain bit, in chain order) into qpos[q] (relative to the chain; ascending inside
 * a source when the queries of a source ascend by market), and the market of bit qpos - 1 into
 * qlast[e] (-1: none).  slast[s], for every source, is the market of its chain's last bit (-1: no
 * bit).  With resolve == forecast these are the qpos / qlast / slast of the walk above.  A start
 * that is no range inside [0, n_bits], a bit_market or emarket outside [0, n_markets), a usid
 * outside [0, n_sources), a qentry outside [0, n_entries) raise the fault word; that query reads as
 * qpos = 0, qlast = -1 (slast: -1) and nothing is read out of bounds.  The position a bisection
 * ends on has a bit that satisfies the predicate on its left and one that does not on its right
 * whatever the array holds, so the neighbours of qpos cannot contradict it and a chain whose bits
 * are out of order is not detected: the order is the caller's (a stable sort on the host).
 *
 * bce_walk_read_lag: bce_walk_read with two time arrays: the traced state is stamped with
 * stamp_time_us[qlast] and every state decayed to now_time_us[emarket] (the resolve and the
 * forecast times).  One kernel serves both entries. */
int bce_walk_lag_queries(int64_t n_queries, const int32_t* qentry, const int32_t* usid, const int32_t* emarket,
                         int64_t n_entries, const int64_t* start, int32_t n_sources, const int32_t* bit_market,
                         int64_t n_bits, const int64_t* forecast_time_us, const int64_t* resolve_time_us,
                         int64_t n_markets, int64_t* qpos, int32_t* qlast, int64_t* slast, void* stream);
int bce_walk_read_lag(int64_t n_entries, const int32_t* usid, const int32_t* emarket, const int32_t* qlast,
                      const double* trace, const int64_t* stamp_time_us, const int64_t* now_time_us,
                      int64_t n_markets, const double* rel, const double* conf, const int64_t* t_us,
                      const uint8_t* present, int32_t n_sources, double half_life_days, double min_rel,
                      double default_rel, double default_conf, int mark_cold, int sid_clamped, double* relconf,
                      uint32_t* present_bits, uint8_t* exists, void* stream);

/* ---- live consensus history: the reliabilities re-read at every arrival -----------------------
 * The event loop above one level finer: the events are (arrival_us[i], m, 0, k) for signal k of
 * market m and (resolve_time_us[m], m, 1) for every resolved market, ascending.  At an arrival
 * compute_consensus(signals[:k + 1], table) runs with every source of the prefix fetched by
 * get_reliability(s, scope, apply_decay=True) with the clock at that arrival; a resolution runs
 * update_reliability per signal in position order and stamps the resolve time.  Arrivals do not
 * decrease inside a market and a resolved market resolves no earlier than its last arrival; the
 * markets may come in any order (the market index only breaks ties).  The chains are compiled in
 * (resolve time, market, position) order with bit_market[n_bits] the market of every chain bit, as
 * for bce_walk_lag_queries.
 *
 * bce_settle_trace_all: the plan of bce_settle_apply (bits .. chunk_bits; the same workers) and
 * the start table of bce_settle_trace.  states[2 * g] receives {rel, conf}, raw, after chain bit g
 * (the global bit index start[s] + k) as one 16-byte store; each exactly once, by the worker that
 * applied the bit.  The table is only read; the result does not depend on n_long / chunk_bits.
 * 16 bytes per chain bit.
 *
 * bce_consensus_history_live: the arguments, the three launch routes, the outputs and the fault
 * word of bce_consensus_history, with `states` (16-byte aligned; NULL where n_bits == 0) in the
 * place of relconf and present_bits not read.  Point i (CSR position) of market j sees bit b of
 * source s iff (resolve_time_us[bit_market[b]], bit_market[b]) < (arrival_us[i], j)
 * lexicographically: a prefix of the chain of length pos, found by bisection per (point, source).
 * pos > 0: the row is states[2 * (start[s] + pos - 1)] stamped with the resolve time of that bit's
 * market; else the start row rel / conf / t_us of s (present nullable: every row exists), else the
 * cold defaults, undecayed.  A row that exists is decayed to arrival_us[i] (decay.py:90-145).  A
 * start that is no range inside [0, n_bits] or a bit_market outside [0, n_markets) raises the fault
 * word and that read sees no visible bit; nothing is read out of bounds.  A NULL required pointer,
 * a negative size, n_sources <= 0 with signals, or max_len outside [0, 4096]: BCE_EINVAL before
 * anything touches the GPU. */
int bce_settle_trace_all(const uint64_t* bits, int64_t n_bits, const int64_t* start, const int32_t* order,
                         int64_t n_touched, int64_t n_long, const int64_t* chunk_start, int64_t n_chunks,
                         int64_t chunk_bits, int32_t n_sources, const double* rel, const double* conf,
                         const uint8_t* present, double default_rel, double default_conf, double* states,
                         void* stream);
int bce_consensus_history_live(const int64_t* offsets, int64_t n_markets, const int32_t* sid, const double* prob,
                               int64_t n_signals, const double* states, const uint32_t* present_bits,
                               int32_t n_sources, const int32_t* market_list, int64_t n_list,
                               const int64_t* bin_start_host, const int64_t* bin_start_dev, int32_t max_len,
                               double* consensus, double* confidence, double* total_weight, int32_t* n_unique,
                               const int64_t* arrival_us, const int64_t* start, const int32_t* bit_market,
                               int64_t n_bits, const int64_t* resolve_time_us, const double* rel,
                               const double* conf, const int64_t* t_us, const uint8_t* present,
                               double half_life_days, double min_rel, double default_rel, double default_conf,
                               void* stream);

/* ---- namespaced walk-forward: the market -> domain -> global fallback at every read ----------
 * The walk above with NamespacedReliabilityStore in the store's place: market m fetches every
 * source with get_reliability(s, market_id, domain_of(m), apply_decay=True)
 * (reliability_abstraction.py:119-188) at market_time_us[m], and a resolved market then runs
 * update_reliability(s, correct, domain=domain_of(m), update_global=) per signal (:190-239), which
 * writes the domain row (the global row for a market without a domain) and, with update_global,
 * the global row as well.  Two chain families are traced by bce_settle_trace, each into a buffer
 * of its own over the entry index: the (domain, source) chains (n_dentries chain ids; dentry
 * [n_entries] = the chain of every entry, -1 = its market has no domain) and the per-source global
 * chains.  Market rows (the table of bce_pair_resolve) are read only.
 *
 * bce_walk_scope_read: per entry e of market m = emarket[e] and source s = usid[e], the first of
 *   1. the market row of (m, s) where it exists and phas (poffsets NULL: no market scope);
 *   2. with f = dentry[e] >= 0: dtrace[e] stamped with market_time_us[dqlast[e]] where
 *      dqlast[e] >= 0, else the start row f of drel / dconf / dt_us where dhas[f] (dentry NULL:
 *      no domain scope);
 *   3. gtrace[e] stamped with market_time_us[gqlast[e]] where gqlast[e] >= 0, else the dense
 *      start row s of grel / gconf / gt_us where ghas[s] (grel NULL: the scope is not requested;
 *      gqlast NULL: no global chain has a bit);
 *   4. (default_rel, default_conf), undecayed.
 * A chain with a bit before the entry's market has a truthy stamp whatever its start row was;
 * dhas / ghas are "updated_at is truthy" of the start rows (the start STATE of a chain is the
 * row where it exists at all: that is bce_settle_trace's `present`).  The picked state is decayed
 * from its stamp to market_time_us[m] (equal or earlier times, BCE_NO_TIMESTAMP: no decay).
 * Outputs: relconf[2 * n_entries] (16-byte aligned; may be dtrace or gtrace itself: entry e reads
 * only element e of either, before it stores), present_bits[ceil(n_entries / 32)] (all set, or
 * with mark_cold only where scope != 3) and scope[n_entries] (0 / 1 / 2 / 3).
 * No input makes the kernel read or write outside its arrays: an emarket, dqlast or gqlast outside
 * the batch (read as market 0 / "no earlier bit"), a dentry outside [-1, n_dentries) (read as -1)
 * and market-row offsets that are no segment of [0, n_rows] (searched as empty) raise the fault
 * word; a usid outside [0, n_sources) is clamped and raises it, as does sid_clamped != 0.
 *
 * bce_walk_scope_read_lag: bce_walk_scope_read with two time arrays in market_time_us's place, for
 * a batch with resolution lag: dtrace[e] / gtrace[e] are stamped with stamp_time_us[dqlast[e]] /
 * stamp_time_us[gqlast[e]] (the RESOLVE time of the market of the last visible bit) and the picked
 * state is decayed to now_time_us[m] (the FORECAST time of the entry's market).  dqlast / gqlast
 * are then the qlast of bce_walk_lag_queries, launched once per chain family: the global family
 * with usid as the chain of an entry over n_sources chains, the domain family with dentry as the
 * chain of an entry over n_dentries chains and a qentry that lists only the entries with
 * dentry >= 0 (qlast pre-filled with -1).  One kernel serves both entries: bce_walk_scope_read
 * passes its one array twice.  Same checks, same fault rules, both arrays non-NULL. */
int bce_walk_scope_read_lag(int64_t n_entries, const int32_t* usid, const int32_t* emarket,
                            const int64_t* stamp_time_us, const int64_t* now_time_us, int64_t n_markets,
                            int32_t n_sources, const int64_t* poffsets, const int32_t* psid, const double* prel,
                            const double* pconf, const int64_t* pt_us, const uint8_t* phas, int64_t n_rows,
                            const int32_t* dentry, const int32_t* dqlast, const double* dtrace, const double* drel,
                            const double* dconf, const int64_t* dt_us, const uint8_t* dhas, int64_t n_dentries,
                            const int32_t* gqlast, const double* gtrace, const double* grel, const double* gconf,
                            const int64_t* gt_us, const uint8_t* ghas, double half_life_days, double min_rel,
                            double default_rel, double default_conf, int mark_cold, int sid_clamped,
                            double* relconf, uint32_t* present_bits, uint8_t* scope, void* stream);
int bce_walk_scope_read(int64_t n_entries, const int32_t* usid, const int32_t* emarket,
                        const int64_t* market_time_us, int64_t n_markets, int32_t n_sources,
                        const int64_t* poffsets, const int32_t* psid, const double* prel, const double* pconf,
                        const int64_t* pt_us, const uint8_t* phas, int64_t n_rows, const int32_t* dentry,
                        const int32_t* dqlast, const double* dtrace, const double* drel, const double* dconf,
                        const int64_t* dt_us, const uint8_t* dhas, int64_t n_dentries, const int32_t* gqlast,
                        const double* gtrace, const double* grel, const double* gconf, const int64_t* gt_us,
                        const uint8_t* ghas, double half_life_days, double min_rel, double default_rel,
                        double default_conf, int mark_cold, int sid_clamped, double* relconf,
                        uint32_t* present_bits, uint8_t* scope, void* stream);

/* ---- market-scope rows: the (source, market) rows of the store, looked up per pair ----------
 * Replaces, for every unique (market, source) pair of a batch, one call of
 *   BCE_PAIR_STORE       SQLiteReliabilityStore.get_reliability(sid, market_id, apply_decay)
 *                        (reliability.py:104-140) -- what MarketStore.compute_all_consensus reads
 *                        per signal (market.py:200-221);
 *   BCE_PAIR_NAMESPACED  NamespacedReliabilityStore.get_reliability(sid, market_id, domain,
 *                        apply_decay) (reliability_abstraction.py:137-188);
 *   BCE_PAIR_RAW         the undecayed row compute_update starts from (reliability.py:161), as
 *                        update_reliability(sid, correct, market_id=m) reads it
 *                        (reliability_abstraction.py:211-229).
 * The table is CSR by market over the batch's market index: poffsets[n_markets + 1], psid[n_rows]
 * (source ranks, strictly ascending inside a market), prel / pconf / pt_us (BCE_NO_TIMESTAMP =
 * falsy or unparseable updated_at) / phas (updated_at is truthy).  The queries have the same
 * layout: qoffsets[n_markets + 1], qsid[n_queries] ascending and unique inside a market (the
 * uoffsets / usid of bce_reestimate_csr_compile); emarket[n_queries] (nullable) = the market of
 * every entry, else it is searched in qoffsets.  Per entry e the kernel writes lb[e] = the lower
 * bound of qsid[e] in its market's rows (a global row index in [poffsets[m], poffsets[m + 1]]) and
 * matched[e] = that row holds the same sid; then
 *   STORE: a row that exists supplies (rel, conf) whatever its has, rel decayed at now_us when
 *     apply_decay and t_us != BCE_NO_TIMESTAMP; no row = (default_rel, default_conf).  scope[e] =
 *     0 for a row, 3 for the cold start;
 *   NAMESPACED: the pair's row where has, else the dense domain row drel.. [n_sources] where has,
 *     else the dense global row grel.., else the cold start; each decayed by its own t_us; a NULL
 *     drel / grel skips the scope (a falsy domain, :150).  scope[e] = 0 / 1 / 2 / 3;
 *   both write relconf[2 * n_queries] (the packed consensus table over the ENTRY index, 16-byte
 *     aligned) and present_bits[ceil(n_queries / 32)] (every entry, or with mark_cold only the
 *     entries that resolved to a stored row);
 *   RAW: out_rel / out_conf / out_t_us / out_present [n_queries] = the row, or the defaults,
 *     BCE_NO_TIMESTAMP and 0: the table layout of bce_settle_apply over the entry index.
 * Every output is nullable.  A qsid outside [0, n_sources) is clamped and raises the device fault
 * word; so do offsets that decrease or leave [0, n_queries] / [0, n_rows] (such a market's rows
 * are searched as an empty segment) (bce_fault_check). */
enum bce_pair_mode {
    BCE_PAIR_STORE = 0,
    BCE_PAIR_NAMESPACED = 1,
    BCE_PAIR_RAW = 2
};
int bce_pair_resolve(int32_t mode, const int64_t* qoffsets, int64_t n_markets, const int32_t* qsid,
                     const int32_t* emarket, int64_t n_queries, const int64_t* poffsets, const int32_t* psid,
                     const double* prel, const double* pconf, const int64_t* pt_us, const uint8_t* phas,
                     int64_t n_rows, int32_t n_sources, const double* drel, const double* dconf,
                     const int64_t* dt_us, const uint8_t* dhas, const double* grel, const double* gconf,
                     const int64_t* gt_us, const uint8_t* ghas, int apply_decay, int64_t now_us,
                     double half_life_days, double min_rel, double default_rel, double default_conf,
                     int mark_cold, int64_t* lb, uint8_t* matched, double* relconf, uint32_t* present_bits,
                     uint8_t* scope, double* out_rel, double* out_conf, int64_t* out_t_us, uint8_t* out_present,
                     void* stream);

/* ---- domain scope per market: the namespaced lookup of a batch that spans many domains ------
 * Replaces, for every unique (market, source) pair of a batch, one call of
 *   NamespacedReliabilityStore.get_reliability(sid, market_id=m, domain=domain_of(m), apply_decay)
 * (reliability_abstraction.py:119-188) where the domain differs from market to market;
 * bce_pair_resolve's BCE_PAIR_NAMESPACED takes one dense domain for the whole call.
 * Queries and the market table are those of bce_pair_resolve.  The domain rows are sparse and have
 * the market table's layout with the domain index in the market's place: doffsets[n_domains + 1],
 * dsid[n_drows] (source ranks, strictly ascending inside a domain), drel / dconf / dt_us / dhas.
 * market_domain[n_markets] is the domain index of every market, -1 = the market has no domain (a
 * falsy domain, :150).  Per entry e of market m, in order:
 *   1. the market row (binary search of qsid[e] in the market's segment) where it exists and phas;
 *   2. else, if d = market_domain[m] >= 0, the row of the sid in domain d's segment where it
 *      exists and dhas;
 *   3. else the dense global row grel.. [n_sources] where ghas (NULL grel skips the scope);
 *   4. else (default_rel, default_conf).
 * The chosen row is decayed by its own t_us when apply_decay.  Outputs, all nullable: lb / matched
 * (the market row, as bce_pair_resolve; 0 / 0 without a market table), dlb[e] = the lower bound of
 * the sid in the domain's segment (a global row index in [doffsets[d], doffsets[d + 1]]; 0 without
 * a domain) and dmatched[e], both written whether or not step 2 was reached; relconf, present_bits
 * (mark_cold), scope (0 / 1 / 2 / 3) as bce_pair_resolve.  poffsets == NULL (with n_rows == 0)
 * means no market scope: get_reliability(sid, market_id=None, domain=d).
 * No input makes the kernel read outside its arrays: a qsid outside [0, n_sources) is clamped and
 * raises the device fault word; so do query / market / domain offsets that decrease or leave their
 * array (such a segment is searched as empty) and a market_domain entry outside [-1, n_domains)
 * (the market is treated as having no domain) (bce_fault_check). */
int bce_scope_resolve(const int64_t* qoffsets, int64_t n_markets, const int32_t* qsid, const int32_t* emarket,
                      int64_t n_queries, const int64_t* poffsets, const int32_t* psid, const double* prel,
                      const double* pconf, const int64_t* pt_us, const uint8_t* phas, int64_t n_rows,
                      const int32_t* market_domain, const int64_t* doffsets, int64_t n_domains,
                      const int32_t* dsid, const double* drel, const double* dconf, const int64_t* dt_us,
                      const uint8_t* dhas, int64_t n_drows, int32_t n_sources, const double* grel,
                      const double* gconf, const int64_t* gt_us, const uint8_t* ghas, int apply_decay,
                      int64_t now_us, double half_life_days, double min_rel, double default_rel,
                      double default_conf, int mark_cold, int64_t* lb, uint8_t* matched, int64_t* dlb,
                      uint8_t* dmatched, double* relconf, uint32_t* present_bits, uint8_t* scope, void* stream);

/* ---- market-id glob patterns: MarketId.matches for every (pattern, market) pair ------
 *
 * Replaces, for a batch: MarketId.matches (market.py:74-82) under MarketStore.list_markets(
 * pattern=...) (:184-198), one fnmatch call per pair, and the member loop of
 * CrossMarketAggregator.aggregate_consensus (:352-357).  Names are the ids in list_markets order,
 * UTF-8 ('surrogatepass': a lone surrogate is its 3-byte sequence): name m is
 * name_bytes[name_off[m] .. name_off[m+1]).  Patterns are compiled on the host
 * (batch.GlobSet.compile, CPython 3.10's fnmatch.translate restated) into 32-bit ops, pattern p
 * = prog[prog_off[p] .. prog_off[p+1]), kind in bits 31..29:
 *   0 literal   bits 20..0 = the code point
 *   1 any one code point ('?')
 *   2 star      any run of code points, newline included (a run of '*' is one op)
 *   3 class     bits 27..0 = class index c, bit 28 = negate; class c is the inclusive code-point
 *               ranges (cls_rng[2r], cls_rng[2r+1]) for r in cls_off[c] .. cls_off[c+1]; a class
 *               without ranges never matches (negated: always)
 * A pattern matches a name exactly when fnmatch.fnmatchcase(name, pattern) is true (csrc/
 * glob_match.hpp: the iterative matcher, one saved position per star, decoding forward).  The
 * compiler declines a pattern of more than BCE_GLOB_MAX_OPS ops or with a class of more than
 * BCE_GLOB_MAX_RANGES ranges; the caller evaluates a declined pattern with fnmatch on the host and
 * uploads its row (the kernels themselves have no such limit).
 *
 * bce_glob_match: bits[P][ceil(M / 64)]: bit m % 64 of word m / 64 of row p is set iff pattern p
 *   matches name m; bits at positions >= M are zero; every word is written exactly once.  Names of
 *   at most 64 bytes are matched from LDS, longer ones from global memory.  Names that are not
 *   UTF-8 give unspecified bits.
 * bce_glob_match_host: the same matcher compiled for the CPU over HOST arrays, no GPU (the
 *   tradition of bce_debug_py_round); malformed offsets or programs return BCE_EINVAL.
 * bce_glob_count: cnt[r] = the number of set bits of row rows[r] (a row may be listed many times).
 * bce_glob_fill: members[slot_off[r] .. slot_off[r+1]) = the set bit positions of row rows[r],
 *   ascending; slot_off = the exclusive cumulative sum of cnt, n_members = slot_off[R].  A group is
 *   a run of consecutive slots, so bce_aggregate_groups' group_offsets is slot_off sampled at the
 *   group boundaries: members per pattern in list order, inside a pattern in store order,
 *   duplicates kept (:352-357).
 * On the device, offsets that decrease or leave their array, an op kind or class index outside its
 * table, a row outside [0, P) and a slot that does not hold its row's count raise the device fault
 * word (bce_fault_check); the affected pair counts as no match, and nothing is read or written
 * outside the arrays. */
#define BCE_GLOB_MAX_OPS 256   /* ops of a compiled pattern */
#define BCE_GLOB_MAX_RANGES 64 /* ranges of one bracket expression */
int bce_glob_match(const uint8_t* name_bytes, int64_t n_bytes, const int64_t* name_off, int64_t M,
                   const uint32_t* prog, int64_t n_ops, const int64_t* prog_off, int64_t P,
                   const uint32_t* cls_rng, int64_t n_rng, const int32_t* cls_off, int64_t n_cls,
                   uint64_t* bits, void* stream);
int bce_glob_match_host(const uint8_t* name_bytes, int64_t n_bytes, const int64_t* name_off, int64_t M,
                        const uint32_t* prog, int64_t n_ops, const int64_t* prog_off, int64_t P,
                        const uint32_t* cls_rng, int64_t n_rng, const int32_t* cls_off, int64_t n_cls,
                        uint64_t* bits);
int bce_glob_count(const uint64_t* bits, int64_t M, int64_t P, const int64_t* rows, int64_t R, int64_t* cnt,
                   void* stream);
int bce_glob_fill(const uint64_t* bits, int64_t M, int64_t P, const int64_t* rows, int64_t R,
                  const int64_t* slot_off, int64_t n_members, int64_t* members, void* stream);

/* ---- scoring a back-test: Brier score, log loss, hits and calibration per group of items -------
 * The yardstick behind the walk-forward entry points: how good were the forecasts of a history
 * whose markets have resolved?  A group is a CSR list of items, group g = items
 * [group_offsets[g], group_offsets[g + 1]) (the layout of bce_aggregate_groups / bce_glob_fill).
 * Item i reads its forecast v = value[pidx[i]] (n_values entries) and its market m = oidx[i]
 * (oidx NULL: m = pidx[i]) with o = outcome[m] (int8: -1 unresolved, 0, 1), valid[m] (u8,
 * nullable: the market's consensus is not None) and base[m] (fp64, nullable: a second forecast of
 * the same market), all over n_markets.  Two uses:
 *   market groups  value = consensus, pidx = oidx = members (market indices; groups may overlap,
 *                  a market may appear twice) -- what bce_glob_fill emits;
 *   per source     value = prob (per signal), pidx = the signal indices stably sorted by source,
 *                  oidx = the market of each of them, one group per source, every signal counted
 *                  (summarize_sources, market.py:279-304); base = consensus.
 * Item rule, the first that applies: o < 0 -> n_unresolved; valid[m] == 0 -> n_null; not
 * 0 <= v <= 1 (NaN included), or base given and not 0 <= base[m] <= 1 -> n_bad; else n_scored.
 * Per scored item: brier += (v - o)^2 (difference, then product, then the add: no contraction);
 * n_hit += (v >= 0.5) == (o == 1) (market.py:298-301); logloss += -log(max(q, eps)) with
 * q = o ? v : 1 - v; brier_base += (base[m] - o)^2 when base is given (else 0); calibration bin
 * b = min((int)(v * n_bins), n_bins - 1): bin_n[b] += 1, bin_pos[b] += (o == 1), bin_psum[b] += v.
 * Outputs per group (all nullable except counts): counts int64[G][5] = {n_scored, n_hit,
 * n_unresolved, n_null, n_bad}, sums fp64[G][3] = {brier, logloss, brier_base}, bin_n / bin_pos
 * int64[G][n_bins], bin_psum fp64[G][n_bins].  An empty group writes zeros.
 *
 * REDUCTION SHAPE (every fp64 output depends on the arguments alone -- not on the grid, the CU
 * count, timing or the other groups of the call; no floating-point atomics):
 *   1. a group of n items is cut into ceil(n / BCE_SCORE_SEG) segments of BCE_SCORE_SEG
 *      consecutive items (the last one shorter; an empty group has one empty segment);
 *   2. inside a segment, lane l of BCE_SCORE_LANES = 256 adds the terms of the segment's items
 *      l, l + 256, l + 512, ... left to right starting from 0.0; an item that is not scored
 *      contributes the term 0.0 (x + 0.0 == x for these non-negative terms);
 *   3. the 256 lane sums p[] are folded by the halving tree: for o = 128, 64, ..., 1:
 *      p[l] = p[l] + p[l + o] for l < o; the segment's sum is p[0];
 *   4. the group's sum is 0.0 + segment 0 + segment 1 + ..., left to right.
 * bin_psum[b] is the same shape over the masked terms (bin == b ? v : 0.0).  One workgroup runs
 * one segment, so a group of millions of items spreads over the device.
 *
 * seg_start int64[G + 1]: seg_start[g + 1] - seg_start[g] = max(1, ceil(n_g / BCE_SCORE_SEG)),
 * seg_start[0] = 0, n_segments = seg_start[G] (the caller's cumulative sum; batch.ScorePlan);
 * seg_group int64[n_segments]: the group of every segment (seg_start[g] <= s < seg_start[g + 1]).
 * scratch: device buffer of bce_score_scratch_bytes(n_segments, n_bins) bytes, 8-byte aligned
 * (one row of partial results per segment).  Nothing synchronises.
 * Bad arguments (a negative size, n_bins outside [1, BCE_SCORE_MAX_BINS], eps < 0 or NaN, a NULL
 * required pointer) return BCE_EINVAL before anything touches the GPU.  On the device, group
 * offsets that decrease or leave [0, n_items] (the group reads as empty), a segment table that
 * does not hold every group's own segment count (the group's outputs are zeros), a seg_group
 * entry that is not the segment's group (the segment scores nothing) and a pidx /
 * oidx outside its array (the item counts as n_bad) raise the device fault word
 * (bce_fault_check); nothing is read or written outside the arrays. */
#define BCE_SCORE_MAX_BINS 32
#define BCE_SCORE_SEG 2048  /* items of a segment */
#define BCE_SCORE_LANES 256 /* lane partials of a segment */
int64_t bce_score_scratch_bytes(int64_t n_segments, int32_t n_bins);
int bce_score_groups(const int64_t* group_offsets, int64_t n_groups, const int64_t* seg_start,
                     const int64_t* seg_group, int64_t n_segments, const int64_t* pidx, const int64_t* oidx, int64_t n_items,
                     const double* value, int64_t n_values, const int8_t* outcome, const uint8_t* valid,
                     const double* base, int64_t n_markets, int32_t n_bins, double eps, void* scratch,
                     int64_t scratch_bytes, int64_t* counts, double* sums, int64_t* bin_n,
                     int64_t* bin_pos, double* bin_psum, void* stream);

/* ---- bootstrap of the back-test scores: intervals and paired comparisons -----------------------
 * Is 0.2013 against 0.2017 a difference or noise?  A paired Poisson bootstrap over markets: the
 * sums of bce_score_groups under n_rep resamples of the history, for n_sets forecast sets (the
 * grid points of a sweep) that all see the SAME resample, so the per-replicate difference of two
 * sets is a paired difference.  No index gather: replicate r gives the unit u the integer weight
 *   mix(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *            z ^= z >> 31                                       (uint64, wrapping: splitmix64)
 *   GOLD   = 0x9E3779B97F4A7C15
 *   key(r) = mix(seed + (uint64)r * GOLD)
 *   h(r,u) = mix(key(r) ^ mix((uint64)u + GOLD))
 *   w(r,u) = 1                                 for r == 0 (the sample itself)
 *          = #{k in 0..20 : h(r,u) >= T[k]}    for r >= 1
 *   T[k]   = min(floor(2^64 * sum_{j<=k} e^-1 / j!), 2^64 - 1)   (csrc/boot_weights.hpp: 21
 *            constants, T[0] = 0x5e2d58d8b3bcdf1a ... T[20] = 0xffffffffffffffff)
 * so w is Poisson(1) in 0..21 and no floating point enters the sampler.  seed is a uint64 passed
 * as the int64 of the same bit pattern.  u is the resampling unit of the item's market m =
 * oidx[i]: unit[m] (int64[n_markets], any value, hashed as its bit pattern), or m itself when
 * unit is NULL.  unit = m / block is a block bootstrap, any id array a cluster bootstrap; with a
 * per-source plan all signals of a market share its weight.
 *
 * bce_boot_weights_host: w[R][U] = w(replicates[i], units[u]) over HOST arrays, no GPU; a negative
 *   replicate returns BCE_EINVAL.
 * bce_score_bootstrap: groups, segment table, items and markets as bce_score_groups.  Set k reads
 *   value[k * value_stride + pidx[i]] and valid[k * valid_stride + m] (valid nullable;
 *   valid_stride 0: one mask for all sets); outcome, base and unit are shared.  Classes and
 *   per-item terms are exactly those of bce_score_groups, per set (csrc/score_item.hpp: one copy);
 *   only scored items contribute: W += w, W_hit += w where the item is a hit, and each sum adds
 *   (double)w * term, the product and then the add (no contraction).  Replicate rep0 + j is row j:
 *   counts int64[n_rep][G][n_sets][2] = {W, W_hit}, sums fp64[n_rep][G][n_sets][3] = {brier,
 *   logloss, brier_base}.  An infinite term (eps = 0) under w = 0 gives NaN, as the product does.
 *
 * REDUCTION SHAPE (every output depends on the arguments alone -- not on the grid, the tiling,
 * rep0, n_sets, n_rep or the other groups of the call; no floating-point atomics):
 *   1. a group is cut into segments of BCE_SCORE_SEG consecutive items as in bce_score_groups;
 *   2. inside a segment, the terms w * term of its items are added left to right from 0.0 (an
 *      item that is not scored contributes 0.0);
 *   3. the group's sum is 0.0 + segment 0 + segment 1 + ..., left to right.
 * Integers are plain sums.  (Row 0 therefore holds the same counts as bce_score_groups, and sums
 * that differ from its sums by the summation order only.)
 *
 * scratch: device buffer of bce_boot_scratch_bytes(n_segments, n_rep, n_sets) bytes, 8-byte
 * aligned (one row per segment, replicate and set); the function returns 0 for arguments out of
 * range.  The kernel stages BCE_BOOT_TILE items of a segment at a time.  Nothing synchronises.
 * Bad arguments (a negative size or stride, n_sets outside [1, BCE_BOOT_MAX_SETS], rep0 < 0,
 * eps < 0 or NaN, a NULL required pointer, a short or misaligned scratch) return BCE_EINVAL before
 * anything touches the GPU.  On the device, broken offsets, segment tables and indices behave as
 * in bce_score_groups: the item or group contributes nothing and the device fault word is raised
 * (bce_fault_check); nothing is read or written outside the arrays. */
#define BCE_BOOT_MAX_SETS 8
#define BCE_BOOT_TILE 256 /* items staged at a time */
int bce_boot_weights_host(int64_t seed, const int64_t* replicates, int64_t R, const int64_t* units, int64_t U,
                          int32_t* w);
int64_t bce_boot_scratch_bytes(int64_t n_segments, int64_t n_rep, int32_t n_sets);
int bce_score_bootstrap(const int64_t* group_offsets, int64_t n_groups, const int64_t* seg_start,
                        const int64_t* seg_group, int64_t n_segments, const int64_t* pidx, const int64_t* oidx,
                        int64_t n_items, const double* value, int64_t n_values, int64_t value_stride,
                        int32_t n_sets, const int8_t* outcome, const uint8_t* valid, int64_t valid_stride,
                        const double* base, const int64_t* unit, int64_t n_markets, double eps, int64_t seed,
                        int64_t rep0, int64_t n_rep, void* scratch, int64_t scratch_bytes, int64_t* counts,
                        double* sums, void* stream);

/* ---- JSONL front end (host C++, no GPU): SURVEY §8 f2 -----------------------------------
 *
 * Replaces, for a batch: cli._cmd_consensus_legacy / _cmd_consensus (cli.py:25-52,163-174)
 * per payload = json.load + core.validate_input_payload (core.py:24-60) + the result's
 * json.dumps(indent=2).  bce_jsonl_parse splits `text` (UTF-8; lone surrogates as 3-byte
 * sequences) on '\n', parses each non-blank line as CPython's json.loads would and runs
 * check_structure (core.py:34-58) with the reference's messages; lines it cannot restate
 * exactly get kind 2 (the caller's Python path handles them).  sourceIds of every checked
 * signal are interned over the batch in code-point order.  bce_jsonl_counts: [lines, checked
 * probabilities, names, name bytes].  bce_jsonl_arrays: per line kind (0 structure ok, 1 header
 * error, 2 hand over), first type-error index (-1), len(signals), byte span (2 x int64); the
 * CSR voff [L+1] of the checked probabilities (those before a line's first type error), their
 * values and sourceId ranks; the sorted names (bytes + [N+1] offsets).  NULL outputs skipped.
 * bce_jsonl_render: after the caller's range check (err_idx per line, bce_validate_csr) and
 * consensus launch over the computed lines (res_of: line -> row or -1; res_off: row -> CSR
 * start of its per-unique outputs; usid / nweight as bce_consensus_* writes them), every
 * line's text: "Validation error: ..." or json.dumps(result, indent=2) byte for byte (wtext:
 * per name, the JSON text of its weight object).  Call with out == NULL to render and size,
 * then with buffers to copy (text_off [L+1], ok [L]).  `threads` host threads. */
int bce_jsonl_parse(const char* text, int64_t len, int32_t threads, void** handle);
int bce_jsonl_counts(void* handle, int64_t* counts);
int bce_jsonl_arrays(void* handle, int32_t* kind, int32_t* type_err, int32_t* n_signals, int64_t* span,
                     int64_t* voff, double* prob, int32_t* sid, char* names, int64_t* name_off);
int bce_jsonl_render(void* handle, const int32_t* err_idx, const int64_t* res_of, const double* consensus,
                     const double* confidence, const double* total_weight, const int32_t* n_unique,
                     const int64_t* res_off, const int32_t* usid, const double* nweight, const char* wtext,
                     const int64_t* wtext_off, int32_t dry_run, int32_t threads, char* out, int64_t* text_off,
                     uint8_t* ok, int64_t* n_bytes);
void bce_jsonl_free(void* handle);
/* Test hook: float.__repr__ of x (the renderer's number format) into buf; returns its length. */
int32_t bce_debug_float_repr(double x, char* buf, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* BCE_H */
