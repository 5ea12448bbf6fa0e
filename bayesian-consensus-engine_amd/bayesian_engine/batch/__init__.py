"""Batched entry points over millions of markets.

All array arguments are device tensors (torch, ``cuda:N``); results stay in HBM.  Each
function is one or a few launches of the HIP kernels in ``libbce_hip.so`` on the current
stream -- there is no CPU fallback (see :mod:`bayesian_engine._native`).

Layout (include/bce.h):
  markets  CSR  offsets int64[M+1], sid int32[N] (interned source ranks in Python
           ``sorted()`` order), prob fp64[N]
  sources  dense table over ranks: rel fp64[S], conf fp64[S] (cold-start defaults baked
           in), present u8[S]; optional t_us int64[S] for decay

Every name lives in one submodule and is re-exported here; a submodule imports only from those
listed before it: elementwise, tables, consensus, tiebreak, stats, reestimate_csr, settle, pairs,
walk, glob, score, history, leave_one_out, bootstrap (which imports from score only), update_sweep
(which imports from walk and score), live (which imports from settle, walk and history).
"""
from .elementwise import (DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM, DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY, decay_apply,
                          decay_view, outcome_update, pack_flags2, replay_step)
from .tables import (NS_COLD, NS_DOMAIN, NS_GLOBAL, NS_MARKET, PairTable, ReliabilityTable, ScopeTable, SourceTable,
                     intern, to_device)
from .consensus import _MODES, ConsensusResult, Plan, _alloc, consensus, validate
from .tiebreak import (_BUCKET_GAIN, _TILE_COST, TieBreakResult, TiePlan, _round_overflow_check, tiebreak,
                       tiebreak_plan)
from .stats import AggregateResult, aggregate, agreement_stats, namespace_resolve, reestimate
from .reestimate_csr import (_RC_MAX_RUN, ReestimateCsrPlan, ReestimateCsrResult, _reestimate_csr_order,
                             reestimate_csr, reestimate_csr_step, reestimate_csr_weights)
from .settle import SETTLE_CHUNK_BITS, SETTLE_LONG_MIN, SETTLE_LONG_OFF, SettlePlan, _settle_order, settle
from .pairs import (_PAIR_MODES, DomainPlan, PairConsensusResult, PairPlan, PairResolveResult, _bins_as_plan,
                    _check_queries, _cut, _dense_scope, _entry_outputs, _pair_merge, _pair_merge_index,
                    _pair_pointers, consensus_pairs, pair_resolve, scope_resolve, settle_domains, settle_pairs)
from .walk import (WALK_CHUNK_BITS, WALK_LONG_MIN, WalkPlan, WalkQueries, WalkResult, WalkScopePlan, WalkScopeResult,
                   _chain_queries, _check_lag_times, _entry_signals, _global_outcome, _lag_family, _resolve_rank,
                   _walk_buffers, _walk_queries, _walk_read, _walk_scope_launch, _walk_scope_read, _walk_scope_traces,
                   _walk_settle_trace, _walk_times, walk_forward, walk_forward_scoped, walk_scope_trace, walk_trace)
from .glob import (_GLOB_ANY, _GLOB_CLS, _GLOB_LIT, _GLOB_NEGATE, _GLOB_STAR, GLOB_MAX_OPS, GLOB_MAX_RANGES, GlobSet,
                   NameTable, _glob_bracket, _glob_compile_one, _glob_host_row, _GlobDeclined, _np_or_dummy, glob_any,
                   glob_count, glob_mask, glob_match, glob_match_host, glob_members)
from .score import (SCORE_COUNTS, SCORE_LANES, SCORE_MAX_BINS, SCORE_SEG, SCORE_SUMS, ScorePlan, ScoreResult,
                    _nan_div, _score_segments, score, score_markets, score_sources, walk_sweep,
                    walk_sweep_scoped)
from .history import (HISTORY_MAX_LEN, HistoryResult, _check_arrival_order, _history_items, _market_of_point,
                      consensus_history, history_at, score_history, walk_history)
from .leave_one_out import (LeaveOneOutResult, _loo_items, leave_one_out, score_leave_one_out, walk_leave_one_out)
from .bootstrap import (BOOT_COUNTS, BOOT_MAX_SETS, BOOT_METRICS, BOOT_TILE, BootstrapResult, boot_units, boot_weights,
                        score_bootstrap)
from .update_sweep import (UPDATE_MAX_POINTS, commit_update_point, update_steps, walk_sweep_update, walk_trace_grid)
from .live import LivePlan, _check_live_times, live_trace, walk_history_live
