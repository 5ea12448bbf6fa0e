"""CPU checks of the ``bayesian_engine.batch`` facade: every name the single-file module offered
is still reachable on the package, is the very object of its home submodule, and every submodule
imports on its own (no GPU, no library call at import)."""
import importlib
import sys

import pytest

import bayesian_engine
from bayesian_engine import batch

# The module-level names of the single-file bayesian_engine/batch.py (its ``vars()`` without
# dunders, modules and objects defined elsewhere), grouped by the submodule that now defines them.
HOMES = {
    "elementwise": """
        DECAY_HALF_LIFE_DAYS DECAY_MINIMUM DEFAULT_CONFIDENCE DEFAULT_RELIABILITY
        decay_view decay_apply outcome_update replay_step pack_flags2
    """,
    "tables": """
        intern to_device SourceTable ReliabilityTable ScopeTable NS_MARKET NS_DOMAIN NS_GLOBAL NS_COLD
        PairTable
    """,
    "consensus": """
        _MODES Plan ConsensusResult _alloc consensus validate
    """,
    "tiebreak": """
        TieBreakResult TiePlan _TILE_COST _BUCKET_GAIN tiebreak_plan tiebreak _round_overflow_check
    """,
    "stats": """
        agreement_stats namespace_resolve AggregateResult aggregate reestimate
    """,
    "reestimate_csr": """
        _RC_MAX_RUN _reestimate_csr_order ReestimateCsrPlan ReestimateCsrResult reestimate_csr_step
        reestimate_csr_weights reestimate_csr
    """,
    "settle": """
        SETTLE_LONG_MIN SETTLE_CHUNK_BITS SETTLE_LONG_OFF _settle_order SettlePlan settle
    """,
    "pairs": """
        PairPlan PairResolveResult _PAIR_MODES _check_queries _entry_outputs _dense_scope _pair_pointers _cut
        _bins_as_plan pair_resolve PairConsensusResult consensus_pairs _pair_merge_index settle_pairs
        _pair_merge scope_resolve DomainPlan settle_domains
    """,
    "walk": """
        WALK_LONG_MIN WALK_CHUNK_BITS _walk_queries _entry_signals _chain_queries WalkPlan WalkResult
        walk_trace _walk_buffers _walk_settle_trace _walk_read walk_forward WalkQueries _global_outcome
        WalkScopePlan WalkScopeResult _walk_scope_read walk_scope_trace walk_forward_scoped
    """,
    "glob": """
        GLOB_MAX_OPS GLOB_MAX_RANGES _GLOB_LIT _GLOB_ANY _GLOB_STAR _GLOB_CLS _GLOB_NEGATE _GlobDeclined
        _glob_bracket _glob_compile_one NameTable GlobSet _glob_host_row _np_or_dummy glob_match_host
        glob_match glob_count glob_members glob_any glob_mask
    """,
    "score": """
        SCORE_SEG SCORE_LANES SCORE_MAX_BINS SCORE_COUNTS SCORE_SUMS _score_segments ScorePlan _nan_div
        ScoreResult score score_markets score_sources walk_sweep
    """,
}
NAMES = [(mod, name) for mod, names in HOMES.items() for name in names.split()]


def test_the_list_is_the_single_file_surface():
    assert len(NAMES) == 120 and len({n for _, n in NAMES}) == 120
    assert sum(not n.startswith("_") for _, n in NAMES) == 83


@pytest.mark.parametrize("mod,name", NAMES, ids=[n for _, n in NAMES])
def test_name_is_reachable_and_is_its_home_object(mod, name):
    home = importlib.import_module(f"bayesian_engine.batch.{mod}")
    assert hasattr(batch, name), f"bayesian_engine.batch.{name} is gone"
    assert getattr(batch, name) is getattr(home, name), f"batch.{name} is not {mod}.{name}"


def test_table_methods_are_attached():
    t = batch.ReliabilityTable
    assert callable(t.settle) and callable(t.walk_forward) and callable(t.view)


def test_shared_checks_on_the_host():
    """The checks the builders and the walks share, called directly (CPU tensors, no library)."""
    import torch
    from bayesian_engine.batch import tables as T

    off = torch.tensor([0, 2, 3])
    sid = torch.tensor([0, 1, 0], dtype=torch.int32)
    M, Nsig, S, off64, lens = T._check_csr(off, sid, 2)
    assert (M, Nsig, S, off64.dtype, lens.tolist()) == (2, 3, 2, torch.int64, [2, 1])
    assert T._check_csr(off, sid, 2, values=False) == (2, 3, 2, None, None)
    T._check_csr(torch.tensor([0, 2, 9]), sid, 2, values=False)  # shapes alone: the values are not read
    with pytest.raises(ValueError, match="offsets must rise from 0 to len\\(sid\\)"):
        T._check_csr(torch.tensor([0, 2, 9]), sid, 2)
    big = torch.empty((1 << 31) + 1, dtype=torch.int64, device="meta")
    none = torch.empty(0, dtype=torch.int32, device="meta")
    with pytest.raises(ValueError, match="^here: 2147483648 markets$"):
        T._check_csr(big, none, 2, too_many="here: {} markets")
    with pytest.raises(ValueError, match="n_domains must be in"):
        T._check_csr(off, sid, 2, n_domains=1 << 31)
    with pytest.raises(ValueError, match="market_domain must have one entry per market \\(2\\)"):
        T._check_csr(off, sid, 2, market_domain=torch.zeros(3, dtype=torch.int32), n_domains=1)

    f64, i64, u8 = (torch.zeros(4, dtype=d) for d in (torch.float64, torch.int64, torch.uint8))
    T._check_table(f64, f64, i64, u8, 4)
    T._check_table(f64, f64, i64, None, 4)
    with pytest.raises(AssertionError, match="rel / conf must be fp64 and t_us int64"):
        T._check_table(f64.float(), f64, i64, u8, 4)
    with pytest.raises(AssertionError, match="the global table must have n_sources rows"):
        T._check_table(f64, f64, i64, u8, 5, "the global table must have n_sources rows")
    with pytest.raises(AssertionError, match="present must be u8"):
        T._check_table(f64, f64, i64, u8.bool(), 4)
    T._check_market_time(i64, 4)
    for bad in (i64[:3], i64.int(), i64.reshape(2, 2)):
        with pytest.raises(ValueError, match="market_time_us must be int64 with one entry per market \\(4\\)"):
            T._check_market_time(bad, 4)

    for E, rows, words in ((0, 1, 1), (1, 1, 1), (32, 32, 1), (33, 33, 2)):
        relconf, bits, flag = T._entry_buffers(E, "cpu")
        assert relconf.shape == (rows, 2) and relconf.dtype == torch.float64
        assert bits.shape == (words,) and bits.dtype == torch.int32 and not bits.any()
        assert flag.shape == (rows,) and flag.dtype == torch.uint8


@pytest.mark.parametrize("mod", list(HOMES))
def test_submodule_imports_on_its_own(mod):
    """The submodule as the first thing imported from the package (the package's modules are
    dropped from ``sys.modules`` for the import and put back after it)."""
    saved = {k: v for k, v in sys.modules.items() if k == "bayesian_engine.batch" or
             k.startswith("bayesian_engine.batch.")}
    try:
        for k in saved:
            del sys.modules[k]
        fresh = importlib.import_module(f"bayesian_engine.batch.{mod}")
        assert fresh is not saved[f"bayesian_engine.batch.{mod}"]
        assert all(hasattr(fresh, n) for m, n in NAMES if m == mod)
    finally:
        for k in [k for k in sys.modules if k == "bayesian_engine.batch" or k.startswith("bayesian_engine.batch.")]:
            del sys.modules[k]
        sys.modules.update(saved)
        bayesian_engine.batch = saved["bayesian_engine.batch"]
