"""CPU checks of the leave-one-source-out consensus: the restatement
(tests/leave_one_out_ref.py) against the fixture recorded from the reference and against the
oracle on the expanded batch; the item lists of ``score_leave_one_out`` and
``LeaveOneOutResult`` on CPU tensors; the argument checks of bce_consensus_leave_one_out, which
need no GPU."""
import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from leave_one_out_ref import FIELDS, expand, load_fixture, loo_ref
from oracle import oracle as orc
from score_ref import score_ref


def _random_batch(seed, lens, S, n_zero):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    prob[rng.random(n) < 0.05] = 1.25
    rel, conf = rng.uniform(0.1, 1.0, S), rng.random(S)
    rel[:n_zero] = 0.0
    return off, sid, prob, rel, conf, np.ones(S, np.uint8)


def test_restatement_equals_the_reference_fixture(golden_dir):
    g, off, sid, prob, rel, conf, _ = load_fixture(golden_dir)
    got, full = loo_ref(off, sid, prob, rel, conf)
    names = g["names"]
    pairs = nulls = 0
    for m, mk in enumerate(g["markets"]):
        a, b = int(off[m]), int(off[m + 1])
        assert [r["sourceId"] for r in mk["leave_out"]] == sorted({name for name, _ in mk["signals"]})
        for r in mk["leave_out"]:
            at = [p for p in range(a, b) if sid[p] == names.index(r["sourceId"])]
            assert at
            pairs += 1
            nulls += r["consensus"] is None
            for p in at:  # every signal of the source holds the source's values
                assert (r["consensus"] is None) == (got["total_weight"][p] == 0.0), (m, p)
                want = "0.0" if r["consensus"] is None else r["consensus"]
                assert repr(float(got["consensus"][p])) == want, (m, p)
                assert repr(float(got["confidence"][p])) == r["confidence"], (m, p)
                assert repr(float(got["total_weight"][p])) == r["totalWeight"], (m, p)
                assert int(got["n_unique"][p]) == r["sourceCount"], (m, p)
        f = mk["full"]
        assert repr(float(full["consensus"][m])) == ("0.0" if f["consensus"] is None else f["consensus"]), m
        assert (repr(float(full["confidence"][m])), repr(float(full["total_weight"][m])),
                int(full["n_unique"][m])) == (f["confidence"], f["totalWeight"], f["sourceCount"]), m
    # the nulls: the only source of three markets, and either source of the zero-weight pair
    assert len(g["markets"]) == 12 and len(sid) == 112 and pairs == 51 and nulls == 5


def test_restatement_equals_the_oracle_on_the_expanded_batch(golden_dir):
    batches = [load_fixture(golden_dir)[1:],
               _random_batch(7, [0, 1, 2, 7, 31, 32, 33, 63, 64, 65, 100], 9, 2),
               _random_batch(8, [5, 40, 3, 0, 12], 40, 30)]  # mostly zero-weight sources: null leave-outs
    nulls = 0
    for off, sid, prob, rel, conf, present in batches:
        got, full = loo_ref(off, sid, prob, rel, conf)
        exp = orc.consensus_csr(*expand(off, sid, prob), rel, conf, present)
        own = orc.consensus_csr(off, sid, prob, rel, conf, present)
        for k in FIELDS:
            assert np.array_equal(got[k], exp[k]), k
            assert np.array_equal(full[k], own[k]), k
        nulls += int((got["total_weight"] == 0).sum())
    assert nulls >= 10


def test_expand():
    off = np.array([0, 4, 4, 6, 7], np.int64)
    off2, sid2, prob2 = expand(off, np.array([7, 8, 7, 9, 1, 1, 5], np.int32), np.arange(7.0))
    assert off2.tolist() == [0, 2, 5, 7, 10, 10, 10, 10]
    assert sid2.tolist() == [8, 9, 7, 7, 9, 8, 9, 7, 8, 7]
    assert prob2.tolist() == [1, 3, 0, 2, 3, 1, 3, 0, 1, 2]
    none = expand(np.array([0, 0]), np.zeros(0, np.int32), np.zeros(0))
    assert none[0].tolist() == [0] and none[1].size == 0


# ---------------------------------------------------------------- score_leave_one_out's items
def test_item_selection_per_pair_and_per_signal():
    off = torch.tensor([0, 5, 5, 8, 9])
    sid = torch.tensor([2, 0, 2, 2, 0, 1, 1, 2, 3], dtype=torch.int32)
    pair = batch._loo_items(off, sid, 5, "pair")
    assert pair.group_offsets.tolist() == [0, 1, 2, 4, 5, 5]
    assert pair.pidx.tolist() == [1, 5, 0, 7, 8] and pair.oidx is None and pair.n_clamped == 0
    assert pair.n_segments == 5 and pair.seg_group.tolist() == [0, 1, 2, 3, 4]
    sig = batch._loo_items(off, sid, 5, "signal")
    by = batch.ScorePlan.by_source(off, sid, 5)
    assert sig.group_offsets.tolist() == by.group_offsets.tolist() == [0, 2, 4, 8, 9, 9]
    assert sig.pidx.tolist() == by.pidx.tolist() == [1, 4, 5, 6, 0, 2, 3, 7, 8] and sig.oidx is None
    clamped = batch._loo_items(off, torch.tensor([2, 0, 2, 9, 0, 1, 1, -4, 3], dtype=torch.int32), 4, "pair")
    assert clamped.n_clamped == 2 and clamped.pidx.tolist() == [1, 7, 5, 0, 3, 8]
    assert clamped.group_offsets.tolist() == [0, 2, 3, 4, 6]
    with pytest.raises(ValueError, match="per must be"):
        batch._loo_items(off, sid, 5, "market")
    empty = batch._loo_items(torch.tensor([0, 0]), torch.zeros(0, dtype=torch.int32), 3, "pair")
    assert empty.n_items == 0 and empty.group_offsets.tolist() == [0, 0, 0, 0]


def test_items_against_the_plain_statement_and_score_ref():
    """Random batch: the per-pair items are the first signal of every (market, source), a source's
    items in market order; scored by tests/score_ref.py they count one item per pair."""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 12, 40)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n, S = int(off[-1]), 6
    sid = rng.integers(0, S, n).astype(np.int32)
    want = [[] for _ in range(S)]
    every = [[] for _ in range(S)]
    for m in range(len(lens)):
        seen = set()
        for p in range(off[m], off[m + 1]):
            every[sid[p]].append(p)
            if sid[p] not in seen:
                seen.add(sid[p])
                want[sid[p]].append(p)
    for per, lists in (("pair", want), ("signal", every)):
        plan = batch._loo_items(torch.from_numpy(off), torch.from_numpy(sid), S, per)
        assert plan.pidx.tolist() == [p for lst in lists for p in lst], per
        assert plan.group_offsets.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in lists])]).tolist()
        market = np.repeat(np.arange(len(lens)), lens)
        outcome = rng.choice(np.array([-1, 0, 1], np.int8), len(lens))
        ref = score_ref(dict(goff=plan.group_offsets.numpy(), pidx=plan.pidx.numpy(), oidx=None, value=rng.random(n),
                             outcome=outcome[market], valid=np.ones(n, np.uint8), base=rng.random(n), B=10,
                             eps=1e-15))
        assert ref["counts"][:, [0, 2]].sum(1).tolist() == [len(x) for x in lists], per


def test_result_on_cpu_tensors():
    f64 = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    full = batch.ConsensusResult(f64([0.6, 0.0, 0.0]), f64([0.3, 0.0, 0.0]), f64([2.0, 0.0, 0.0]),
                                 torch.tensor([2, 1, 0], dtype=torch.int32), None, None, None, None)
    r = batch.LeaveOneOutResult(f64([0.5, 0.0, 0.7]), f64([0.1, 0.0, 0.3]), f64([1.0, 0.0, 2.0]),
                                torch.tensor([1, 1, 0], dtype=torch.int32), full)
    off = torch.tensor([0, 2, 3, 3])
    assert r.is_null().tolist() == [False, True, False]
    inf = r.influence(off)
    assert inf.dtype == torch.float64 and inf[0].item() == 0.6 - 0.5
    assert torch.isnan(inf[1:]).all()  # a null leave-out; a null full consensus
    assert torch.equal(r.influence(off, full=full)[:1], inf[:1])
    r.full = None
    with pytest.raises(ValueError, match="full"):
        r.influence(off)
    with pytest.raises(ValueError, match="full"):
        batch.score_leave_one_out(r, off, torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int8), 1)
    a = batch.LeaveOneOutResult.alloc(5, "cpu", n_markets=2)
    assert a.consensus.shape == (5,) and a.n_unique.dtype == torch.int32 and a.full.consensus.shape == (2,)
    assert batch.LeaveOneOutResult.alloc(0, "cpu").consensus.shape == (0,)
    with pytest.raises(ValueError, match="max_len"):
        batch.leave_one_out(torch.tensor([0, 1]), torch.zeros(1, dtype=torch.int32), torch.zeros(1), None,
                            max_len=4097)
    with pytest.raises(ValueError, match="market 1 has 4097 signals"):
        batch.leave_one_out(None, None, None, None, offsets_host=np.array([0, 3, 4100, 4101]))


# ------------------------------------------------------------------------------ the C entry
def _call(**over):
    a = dict(offsets=1, n_markets=1, sid=1, prob=1, n_signals=1, relconf=16, bits=None, n_sources=1, list=None,
             n_list=0, bins_host=None, bins_dev=None, max_len=8, cons=1, conf=1, tot=1, nu=1, fcons=None,
             fconf=None, ftot=None, fnu=None, stream=None)
    a.update(over)
    return N.load_library().bce_consensus_leave_one_out(*a.values())


def test_argument_errors_need_no_gpu():
    """Every refusal comes before anything touches the GPU (the pointers here are never read)."""
    lib = N.load_library()
    assert lib.bce_consensus_leave_one_out(None, 5, None, None, 0, None, None, 0, None, 0, None, None, 32,
                                           None, None, None, None, None, None, None, None, None) == -1
    assert b"leave_one_out" in lib.bce_last_error() and b"offsets" in lib.bce_last_error()
    for over in (dict(offsets=None), dict(sid=None), dict(prob=None), dict(relconf=None), dict(cons=None),
                 dict(conf=None), dict(tot=None), dict(nu=None), dict(n_markets=-1), dict(n_signals=-1),
                 dict(n_sources=-1), dict(n_list=-1), dict(max_len=-1), dict(max_len=4097), dict(relconf=8),
                 dict(bins_host=1), dict(bins_host=1, bins_dev=1, list=1),
                 dict(fcons=1), dict(fcons=1, fconf=1, ftot=1), dict(fconf=1, ftot=1, fnu=1), dict(fnu=1)):
        assert _call(**over) == -1, over
        assert b"leave_one_out" in lib.bce_last_error(), over
    assert b"full_" in lib.bce_last_error()
    assert _call(n_markets=0) == 0 and _call(n_signals=0, sid=None, prob=None, cons=None) == 0  # nothing to do
    assert _call(n_markets=0, fcons=1, fconf=1, ftot=1, fnu=1) == 0


def test_names_are_reachable():
    import importlib
    home = importlib.import_module("bayesian_engine.batch.leave_one_out")  # batch.leave_one_out is the function
    for name in ("LeaveOneOutResult", "leave_one_out", "score_leave_one_out", "walk_leave_one_out", "_loo_items"):
        assert getattr(batch, name) is getattr(home, name), name
    assert "bce_consensus_leave_one_out" in N.EXPORTED
    from bayesian_engine.market import CrossMarketAggregator, Market, MarketStore
    assert callable(Market.leave_one_out) and callable(MarketStore.compute_all_leave_one_out)
    assert callable(CrossMarketAggregator.source_influence)
    order = batch.__doc__.split("listed before it:")[1]
    assert order.index("history") < order.index("leave_one_out") < order.index("bootstrap")
