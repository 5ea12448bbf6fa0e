"""GPU checks of the CSR re-estimation (batch.ReestimateCsrPlan / reestimate_csr*): every
round's consensus, null flags, outcomes, counts and weights equal the oracle composition of
tests/reestimate_csr_ref.py exactly (``==``; NaN-aware for the consensus)."""
import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from reestimate_csr_ref import reference_rounds

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


def _same_round(got, exp, what=""):
    """got: a history tuple of device tensors; exp: reestimate_csr_ref.Round."""
    names = ("cons", "null", "outcome", "correct", "total", "w")
    for name, g, e in zip(names, got, exp):
        g = g.cpu().numpy()
        assert g.dtype == e.dtype, (what, name, g.dtype, e.dtype)
        assert np.array_equal(g, e, equal_nan=(name == "cons")), (what, name, np.flatnonzero(g != e)[:8])


def _check(history, rounds, what=""):
    assert len(history) == len(rounds)
    for k, (got, exp) in enumerate(zip(history, rounds)):
        _same_round(got, exp, f"{what} round {k}")


def _edge_batch():
    rng = np.random.default_rng(7)
    S = 300
    lens = [0, 1, 2, 31, 32, 33, 63, 64, 65, 200, 5000] + [int(x) for x in rng.integers(1, 40, 59)]
    lens[20] = 0  # a second empty market, inside the first tile
    off = _offsets(lens)
    n = int(off[-1])
    sid = rng.integers(0, 290, n).astype(np.int32)  # sources 290..299: see below
    prob = rng.random(n)
    # market 3 (31 signals): all one source
    sid[off[3]:off[4]] = 17
    # market 4 (32 signals): source 5 three times with mixed votes (the vote is the raw signal's)
    a = int(off[4])
    sid[a:a + 32] = np.arange(100, 132)
    sid[[a + 1, a + 9, a + 30]] = 5
    prob[[a + 1, a + 9, a + 30]] = [0.9, 0.2, 0.45]
    # special values: NaN, the threshold itself, both sides out of range
    prob[int(off[6]) + 3] = np.nan
    prob[int(off[7]) + 5] = 0.5
    prob[int(off[8]) + 7] = -0.1   # market 8 is skipped
    prob[int(off[9]) + 11] = 1.5   # market 9 is skipped
    # market 5 (33 signals) holds only sources 290..295, whose initial weight is 0: null, not empty
    sid[off[5]:off[6]] = 290 + (np.arange(33) % 6)
    # source 299 is in no market; 296..298 appear with weight zero beside weighted sources
    sid[int(off[10]):int(off[10]) + 3] = [296, 297, 298]
    w = rng.uniform(0.05, 1.0, S)
    w[290:] = 0.0
    return off, sid, prob, S, w


def test_edge_batch():
    off, sid, prob, S, w = _edge_batch()
    iters = 4
    rounds = reference_rounds(off, sid, prob, S, iters, w=w)
    first = rounds[0]
    lens = np.diff(off)
    assert len(lens) == 70 and lens.max() == 5000
    assert first.null[5] == 1 and lens[5] > 0                       # null, not empty
    assert first.outcome[8] == -1 and first.outcome[9] == -1 and first.null[8] == 0   # skipped, out of range
    assert first.total[299] == 0 and first.w[299] == 0.5            # a source in no market
    assert np.isnan(first.cons[6])
    plan = batch.ReestimateCsrPlan.build(_T(off), _T(sid), _T(prob), S)
    assert plan.n_markets == 70 and plan.n_entries < len(sid)
    r = batch.reestimate_csr(plan, iters, w=_T(w), keep_history=True)
    torch.cuda.synchronize()
    _check(r.history, rounds, "edge")
    _same_round((r.consensus, r.null, r.outcome, r.correct, r.total, r.w), rounds[-1], "edge result")
    N.check_faults(_dev(), "edge batch")


@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(11)
    M, S = 3000, 500
    lens = rng.integers(1, 97, M)
    off = _offsets(lens)
    n = int(off[-1])
    p = 1.0 / np.arange(1, S + 1)
    sid = rng.choice(S, size=n, p=p / p.sum()).astype(np.int32)
    # ~10% of the signals repeat the source of the signal before them in the same market
    dup = np.flatnonzero(rng.random(n) < 0.10)
    starts = set(off[:-1].tolist())
    dup = np.array([i for i in dup if i not in starts], np.int64)
    sid[dup] = sid[dup - 1]
    prob = rng.random(n)
    known = np.where(rng.random(M) < 1 / 3, rng.integers(0, 2, M), -1).astype(np.int8)
    iters = 5
    return dict(off=off, sid=sid, prob=prob, S=S, M=M, known=known, iters=iters,
                rounds=reference_rounds(off, sid, prob, S, iters),
                rounds_known=reference_rounds(off, sid, prob, S, iters, known=known))


@pytest.mark.parametrize("with_known", [False, True])
def test_random_ragged(ragged, with_known):
    g = ragged
    plan = batch.ReestimateCsrPlan.build(_T(g["off"]), _T(g["sid"]), _T(g["prob"]), g["S"])
    known = _T(g["known"]) if with_known else None
    r = batch.reestimate_csr(plan, g["iters"], known=known, keep_history=True)
    torch.cuda.synchronize()
    _check(r.history, g["rounds_known" if with_known else "rounds"], f"ragged known={with_known}")


def test_plan_reuse(ragged):
    g = ragged
    args = (_T(g["off"]), _T(g["sid"]), _T(g["prob"]), g["S"])
    plan = batch.ReestimateCsrPlan.build(*args)
    for w0 in (0.5, 0.125):
        a = batch.reestimate_csr(plan, 3, w0=w0, keep_history=True)
        b = batch.reestimate_csr(batch.ReestimateCsrPlan.build(*args), 3, w0=w0, keep_history=True)
        torch.cuda.synchronize()
        for ha, hb in zip(a.history, b.history):
            for x, y in zip(ha, hb):
                assert torch.equal(x, y) or (x.is_floating_point() and torch.equal(x.isnan(), y.isnan())
                                             and torch.equal(x.nan_to_num(), y.nan_to_num()))
    _check(a.history, reference_rounds(g["off"], g["sid"], g["prob"], g["S"], 3, w0=0.125), "reuse")


def test_market_shards_share_the_counts(ragged):
    g = ragged
    off, sid, prob, S, M = g["off"], g["sid"], g["prob"], g["S"], g["M"]
    h = M // 2 + 7  # not a multiple of the 64-market tile
    cut = int(off[h])
    halves = [(off[:h + 1], sid[:cut], prob[:cut]), (off[h:] - cut, sid[cut:], prob[cut:])]
    plans = [batch.ReestimateCsrPlan.build(_T(o), _T(s), _T(p), S) for o, s, p in halves]
    w = torch.full((S,), 0.5, dtype=torch.float64, device=_dev())
    correct = torch.zeros(S, dtype=torch.int64, device=_dev())
    total = torch.zeros(S, dtype=torch.int64, device=_dev())
    for k, exp in enumerate(g["rounds"]):
        correct.zero_()
        total.zero_()
        parts = [batch.reestimate_csr_step(p, w, correct, total) for p in plans]
        batch.reestimate_csr_weights(correct, total, w)
        torch.cuda.synchronize()
        got = tuple(torch.cat([a[i] for a in parts]) for i in range(3)) + (correct, total, w)
        _same_round(got, exp, f"shards round {k}")


def test_bad_sid_raises_like_consensus():
    rng = np.random.default_rng(5)
    S, M = 500, 64
    off = _offsets([32] * M)  # the shape whose consensus kernel checks sids (contiguous markets of 32)
    sid = rng.integers(0, S, 32 * M).astype(np.int32)
    sid[777] = S  # clamped on the device, never dereferenced
    prob = rng.random(32 * M)
    table = batch.SourceTable.from_arrays(_T(np.full(S, 0.5)), _T(np.full(S, 0.25)), None)
    N.check_faults(_dev(), "clean slate")
    with pytest.raises(N.BCEError) as e_cons:
        batch.consensus(_T(off), _T(sid), _T(prob), table, max_len=32, check=True)
    with pytest.raises(N.BCEError) as e_plan:
        batch.ReestimateCsrPlan.build(_T(off), _T(sid), _T(prob), S)
    assert type(e_cons.value) is type(e_plan.value)
    assert "sid" in str(e_plan.value)
    N.check_faults(_dev(), "fault word is cleared")


def test_reestimate_sources_matches_helper():
    from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore

    store = MarketStore()
    rng = np.random.default_rng(3)
    names = [f"agent-{c}" for c in "abcdefg"]
    ids = [MarketId(f"test:m{m}") for m in range(6)]
    for mid in ids:
        for j in rng.integers(0, len(names), int(rng.integers(2, 7))):
            store.add_signal(mid, {"sourceId": names[j], "probability": float(np.round(rng.random(), 3))})
    store.create_market(MarketId("test:empty"))  # no signals: not part of the batch
    store.get_market(ids[1]).resolve(True)
    store.get_market(ids[4]).resolve(False)
    agg = CrossMarketAggregator(store)
    perf = agg.reestimate_sources(iters=3)
    # the same batch, interned the same way
    markets = [mk for mk in store.list_markets() if mk.signals]
    rank = batch.intern(x["sourceId"] for mk in markets for x in mk.signals)
    off = _offsets([len(mk.signals) for mk in markets])
    sid = np.array([rank[x["sourceId"]] for mk in markets for x in mk.signals], np.int32)
    prob = np.array([x["probability"] for mk in markets for x in mk.signals], np.float64)
    known = np.array([-1 if mk.outcome is None else int(mk.outcome) for mk in markets], np.int8)
    assert (known >= 0).sum() == 2
    last = reference_rounds(off, sid, prob, len(rank), 3, known=known)[-1]
    assert set(perf) == {n for n in rank if last.total[rank[n]] > 0}
    for name, p in perf.items():
        s = rank[name]
        assert p.reliability == last.w[s]
        assert p.total_markets == last.total[s]
        assert p.correct_predictions == last.correct[s]
        assert p.wrong_predictions == last.total[s] - last.correct[s]
        exp_markets = [str(mk.id) for mk, o in zip(markets, last.outcome) if o >= 0
                       for x in mk.signals if x["sourceId"] == name]
        assert p.markets == exp_markets
