"""GPU checks of the consensus history (bce_consensus_history, batch.consensus_history and the
layers above it).  Every expectation is the oracle's consensus of the host-expanded
batch (tests/history_ref.expand: one prefix market per point), compared with ``np.array_equal`` on
every point -- null points compare as their 0.0 values, none is left out."""
import json
import os
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from golden_util import load_json
from history_ref import FIELDS, expand, fixture_points, fixture_table, load_fixture
from oracle import oracle as orc
from score_ref import score_ref

pytestmark = pytest.mark.gpu

EDGE_LENS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096)
SENTINEL = -12345.0


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


def _table(b):
    return batch.SourceTable.from_arrays(_T(b["rel"]), _T(b["conf"]), _T(b["present"]))


def _expected(b):
    off2, sid2, prob2 = expand(b["off"], b["sid"], b["prob"])
    exp = orc.consensus_csr(off2, sid2, prob2, b["rel"], b["conf"], b["present"])
    return {k: exp[k] for k in FIELDS}


def _host(h):
    torch.cuda.synchronize()
    return {k: getattr(h, k).cpu().numpy() for k in FIELDS}


def _same(got, exp, what="", at=slice(None)):
    for k in FIELDS:
        g, e = got[k][at], exp[k][at]
        assert g.dtype == e.dtype and np.array_equal(g, e), (what, k, np.flatnonzero(g != e)[:8])


def _run(b, **kw):
    return _host(batch.consensus_history(_T(b["off"]), _T(b["sid"]), _T(b["prob"]), _table(b), **kw))


def _batch(lens, S, seed, zipf=None, p_cold=0.2, p_zero=0.1):
    rng = np.random.default_rng(seed)
    off = _offsets(lens)
    n = int(off[-1])
    if zipf:
        w = 1.0 / np.arange(1, S + 1) ** zipf
        sid = rng.choice(S, n, p=w / w.sum()).astype(np.int32)
    else:
        sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    rel, conf = rng.uniform(0.05, 1.0, S), rng.random(S)
    rel[rng.random(S) < p_zero] = 0.0
    present = (rng.random(S) >= p_cold).astype(np.uint8)
    rel[present == 0], conf[present == 0] = 0.5, 0.25
    return dict(off=off, sid=sid, prob=prob, rel=rel, conf=conf, present=present)


# ----------------------------------------------------------------------------- lengths at the edges
@pytest.fixture(scope="module")
def edges():
    b = _batch(EDGE_LENS, 3000, 1, zipf=1.1)
    return b, _expected(b)


def test_edge_lengths_on_every_route(edges):
    b, exp = edges
    assert len(b["sid"]) == sum(EDGE_LENS) and (exp["total_weight"] == 0).any()
    routes = {"build_device": {}, "offsets_host": dict(offsets_host=b["off"]), "device plan": dict(max_len=4096),
              "Plan": dict(plan=batch.Plan.build(b["off"], _dev()))}
    for what, kw in routes.items():
        _same(_run(b, check=True, **kw), exp, what)
    N.check_faults(_dev(), "edge lengths")


def test_each_edge_length_alone_in_one_launch(edges):
    """One market per call through the unplanned entry: the short kernel of every width and the
    long kernel of every LDS size, with max_len exactly the market's length."""
    b, exp = edges
    L = N.lib()
    table = _table(b)
    for m, n in enumerate(EDGE_LENS):
        if n == 0:
            continue
        a = int(b["off"][m])
        off = _T(np.array([0, n], np.int64))
        sid, prob = _T(b["sid"][a:a + n]), _T(b["prob"][a:a + n])
        for max_len in {n, min(4096, n + 1)}:
            h = batch.HistoryResult.alloc(n, _dev())
            N.check(L.bce_consensus_history(N.ptr(off), 1, N.ptr(sid), N.ptr(prob), n, N.ptr(table.relconf),
                                            N.ptr(table.bits), table.n, N.ptr(None), 0, N.ptr(None), N.ptr(None),
                                            max_len, N.ptr(h.consensus), N.ptr(h.confidence), N.ptr(h.total_weight),
                                            N.ptr(h.n_unique), N.stream(_dev())), "bce_consensus_history")
            got = _host(h)
            for k in FIELDS:
                assert np.array_equal(got[k], exp[k][a:a + n]), (n, max_len, k)
    N.check_faults(_dev(), "single markets")


# ----------------------------------------------------------------------------- short markets in bulk
def test_short_markets_in_bulk():
    rng = np.random.default_rng(2)
    for count, top in ((70_000, 8), (5_000, 64)):  # more markets than one pass of the grid
        b = _batch(rng.integers(1, top + 1, count), 3, 20 + top, p_cold=0.0, p_zero=0.0)
        exp = _expected(b)
        _same(_run(b, max_len=top, check=True), exp, f"1..{top} in one launch")
        _same(_run(b, offsets_host=b["off"], check=True), exp, f"1..{top} host lengths")
    both = _batch(np.concatenate([rng.integers(0, 9, 3000), rng.integers(0, 65, 500)]), 3, 5, p_cold=0.0)
    exp = _expected(both)
    _same(_run(both, check=True), exp, "planned")
    _same(_run(both, max_len=64, check=True), exp, "one launch")
    _same(_run(both, max_len=100, check=True), exp, "device plan")
    N.check_faults(_dev(), "bulk")


# ----------------------------------------------------------------------------- orderings
def test_orderings_that_stress_the_sort_and_the_runs():
    lens = (7, 40, 64, 65, 300)
    S = 400
    base = _batch(lens, S, 3, p_zero=0.0)
    off = base["off"]
    n = int(off[-1])
    pos = np.arange(n) - np.repeat(off[:-1], lens)
    rng = np.random.default_rng(4)
    cases = {"one source": np.full(n, 17), "descending": 350 - pos, "ascending": 20 + pos}
    for what, sid in cases.items():
        b = dict(base, sid=sid.astype(np.int32))
        exp = _expected(b)
        _same(_run(b, check=True), exp, what)
        if what == "one source":
            assert (exp["n_unique"] == 1).all()
        else:
            assert np.array_equal(exp["n_unique"], pos + 1)
    # reliability 0.0 for every source of the first half of every market: null until the second half
    sid = rng.integers(0, 200, n)
    half = pos >= np.repeat(np.asarray(lens) // 2, lens)
    sid[half] += 200
    rel = base["rel"].copy()
    rel[:200] = 0.0
    rel[200:] = np.maximum(rel[200:], 0.05)
    b = dict(base, sid=sid.astype(np.int32), rel=rel, present=np.ones(S, np.uint8))
    exp = _expected(b)
    assert np.array_equal(exp["total_weight"] == 0, ~half) and (exp["consensus"][~half] == 0).all()
    _same(_run(b, check=True), exp, "zero-weight opening")
    # probabilities of 1.25 sprinkled in: computed, not rejected
    prob = base["prob"].copy()
    prob[rng.random(n) < 0.05] = 1.25
    prob[off[:-1]] = 1.25  # every market opens with one: its first point is 1.25 itself
    b = dict(base, prob=prob)
    exp = _expected(b)
    assert (prob == 1.25).sum() > 15 and (exp["consensus"][off[:-1]] == 1.25).all()
    _same(_run(b, check=True), exp, "1.25")
    N.check_faults(_dev(), "orderings")


# ----------------------------------------------------------------------------- last point
def test_last_point_equals_the_consensus_kernels():
    rng = np.random.default_rng(6)
    lens = np.concatenate([rng.integers(0, 70, 300), [0, 64, 65, 128, 129, 700, 1536, 2049, 4096]])
    b = _batch(lens, 500, 7, zipf=1.2)
    off, sid, prob, table = _T(b["off"]), _T(b["sid"]), _T(b["prob"]), _table(b)
    hist = batch.consensus_history(off, sid, prob, table, check=True)
    res = batch.consensus(off, sid, prob, table, check=True)
    last = hist.last(off)
    for k in FIELDS:
        g, e = getattr(last, k), getattr(res, k)
        assert g.dtype == e.dtype and torch.equal(g, e), k
    assert torch.equal(last.is_null(off), res.is_null(off)) and bool(last.is_null(off)[300])
    assert torch.equal(hist.is_null(), hist.total_weight == 0)


# ----------------------------------------------------------------------------- market list
def test_market_list_leaves_every_other_market_untouched():
    rng = np.random.default_rng(8)
    lens = np.concatenate([rng.integers(0, 70, 200), [65, 300, 1000, 0, 64]])
    b = _batch(lens, 50, 9)
    exp = _expected(b)
    listed = np.sort(rng.choice(len(lens), 60, replace=False))
    listed = np.union1d(listed, [200, 202, 203])
    n = len(b["sid"])
    mine = np.zeros(n, bool)
    for m in listed:
        mine[b["off"][m]:b["off"][m + 1]] = True
    plan = batch.Plan.for_markets(b["off"], listed, _dev())
    out = batch.HistoryResult(*(torch.full((n,), SENTINEL, dtype=torch.float64, device=_dev()) for _ in range(3)),
                              torch.full((n,), -7, dtype=torch.int32, device=_dev()))
    got = _run(b, plan=plan, out=out, check=True)
    _same(got, exp, "listed", mine)
    for k in FIELDS:
        assert (got[k][~mine] == (-7 if k == "n_unique" else SENTINEL)).all(), k
    # the same through the C entry's plain list: one launch sized by max_len
    short = listed[lens[listed] <= 64]
    mine = np.zeros(n, bool)
    for m in short:
        mine[b["off"][m]:b["off"][m + 1]] = True
    for t in (out.consensus, out.confidence, out.total_weight):
        t.fill_(SENTINEL)
    out.n_unique.fill_(-7)
    table, lst = _table(b), _T(short.astype(np.int32))
    off, sid, prob = _T(b["off"]), _T(b["sid"]), _T(b["prob"])
    N.check(N.lib().bce_consensus_history(N.ptr(off), len(lens), N.ptr(sid), N.ptr(prob), n, N.ptr(table.relconf),
                                          N.ptr(table.bits), table.n, N.ptr(lst), len(short), N.ptr(None),
                                          N.ptr(None), 64, N.ptr(out.consensus), N.ptr(out.confidence),
                                          N.ptr(out.total_weight), N.ptr(out.n_unique), N.stream(_dev())),
            "bce_consensus_history")
    got = _host(out)
    _same(got, exp, "plain list", mine)
    for k in FIELDS:
        assert (got[k][~mine] == (-7 if k == "n_unique" else SENTINEL)).all(), k
    N.check_faults(_dev(), "market list")


# ----------------------------------------------------------------------------- large table
def test_large_table_uses_the_whole_sid():
    """2^26 + 8 rows: (sid, position) needs more than 32 bits at either market length."""
    S = (1 << 26) + 8
    small = _batch((40, 300), 8, 10, p_zero=0.0)
    exp = _expected(small)  # the top 8 rows hold the small table: same order, same values
    relconf = torch.zeros((S, 2), dtype=torch.float64, device=_dev())
    relconf[S - 8:, 0] = _T(small["rel"])
    relconf[S - 8:, 1] = _T(small["conf"])
    bits = torch.zeros((S + 31) // 32, dtype=torch.int32, device=_dev())
    table = batch.SourceTable(relconf, bits, range(S))
    assert table.n == S
    sid = _T((small["sid"].astype(np.int64) + (S - 8)).astype(np.int32))
    for kw in (dict(offsets_host=small["off"]), dict(max_len=512)):
        h = batch.consensus_history(_T(small["off"]), sid, _T(small["prob"]), table, check=True, **kw)
        _same(_host(h), exp, f"large table {kw}")
    del relconf, table


# ----------------------------------------------------------------------------- rejection
def test_too_long_markets_and_bad_sids_are_reported():
    b = _batch((5, 4097, 3), 10, 11)
    args = (_T(b["off"]), _T(b["sid"]), _T(b["prob"]), _table(b))
    N.check_faults(_dev(), "clean slate")
    with pytest.raises(ValueError, match="market 1 has 4097 signals"):
        batch.consensus_history(*args, offsets_host=b["off"])
    with pytest.raises(ValueError, match="market 1 has 4097 signals"):
        batch.consensus_history(*args)  # Plan.build_device: the host learns the lengths
    with pytest.raises(ValueError, match="market 1 has 4097 signals"):
        batch.consensus_history(*args, plan=batch.Plan.build(b["off"], _dev()))
    N.check_faults(_dev(), "refused on the host")
    # a bound without host lengths: the market is left untouched and the fault word raised
    for lens, bound, who in (((5, 70, 3, 64), 64, "one launch"), ((5, 4097, 3, 64), 4096, "device plan")):
        b = _batch(lens, 10, 12)
        n = len(b["sid"])
        long_ = np.zeros(n, bool)
        long_[5:5 + lens[1]] = True
        rest = _expected(dict(b, off=_offsets((5, 0, 3, 64)), sid=b["sid"][~long_], prob=b["prob"][~long_]))
        out = batch.HistoryResult(*(torch.full((n,), SENTINEL, dtype=torch.float64, device=_dev())
                                    for _ in range(3)), torch.full((n,), -7, dtype=torch.int32, device=_dev()))
        h = batch.consensus_history(_T(b["off"]), _T(b["sid"]), _T(b["prob"]), _table(b), max_len=bound, out=out)
        with pytest.raises(N.BCEError):
            N.check_faults(_dev(), who)
        got = _host(h)
        for k in FIELDS:
            assert (got[k][long_] == (-7 if k == "n_unique" else SENTINEL)).all(), (who, k)
            assert np.array_equal(got[k][~long_], rest[k]), (who, k)
    N.check_faults(_dev(), "fault word is cleared")
    # a sid outside the table: its row read is clamped, the sid fault raised
    b = _batch((5, 70, 3), 10, 13)
    for bad in (10, -1, 2 ** 31 - 1):
        for where in (2, 40):
            sid = b["sid"].copy()
            sid[where] = bad
            batch.consensus_history(_T(b["off"]), _T(sid), _T(b["prob"]), _table(b), offsets_host=b["off"])
            with pytest.raises(N.BCEError, match="sid"):
                N.check_faults(_dev(), "bad sid")
            exp = _expected(dict(b, sid=np.where(np.arange(len(sid)) == where, 9, sid).astype(np.int32)))
            _same(_run(dict(b, sid=sid), offsets_host=b["off"]), exp, f"clamped {bad}")
            with pytest.raises(N.BCEError, match="sid"):
                N.check_faults(_dev(), "bad sid")
    N.check_faults(_dev(), "fault word is cleared")


# G lanes per market: the first 64 / G markets share the first wave; the too-long one is not its first
SAME_WAVE_LENS = {8: (5, 8, 9, 3, 0, 1, 8, 7, 2, 8, 6, 4), 16: (16, 17, 0, 9, 1, 16, 12, 3, 15, 2, 16, 8)}


@pytest.mark.parametrize("G", sorted(SAME_WAVE_LENS))
def test_too_long_market_shares_a_wave_with_valid_ones(G):
    """A dozen markets under max_len = G: one wave of the short kernel holds a too-long market (not
    its first), an empty one and valid ones.  The neighbours are bit-exact, the too-long market
    keeps what ``out`` held, and the fault word reads kFaultTooLong (4)."""
    lens = SAME_WAVE_LENS[G]
    bad = int(np.argmax(np.array(lens) > G))
    per_wave = 64 // G
    assert 0 < bad < per_wave and 0 in lens[:per_wave] and sum(0 < x <= G for x in lens[:per_wave]) >= 2
    b = _batch(lens, 10, 20 + G)
    n = len(b["sid"])
    long_ = np.zeros(n, bool)
    long_[b["off"][bad]:b["off"][bad + 1]] = True
    rest = _expected(dict(b, off=_offsets([0 if m == bad else x for m, x in enumerate(lens)]), sid=b["sid"][~long_],
                          prob=b["prob"][~long_]))
    out = batch.HistoryResult(*(torch.full((n,), SENTINEL, dtype=torch.float64, device=_dev()) for _ in range(3)),
                              torch.full((n,), -7, dtype=torch.int32, device=_dev()))
    N.check_faults(_dev(), "clean slate")
    got = _run(b, max_len=G, out=out)
    with pytest.raises(N.BCEError, match="device fault 4"):
        N.check_faults(_dev(), "too long in the wave")
    for k in FIELDS:
        assert (got[k][long_] == (-7 if k == "n_unique" else SENTINEL)).all(), k
        assert got[k].dtype == rest[k].dtype and np.array_equal(got[k][~long_], rest[k]), k
    N.check_faults(_dev(), "fault word is cleared")


# ----------------------------------------------------------------------------- walks
def _walk_fixture(golden_dir, name):
    from bayesian_engine.timeutil import iso_to_us

    g = json.load(open(os.path.join(golden_dir, name)))
    names = g["names"]
    S = len(names)
    off, sid, prob, outcome = [0], [], [], []
    for mk in g["markets"]:
        for s, p in mk["signals"]:
            sid.append(s)
            prob.append(float(p))
        off.append(len(sid))
        outcome.append(-1 if mk["outcome"] is None else int(mk["outcome"]))
    rel, conf = np.full(S, 0.5), np.full(S, 0.25)
    t_us, present = np.full(S, orc.NO_TIMESTAMP, np.int64), np.zeros(S, np.uint8)
    for nm, r, c, ts in g["seeds"]:
        s = names.index(nm)
        rel[s], conf[s], t_us[s], present[s] = float(r), float(c), iso_to_us(ts), 1
    csr = (_T(np.array(off, np.int64)), _T(np.array(sid, np.int32)), _T(np.array(prob)))
    return g, csr, _T(np.array(outcome, np.int8)), S, (rel, conf, t_us, present)


def _rtable(state):
    rel, conf, t_us, present = state
    return batch.ReliabilityTable(_T(rel), _T(conf), _T(t_us), _T(present), [""] * len(rel))


@pytest.mark.parametrize("name", ["walk_forward_small.json", "walk_lag_small.json"])
def test_walk_history_on_the_walk_fixtures(golden_dir, name):
    g, (off, sid, prob), outcome, S, state = _walk_fixture(golden_dir, name)
    if "forecast_times_us" in g:
        resolve = [0 if t is None else t for t in g["resolve_times_us"]]
        plan = batch.WalkPlan.build_lagged(off, sid, prob, outcome, S, _T(np.array(g["forecast_times_us"], np.int64)),
                                           _T(np.array(resolve, np.int64)))
        times = ()
    else:
        plan = batch.WalkPlan.build(off, sid, prob, outcome, S)
        times = (_T(np.array(g["times_us"], np.int64)),)
    table = _rtable(state)
    hist = batch.walk_history(plan, table, *times, offsets=off, prob=prob, check=True)
    wt, _ = batch.walk_trace(plan, _rtable(state), *times)
    direct = batch.consensus_history(off, plan.pairs.esid, prob, wt, check=True)
    walk = batch.walk_forward(plan, _rtable(state), *times, offsets=off, prob=prob, commit=False)
    last = hist.last(off)
    for k in FIELDS:
        assert torch.equal(getattr(hist, k), getattr(direct, k)), k
        assert torch.equal(getattr(last, k), getattr(walk, k)), k
    for x, before in zip((table.rel, table.conf, table.t_us, table.present), state):  # nothing is committed
        assert x.cpu().numpy().tobytes() == np.asarray(before, x.cpu().numpy().dtype).tobytes()
    # the entry table against the oracle, point by point
    E = plan.pairs.n_entries
    b = dict(off=off.cpu().numpy(), sid=plan.pairs.esid.cpu().numpy(), prob=prob.cpu().numpy(),
             rel=wt.relconf[:E, 0].cpu().numpy().copy(), conf=wt.relconf[:E, 1].cpu().numpy().copy(),
             present=np.ones(E, np.uint8))
    _same(_host(hist), _expected(b), name)
    # ... and the reference's own numbers at every market's last point
    got = _host(hist)
    for m, r in enumerate(g["results"]):
        p = int(b["off"][m + 1]) - 1
        assert (r["consensus"] is None) == bool(got["total_weight"][p] == 0), m
        assert r["consensus"] is None or repr(float(got["consensus"][p])) == r["consensus"], m
        assert repr(float(got["confidence"][p])) == r["confidence"], m
    N.check_faults(_dev(), name)


# ----------------------------------------------------------------------------- scoring
def _same_score(r, ref, what):
    torch.cuda.synchronize()
    for k in ("counts", "sums", "bin_n", "bin_pos", "bin_psum"):
        g = getattr(r, k).cpu().numpy()
        assert g.shape == ref[k].shape and np.array_equal(g, ref[k]), (what, k)


def test_score_history_both_forms():
    rng = np.random.default_rng(14)
    lens = np.concatenate([rng.integers(0, 40, 120), [2100, 0, 65]])  # a group longer than a score segment
    M = len(lens)
    b = _batch(lens, 30, 15, p_zero=0.3)
    off = _T(b["off"])
    hist = batch.consensus_history(off, _T(b["sid"]), _T(b["prob"]), _table(b), offsets_host=b["off"], check=True)
    exp = _expected(b)  # the expanded arrays: one "market" per point
    assert (exp["total_weight"] == 0).sum() > 5
    outcome = rng.choice(np.array([-1, 0, 1], np.int8), M, p=[0.15, 0.45, 0.4])
    market = np.repeat(np.arange(M), lens)
    goff = np.array([0, 60, 60, 130], np.int64)
    members = np.concatenate([rng.permutation(M)[:60], rng.integers(0, M, 69), [120]]).astype(np.int64)
    items = [np.concatenate([np.arange(b["off"][m], b["off"][m + 1]) for m in members[goff[g]:goff[g + 1]]] +
                            [np.zeros(0, np.int64)]) for g in range(3)]
    for plan, lists in ((None, [np.arange(len(market))]),
                        (batch.ScorePlan.groups(_T(goff), _T(members)), items)):
        ref = score_ref(dict(goff=_offsets([len(x) for x in lists]), pidx=np.concatenate(lists), oidx=None,
                             value=exp["consensus"], outcome=outcome[market], valid=exp["total_weight"] != 0,
                             base=None, B=10, eps=1e-15))
        _same_score(batch.score_history(hist, off, _T(outcome), plan=plan), ref, "every point")
    # one chosen point per market: what history_at returns
    arrival = np.concatenate([np.sort(rng.integers(0, 1000, n)) for n in lens] + [np.zeros(0, np.int64)])
    at = rng.integers(-50, 1100, M)
    points = batch.history_at(off, _T(arrival), _T(at))
    hp = points.cpu().numpy()
    assert (hp == -1).sum() > 3 and (hp >= 0).sum() > 100
    assert np.array_equal(hp, batch.history_at(torch.from_numpy(b["off"]), torch.from_numpy(arrival),
                                               torch.from_numpy(at)).numpy())
    value = np.where(hp >= 0, exp["consensus"][np.maximum(hp, 0)], 0.0)
    valid = (hp >= 0) & (exp["total_weight"][np.maximum(hp, 0)] != 0)
    for plan, mgoff, mem in ((None, np.array([0, M]), np.arange(M)),
                             (batch.ScorePlan.groups(_T(goff), _T(members)), goff, members)):
        ref = score_ref(dict(goff=mgoff, pidx=mem, oidx=None, value=value, outcome=outcome, valid=valid, base=None,
                             B=10, eps=1e-15))
        _same_score(batch.score_history(hist, off, _T(outcome), points=points, plan=plan), ref, "chosen points")
        assert (hp[mem] == -1).sum() > 0 and ref["counts"][:, 3].sum() > 0
    N.check_faults(_dev(), "score_history")


# ----------------------------------------------------------------------------- drop-in layer
def _entry_of(res, k, signal):
    return {"signals": k + 1, "sourceId": signal["sourceId"], "consensus": res["consensus"],
            "confidence": res["confidence"], "totalWeight": res["normalization"]["totalWeight"],
            "sourceCount": res["normalization"]["sourceCount"]}


def test_market_history_against_the_fixture_and_the_prefix_calls(golden_dir):
    from bayesian_engine.core import compute_consensus
    from bayesian_engine.market import Market, MarketId, MarketStore

    g = load_fixture(golden_dir)[0]
    table = fixture_table(g)
    points = iter(fixture_points(g))
    store = MarketStore()
    for i, mk in enumerate(g["markets"]):
        market = store.create_market(MarketId(f"h:m{i}"))
        for name, p in mk["signals"]:
            market.add_signal({"sourceId": name, "probability": float(p)})
        got = market.consensus_history(table)
        assert market.consensus_result is None and len(got) == len(mk["signals"])
        for k, (row, signal) in enumerate(zip(got, market.signals)):
            cons, confd, tot, count = next(points)
            assert list(row) == ["signals", "sourceId", "consensus", "confidence", "totalWeight", "sourceCount"]
            assert (None if row["consensus"] is None else repr(row["consensus"])) == cons, (i, k)
            assert (repr(row["confidence"]), repr(row["totalWeight"]), row["sourceCount"]) == (confd, tot, count)
            assert row == _entry_of(compute_consensus(market.signals[:k + 1], table), k, signal), (i, k)
            assert type(row["sourceCount"]) is int and type(row["totalWeight"]) is float
    assert Market(id=MarketId("h:none")).consensus_history() == []
    # all open markets in one batch, cold-start table: the per-prefix calls of this package
    store.get_market(MarketId("h:m3")).resolve(True)  # not open: left out
    everything = store.compute_all_history()
    assert list(everything) == [f"h:m{i}" for i in range(len(g["markets"])) if i != 3]
    assert everything["h:m0"] == []
    for key, rows in everything.items():
        market = store.get_market(MarketId(key))
        assert rows == [_entry_of(compute_consensus(market.signals[:k + 1]), k, s)
                        for k, s in enumerate(market.signals)], key
        assert market.consensus_result is None
    N.check_faults(_dev(), "market history")


def test_store_history_and_compute_all_consensus_on_market_cases():
    import bayesian_engine.decay as dmod
    from bayesian_engine.market import MarketId, MarketStore
    from bayesian_engine.reliability import SQLiteReliabilityStore

    epoch = datetime(1970, 1, 1, tzinfo=timezone.utc)
    for case in load_json("market_cases.json"):
        store = SQLiteReliabilityStore(":memory:")
        for row in case["rows"]:
            store._conn.execute("INSERT INTO sources VALUES (?,?,?,?,?)", tuple(row))
        ms = MarketStore()
        for mk in case["markets"]:
            m = ms.create_market(MarketId(mk["marketId"]))
            for s in mk["signals"]:
                m.add_signal(s)
            if mk["resolved"]:
                m.resolve(True)
        now = epoch + timedelta(microseconds=case["now_us"])

        class _Frozen(datetime):
            @classmethod
            def now(cls, tz=None):
                return now

        old = dmod.datetime
        dmod.datetime = _Frozen
        try:
            hist = ms.compute_all_history(store)
            assert all(m.consensus_result is None for m in ms.list_markets())
            got = ms.compute_all_consensus(store)
        finally:
            dmod.datetime = old
        assert got == case["expected"] and list(got) == list(case["expected"])  # unchanged
        assert ms.compute_all_consensus(None) == case["expected_no_store"]
        assert list(hist) == list(got)
        for key, rows in hist.items():
            market = ms.get_market(MarketId(key))
            assert len(rows) == len(market.signals)
            if rows:  # the last point is the market's consensus, from the same decayed table
                e = got[key]
                assert rows[-1] == _entry_of(e, len(rows) - 1, market.signals[-1]), key
        store.close()
    N.check_faults(_dev(), "market cases")
