"""GPU checks of walk-forward consensus (batch.WalkPlan / batch.walk_forward and the store
layers): every market's consensus, every slot's weight, every entry's read state and the final
table equal the reference composition of tests/walk_ref.py exactly (``==``; NaN-aware), and the
fixture recorded from the reference itself, with the chunked long-chain path forced, disabled and
at its defaults."""
import json
import os

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.timeutil import iso_to_us
from oracle import oracle as orc
from walk_ref import walk_ref

pytestmark = pytest.mark.gpu

OFF = batch.SETTLE_LONG_OFF
MASK = 0x7FFFFFFF
DAY = 86_400_000_000
T0 = 1_790_000_000_000_000


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _plan(off, sid, prob, outcome, S, **kw):
    return batch.WalkPlan.build(_T(np.asarray(off, np.int64)), _T(np.asarray(sid, np.int32)),
                                _T(np.asarray(prob, np.float64)), _T(np.asarray(outcome, np.int8)), S, **kw)


def _table(state):
    rel, conf, t_us, present = state
    return batch.ReliabilityTable(_T(np.array(rel, np.float64)), _T(np.array(conf, np.float64)),
                                  _T(np.array(t_us, np.int64)), _T(np.array(present, np.uint8)),
                                  [""] * len(rel))


def _run(plan, state, mtime, off, prob, **kw):
    """(result fields as numpy, relconf by entry, final table arrays)."""
    table = _table(state)
    mt = _T(np.asarray(mtime, np.int64))
    res = batch.walk_forward(plan, table, mt, offsets=_T(np.asarray(off, np.int64)),
                             prob=_T(np.asarray(prob, np.float64)), **kw)
    trace_kw = {k: v for k, v in kw.items() if k in ("all_present", "long_min", "chunk_bits")}
    torch.cuda.synchronize()
    out = {k: getattr(res, k).cpu().numpy() for k in ("consensus", "confidence", "total_weight", "n_unique", "usid",
                                                      "weight", "nweight")}
    out["scope_present"] = res.scope_present.cpu().numpy()
    out["total"], out["correct"] = res.total.cpu().numpy(), res.correct.cpu().numpy()
    final = tuple(x.cpu().numpy() for x in (table.rel, table.conf, table.t_us, table.present))
    # the read states themselves, from the table the committed call left: a fresh start table
    wt, _ = batch.walk_trace(plan, _table(state), mt, **trace_kw)
    torch.cuda.synchronize()
    E = plan.pairs.n_entries
    return out, wt.relconf[:E].cpu().numpy(), final


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _compare(got, relconf, plan, exp, off, what=""):
    """Every market and every entry against walk_ref's output."""
    for k in ("consensus", "confidence", "total_weight", "n_unique"):
        assert _eq(got[k], exp[k]), (what, k, np.flatnonzero(~(got[k] == exp[k]))[:8])
    esrc = plan.pairs.usid.cpu().numpy()
    uoff = plan.pairs.uoffsets.cpu().numpy()
    for m in range(len(off) - 1):
        a, u = int(off[m]), int(exp["n_unique"][m])
        assert uoff[m + 1] - uoff[m] == u, (what, m)
        ent = got["usid"][a:a + u] & MASK
        assert np.array_equal(ent, np.arange(uoff[m], uoff[m] + u)), (what, m)  # slot j is entry uoff[m] + j
        assert np.array_equal(esrc[ent], exp["usid"][a:a + u] & MASK), (what, m)
        assert np.array_equal(got["usid"][a:a + u] < 0, exp["usid"][a:a + u] < 0), (what, m, "cold bit")
        assert _eq(got["weight"][a:a + u], exp["weight"][a:a + u]), (what, m)
        assert _eq(got["nweight"][a:a + u], exp["nweight"][a:a + u]), (what, m)
        assert np.array_equal(got["scope_present"][ent], exp["exists"][a:a + u]), (what, m)
        assert _eq(relconf[ent, 0], exp["rel_read"][a:a + u]), (what, m, "reliability read")
        assert _eq(relconf[ent, 1], exp["conf_read"][a:a + u]), (what, m, "confidence read")


def _same_state(got, exp, what=""):
    for name, g, e in zip(("rel", "conf", "t_us", "present"), got, exp):
        assert g.dtype == e.dtype, (what, name)
        assert _eq(g, e), (what, name, np.flatnonzero(g != e)[:8])


# ----------------------------------------------------------------------------- golden fixture
def _fixture(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "walk_forward_small.json")))
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
    for name, r, c, ts in g["seeds"]:
        s = names.index(name)
        rel[s], conf[s], t_us[s], present[s] = float(r), float(c), iso_to_us(ts), 1
    return g, (np.array(off, np.int64), np.array(sid, np.int32), np.array(prob), np.array(outcome, np.int8), S), \
        (rel, conf, t_us, present)


def _check_dicts(results, g, first=None):
    for m, (res, exp) in enumerate(zip(results, g["results"][:first])):
        assert (None if res["consensus"] is None else repr(res["consensus"])) == exp["consensus"], m
        assert repr(res["confidence"]) == exp["confidence"], m
        assert repr(res["normalization"]["totalWeight"]) == exp["totalWeight"], m
        assert [[w["sourceId"], repr(w["weight"]), repr(w["normalizedWeight"])] for w in res["sourceWeights"]] == \
            exp["sourceWeights"], m
        assert res["diagnostics"]["coldStartSources"] == [] and res["diagnostics"]["status"] == "computed"
        assert res["diagnostics"]["sources"] == len(g["markets"][m]["signals"])
        assert res["diagnostics"]["uniqueSources"] == res["normalization"]["sourceCount"] == len(exp["read"])


def test_fixture_through_the_batch_call(golden_dir):
    g, (off, sid, prob, outcome, S), state = _fixture(golden_dir)
    plan = _plan(off, sid, prob, outcome, S)
    exp, exp_state = walk_ref(off, sid, prob, outcome, S, *state, g["times_us"])
    for kw in ({}, {"long_min": OFF}, {"long_min": 1, "chunk_bits": 64}):
        got, relconf, final = _run(plan, state, g["times_us"], off, prob, **kw)
        _compare(got, relconf, plan, exp, off, f"fixture {kw}")
        _same_state(final, exp_state, f"fixture {kw}")
        uoff = plan.pairs.uoffsets.cpu().numpy()
        for m, r in enumerate(g["results"]):  # the reference's own numbers
            null = r["consensus"] is None
            assert null == bool(got["total_weight"][m] == 0)
            assert null or repr(float(got["consensus"][m])) == r["consensus"], m
            assert repr(float(got["confidence"][m])) == r["confidence"], m
            assert repr(float(got["total_weight"][m])) == r["totalWeight"], m
            ent = slice(int(uoff[m]), int(uoff[m + 1]))
            assert [[repr(float(x)), repr(float(y))] for x, y in relconf[ent]] == [x[1:] for x in r["read"]], m
        frows = {n: (r, c, ts) for n, r, c, ts in g["final"]}
        for s, n in enumerate(g["names"]):
            assert (repr(float(final[0][s])), repr(float(final[1][s]))) == frows[n][:2], n
            if got["total"][s] > 0:
                assert final[2][s] == iso_to_us(frows[n][2]), n
    N.check_faults(_dev(), "fixture")


def _seed_store(store, g):
    for name, r, c, ts in g["seeds"]:
        store._store._conn.execute(
            "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
            (name, g["scope"], float(r), float(c), ts))


def _rows(store, scope):
    return [[r.source_id, repr(r.reliability), repr(r.confidence), r.updated_at]
            for r in store._store.list_sources(scope)]


def _fixture_markets(g):
    return [([{"sourceId": g["names"][s], "probability": float(p)} for s, p in mk["signals"]], mk["outcome"])
            for mk in g["markets"]]


def test_fixture_through_the_namespaced_store(golden_dir, tmp_path):
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    g = json.load(open(os.path.join(golden_dir, "walk_forward_small.json")))
    store = NamespacedReliabilityStore(str(tmp_path / "walk.db"))
    _seed_store(store, g)
    before = _rows(store, g["scope"])
    dry, dsum = store.walk_forward(_fixture_markets(g), g["times"], domain=g["domain"], dry_run=True)
    assert _rows(store, g["scope"]) == before  # dry run: the database is untouched
    wet, wsum = store.walk_forward(_fixture_markets(g), g["times"], domain=g["domain"])
    assert dry == wet and dsum == wsum
    _check_dicts(wet, g)
    assert _rows(store, g["scope"]) == g["final"]  # updated_at included: each source's last resolved market
    assert {n: [repr(r.reliability), repr(r.confidence), r.updated_at] for n, r in wsum.records.items()} == \
        {row[0]: row[1:] for row in g["final"] if row[0] in wsum.records}
    assert set(wsum.total) == set(wsum.records) and all(wsum.correct[n] <= wsum.total[n] for n in wsum.total)
    store.close()
    N.check_faults(_dev(), "namespaced store")


def test_aggregator_orders_by_time_then_store_position(golden_dir, tmp_path):
    from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    g = json.load(open(os.path.join(golden_dir, "walk_forward_small.json")))

    def fill(n_markets):
        ms = MarketStore()
        for i, ((signals, outcome), t) in enumerate(list(zip(_fixture_markets(g), g["times"]))[:n_markets]):
            market = ms.create_market(MarketId(f"walk:m{i}"))
            for s in signals:
                market.add_signal(s)
            market.created_at = "2020-01-01T00:00:00+00:00" if outcome is not None else t
            if outcome is not None:
                market.resolve(outcome)
                market.resolved_at = t
        ms.create_market(MarketId("walk:empty"))  # no signals: not part of the walk
        return ms

    # the first five markets are in time order (3 and 4 tie: store position decides): the fixture itself
    store = NamespacedReliabilityStore(str(tmp_path / "agg5.db"))
    _seed_store(store, g)
    out, _ = CrossMarketAggregator(fill(5)).walk_forward(store, domain=g["domain"], dry_run=True)
    assert list(out) == [f"walk:m{i}" for i in range(5)]
    assert all(out[k]["marketId"] == k for k in out)
    _check_dicts(list(out.values()), g, first=5)
    store.close()
    # all ten: market 6 is earlier than market 5, so it is walked first; the unresolved market 5 reads, commits nothing
    order = sorted(range(10), key=lambda i: (g["times_us"][i], i))
    assert order.index(6) < order.index(5)
    agg = NamespacedReliabilityStore(str(tmp_path / "agg.db"))
    ref = NamespacedReliabilityStore(str(tmp_path / "ref.db"))
    for st in (agg, ref):
        _seed_store(st, g)
    out, summary = CrossMarketAggregator(fill(10)).walk_forward(agg, patterns=["walk:*"], domain=g["domain"])
    mk = _fixture_markets(g)
    exp, esummary = ref.walk_forward([mk[i] for i in order], [g["times"][i] for i in order], domain=g["domain"])
    assert list(out) == [f"walk:m{i}" for i in order]
    for k, e in zip(out, exp):
        assert {x: v for x, v in out[k].items() if x != "marketId"} == e
    assert summary == esummary and _rows(agg, g["scope"]) == _rows(ref, g["scope"])
    for st in (agg, ref):
        st.close()
    N.check_faults(_dev(), "aggregator")


# ----------------------------------------------------------------------------- edge batch
@pytest.fixture(scope="module")
def edge():
    """12 markets, 8 sources.  Source 3: a row without a timestamp; 4: NaN reliability; 6: no row,
    first seen in a resolved market; 7: no row, first seen in the unresolved market 2, settled in
    market 5.  Market 4 is empty, markets 2 and 8 unresolved; times repeat and go backwards."""
    rng = np.random.default_rng(5)
    S, M = 8, 12
    outcome = rng.integers(0, 2, M).astype(np.int8)
    outcome[[2, 8]] = -1
    markets = []
    for m in range(M):
        n = 0 if m == 4 else int(rng.integers(2, 7))
        sig = [(int(rng.integers(0, 7)), float(np.round(rng.random(), 3))) for _ in range(n)]
        if m in (1, 6, 9):  # a source twice in one market
            sig.append((sig[0][0], float(np.round(rng.random(), 3))))
        markets.append(sig)
    markets[2] += [(7, 0.9), (7, 0.2)]
    markets[5] += [(7, 0.6), (3, 0.5), (6, 0.5)]  # exactly on the threshold: votes True
    markets[3].append((4, 0.3))
    markets[7].append((4, 0.8))
    markets[9].append((7, 0.1))
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in markets])
    sid = np.array([s for x in markets for s, _ in x], np.int32)
    prob = np.array([p for x in markets for _, p in x], np.float64)
    days = np.array([0.0, 0.5, 0.5, 7.0, 8.0, 6.0, 30.0, 30.0, 31.5, 120.0, 121.0, 121.0])
    mtime = (T0 + days * DAY).astype(np.int64) + 123
    present = np.array([1, 1, 1, 1, 1, 1, 0, 0], np.uint8)
    rel = np.array([0.9, 0.05, 1.0, 0.66, np.nan, 0.0, 0.5, 0.5])
    conf = np.array([0.3, 0.99, 1.0, 0.41, 0.5, 0.0, 0.25, 0.25])
    # source 4's stamp lies after market 3: read there undecayed, so the NaN reaches a consensus
    t_us = np.array([T0 - 3 * DAY, T0 - 40 * DAY, T0 + DAY, orc.NO_TIMESTAMP, T0 + 8 * DAY, T0 - 90 * DAY,
                     orc.NO_TIMESTAMP, orc.NO_TIMESTAMP], np.int64)
    assert {4, 6, 7} <= set(sid.tolist()) and 6 not in sid[off[2]:off[3]]
    return dict(off=off, sid=sid, prob=prob, outcome=outcome, S=S, mtime=mtime, state=(rel, conf, t_us, present))


@pytest.mark.parametrize("all_present", [True, False])
@pytest.mark.parametrize("kw", [{}, {"long_min": OFF}, {"long_min": 1, "chunk_bits": 64}],
                         ids=["default", "off", "long1"])
def test_edge_batch(edge, kw, all_present):
    e = edge
    exp, exp_state = walk_ref(e["off"], e["sid"], e["prob"], e["outcome"], e["S"], *e["state"], e["mtime"],
                              all_present=all_present)
    slots = np.concatenate([np.arange(a, a + u) for a, u in zip(e["off"][:-1], exp["n_unique"])])
    assert (exp["usid"][slots] < 0).any() != all_present  # the absent sources show as cold only when asked to
    plan = _plan(e["off"], e["sid"], e["prob"], e["outcome"], e["S"])
    got, relconf, final = _run(plan, e["state"], e["mtime"], e["off"], e["prob"], all_present=all_present, **kw)
    _compare(got, relconf, plan, exp, e["off"], f"edge {kw} {all_present}")
    _same_state(final, exp_state, f"edge {kw}")
    assert np.isnan(got["consensus"]).any()  # the NaN row reaches a market
    N.check_faults(_dev(), "edge batch")


def test_single_market_and_empty_batch_of_one():
    state = (np.array([0.8, 0.2]), np.array([0.5, 0.6]), np.array([T0 - DAY, T0 - 2 * DAY], np.int64),
             np.ones(2, np.uint8))
    one = ([0, 3], [1, 0, 1], [0.7, 0.4, 0.2])
    for off, sid, prob, outcome in ((*one, [1]), (*one, [-1]), ([0, 0], [], [], [1])):
        exp, exp_state = walk_ref(off, sid, prob, outcome, 2, *state, [T0])
        plan = _plan(off, sid, prob, outcome, 2)
        got, relconf, final = _run(plan, state, [T0], off, prob)
        _compare(got, relconf, plan, exp, off, f"M=1 {outcome}")
        _same_state(final, exp_state, f"M=1 {outcome}")
    N.check_faults(_dev(), "M = 1")


def test_all_unresolved_equals_consensus_on_the_decayed_start_table(edge):
    e = edge
    outcome = np.full(len(e["outcome"]), -1, np.int8)
    plan = _plan(e["off"], e["sid"], e["prob"], outcome, e["S"])
    assert plan.settle.n_touched == 0
    got, _, final = _run(plan, e["state"], e["mtime"], e["off"], e["prob"])
    for g, before in zip(final, e["state"]):
        assert g.tobytes() == np.asarray(before, g.dtype).tobytes()
    table = _table(e["state"])
    esrc = plan.pairs.usid.cpu().numpy()
    for m in range(len(outcome)):  # market by market
        a, b = int(e["off"][m]), int(e["off"][m + 1])
        one = batch.consensus(_T(np.array([0, b - a], np.int64)), _T(e["sid"][a:b]), _T(e["prob"][a:b]),
                              table.consensus_table(int(e["mtime"][m])), max_len=64)
        torch.cuda.synchronize()
        for k in ("consensus", "confidence", "total_weight", "n_unique"):
            assert _eq(getattr(one, k).cpu().numpy()[0], got[k][m]), (m, k)
        u = int(got["n_unique"][m])
        assert np.array_equal(one.usid.cpu().numpy()[:u], esrc[got["usid"][a:a + u] & MASK]), m
        assert _eq(one.weight.cpu().numpy()[:u], got["weight"][a:a + u]), m
        assert _eq(one.nweight.cpu().numpy()[:u], got["nweight"][a:a + u]), m
    N.check_faults(_dev(), "all unresolved")


def test_out_of_range_sid_raises_and_is_clamped(edge):
    e = edge
    mk = np.repeat(np.arange(len(e["off"]) - 1), np.diff(e["off"]))
    for where in (int(np.flatnonzero(e["outcome"][mk] >= 0)[4]), int(np.flatnonzero(e["outcome"][mk] < 0)[1])):
        sid = e["sid"].copy()
        sid[where] = e["S"] + 5
        N.check_faults(_dev(), "clean slate")
        with pytest.raises(N.BCEError, match="sid"):
            _plan(e["off"], sid, e["prob"], e["outcome"], e["S"])
        N.check_faults(_dev(), "fault word is cleared")
        plan = _plan(e["off"], sid, e["prob"], e["outcome"], e["S"], check=False)
        got, relconf, final = _run(plan, e["state"], e["mtime"], e["off"], e["prob"])
        with pytest.raises(N.BCEError, match="sid"):
            N.check_faults(_dev(), "walk_forward")
        # the stray signal went to the clamped row; everything is what the reference gives for that
        exp, exp_state = walk_ref(e["off"], sid, e["prob"], e["outcome"], e["S"], *e["state"], e["mtime"])
        _compare(got, relconf, plan, exp, e["off"], "clamped sid")
        _same_state(final, exp_state, "clamped sid")
    N.check_faults(_dev(), "clamped sid")


def test_commit_false_leaves_the_table_and_commit_true_is_settle(edge):
    e = edge
    plan = _plan(e["off"], e["sid"], e["prob"], e["outcome"], e["S"])
    mt = _T(e["mtime"])
    args = dict(offsets=_T(e["off"]), prob=_T(e["prob"]))
    dry = _table(e["state"])
    a = batch.walk_forward(plan, dry, mt, commit=False, **args)
    torch.cuda.synchronize()
    for x, before in zip((dry.rel, dry.conf, dry.t_us, dry.present), e["state"]):
        assert x.cpu().numpy().tobytes() == np.asarray(before, x.cpu().numpy().dtype).tobytes()
    wet = _table(e["state"])
    b = wet.walk_forward(plan, mt, **args)
    for k in ("consensus", "confidence", "total_weight", "n_unique"):
        assert getattr(a, k).cpu().numpy().tobytes() == getattr(b, k).cpu().numpy().tobytes(), k
    slots = np.concatenate([np.arange(x, x + u) for x, u in zip(e["off"][:-1], a.n_unique.cpu().numpy())])
    for k in ("weight", "nweight", "usid"):  # the slots past a market's unique sources are not written
        assert getattr(a, k).cpu().numpy()[slots].tobytes() == getattr(b, k).cpu().numpy()[slots].tobytes(), k
    settled = _table(e["state"])
    settled.settle(plan.settle, 77)
    torch.cuda.synchronize()
    for name in ("rel", "conf", "present"):
        assert getattr(wet, name).cpu().numpy().tobytes() == getattr(settled, name).cpu().numpy().tobytes(), name
    touched = plan.total.cpu().numpy() > 0
    t_wet, t_set = wet.t_us.cpu().numpy(), settled.t_us.cpu().numpy()
    assert (t_set[touched] == 77).all() and np.array_equal(t_wet[~touched], e["state"][2][~touched])
    mk = np.repeat(np.arange(len(e["off"]) - 1), np.diff(e["off"]))
    for s in np.flatnonzero(touched):  # the time of the source's last resolved market
        last = mk[(e["sid"] == s) & (e["outcome"][mk] >= 0)].max()
        assert t_wet[s] == e["mtime"][last], s
    assert b.total is plan.total and b.correct is plan.correct
    N.check_faults(_dev(), "commit")


# ----------------------------------------------------------------------------- long path forced
LONG_MIN = 128
N_CUTS = 61  # 60 resolved markets


def _long_chains():
    """The chains of the settlement suite's forced-long test, with the start of every planted
    run of exactly 11 equal bits."""
    rng = np.random.default_rng(41)
    alt = lambda n: (np.arange(n) & 1).astype(np.uint8)  # noqa: E731
    ch, planted = {}, {}
    ch["alternating"] = alt(5000)                       # no sync run: worker 0 walks all of it
    ch["ones"] = np.ones(5000, np.uint8)
    ch["random50"] = (rng.random(20000) < 0.5).astype(np.uint8)
    ch["random90"] = (rng.random(20000) < 0.9).astype(np.uint8)
    ch["runs_of_10"] = np.tile(np.r_[np.ones(10, np.uint8), np.zeros(1, np.uint8)], 300)  # never 11 equal
    for C in (64, 256):  # runs of exactly 11 that just fit a chunk (53), straddle (54, 63), open one (64)
        b = alt(C * 16)
        starts = []
        for chunk, at in ((3, 53), (6, 54), (9, 63), (12, 64)):
            a = chunk * C + (at if C == 64 else C - 64 + at)
            b[a:a + 11] = b[a]
            assert b[a - 1] != b[a] and b[a + 11] != b[a]
            starts.append(a)
        ch[f"runs_of_11_c{C}"] = b
        planted[f"runs_of_11_c{C}"] = (C, starts)
    tail = alt(1500)
    tail[-11:] = tail[-11]
    ch["run_ends_on_last_bit"] = tail
    planted["run_ends_on_last_bit"] = (64, [1500 - 11])
    ch["exactly_long_min"] = (rng.random(LONG_MIN) < 0.5).astype(np.uint8)
    ch["long_min_minus_1"] = (rng.random(LONG_MIN - 1) < 0.5).astype(np.uint8)
    return ch, planted


def _cuts(L, C, starts):
    """N_CUTS market boundaries of a chain of L bits: 0, L, a + 10 / 11 / 12 of every planted run,
    and j * C - 1, j * C, j * C + 1 -- every j where they fit (the planted chains), else j spread
    evenly over the chain, every other one moved to a multiple of 256."""
    cuts = {0, L}
    for a in starts:
        cuts |= {x for x in (a + 10, a + 11, a + 12) if 0 < x < L}
    room = (N_CUTS - len(cuts)) // 3
    js = np.arange(1, (L - 1) // C + 1)
    if len(js) > room:
        js = np.unique(np.linspace(1, len(js), room).astype(np.int64))
        if C == 64:
            js[1::2] = np.maximum(4, js[1::2] // 4 * 4)
    for j in np.unique(js):
        for x in (j * C - 1, j * C, j * C + 1):
            if 0 < x < L and len(cuts) < N_CUTS:
                cuts.add(int(x))
    cuts = sorted(cuts)
    return cuts + [L] * (N_CUTS - len(cuts))  # short chains: the source is absent from the last markets


@pytest.fixture(scope="module")
def forced():
    ch, planted = _long_chains()
    names = list(ch)
    S = len(names)
    cuts = [_cuts(len(ch[n]), *planted.get(n, (64, []))) for n in names]
    for n, c in zip(names, cuts):
        C, starts = planted.get(n, (64, []))
        assert len(c) == N_CUTS and c[0] == 0 and c[-1] == len(ch[n]) and c == sorted(c)
        assert all(x in c for a in starts for x in (a + 10, a + 11, a + 12) if x <= len(ch[n]))
        if n.startswith("runs_of_11"):
            assert all(j * C + d in c for j in range(1, 16) for d in (-1, 0, 1)), n
    off, sid, prob, outcome = [0], [], [], []
    k = 0
    for m in range(N_CUTS - 1 + 3):
        if m in (7, 30, 55):  # unresolved markets in between: every source is read again, decoys
            outcome.append(-1)
            for s in range(S):
                sid += [s] * 2
                prob += [0.9, 0.1]
            off.append(len(sid))
            continue
        o = k & 1
        outcome.append(o)
        for s, n in enumerate(names):
            seg = ch[n][cuts[s][k]:cuts[s][k + 1]]
            sid += [s] * len(seg)
            prob += np.where(seg == o, 0.75, 0.25).tolist()  # (p >= 0.5) == outcome <=> bit
        off.append(len(sid))
        k += 1
    off, sid = np.array(off, np.int64), np.array(sid, np.int32)
    prob, outcome = np.array(prob), np.array(outcome, np.int8)
    M = len(outcome)
    mtime = T0 + (np.arange(M) // 2 * 2) * DAY + 500_000  # pairs of markets share a time
    mtime[40] = mtime[38] - DAY                           # and one goes back
    rel = np.array([0.37, np.nan, 1.7, 0.0, 1.0, 0.37, 0.5, -0.3, 0.9, 0.37])
    present = np.r_[np.ones(S - 1, np.uint8), 0].astype(np.uint8)  # the last source has no row
    state = (rel, np.linspace(0.0, 1.0, S), np.full(S, T0 - 5 * DAY, np.int64), present)
    exp = walk_ref(off, sid, prob, outcome, S, *state, mtime, all_present=False)
    return dict(names=names, args=(off, sid, prob, outcome, S), mtime=mtime, state=state, exp=exp)


@pytest.mark.parametrize("chunk_bits", [64, 256])
def test_long_path_forced(forced, chunk_bits):
    f = forced
    off, sid, prob, outcome, S = f["args"]
    plan = _plan(*f["args"])
    n_long, _, n_chunks = plan.settle.chunks(LONG_MIN, chunk_bits)
    assert n_long == len(f["names"]) - 1  # every chain but the one of long_min - 1 bits
    assert plan.total.cpu().tolist() == [len(x) for x in _long_chains()[0].values()]
    on = _run(plan, f["state"], f["mtime"], off, prob, all_present=False, long_min=LONG_MIN, chunk_bits=chunk_bits)
    flat = _run(plan, f["state"], f["mtime"], off, prob, all_present=False, long_min=OFF)
    slots = np.concatenate([np.arange(a, a + u) for a, u in zip(off[:-1], on[0]["n_unique"])])
    for k in on[0]:  # the slots past a market's unique sources are not written
        pick = slots if k in ("usid", "weight", "nweight") else slice(None)
        assert on[0][k][pick].tobytes() == flat[0][k][pick].tobytes(), (k, chunk_bits)
    assert on[1].tobytes() == flat[1].tobytes(), chunk_bits
    for x, y in zip(on[2], flat[2]):
        assert x.tobytes() == y.tobytes(), chunk_bits
    exp, exp_state = f["exp"]
    _compare(on[0], on[1], plan, exp, off, f"forced {chunk_bits}")
    _same_state(on[2], exp_state, f"forced {chunk_bits}")
    N.check_faults(_dev(), "forced long path")
