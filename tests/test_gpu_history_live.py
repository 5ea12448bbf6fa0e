"""GPU checks of the live consensus history (batch.LivePlan, batch.live_trace,
batch.walk_history_live, bce_settle_trace_all, bce_consensus_history_live and the store method,
DESIGN §4.27): every point equals the arrival-level event loop of tests/history_live_ref.py, the
fixture recorded from the reference itself, and the existing lagged ``walk_forward`` run over the
batch expanded into its prefixes -- byte for byte, null points as their 0.0 values."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.batch.settle import _settle_trace
from oracle import oracle as orc
from history_live_ref import FIELDS, expand_prefixes, history_live_ref, load_fixture

pytestmark = pytest.mark.gpu

OFF = batch.SETTLE_LONG_OFF
HALF = 43_200_000_000
DAY = 2 * HALF
T0 = 1_790_000_000_000_000
PATHS = ({}, {"long_min": OFF}, {"long_min": 1, "chunk_bits": 64})


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _csr(b):
    return _T(np.asarray(b["off"], np.int64)), _T(np.asarray(b["sid"], np.int32)), _T(np.asarray(b["prob"], np.float64))


def _plan(b, **kw):
    return batch.LivePlan.build(*_csr(b), _T(np.asarray(b["outcome"], np.int8)), b["S"], _T(b["arrival"]),
                                _T(b["resolve"]), **kw)


def _table(state):
    rel, conf, t_us, present = state
    return batch.ReliabilityTable(_T(np.array(rel, np.float64)), _T(np.array(conf, np.float64)),
                                  _T(np.array(t_us, np.int64)), _T(np.array(present, np.uint8)), [""] * len(rel))


def _host(h):
    torch.cuda.synchronize()
    return {f: getattr(h, f).cpu().numpy() for f in FIELDS}


def _live(b, plan=None, table=None, **kw):
    off, sid, prob = _csr(b)
    return _host(batch.walk_history_live(plan or _plan(b), table or _table(b["state"]), offsets=off, sid=sid,
                                         prob=prob, **kw))


def _same(got, exp, what=""):
    for f in FIELDS:
        g, e = np.asarray(got[f]), np.asarray(exp[f])
        assert g.dtype == e.dtype and g.tobytes() == e.tobytes(), (what, f, np.flatnonzero(g != e)[:8])


def _state(table):
    return tuple(x.cpu().numpy() for x in (table.rel, table.conf, table.t_us, table.present))


def _expected(b, **kw):
    return history_live_ref(b["off"], b["sid"], b["prob"], b["outcome"], b["S"], *b["state"], b["arrival"],
                            b["resolve"], **kw)


def _batch(rng, lens, S, used=None, span=40, ordered=False):
    """Markets of the given lengths over sources [0, used): arrivals and resolve times on a grid of
    half days, so that signals of one market tie, and resolve times meet the arrivals of markets of
    lower and of higher index.  ``ordered``: the last arrivals do not decrease with the market."""
    lens = np.asarray(lens, np.int64)
    M, used = len(lens), used or S
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    arrival = np.zeros(n, np.int64)
    for m in range(M):
        t = np.sort(rng.integers(0, span, lens[m]))
        arrival[off[m]:off[m + 1]] = T0 + (t + (m // 4 if ordered else 0)) * HALF
    last = np.array([arrival[off[m + 1] - 1] if lens[m] else T0 for m in range(M)], np.int64)  # empty: no arrival
    if ordered:
        last = np.maximum.accumulate(last)
        for m in range(M):
            if lens[m]:
                arrival[off[m + 1] - 1] = last[m]
    outcome = rng.integers(-1, 2, M).astype(np.int8)
    resolve = last + rng.choice(np.array([0, 0, HALF, DAY, 3 * DAY, 45 * DAY + 1]), M)
    state = (rng.random(S), rng.random(S), T0 - rng.integers(0, 60, S) * DAY, (rng.random(S) < 0.7).astype(np.uint8))
    state[0][:2], state[3][:2] = (1.0, 0.0), 1
    state[2][1:3] = orc.NO_TIMESTAMP  # the row at 0.0 is never decayed: a prefix of source 1 alone is a null point
    return dict(off=off, sid=rng.integers(0, used, n).astype(np.int32), prob=np.round(rng.random(n), 3),
                outcome=outcome, S=S, arrival=arrival, resolve=resolve, state=state)


def _expanded_walk(b, **kw):
    """The lagged walk_forward over the prefix-expanded batch, picked at the history points."""
    xoff, xsid, xprob, xout, fc, rs, point = expand_prefixes(b["off"], b["sid"], b["prob"], b["outcome"],
                                                            b["arrival"], b["resolve"])
    plan = batch.WalkPlan.build_lagged(_T(xoff), _T(xsid), _T(xprob), _T(xout), b["S"], _T(fc), _T(rs))
    res = batch.walk_forward(plan, _table(b["state"]), offsets=_T(xoff), prob=_T(xprob), commit=False, **kw)
    torch.cuda.synchronize()
    sel = point >= 0
    out = {}
    for f in FIELDS:
        x = getattr(res, f).cpu().numpy()
        out[f] = np.zeros(len(b["sid"]), x.dtype)
        out[f][point[sel]] = x[sel]
    return out


# ----------------------------------------------------------------------------- golden fixture
def test_fixture_through_the_batch_call(golden_dir):
    from bayesian_engine.timeutil import iso_to_us

    g, (off, sid, prob, outcome, S), state, arrival, resolve = load_fixture(golden_dir)
    b = dict(off=off, sid=sid, prob=prob, outcome=outcome, S=S, arrival=arrival, resolve=resolve, state=state)
    exp, exp_state = _expected(b)
    plan = _plan(b)
    for kw in PATHS:
        table = _table(state)
        got = _live(b, plan, table, commit=True, check=True, **kw)
        _same(got, exp, f"fixture {kw}")
        for m, points in enumerate(g["results"]):  # the reference's own numbers
            for k, r in enumerate(points):
                at = int(off[m]) + k
                null = r["consensus"] is None
                assert null == bool(got["total_weight"][at] == 0), (m, k)
                assert null or repr(float(got["consensus"][at])) == r["consensus"], (m, k)
                assert repr(float(got["confidence"][at])) == r["confidence"], (m, k)
                assert repr(float(got["total_weight"][at])) == r["totalWeight"], (m, k)
                assert int(got["n_unique"][at]) == r["sourceCount"], (m, k)
        final = _state(table)
        rows = {n: (r, c, ts) for n, r, c, ts in g["final"]}
        for s, n in enumerate(g["names"]):
            assert (repr(float(final[0][s])), repr(float(final[1][s]))) == rows[n][:2], n
            assert final[2][s] == iso_to_us(rows[n][2]) and final[3][s] == 1, n
        for x, y in zip(final, exp_state):
            assert np.array_equal(x, y)
    N.check_faults(_dev(), "fixture")


def test_fixture_through_the_namespaced_store(golden_dir, tmp_path):
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    g = load_fixture(golden_dir)[0]
    store = NamespacedReliabilityStore(str(tmp_path / "live.db"))
    for name, r, c, ts in g["seeds"]:
        store._store._conn.execute(
            "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
            (name, g["scope"], float(r), float(c), ts))
    rows = lambda: [[r.source_id, repr(r.reliability), repr(r.confidence), r.updated_at]  # noqa: E731
                    for r in store._store.list_sources(g["scope"])]
    markets = [([{"sourceId": g["names"][s], "probability": float(p)} for s, p in mk["signals"]], mk["outcome"])
               for mk in g["markets"]]
    before = rows()
    dry, dsum = store.walk_history_live(markets, g["arrival_times"], g["resolve_times"], domain=g["domain"], dry_run=True)
    assert rows() == before  # dry run: the database is untouched
    wet, wsum = store.walk_history_live(markets, g["arrival_times"], g["resolve_times"], domain=g["domain"])
    assert dry == wet and dsum == wsum
    for m, (hist, points, (signals, _)) in enumerate(zip(wet, g["results"], markets)):
        assert len(hist) == len(points)
        for k, (row, r) in enumerate(zip(hist, points)):
            assert row["signals"] == k + 1 and row["sourceId"] == signals[k]["sourceId"], (m, k)
            assert (None if row["consensus"] is None else repr(row["consensus"])) == r["consensus"], (m, k)
            assert repr(row["confidence"]) == r["confidence"] and repr(row["totalWeight"]) == r["totalWeight"], (m, k)
            assert row["sourceCount"] == r["sourceCount"], (m, k)
    assert rows() == g["final"]
    assert {n: [repr(r.reliability), repr(r.confidence), r.updated_at] for n, r in wsum.records.items()} == \
        {row[0]: row[1:] for row in g["final"]}
    with pytest.raises(ValueError, match="arrival_times\\[1\\] has 2 entries for 6 signals"):
        bad = [list(a) for a in g["arrival_times"]]
        bad[1] = bad[1][:2]
        store.walk_history_live(markets, bad, g["resolve_times"], domain=g["domain"])
    with pytest.raises(ValueError, match="market 3 resolves before its last signal arrives"):
        early = list(g["resolve_times"])
        early[3] = g["arrival_times"][3][0]
        store.walk_history_live(markets, g["arrival_times"], early, domain=g["domain"], dry_run=True)
    store.close()
    N.check_faults(_dev(), "namespaced store")


# ----------------------------------------------------------------------------- the event loop
@pytest.mark.parametrize("seed", range(3))
def test_random_batches_against_the_event_loop(seed):
    rng = np.random.default_rng(100 + seed)
    cases = {
        "short": _batch(rng, rng.integers(1, 21, 40), 12),
        "every G": _batch(rng, [8, 9, 0, 16, 17, 1, 32, 33, 64, 5, 3], 9, used=7),  # sources 7, 8: no chain, never seen
        "long": _batch(rng, [65, 4, 128, 129, 7, 300, 0, 1], 10, span=90),
    }
    for name, b in cases.items():
        exp, exp_state = _expected(b)
        plan = _plan(b)
        longest = int(np.diff(b["off"]).max())
        routes = [dict(), dict(offsets_host=b["off"]), dict(max_len=longest)]
        for route in routes:
            table = _table(b["state"])
            got = _live(b, plan, table, check=True, **route)
            _same(got, exp, f"{name} seed {seed} {sorted(route)}")
            for x, y in zip(_state(table), b["state"]):  # nothing is committed
                assert x.tobytes() == np.asarray(y, x.dtype).tobytes()
        table = _table(b["state"])
        _same(_live(b, plan, table, commit=True), exp, f"{name} seed {seed} commit")
        for x, y in zip(_state(table), exp_state):
            assert x.dtype == y.dtype and np.array_equal(x, y), (name, seed)
    assert (cases["every G"]["sid"] < 7).all()
    N.check_faults(_dev(), "random batches")


def test_decay_parameters_reach_the_points_and_states_are_reused():
    rng = np.random.default_rng(7)
    b = _batch(rng, rng.integers(1, 30, 30), 8)
    plan, table = _plan(b), _table(b["state"])
    states = batch.live_trace(plan, table)
    grid = [(h, m) for h in (30.0, 5.0) for m in (0.1, 0.4)]
    outs = [_live(b, plan, table, states=states, half_life_days=h, min_rel=m) for h, m in grid]
    for (h, m), got in zip(grid, outs):
        _same(got, _live(b, half_life_days=h, min_rel=m), f"alone {h} {m}")
        _same(got, _expected(b, half_life=h, min_rel=m)[0], f"event loop {h} {m}")
    assert outs[0]["consensus"].tobytes() != outs[3]["consensus"].tobytes()
    with pytest.raises(ValueError, match="states must be"):
        _live(b, plan, table, states=states[:-1])
    N.check_faults(_dev(), "decay grid")


# ----------------------------------------------------------------------------- against the expanded walk
def test_a_4096_signal_market_against_the_expanded_walk():
    rng = np.random.default_rng(5)
    b = _batch(rng, [3, 4096, 5, 2, 6, 4, 1], 50, span=400)
    short = [0, 2, 3, 4, 5]
    b["outcome"][short] = [1, 0, 1, 1, 0]  # the short markets resolve inside the long one's life
    a, e = int(b["off"][1]), int(b["off"][2])
    assert ((b["arrival"][a] < b["resolve"][short]) & (b["resolve"][short] < b["arrival"][e - 1])).sum() >= 3
    got = _live(b, offsets_host=b["off"], check=True)
    _same(got, _expanded_walk(b), "4096")
    assert got["n_unique"][e - 1] == 50
    N.check_faults(_dev(), "4096")


def test_a_zipf_batch_on_the_chunked_trace_path_against_the_expanded_walk():
    rng = np.random.default_rng(9)
    M, S = 2000, 200
    b = _batch(rng, rng.integers(1, 49, M), S, span=60)
    b["sid"] = np.minimum(rng.zipf(1.3, len(b["sid"])) - 1, S - 1).astype(np.int32)
    plan = _plan(b)
    assert plan.settle.chunks(1, 64)[0] == plan.settle.n_touched and plan.settle.chunks(1, 64)[2] > plan.settle.n_touched
    assert plan.settle.chunks(batch.WALK_LONG_MIN, batch.WALK_CHUNK_BITS)[0] > 0  # the default takes the long path too
    exp = _expanded_walk(b)
    runs = [_live(b, plan, check=True, **kw) for kw in PATHS]
    for kw, got in zip(PATHS, runs):
        _same(got, exp, f"zipf {kw}")
    N.check_faults(_dev(), "zipf")


def _position_queries(sp):
    """One query per chain position: query g reads the state behind chain bit g, into row g."""
    start = sp.start.cpu().numpy()
    chain = np.repeat(np.arange(sp.n_sources), np.diff(start))
    g = np.arange(sp.n_bits)
    return SimpleNamespace(qstart=sp.start, qpos=_T((g - start[chain] + 1).astype(np.int64)), qentry=_T(g.astype(np.int32)))


def test_live_trace_equals_the_settle_trace_with_a_query_per_position():
    rng = np.random.default_rng(3)
    b = _batch(rng, rng.integers(0, 40, 300), 24, used=20)
    b["sid"][rng.random(len(b["sid"])) < 0.4] = 0  # one chain of thousands of bits
    plan, table = _plan(b), _table(b["state"])
    sp = plan.settle
    assert sp.n_bits > 1000 and int(sp.total.max()) > 1000 and int((sp.total == 0).sum()) >= 4
    q = _position_queries(sp)
    outs = []
    for kw in PATHS + ({"long_min": 64, "chunk_bits": 128},):
        want = torch.full((sp.n_bits, 2), -3.0, dtype=torch.float64, device=_dev())
        _settle_trace(sp, q, table.rel, table.conf, table.present, sp.n_bits, want, kw.get("long_min"),
                                   kw.get("chunk_bits"), N.stream(_dev()))
        got = batch.live_trace(plan, table, **kw)
        torch.cuda.synchronize()
        assert got.shape == want.shape and got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), kw
        assert not (want == -3.0).any()
        outs.append(got.cpu().numpy())
    N.check_faults(_dev(), "live_trace")
    for x, y in zip(_state(table), b["state"]):  # the table is only read
        assert x.tobytes() == np.asarray(y, x.dtype).tobytes()


# ----------------------------------------------------------------------------- against the walks
@pytest.fixture(scope="module")
def ordered():
    rng = np.random.default_rng(21)
    lens = rng.integers(0, 30, 60)
    lens[[3, 17]] = [70, 0]
    return _batch(rng, lens, 10, ordered=True)


def _lagged(b, forecast):
    off, sid, prob = _csr(b)
    return batch.WalkPlan.build_lagged(off, sid, prob, _T(b["outcome"]), b["S"], _T(forecast), _T(b["resolve"]))


def _last_arrival(b):
    lens = np.diff(b["off"])
    last = np.where(lens > 0, b["arrival"][np.maximum(b["off"][1:] - 1, 0)] if len(b["arrival"]) else 0, 0)
    for m in np.flatnonzero(lens == 0):  # an empty market is forecast with the market before it
        last[m] = last[m - 1] if m else b["arrival"].min()
    return last


def test_arrivals_at_the_forecast_time_give_walk_history(ordered):
    b = dict(ordered)
    forecast = _last_arrival(b)
    assert (np.diff(forecast) >= 0).all()
    b["arrival"] = np.repeat(forecast, np.diff(b["off"]))
    plan = _lagged(b, forecast)
    off, _, prob = _csr(b)
    want = _host(batch.walk_history(plan, _table(b["state"]), offsets=off, prob=prob, offsets_host=b["off"]))
    _same(_live(b, offsets_host=b["off"]), want, "walk_history")
    N.check_faults(_dev(), "walk_history")


def test_the_last_points_and_the_commit_are_the_lagged_walks(ordered):
    b = ordered
    forecast = _last_arrival(b)
    assert (np.diff(forecast) >= 0).all() and (b["resolve"][b["outcome"] >= 0] >= forecast[b["outcome"] >= 0]).all()
    plan = _lagged(b, forecast)
    off, sid, prob = _csr(b)
    dry, wet = _table(b["state"]), _table(b["state"])
    res = batch.walk_forward(plan, dry, offsets=off, prob=prob, commit=False)
    batch.walk_forward(plan, wet, offsets=off, prob=prob, commit=True)
    lplan, ltable = _plan(b), _table(b["state"])
    h = batch.walk_history_live(lplan, ltable, offsets=off, sid=sid, prob=prob, commit=True)
    last = h.last(off)
    torch.cuda.synchronize()
    for f in FIELDS:
        x, y = getattr(last, f).cpu().numpy(), getattr(res, f).cpu().numpy()
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f
    for x, y, z in zip(_state(ltable), _state(wet), _state(dry)):
        assert x.tobytes() == y.tobytes()
    assert _state(ltable)[0].tobytes() != _state(dry)[0].tobytes()
    assert torch.equal(lplan.slast, plan.slast) and torch.equal(lplan.settle.bits, plan.settle.bits)
    N.check_faults(_dev(), "last points")


def test_score_history_takes_the_result(ordered):
    b = ordered
    off, sid, prob = _csr(b)
    h = batch.walk_history_live(_plan(b), _table(b["state"]), offsets=off, sid=sid, prob=prob)
    sc = batch.score_history(h, off, _T(b["outcome"]))
    torch.cuda.synchronize()
    res = b["outcome"][np.repeat(np.arange(len(b["outcome"])), np.diff(b["off"]))] >= 0
    null = h.is_null().cpu().numpy()
    assert int(sc.counts[0, 0]) == int((res & ~null).sum())
    N.check_faults(_dev(), "score_history")


# ----------------------------------------------------------------------------- the fault word
def test_out_of_range_sid_raises_and_is_clamped():
    rng = np.random.default_rng(13)
    b = _batch(rng, rng.integers(1, 12, 20), 6)
    mk = np.repeat(np.arange(20), np.diff(b["off"]))
    for where in (int(np.flatnonzero(b["outcome"][mk] >= 0)[3]), int(np.flatnonzero(b["outcome"][mk] < 0)[1])):
        c = dict(b, sid=b["sid"].copy())
        c["sid"][where] = b["S"] + 5
        N.check_faults(_dev(), "clean slate")
        with pytest.raises(N.BCEError, match="sid"):
            _plan(c)
        N.check_faults(_dev(), "fault word is cleared")
        plan = _plan(c, check=False)
        assert plan.n_clamped == 1
        got = _live(c, plan)
        with pytest.raises(N.BCEError, match="sid"):
            N.check_faults(_dev(), "walk_history_live")
        _same(got, _expected(c)[0], "clamped sid")  # the stray signal went to the clamped row
    N.check_faults(_dev(), "clamped sid")


def test_bad_chains_raise_the_fault_word_and_read_as_no_visible_bit():
    rng = np.random.default_rng(17)
    b = _batch(rng, list(rng.integers(1, 12, 20)) + [80], 6)
    plan, table = _plan(b), _table(b["state"])
    states = batch.live_trace(plan, table)
    sp = plan.settle
    assert sp.n_bits > 20
    unresolved = dict(b, outcome=np.full(len(b["outcome"]), -1, np.int8))
    want = _expected(unresolved)[0]  # no resolution is ever seen
    assert want["consensus"].tobytes() != _expected(b)[0]["consensus"].tobytes()
    start = sp.start.cpu().numpy()
    bm = plan.bit_market.cpu().numpy()
    backwards = start[::-1].copy()                      # every chain ends before it begins (or is empty)
    beyond = start + (np.arange(len(start)) + 1) * sp.n_bits  # every chain lies past the bits
    N.check_faults(_dev(), "clean slate")
    for what, bad in (("start decreases", dataclasses.replace(plan, settle=dataclasses.replace(sp, start=_T(backwards)))),
                      ("start past the bits", dataclasses.replace(plan, settle=dataclasses.replace(sp, start=_T(beyond)))),
                      ("market past the batch", dataclasses.replace(plan, bit_market=_T(np.full_like(bm, len(b["outcome"]))))),
                      ("negative market", dataclasses.replace(plan, bit_market=_T(np.full_like(bm, -2))))):
        got = _live(b, bad, table, states=states, offsets_host=b["off"])
        with pytest.raises(N.BCEError):
            N.check_faults(_dev(), what)
        _same(got, want, what)
    _same(_live(b, plan, table, states=states, check=True), _expected(b)[0], "the plan's own arrays")
    N.check_faults(_dev(), "fault word is cleared")


def test_a_market_over_the_bound_is_left_untouched():
    rng = np.random.default_rng(19)
    b = _batch(rng, [3, 9, 8, 20, 1, 0, 7], 5)
    exp = _expected(b)[0]
    off, sid, prob = _csr(b)
    n = len(b["sid"])
    out = batch.HistoryResult(*(torch.full((n,), -7, dtype=t, device=_dev())
                                for t in (torch.float64, torch.float64, torch.float64, torch.int32)))
    N.check_faults(_dev(), "clean slate")
    batch.walk_history_live(_plan(b), _table(b["state"]), offsets=off, sid=sid, prob=prob, max_len=8, out=out)
    with pytest.raises(N.BCEError):
        N.check_faults(_dev(), "over the bound")
    got = _host(out)
    over = np.repeat(np.diff(b["off"]) > 8, np.diff(b["off"]))
    assert over.sum() == 29
    for f in FIELDS:
        assert (got[f][over] == -7).all() and got[f][~over].tobytes() == exp[f][~over].tobytes(), f
    with pytest.raises(ValueError, match="max_len"):
        batch.walk_history_live(_plan(b), _table(b["state"]), offsets=off, sid=sid, prob=prob, max_len=4097)
    with pytest.raises(ValueError, match="not the batch"):
        batch.walk_history_live(_plan(b), _table(b["state"]), offsets=off[:-1], sid=sid, prob=prob)
    N.check_faults(_dev(), "fault word is cleared")


def test_bad_arguments_are_refused_before_any_launch():
    rng = np.random.default_rng(23)
    b = _batch(rng, rng.integers(1, 9, 12), 5)
    plan, table = _plan(b), _table(b["state"])
    states = batch.live_trace(plan, table)
    sp = plan.settle
    off, sid, prob = _csr(b)
    n, M = len(b["sid"]), len(b["outcome"])
    h = batch.HistoryResult.alloc(n, _dev())
    p = N.ptr
    full = [p(off), M, p(sid), p(prob), n, p(states), None, b["S"], None, 0, None, None, 8, p(h.consensus),
            p(h.confidence), p(h.total_weight), p(h.n_unique), p(plan.arrival_us), p(sp.start), p(plan.bit_market),
            sp.n_bits, p(plan.resolve_time_us), p(table.rel), p(table.conf), p(table.t_us), p(table.present), 30.0, 0.1,
            0.5, 0.25, N.stream(_dev())]
    L = N.lib()
    N.check_faults(_dev(), "clean slate")
    assert L.bce_consensus_history_live(*full) == 0
    for at, value in ((0, None), (2, None), (3, None), (5, None), (13, None), (16, None), (17, None), (18, None),
                      (19, None), (21, None), (22, None), (23, None), (24, None), (1, -1), (4, -1), (7, 0), (9, -1),
                      (12, -1), (12, 4097), (20, -1)):
        args = list(full)
        args[at] = value
        assert L.bce_consensus_history_live(*args) == -1, at
        assert b"history_live" in L.bce_last_error(), at
    chunks = sp.chunks(batch.SETTLE_LONG_MIN, batch.SETTLE_CHUNK_BITS)
    tfull = [p(sp.bits), sp.n_bits, p(sp.start), p(sp.order), sp.n_touched, chunks[0], p(chunks[1]), chunks[2],
             batch.SETTLE_CHUNK_BITS, b["S"], p(table.rel), p(table.conf), p(table.present), 0.5, 0.25, p(states),
             N.stream(_dev())]
    assert L.bce_settle_trace_all(*tfull) == 0
    for at, value in ((0, None), (2, None), (3, None), (10, None), (11, None), (15, None), (1, -1), (4, -1), (9, 0),
                      (5, sp.n_touched + 1)):
        args = list(tfull)
        args[at] = value
        assert L.bce_settle_trace_all(*args) == -1, at
        assert b"settle_trace_all" in L.bce_last_error(), at
    N.check_faults(_dev(), "argument errors launch nothing")
