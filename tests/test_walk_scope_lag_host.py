"""CPU checks of the namespaced walk-forward with resolution lag: the argument errors of
batch.WalkScopePlan.build_lagged and of the walks that take its plan (torch checks on CPU tensors,
no kernel), and the event-loop reference the GPU suite compares against
(tests/walk_scope_lag_ref.py) -- against tests/walk_scope_ref.py where nothing lags, and against
the fixture recorded from the reference's NamespacedReliabilityStore itself."""
import os
import re

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.timeutil import iso_to_us
from walk_scope_lag_ref import load_fixture, walk_scope_lag_ref
from walk_scope_ref import GLOBAL, scope_key, walk_scope_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAY = 86_400_000_000
T0 = 1_790_000_000_000_000
NOTS = np.iinfo(np.int64).min
NS = {0: "market", 1: "domain", 2: "global", 3: "global"}
R = lambda x: repr(float(x))  # noqa: E731


def _T(a, dt):
    return torch.tensor(np.asarray(a, dt))


OK = dict(off=[0, 2, 3, 5], sid=[0, 1, 0, 1, 1], prob=[0.5, 0.6, 0.1, 0.9, 0.2], outcome=[1, -1, 0], md=[0, -1, 0],
          S=2, D=1, forecast=[T0, T0, T0 + DAY], resolve=[T0 + DAY, 0, T0 + DAY])


def _build(**kw):
    a = {**OK, **kw}
    f, r = a["forecast"], a["resolve"]
    return batch.WalkScopePlan.build_lagged(
        _T(a["off"], np.int64), _T(a["sid"], np.int32), _T(a["prob"], np.float64), _T(a["outcome"], np.int8),
        _T(a["md"], np.int32), a["S"], a["D"], f if isinstance(f, torch.Tensor) else _T(f, np.int64),
        r if isinstance(r, torch.Tensor) else _T(r, np.int64))


def test_build_lagged_refuses_bad_times_before_the_library():
    with pytest.raises(ValueError, match="must not decrease: market 2 is forecast before market 1"):
        _build(forecast=[T0, T0 + DAY, T0])
    with pytest.raises(ValueError, match="market 2 resolves before"):
        _build(resolve=[T0 + DAY, 0, T0 + DAY - 1])
    for name in ("forecast", "resolve"):
        with pytest.raises(ValueError, match=f"{name}_time_us must be int64 with one entry per market \\(3\\)"):
            _build(**{name: OK[name][:2]})
        with pytest.raises(ValueError, match=f"{name}_time_us must be int64"):
            _build(**{name: torch.tensor(OK[name], dtype=torch.float64)})
        with pytest.raises(ValueError, match=f"{name}_time_us must be int64"):
            _build(**{name: torch.tensor([0, 1, 2], dtype=torch.int32)})
        with pytest.raises(ValueError, match=f"{name}_time_us must be int64"):
            _build(**{name: torch.tensor([OK[name]], dtype=torch.int64)})
        with pytest.raises(ValueError, match="must be on the batch's device"):
            _build(**{name: torch.empty(3, dtype=torch.int64, device="meta")})
    with pytest.raises(ValueError, match="one entry per market"):
        _build(outcome=[1, -1])
    with pytest.raises(ValueError, match="n_sources"):
        _build(S=0)


def test_the_walks_refuse_the_two_argument_conflicts():
    a = OK
    off, prob = _T(a["off"], np.int64), _T(a["prob"], np.float64)
    outcome = _T(a["outcome"], np.int8)
    pairs, dplan, dentry, dq, gq, nc = batch.WalkScopePlan.order(off, _T(a["sid"], np.int32), prob, outcome,
                                                                 _T(a["md"], np.int32), a["S"], a["D"])
    plain = batch.WalkScopePlan(pairs, dplan, dentry, None, None, dq, gq, False, nc, outcome)
    lagged = batch.WalkScopePlan(pairs, dplan, dentry, None, None, dq, gq, False, nc, outcome,
                                 _T(a["forecast"], np.int64), _T(a["resolve"], np.int64))
    assert lagged.lagged and not plain.lagged and plain.outcome is outcome
    assert batch.WalkScopePlan(pairs, dplan, dentry, None, None, dq, gq, False, nc).outcome is None
    z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731
    domains = batch.PairTable.from_rows(z(0, torch.int64), z(0, torch.int32), z(0, torch.float64), z(0, torch.float64),
                                        z(0, torch.int64), z(0, torch.uint8), a["D"], a["S"])
    mt = _T(a["forecast"], np.int64)
    for call in (lambda p, *t: batch.walk_forward_scoped(p, domains, None, *t, offsets=off, prob=prob),
                 lambda p, *t: batch.walk_scope_trace(p, domains, None, *t),
                 lambda p, *t: batch.walk_sweep_scoped(p, domains, None, *t, offsets=off, prob=prob,
                                                       half_life_days=[30.0], min_rel=[0.1])):
        with pytest.raises(ValueError, match="carries its own times"):
            call(lagged, mt)
        with pytest.raises(ValueError, match="market_time_us is needed"):
            call(plain)
    with pytest.raises(ValueError, match="one entry per market"):
        batch.walk_forward_scoped(plain, domains, None, mt[:2], offsets=off, prob=prob)
    with pytest.raises(ValueError, match="at least one half_life_days"):
        batch.walk_sweep_scoped(lagged, domains, None, offsets=off, prob=prob, half_life_days=[], min_rel=[0.1])
    with pytest.raises(ValueError, match="keeps the outcomes"):
        batch.walk_sweep_scoped(batch.WalkScopePlan(pairs, dplan, dentry, None, None, dq, gq, False, nc), domains,
                                None, mt, offsets=off, prob=prob, half_life_days=[30.0], min_rel=[0.1])


def test_new_entry_is_declared_exported_and_refuses_null_times():
    src = open(os.path.join(ROOT, "include", "bce.h")).read()
    assert re.search(r"\bint\s+bce_walk_scope_read_lag\s*\(", src)
    assert "bce_walk_scope_read_lag" in N.EXPORTED
    lib = N.load_library()
    assert lib.bce_abi_version() == 3
    one = torch.zeros(4, dtype=torch.int64)
    for stamp, now in ((None, N.ptr(one)), (N.ptr(one), None)):
        assert lib.bce_walk_scope_read_lag(4, N.ptr(one), N.ptr(one), stamp, now, 1, 1, *([None] * 6), 0,
                                           *([None] * 7), 0, *([None] * 6), 30.0, 0.1, 0.5, 0.25, 0, 0, N.ptr(one),
                                           N.ptr(one), N.ptr(one), None) == -1
        assert b"walk_scope_read: NULL argument" in lib.bce_last_error()


# ----------------------------------------------------------------------------- the event loop
def _random_batch(seed, M=60, S=7, D=3):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6, M)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = np.round(rng.random(n), 3)
    outcome = rng.integers(-1, 2, M).astype(np.int8)
    md = rng.integers(-1, D, M).astype(np.int32)
    forecast = T0 + np.sort(rng.integers(0, 20, M)) * 5 * DAY  # ties included
    rows = {}
    for scope in [GLOBAL] + [("d", d) for d in range(D)] + [("m", m) for m in range(0, M, 4)]:
        for s in range(S):
            if rng.random() < 0.5:
                has = int(rng.random() < 0.7)
                rows[(scope, s)] = (float(rng.random()), float(rng.random()),
                                    int(T0 - rng.integers(0, 60) * DAY) if has else NOTS, has)
    return off, sid, prob, outcome, md, S, rows, forecast


def _same(got, exp):
    for k in exp[0]:
        assert np.array_equal(got[0][k], exp[0][k], equal_nan=exp[0][k].dtype.kind == "f"), k
    assert got[1] == exp[1]


@pytest.mark.parametrize("update_global", [False, True])
def test_event_loop_without_lag_is_the_ordinary_namespaced_walk(golden_dir, update_global):
    off, sid, prob, outcome, md, S, rows, forecast = _random_batch(5)
    assert (np.diff(forecast) == 0).any() and (outcome >= 0).any() and (outcome < 0).any() and (md < 0).any()
    for mark_cold in (False, True):
        exp = walk_scope_ref(off, sid, prob, outcome, md, S, rows, forecast, update_global=update_global,
                             mark_cold=mark_cold)
        got = walk_scope_lag_ref(off, sid, prob, outcome, md, S, rows, forecast, forecast,
                                 update_global=update_global, mark_cold=mark_cold)
        assert {0, 1, 2, 3} <= set(exp[0]["scope"].tolist())
        _same(got, exp)
    g, b, frows, forecast, _ = load_fixture(golden_dir)
    _same(walk_scope_lag_ref(*b[:5], b[6], frows, forecast, forecast, update_global=update_global),
          walk_scope_ref(*b[:5], b[6], frows, forecast, update_global=update_global))


def test_a_lag_changes_the_scope_later_markets_read_at():
    """The model is not vacuous: delaying every resolution past the last forecast leaves every
    market reading the start rows, and the final rows carry the resolve times."""
    off, sid, prob, outcome, md, S, rows, forecast = _random_batch(6)
    late = forecast[-1] + (1 + np.arange(len(forecast))) * DAY
    got, final = walk_scope_lag_ref(off, sid, prob, outcome, md, S, rows, forecast, late, update_global=True)
    none, same = walk_scope_lag_ref(off, sid, prob, np.full_like(outcome, -1), md, S, rows, forecast, late)
    assert same == rows
    for k in ("consensus", "confidence", "total_weight", "scope", "rel_read", "conf_read"):
        assert np.array_equal(got[k], none[k], equal_nan=True), k
    nolag, _ = walk_scope_lag_ref(off, sid, prob, outcome, md, S, rows, forecast, forecast, update_global=True)
    assert not np.array_equal(nolag["scope"], got["scope"])
    mk = np.repeat(np.arange(len(off) - 1), np.diff(off))
    for s in range(S):
        ms = mk[(sid == s) & (outcome[mk] >= 0)]
        if len(ms):
            assert final[(GLOBAL, s)][2:] == (late[ms.max()], 1), s
        for d in range(3):
            md_ms = ms[md[ms] == d]
            if len(md_ms):
                assert final[(("d", d), s)][2:] == (late[md_ms.max()], 1), (d, s)


@pytest.mark.parametrize("update_global", [False, True])
def test_event_loop_reproduces_the_reference_fixture(golden_dir, update_global):
    g, (off, sid, prob, outcome, md, D, S), rows, forecast, resolve = load_fixture(golden_dir)
    names = g["names"]
    run = g["runs"]["true" if update_global else "false"]
    assert len(g["markets"]) == 12 and S == 6 and D == 2
    res = [m for m in range(12) if outcome[m] >= 0]
    assert len(res) == 11 and (np.diff(forecast) >= 0).all() and (np.diff(forecast) == 0).sum() == 2
    assert all(resolve[m] >= forecast[m] for m in res)
    assert any(resolve[a] == forecast[b] and md[a] == md[b] for a in res for b in range(12) if a < b)  # seen
    assert any(resolve[b] == forecast[b] == forecast[a] and md[a] == md[b] for a in range(12) for b in res if a < b)
    assert max(resolve[m] for m in res) > forecast[-1]
    assert any(len({s for s, _ in mk["signals"]}) < len(mk["signals"]) for mk in g["markets"])
    exp, final = walk_scope_lag_ref(off, sid, prob, outcome, md, S, rows, forecast, resolve,
                                    update_global=update_global)
    reads = {}
    for m, r in enumerate(run["results"]):
        a, u = off[m], int(exp["n_unique"][m])
        assert R(exp["consensus"][m]) == r["consensus"] and R(exp["confidence"][m]) == r["confidence"], m
        assert R(exp["total_weight"][m]) == r["totalWeight"], m
        assert [[R(x), R(y), NS[int(sc)]] for x, y, sc in
                zip(exp["rel_read"][a:a + u], exp["conf_read"][a:a + u], exp["scope"][a:a + u])] == \
            [x[1:4] for x in r["read"]], m
        assert [int(sc) == 3 for sc in exp["scope"][a:a + u]] == [x[4] == "cold-start" for x in r["read"]], m
        assert [[names[i & 0x7FFFFFFF], R(x), R(y)] for i, x, y in
                zip(exp["usid"][a:a + u], exp["weight"][a:a + u], exp["nweight"][a:a + u])] == r["sourceWeights"], m
        for i, sc in zip(exp["usid"][a:a + u], exp["scope"][a:a + u]):
            reads[(m, int(i) & 0x7FFFFFFF)] = int(sc)
    # the cases the fixture exists for
    assert rows[(("d", 0), 2)][3] == 0 and resolve[0] > forecast[3] and md[0] == md[3] == 0
    assert reads[(3, 2)] == 2 and reads[(5, 2)] == 1        # skipped while market 0 is open, read at domain after
    assert (GLOBAL, 4) not in rows and md[2] == -1 and forecast[4] < resolve[2] < forecast[5]
    assert reads[(4, 4)] == 3 and reads[(5, 4)] == 2        # the global row appears between two forecasts
    assert resolve[1] == forecast[4] and md[1] == md[4] and reads[(1, 3)] == 3 and reads[(4, 3)] == 1
    assert reads[(3, 0)] == 0 and rows[(("m", 4), 1)][3] == 0 and reads[(4, 1)] == 1
    assert rows[(GLOBAL, 3)][3] == 0 and reads[(10, 3)] == 2  # a falsy-stamp global row, stamped by market 7
    assert {0, 1, 2, 3} == set(reads.values())
    rec = {(n, k): (float(r), float(c), iso_to_us(ts), 1 if ts else 0) for n, k, r, c, ts in run["final"]}
    mine = {(names[s], scope_key(g, sc)): v for (sc, s), v in final.items()}
    assert mine == rec
