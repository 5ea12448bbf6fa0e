"""CPU checks of walk-forward with resolution lag: the argument errors of
batch.WalkPlan.build_lagged and batch.walk_forward (torch checks on CPU tensors, no kernel), and
the event-loop reference the GPU suite compares against (tests/walk_lag_ref.py) -- against
tests/walk_ref.py where nothing lags, and against the fixture recorded from the reference itself."""
import json
import os

import numpy as np
import pytest
import torch

from bayesian_engine import batch
from walk_lag_ref import load_fixture, walk_lag_ref
from walk_ref import walk_ref

DAY = 86_400_000_000
T0 = 1_790_000_000_000_000


def _T(a, dt):
    return torch.tensor(np.asarray(a, dt))


OK = dict(off=[0, 2, 3, 5], sid=[0, 1, 0, 1, 1], prob=[0.5, 0.6, 0.1, 0.9, 0.2], outcome=[1, -1, 0], S=2,
          forecast=[T0, T0, T0 + DAY], resolve=[T0 + DAY, 0, T0 + DAY])


def _build(**kw):
    a = {**OK, **kw}
    f, r = a["forecast"], a["resolve"]
    o = a["outcome"]
    return batch.WalkPlan.build_lagged(
        _T(a["off"], np.int64), _T(a["sid"], np.int32), _T(a["prob"], np.float64),
        o if isinstance(o, torch.Tensor) else _T(o, np.int8), a["S"],
        f if isinstance(f, torch.Tensor) else _T(f, np.int64), r if isinstance(r, torch.Tensor) else _T(r, np.int64))


def test_build_lagged_refuses_bad_times_before_the_library(golden_dir):
    with pytest.raises(ValueError, match="must not decrease"):
        _build(forecast=[T0, T0 + DAY, T0])
    with pytest.raises(ValueError, match="market 2 resolves before"):
        _build(resolve=[T0 + DAY, 0, T0 + DAY - 1])
    _check = batch._check_lag_times  # the resolve time of the unresolved market 1 is not looked at
    _check(_T(OK["forecast"], np.int64), _T([T0, -5, T0 + DAY], np.int64), _T(OK["outcome"], np.int8), 3)
    for name in ("forecast", "resolve"):
        with pytest.raises(ValueError, match=f"{name}_time_us must be int64 with one entry per market"):
            _build(**{name: OK[name][:2]})
        with pytest.raises(ValueError, match=f"{name}_time_us must be int64"):
            _build(**{name: torch.tensor(OK[name], dtype=torch.float64)})
        with pytest.raises(ValueError, match=f"{name}_time_us must be int64"):
            _build(**{name: torch.tensor([0, 1, 2], dtype=torch.int32)})
        with pytest.raises(ValueError, match=f"{name}_time_us must be int64"):
            _build(**{name: torch.tensor([OK[name]], dtype=torch.int64)})
    with pytest.raises(ValueError, match="int8"):
        _build(outcome=torch.tensor([1, -1, 0], dtype=torch.int64))
    with pytest.raises(ValueError, match="one entry per market"):
        _build(outcome=[1, -1])
    with pytest.raises(ValueError, match="n_sources"):
        _build(S=0)
    # the ordinary walk's fixture is no lagged batch: its market 6 is earlier than its market 5
    g = json.load(open(os.path.join(golden_dir, "walk_forward_small.json")))
    off, sid, prob = [0], [], []
    for mk in g["markets"]:
        sid += [s for s, _ in mk["signals"]]
        prob += [float(p) for _, p in mk["signals"]]
        off.append(len(sid))
    outcome = [-1 if mk["outcome"] is None else int(mk["outcome"]) for mk in g["markets"]]
    with pytest.raises(ValueError, match="market 6 is forecast before market 5"):
        _build(off=off, sid=sid, prob=prob, outcome=outcome, S=len(g["names"]), forecast=g["times_us"],
               resolve=g["times_us"])


def test_walk_forward_refuses_the_two_argument_conflicts():
    a = OK
    off, prob = _T(a["off"], np.int64), _T(a["prob"], np.float64)
    pairs, qstart, qpos, qentry, qlast, slast, nc = batch.WalkPlan.order(
        off, _T(a["sid"], np.int32), prob, _T(a["outcome"], np.int8), a["S"])
    plain = batch.WalkPlan(None, pairs, qstart, qpos, qentry, qlast, slast, nc, _T(a["outcome"], np.int8))
    lagged = batch.WalkPlan(None, pairs, qstart, qpos, qentry, qlast, slast, nc, _T(a["outcome"], np.int8),
                            _T(a["forecast"], np.int64), _T(a["resolve"], np.int64))
    assert lagged.lagged and not plain.lagged
    f64 = dict(dtype=torch.float64)
    table = batch.ReliabilityTable(torch.full((2,), 0.5, **f64), torch.full((2,), 0.25, **f64),
                                   torch.zeros(2, dtype=torch.int64), torch.ones(2, dtype=torch.uint8), ["a", "b"])
    mt = _T(a["forecast"], np.int64)
    for call in (lambda p, *t: batch.walk_forward(p, table, *t, offsets=off, prob=prob),
                 lambda p, *t: table.walk_forward(p, *t, offsets=off, prob=prob),
                 lambda p, *t: batch.walk_trace(p, table, *t),
                 lambda p, *t: batch.walk_sweep(p, table, *t, offsets=off, prob=prob, half_life_days=[30.0],
                                                min_rel=[0.1])):
        with pytest.raises(ValueError, match="carries its own times"):
            call(lagged, mt)
        with pytest.raises(ValueError, match="market_time_us is needed"):
            call(plain)
    with pytest.raises(ValueError, match="one entry per market"):
        batch.walk_forward(plain, table, mt[:2], offsets=off, prob=prob)


def _random_batch(seed, M=14, S=5):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6, M)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    sid = rng.integers(0, S, int(off[-1])).astype(np.int32)
    prob = np.round(rng.random(int(off[-1])), 3)
    outcome = rng.integers(-1, 2, M).astype(np.int8)
    state = (rng.random(S), rng.random(S), T0 - rng.integers(0, 60, S) * DAY, (rng.random(S) < 0.7).astype(np.uint8))
    forecast = T0 + np.sort(rng.integers(0, 8, M)) * 5 * DAY  # ties included
    return off, sid, prob, outcome, S, state, forecast


@pytest.mark.parametrize("seed", range(3))
def test_event_loop_without_lag_is_the_ordinary_walk(seed):
    off, sid, prob, outcome, S, state, forecast = _random_batch(seed)
    assert (np.diff(forecast) == 0).any() and (outcome >= 0).any() and (outcome < 0).any()
    for all_present in (True, False):
        exp, exp_state = walk_ref(off, sid, prob, outcome, S, *state, forecast, all_present=all_present)
        got, got_state = walk_lag_ref(off, sid, prob, outcome, S, *state, forecast, forecast, all_present=all_present)
        for k in exp:
            assert np.array_equal(got[k], exp[k], equal_nan=exp[k].dtype.kind == "f"), k
        for name, g, e in zip(("rel", "conf", "t_us", "present"), got_state, exp_state):
            assert g.dtype == e.dtype and np.array_equal(g, e), name


def test_a_lag_changes_what_later_markets_read():
    """The model is not vacuous: delaying every resolution past the last forecast leaves every
    market reading the start table, and the final rows carry the resolve times."""
    off, sid, prob, outcome, S, state, forecast = _random_batch(1)
    late = forecast[-1] + (1 + np.arange(len(forecast))) * DAY
    got, got_state = walk_lag_ref(off, sid, prob, outcome, S, *state, forecast, late)
    none, _ = walk_lag_ref(off, sid, prob, np.full_like(outcome, -1), S, *state, forecast, late)
    for k in ("consensus", "confidence", "total_weight", "rel_read", "conf_read"):
        assert np.array_equal(got[k], none[k], equal_nan=True), k
    nolag, _ = walk_lag_ref(off, sid, prob, outcome, S, *state, forecast, forecast)
    assert not np.array_equal(nolag["rel_read"], got["rel_read"])
    mk = np.repeat(np.arange(len(off) - 1), np.diff(off))
    for s in range(S):
        ms = mk[(sid == s) & (outcome[mk] >= 0)]
        assert got_state[2][s] == (late[ms.max()] if len(ms) else state[2][s]), s


def test_event_loop_reproduces_the_reference_fixture(golden_dir):
    g, (off, sid, prob, outcome, S), state, forecast, resolve = load_fixture(golden_dir)
    names = g["names"]
    rel, conf, t_us, present = state
    assert len(g["markets"]) == 10 and S == 6 and (t_us[present == 1] == np.iinfo(np.int64).min).sum() == 1
    assert present[5] == 0 and set(rel[present == 1]) >= {0.0, 1.0}
    res = [m for m in range(10) if outcome[m] >= 0]
    assert len(res) == 9 and (np.diff(forecast) >= 0).all() and (np.diff(forecast) == 0).sum() == 1
    assert all(resolve[m] >= forecast[m] for m in res)
    assert any(resolve[a] > resolve[b] for a in res for b in res if a < b)          # settles out of forecast order
    assert any(resolve[a] == forecast[b] for a in res for b in range(10) if a < b)  # visible on equality
    assert any(resolve[a] == forecast[b] for a in res for b in range(10) if a > b)  # not visible on equality
    assert max(resolve[m] for m in res) > forecast[-1]
    assert any(len({s for s, _ in mk["signals"]}) < len(mk["signals"]) for mk in g["markets"])
    exp, final = walk_lag_ref(off, sid, prob, outcome, S, *state, forecast, resolve)
    R = lambda x: repr(float(x))  # noqa: E731
    for m, r in enumerate(g["results"]):
        a, u = off[m], int(exp["n_unique"][m])
        assert R(exp["consensus"][m]) == r["consensus"] and R(exp["confidence"][m]) == r["confidence"], m
        assert R(exp["total_weight"][m]) == r["totalWeight"], m
        assert [[R(x), R(y)] for x, y in zip(exp["rel_read"][a:a + u], exp["conf_read"][a:a + u])] == \
            [x[1:] for x in r["read"]], m
        assert [[names[i & 0x7FFFFFFF], R(x), R(y)] for i, x, y in
                zip(exp["usid"][a:a + u], exp["weight"][a:a + u], exp["nweight"][a:a + u])] == r["sourceWeights"], m
    from bayesian_engine.timeutil import iso_to_us
    rows = {n: (r, c, ts) for n, r, c, ts in g["final"]}
    assert set(rows) == set(names)
    for s, n in enumerate(names):
        assert (R(final[0][s]), R(final[1][s]), int(final[2][s])) == (*rows[n][:2], iso_to_us(rows[n][2])), n
