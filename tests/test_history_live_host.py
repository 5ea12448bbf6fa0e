"""Host checks of the live consensus history: the event loop of
tests/history_live_ref.py reproduces the fixture recorded from the reference, the prefix expansion
run through the lagged walk's event loop gives the same points (which grounds the GPU cross-checks
against ``walk_forward`` on the expanded batch), ``LivePlan.build`` refuses bad batches from torch
checks before the library is touched, and the C entries refuse bad arguments before any launch.
None of it needs a GPU."""
import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from history_live_ref import FIELDS, expand_prefixes, history_live_ref, load_fixture
from walk_lag_ref import walk_lag_ref

DAY = 86_400_000_000
T0 = 1_790_000_000_000_000


def random_batch(seed, M=None, S=None, max_len=6):
    """A small live batch: arrivals ascend inside a market and tie often, resolve times sit on
    arrival times of other markets often, markets are not in time order."""
    rng = np.random.default_rng(seed)
    M = int(rng.integers(6, 12)) if M is None else M
    S = int(rng.integers(3, 7)) if S is None else S
    lens = rng.integers(0, max_len + 1, M)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    arrival = np.zeros(n, np.int64)
    for m in range(M):
        arrival[off[m]:off[m + 1]] = T0 + np.sort(rng.integers(0, 10, lens[m])) * DAY
    outcome = rng.integers(-1, 2, M).astype(np.int8)
    last = np.array([arrival[off[m + 1] - 1] if lens[m] else T0 for m in range(M)], np.int64)
    resolve = last + rng.choice(np.array([0, 0, DAY, 2 * DAY, 3 * DAY + 1, 30 * DAY]), M)
    state = (rng.random(S), rng.random(S), T0 - rng.integers(0, 60, S) * DAY, (rng.random(S) < 0.7).astype(np.uint8))
    return dict(off=off, sid=rng.integers(0, S, n).astype(np.int32), prob=np.round(rng.random(n), 3), outcome=outcome,
                S=S, arrival=arrival, resolve=resolve, state=state)


def expected(b, **kw):
    return history_live_ref(b["off"], b["sid"], b["prob"], b["outcome"], b["S"], *b["state"], b["arrival"],
                            b["resolve"], **kw)


def test_the_event_loop_reproduces_the_fixture(golden_dir):
    g, (off, sid, prob, outcome, S), state, arrival, resolve = load_fixture(golden_dir)
    out, final = history_live_ref(off, sid, prob, outcome, S, *state, arrival, resolve)
    for m, points in enumerate(g["results"]):
        assert len(points) == off[m + 1] - off[m]
        for k, r in enumerate(points):
            at = int(off[m]) + k
            null = r["consensus"] is None
            assert null == bool(out["total_weight"][at] == 0), (m, k)
            assert null or repr(float(out["consensus"][at])) == r["consensus"], (m, k)
            assert repr(float(out["confidence"][at])) == r["confidence"], (m, k)
            assert repr(float(out["total_weight"][at])) == r["totalWeight"], (m, k)
            assert int(out["n_unique"][at]) == r["sourceCount"], (m, k)
    from bayesian_engine.timeutil import iso_to_us
    rows = {n: (r, c, ts) for n, r, c, ts in g["final"]}
    for s, n in enumerate(g["names"]):
        assert (repr(float(final[0][s])), repr(float(final[1][s]))) == rows[n][:2], n
        assert final[2][s] == iso_to_us(rows[n][2]) and final[3][s] == 1, n


def test_the_fixture_moves_where_it_should(golden_dir):
    """Market 4 resolves between the last two arrivals of market 1, which shares its sources: with
    market 4 left unresolved only market 1's last point changes."""
    g, (off, sid, prob, outcome, S), state, arrival, resolve = load_fixture(golden_dir)
    live, _ = history_live_ref(off, sid, prob, outcome, S, *state, arrival, resolve)
    a, b = int(off[1]), int(off[2])
    assert arrival[b - 2] < resolve[4] < arrival[b - 1] and set(sid[off[4]:off[5]]) & set(sid[a:b])
    without = outcome.copy()
    without[4] = -1
    other, _ = history_live_ref(off, sid, prob, without, S, *state, arrival, resolve)
    for f in ("consensus", "confidence", "total_weight"):
        assert np.array_equal(live[f][a:b - 1], other[f][a:b - 1]) and live[f][b - 1] != other[f][b - 1], f


@pytest.mark.parametrize("seed", range(6))
def test_prefix_expansion_through_the_lagged_event_loop_equals_the_live_one(seed):
    b = random_batch(seed)
    live, live_state = expected(b)
    xoff, xsid, xprob, xout, fc, rs, point = expand_prefixes(b["off"], b["sid"], b["prob"], b["outcome"], b["arrival"],
                                                            b["resolve"])
    assert (np.diff(fc) >= 0).all() and (point >= 0).sum() == len(b["sid"])
    lag, lag_state = walk_lag_ref(xoff, xsid, xprob, xout, b["S"], *b["state"], fc, rs)
    sel = point >= 0
    for f in FIELDS:
        assert np.array_equal(lag[f][sel], live[f][point[sel]]), (seed, f)
    for x, y in zip(lag_state, live_state):
        assert np.array_equal(x, y), seed


# ------------------------------------------------------------------------------ LivePlan.build
def _cpu(b, **over):
    t = dict(offsets=b["off"], sid=b["sid"], prob=b["prob"], outcome=b["outcome"], arrival=b["arrival"],
             resolve=b["resolve"])
    t.update(over)
    T = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))  # noqa: E731
    return (T(t["offsets"]), T(t["sid"]), T(t["prob"]), T(t["outcome"]), b["S"], T(t["arrival"]), T(t["resolve"]))


def test_live_plan_refuses_bad_batches_before_the_library_is_touched():
    b = random_batch(3, M=8, S=4)
    assert (np.diff(b["off"]) >= 2).sum() >= 2
    n, M = len(b["sid"]), len(b["outcome"])
    # a good batch gets as far as the library: without a GPU that is NativeUnavailable, never a ValueError
    if not torch.cuda.is_available():
        with pytest.raises(N.NativeUnavailable):
            batch.LivePlan.build(*_cpu(b))
    for over, match in ((dict(arrival=b["arrival"].astype(np.int32)), "arrival_us must be int64"),
                        (dict(arrival=b["arrival"][:-1]), f"arrival_us must be int64 with one entry per signal \\({n}\\)"),
                        (dict(resolve=b["resolve"].astype(np.float64)), "resolve_time_us must be int64"),
                        (dict(resolve=b["resolve"][:-1]), f"one entry per market \\({M}\\)"),
                        (dict(outcome=b["outcome"].astype(np.int32)), "outcome must be int8"),
                        (dict(outcome=b["outcome"][:-1]), "outcome must have one entry per market"),
                        (dict(prob=b["prob"][:-1]), "sid and prob differ"),
                        (dict(offsets=b["off"][::-1].copy()), "offsets must rise")):
        with pytest.raises(ValueError, match=match):
            batch.LivePlan.build(*_cpu(b, **over))
    with pytest.raises(ValueError, match="n_sources"):
        args = list(_cpu(b))
        args[4] = 0
        batch.LivePlan.build(*args)
    # an arrival that decreases inside a market: the signal and the market are named
    m = int(np.flatnonzero(np.diff(b["off"]) >= 2)[1])
    i = int(b["off"][m]) + 1
    bad = b["arrival"].copy()
    bad[i] = bad[i - 1] - 1
    with pytest.raises(ValueError, match=f"signal {i} \\(market {m}\\) arrived before signal {i - 1}"):
        batch.LivePlan.build(*_cpu(b, arrival=bad))
    # the first signal of a market may be earlier than the last of the market before it
    first = int(b["off"][m])
    ok = b["arrival"].copy()
    ok[first:int(b["off"][m + 1])] -= 400 * DAY
    batch._check_live_times(torch.from_numpy(b["off"]), torch.from_numpy(np.diff(b["off"])),
                            torch.from_numpy(np.full(M, -1, np.int8)), torch.from_numpy(ok), torch.from_numpy(b["resolve"]))
    # a resolved market that resolves before its last arrival is named; an unresolved one is not looked at
    res = np.flatnonzero((np.diff(b["off"]) > 0) & (b["outcome"] >= 0))
    unres = np.flatnonzero((np.diff(b["off"]) > 0) & (b["outcome"] < 0))
    assert len(res) >= 2 and len(unres)
    m = int(res[1])
    early = b["resolve"].copy()
    early[m] = b["arrival"][b["off"][m + 1] - 1] - 1
    early[unres] = 0
    with pytest.raises(ValueError, match=f"market {m} resolves before its last signal arrives"):
        batch.LivePlan.build(*_cpu(b, resolve=early))
    exact = b["resolve"].copy()
    exact[m] = b["arrival"][b["off"][m + 1] - 1]  # exactly at the last arrival: fine
    exact[unres] = 0
    batch._check_live_times(torch.from_numpy(b["off"]), torch.from_numpy(np.diff(b["off"])),
                            torch.from_numpy(b["outcome"]), torch.from_numpy(b["arrival"]), torch.from_numpy(exact))


# ------------------------------------------------------------------------------ the C entries
def _live(**over):
    a = dict(offsets=1, n_markets=1, sid=1, prob=1, n_signals=1, states=16, bits=None, n_sources=1, list=None,
             n_list=0, bins_host=None, bins_dev=None, max_len=8, cons=1, conf=1, tot=1, nu=1, arrival=1, start=1,
             bit_market=1, n_bits=1, resolve=1, rel=1, tconf=1, t_us=1, present=None, hl=30.0, mr=0.1, dr=0.5, dc=0.25,
             stream=None)
    a.update(over)
    return N.load_library().bce_consensus_history_live(*a.values())


def _trace_all(**over):
    a = dict(bits=1, n_bits=1, start=1, order=1, n_touched=1, n_long=0, chunk_start=None, n_chunks=0, chunk_bits=256,
             n_sources=1, rel=1, conf=1, present=None, dr=0.5, dc=0.25, states=16, stream=None)
    a.update(over)
    return N.load_library().bce_settle_trace_all(*a.values())


def test_argument_errors_need_no_gpu():
    """Every refusal comes before anything touches the GPU (the pointers here are never read)."""
    lib = N.load_library()
    for over in (dict(offsets=None), dict(sid=None), dict(prob=None), dict(cons=None), dict(conf=None), dict(tot=None),
                 dict(nu=None), dict(n_markets=-1), dict(n_signals=-1), dict(n_sources=-1), dict(n_sources=0),
                 dict(n_list=-1), dict(max_len=-1), dict(max_len=4097), dict(states=8), dict(states=None),
                 dict(bins_host=1), dict(bins_host=1, bins_dev=1, list=1), dict(arrival=None), dict(start=None),
                 dict(bit_market=None), dict(resolve=None), dict(rel=None), dict(tconf=None), dict(t_us=None),
                 dict(n_bits=-1)):
        assert _live(**over) == -1, over
        assert b"history_live" in lib.bce_last_error(), over
    assert _live(n_markets=0) == 0 and _live(n_signals=0, sid=None, prob=None, cons=None) == 0  # nothing to do
    for over in (dict(bits=None), dict(start=None), dict(order=None), dict(rel=None), dict(conf=None),
                 dict(states=None), dict(states=8), dict(n_bits=-1), dict(n_touched=-1), dict(n_sources=0),
                 dict(n_touched=2), dict(n_long=2), dict(n_long=1, n_chunks=1), dict(n_long=1, n_chunks=1, chunk_start=1,
                                                                                    chunk_bits=32),
                 dict(n_long=1, n_chunks=0, chunk_start=1)):
        assert _trace_all(**over) == -1, over
        assert b"settle_trace_all" in lib.bce_last_error(), over
    assert _trace_all(n_touched=0) == 0 and _trace_all(n_bits=0, states=None) == 0  # nothing to do


def test_names_are_reachable():
    for name in ("LivePlan", "live_trace", "walk_history_live"):
        assert getattr(batch, name) is getattr(batch.live, name), name
    assert "bce_consensus_history_live" in N.EXPORTED and "bce_settle_trace_all" in N.EXPORTED
    assert "live" in batch.__doc__.split("listed before it:")[1]
    assert "walk_history_live" in batch.walk_history.__doc__
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore
    assert callable(NamespacedReliabilityStore.walk_history_live)
