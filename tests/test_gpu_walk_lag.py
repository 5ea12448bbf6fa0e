"""GPU checks of walk-forward with resolution lag (batch.WalkPlan.build_lagged, bce_walk_lag_queries,
bce_walk_read_lag and the store layers): every market's consensus, every slot's weight, every
entry's read state and the final table -- stamps included -- equal the event loop of
tests/walk_lag_ref.py exactly (``==``; NaN-aware) and the fixture recorded from the reference
itself; without lag the plan and the walk equal the ordinary ones byte for byte."""
import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from oracle import oracle as orc
from walk_lag_ref import load_fixture, walk_lag_ref

pytestmark = pytest.mark.gpu

OFF = batch.SETTLE_LONG_OFF
MASK = 0x7FFFFFFF
DAY = 86_400_000_000
HOUR = 3_600_000_000
T0 = 1_790_000_000_000_000
PATHS = ({}, {"long_min": OFF}, {"long_min": 1, "chunk_bits": 64})


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _args(b):
    return (_T(np.asarray(b["off"], np.int64)), _T(np.asarray(b["sid"], np.int32)),
            _T(np.asarray(b["prob"], np.float64)), _T(np.asarray(b["outcome"], np.int8)), b["S"])


def _lagged(b, forecast=None, resolve=None, **kw):
    return batch.WalkPlan.build_lagged(*_args(b), _T(b["forecast"] if forecast is None else forecast),
                                       _T(b["resolve"] if resolve is None else resolve), **kw)


def _table(state):
    rel, conf, t_us, present = state
    return batch.ReliabilityTable(_T(np.array(rel, np.float64)), _T(np.array(conf, np.float64)),
                                  _T(np.array(t_us, np.int64)), _T(np.array(present, np.uint8)), [""] * len(rel))


def _run(plan, b, mtime=None, **kw):
    """(result fields as numpy, relconf by entry, final table arrays)."""
    table = _table(b["state"])
    mt = () if mtime is None else (_T(np.asarray(mtime, np.int64)),)
    off, prob = _T(np.asarray(b["off"], np.int64)), _T(np.asarray(b["prob"], np.float64))
    res = batch.walk_forward(plan, table, *mt, offsets=off, prob=prob, **kw)
    trace_kw = {k: v for k, v in kw.items() if k in ("all_present", "long_min", "chunk_bits")}
    wt, _ = batch.walk_trace(plan, _table(b["state"]), *mt, **trace_kw)  # the read states, from a fresh table
    torch.cuda.synchronize()
    out = {k: getattr(res, k).cpu().numpy() for k in ("consensus", "confidence", "total_weight", "n_unique", "usid",
                                                      "weight", "nweight")}
    out["scope_present"] = res.scope_present.cpu().numpy()
    out["total"], out["correct"] = res.total.cpu().numpy(), res.correct.cpu().numpy()
    final = tuple(x.cpu().numpy() for x in (table.rel, table.conf, table.t_us, table.present))
    return out, wt.relconf[:plan.pairs.n_entries].cpu().numpy(), final


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _slots(off, n_unique):
    return np.concatenate([np.arange(a, a + u) for a, u in zip(off[:-1], n_unique)] + [np.zeros(0, np.int64)])


def _compare(got, relconf, plan, exp, off, what=""):
    """Every market and every entry against the event loop's output."""
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


def _same_bytes(a, b, off, what=""):
    """Two _run results: every written byte equal (slots past a market's unique sources are not written)."""
    slots = _slots(off, a[0]["n_unique"])
    for k in a[0]:
        pick = slots if k in ("usid", "weight", "nweight") else slice(None)
        assert a[0][k][pick].tobytes() == b[0][k][pick].tobytes(), (what, k)
    assert a[1].tobytes() == b[1].tobytes(), what
    for x, y in zip(a[2], b[2]):
        assert x.tobytes() == y.tobytes(), what


# ----------------------------------------------------------------------------- edge batch
def _edge_batch():
    """48 markets, 8 sources, 0..6 signals of sources 1..6 per market (market 20 is empty), plus up
    to 6 signals of source 0 in every other market: its chain is longer than 256 bits.  Source 3:
    a row without a timestamp; 5 and 6: no row; 7: no row, seen in unresolved markets only.
    Forecast times come in tied groups of 2 and 3; the lags are zero, an hour, exactly up to the
    forecast time of the next group and of the one after it (so two markets resolve at one time),
    nine days, and past the last forecast."""
    rng = np.random.default_rng(11)
    S, M = 8, 48
    unresolved = (5, 17, 33)
    outcome = rng.integers(0, 2, M).astype(np.int8)
    outcome[list(unresolved)] = -1
    markets = []
    for m in range(M):
        if m == 20:
            markets.append([])
            continue
        sig = [(int(rng.integers(1, 7)), float(np.round(rng.random(), 3))) for _ in range(int(rng.integers(0, 7)))]
        sig += [(0, float(np.round(rng.random(), 3))) for _ in range(3 if m == 8 else 5 if m == 30 else 6)]
        if m in unresolved:
            sig += [(7, 0.9), (7, 0.2)]
        order = rng.permutation(len(sig))
        markets.append([sig[i] for i in order])
    markets[9].append((3, 0.5))  # exactly on the threshold: votes True
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in markets])
    sid = np.array([s for x in markets for s, _ in x], np.int32)
    prob = np.array([p for x in markets for _, p in x], np.float64)
    group = np.repeat(np.arange(M), np.tile([2, 3], M)[:M])[:M]  # 0 0 1 1 1 2 2 3 3 3 ...
    gtime = T0 + np.arange(group.max() + 3) * 2 * DAY + 123
    forecast = gtime[group]
    kind = np.arange(M) % 6
    resolve = np.select([kind == 1, kind == 2, kind == 3, kind == 4],
                        [forecast + HOUR, gtime[group + 1], gtime[group + 2], forecast + 9 * DAY + 7], forecast)
    present = np.array([1, 1, 1, 1, 1, 0, 0, 0], np.uint8)
    rel = np.array([0.9, 0.05, 1.0, 0.66, 0.37, 0.5, 0.5, 0.5])
    conf = np.array([0.3, 0.99, 1.0, 0.41, 0.5, 0.25, 0.25, 0.25])
    t_us = np.array([T0 - 3 * DAY, T0 - 40 * DAY, T0 + DAY, orc.NO_TIMESTAMP, T0 - 90 * DAY, orc.NO_TIMESTAMP,
                     orc.NO_TIMESTAMP, orc.NO_TIMESTAMP], np.int64)
    # what the batch is meant to hold
    res = np.flatnonzero(outcome >= 0)
    mk = np.repeat(np.arange(M), np.diff(off))
    assert ((sid == 0) & (outcome[mk] >= 0)).sum() > 256
    assert set(np.bincount(group)[:-1].tolist()) == {2, 3}
    assert (np.diff(forecast) >= 0).all() and (resolve[res] >= forecast[res]).all()
    pairs = [(a, b) for a in res for b in range(M) if resolve[a] == forecast[b] and a != b]
    assert any(a < b for a, b in pairs) and any(a > b for a, b in pairs)  # equality, either side of the reader
    assert any(forecast[a] < forecast[b] and resolve[a] == forecast[b] for a, b in pairs)
    assert any(resolve[a] == resolve[b] and forecast[a] != forecast[b] for a in res for b in res if a < b)
    assert any(resolve[a] > resolve[b] for a in res for b in res if a < b)
    assert (resolve[res] > forecast[-1]).any()
    assert set(mk[sid == 7].tolist()) <= set(unresolved) and {5, 6} <= set(sid[outcome[mk] >= 0].tolist())
    return dict(off=off, sid=sid, prob=prob, outcome=outcome, S=S, forecast=forecast, resolve=resolve,
                state=(rel, conf, t_us, present))


def _random(seed):
    rng = np.random.default_rng(seed)
    M, S = int(rng.integers(20, 40)), int(rng.integers(3, 9))
    lens = rng.integers(0, 8, M)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    forecast = T0 + np.sort(rng.integers(0, 12, M)) * DAY
    lag = rng.choice(np.array([0, 0, HOUR, DAY, 2 * DAY, 5 * DAY + 1, 40 * DAY]), M)
    state = (rng.random(S), rng.random(S), T0 - rng.integers(0, 60, S) * DAY, (rng.random(S) < 0.7).astype(np.uint8))
    return dict(off=off, sid=rng.integers(0, S, n).astype(np.int32), prob=np.round(rng.random(n), 3),
                outcome=rng.integers(-1, 2, M).astype(np.int8), S=S, forecast=forecast, resolve=forecast + lag,
                state=state)


@pytest.fixture(scope="module")
def edge():
    return _edge_batch()


def _expected(b, all_present):
    return walk_lag_ref(b["off"], b["sid"], b["prob"], b["outcome"], b["S"], *b["state"], b["forecast"],
                        b["resolve"], all_present=all_present)


@pytest.mark.parametrize("all_present", [True, False])
def test_edge_batch(edge, all_present):
    e = edge
    exp, exp_state = _expected(e, all_present)
    assert (exp["usid"][_slots(e["off"], exp["n_unique"])] < 0).any() != all_present
    plan = _lagged(e)
    assert plan.lagged and plan.settle.chunks(batch.WALK_LONG_MIN, batch.WALK_CHUNK_BITS)[0] == 1  # the long path runs
    runs = [_run(plan, e, all_present=all_present, **kw) for kw in PATHS]
    for kw, run in zip(PATHS, runs):
        _compare(run[0], run[1], plan, exp, e["off"], f"edge {kw} {all_present}")
        _same_state(run[2], exp_state, f"edge {kw}")
        _same_bytes(run, runs[0], e["off"], f"edge {kw}")
    N.check_faults(_dev(), "edge batch")


@pytest.mark.parametrize("seed", range(3))
def test_random_batches(seed):
    b = _random(seed)
    plan = _lagged(b)
    for all_present in (True, False):
        exp, exp_state = _expected(b, all_present)
        runs = [_run(plan, b, all_present=all_present, **kw) for kw in PATHS]
        for kw, run in zip(PATHS, runs):
            _compare(run[0], run[1], plan, exp, b["off"], f"seed {seed} {kw} {all_present}")
            _same_state(run[2], exp_state, f"seed {seed} {kw}")
            _same_bytes(run, runs[0], b["off"], f"seed {seed} {kw}")
    N.check_faults(_dev(), "random batches")


def test_single_market_and_empty_batch_of_one():
    state = (np.array([0.8, 0.2]), np.array([0.5, 0.6]), np.array([T0 - DAY, T0 - 2 * DAY], np.int64),
             np.ones(2, np.uint8))
    one = ([0, 3], [1, 0, 1], [0.7, 0.4, 0.2])
    for off, sid, prob, outcome in ((*one, [1]), (*one, [-1]), ([0, 0], [], [], [1])):
        b = dict(off=np.array(off, np.int64), sid=np.array(sid, np.int32), prob=np.array(prob, np.float64),
                 outcome=np.array(outcome, np.int8), S=2, forecast=np.array([T0], np.int64),
                 resolve=np.array([T0 + 3 * DAY], np.int64), state=state)
        plan = _lagged(b)
        got, relconf, final = _run(plan, b)
        exp, exp_state = _expected(b, True)
        _compare(got, relconf, plan, exp, b["off"], f"M=1 {outcome}")
        _same_state(final, exp_state, f"M=1 {outcome}")
        if outcome == [1] and sid:  # settled three days after it was read, and stamped then
            assert (final[2] == T0 + 3 * DAY).all() and (plan.qpos == 0).all()
    N.check_faults(_dev(), "M = 1")


def test_without_lag_the_plan_and_the_walk_are_the_ordinary_ones(edge):
    e = edge
    f = e["forecast"]
    lag = _lagged(e, resolve=f)
    plain = batch.WalkPlan.build(*_args(e))
    for name in ("qstart", "qpos", "qentry", "qlast", "slast"):
        a, b = getattr(lag, name), getattr(plain, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    for name in ("bits", "start", "order", "total", "correct"):
        assert torch.equal(getattr(lag.settle, name), getattr(plain.settle, name)), name
    assert lag.settle.n_bits == plain.settle.n_bits and np.array_equal(lag.settle.lens_desc, plain.settle.lens_desc)
    a, b = _run(lag, e), _run(plain, e, mtime=f)
    _same_bytes(a, b, e["off"], "no lag")
    # commit=False leaves the table's bytes alone
    dry = _table(e["state"])
    batch.walk_forward(lag, dry, offsets=_T(e["off"]), prob=_T(e["prob"]), commit=False)
    torch.cuda.synchronize()
    for x, before in zip((dry.rel, dry.conf, dry.t_us, dry.present), e["state"]):
        assert x.cpu().numpy().tobytes() == np.asarray(before, x.cpu().numpy().dtype).tobytes()
    dry = _table(e["state"])
    batch.walk_forward(_lagged(e), dry, offsets=_T(e["off"]), prob=_T(e["prob"]), commit=False)
    torch.cuda.synchronize()
    for x, before in zip((dry.rel, dry.conf, dry.t_us, dry.present), e["state"]):
        assert x.cpu().numpy().tobytes() == np.asarray(before, x.cpu().numpy().dtype).tobytes()
    N.check_faults(_dev(), "no lag")


@pytest.mark.parametrize("all_present", [True, False])
def test_both_read_entries_and_the_batch_read_write_the_same_bytes(edge, all_present):
    """bce_walk_read(t), bce_walk_read_lag(t, t) and batch._walk_read with an ordinary plan, from one trace."""
    e = edge
    plan = batch.WalkPlan.build(*_args(e))
    pp, E, M, S = plan.pairs, plan.pairs.n_entries, plan.pairs.n_markets, e["S"]
    assert not plan.lagged and E % 32 and (plan.qlast == -1).any() and (plan.qlast >= 0).any()
    for name, x in zip(("qstart", "qpos", "qentry", "qlast", "slast"), batch.WalkPlan.order(*_args(e))[1:6]):
        assert torch.equal(getattr(plan, name), x) and getattr(plan.queries, name) is getattr(plan, name), name
    table, mt = _table(e["state"]), _T(e["forecast"])
    trace = torch.full((E, 2), -3.0, dtype=torch.float64, device=_dev())
    batch._walk_settle_trace(plan, table, mt, trace, None, None)

    def outputs():
        return (torch.full((E, 2), -7.0, dtype=torch.float64, device=_dev()),
                torch.full(((E + 31) // 32,), 0x5A5A5A5A, dtype=torch.int32, device=_dev()),
                torch.full((E,), 77, dtype=torch.uint8, device=_dev()))

    def args(times, out):
        p = N.ptr
        return [E, p(pp.usid), p(pp.emarket), p(plan.qlast), p(trace), *[p(t) for t in times], M, p(table.rel),
                p(table.conf), p(table.t_us), p(table.present), S, batch.DECAY_HALF_LIFE_DAYS, batch.DECAY_MINIMUM,
                batch.DEFAULT_RELIABILITY, batch.DEFAULT_CONFIDENCE, int(not all_present), 0, *[p(x) for x in out],
                N.stream(_dev())]

    old, new, glue = outputs(), outputs(), outputs()
    L = N.lib()
    N.check(L.bce_walk_read(*args((mt,), old)), "bce_walk_read")
    N.check(L.bce_walk_read_lag(*args((mt, mt), new)), "bce_walk_read_lag")
    batch._walk_read(plan, table, mt, trace, *glue, all_present, batch.DECAY_HALF_LIFE_DAYS, batch.DECAY_MINIMUM)
    torch.cuda.synchronize()
    N.check_faults(_dev(), "the three reads")
    for name, x, y, z in zip(("relconf", "bits", "exists"), old, new, glue):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() == z.cpu().numpy().tobytes(), name
    assert set(old[2].cpu().numpy().tolist()) == {0, 1} and not (old[0] == -7.0).any()  # written, cold sources seen


def test_walk_sweep_on_a_lagged_plan_equals_every_point_run_alone(edge):
    e = edge
    plan = _lagged(e)
    off, prob, outcome = _T(e["off"]), _T(e["prob"]), _T(e["outcome"])
    table = _table(e["state"])
    hl, mr = [30.0, 5.0], [0.1, 0.4]
    scores, (cons, nulls) = batch.walk_sweep(plan, table, offsets=off, prob=prob, half_life_days=hl, min_rel=mr,
                                             keep_consensus=True)
    N.check_faults(_dev(), "walk_sweep")
    for x, before in zip((table.rel, table.conf, table.t_us, table.present), e["state"]):
        assert x.cpu().numpy().tobytes() == np.asarray(before, x.cpu().numpy().dtype).tobytes()  # never committed
    whole = batch.ScorePlan.whole(len(e["outcome"]), device=_dev())
    k = 0
    for h in hl:
        for m in mr:
            wt, _ = batch.walk_trace(plan, _table(e["state"]), half_life_days=h, min_rel=m)
            res = batch.consensus(off, plan.pairs.esid, prob, wt)
            assert torch.equal(res.consensus.view(torch.int64), cons[k].view(torch.int64)), (h, m)
            assert torch.equal(res.is_null(off), nulls[k]), (h, m)
            alone = batch.score(whole, res.consensus, outcome, valid=~res.is_null(off))
            for f in ("counts", "sums", "bin_n", "bin_pos", "bin_psum"):
                a, b = getattr(alone, f), getattr(scores, f)[k]
                assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (h, m, f)
            k += 1
    assert not torch.equal(cons[0], cons[2])  # the decay parameters do reach the consensus
    N.check_faults(_dev(), "walk_sweep")


# ----------------------------------------------------------------------------- the fault word
def _lag_queries(plan, e, bit_market, start):
    """One call of bce_walk_lag_queries on the plan's entries: (qpos, qlast, slast) as numpy."""
    pp, E, S, M = plan.pairs, plan.pairs.n_entries, plan.pairs.n_sources, plan.pairs.n_markets
    qpos = torch.full((E,), -7, dtype=torch.int64, device=_dev())
    qlast = torch.full((E,), -7, dtype=torch.int32, device=_dev())
    slast = torch.full((S,), -7, dtype=torch.int64, device=_dev())
    N.check(N.lib().bce_walk_lag_queries(E, N.ptr(plan.qentry), N.ptr(pp.usid), N.ptr(pp.emarket), E, N.ptr(start), S,
                                         N.ptr(bit_market), bit_market.numel(), N.ptr(plan.forecast_time_us),
                                         N.ptr(plan.resolve_time_us), M, N.ptr(qpos), N.ptr(qlast), N.ptr(slast),
                                         N.stream(_dev())), "bce_walk_lag_queries")
    return qpos, qlast, slast


def _bit_market(e):
    """The market of every chain bit in chain order, restated: (source, resolve time, market, position)."""
    mk = np.repeat(np.arange(len(e["off"]) - 1), np.diff(e["off"]))
    idx = np.flatnonzero(e["outcome"][mk] >= 0)
    order = np.lexsort((idx, mk[idx], e["resolve"][mk[idx]], e["sid"][idx]))
    return mk[idx][order].astype(np.int32)


def test_bad_chains_raise_the_fault_word_and_read_as_no_earlier_bit(edge):
    e = edge
    plan = _lagged(e)
    E, S = plan.pairs.n_entries, e["S"]
    bm = _bit_market(e)
    start = plan.settle.start.cpu().numpy()
    assert len(bm) == plan.settle.n_bits == start[-1]
    N.check_faults(_dev(), "clean slate")
    qpos, qlast, slast = _lag_queries(plan, e, _T(bm), plan.settle.start)
    N.check_faults(_dev(), "the plan's own arrays")
    assert torch.equal(qpos, plan.qpos) and torch.equal(qlast, plan.qlast) and torch.equal(slast, plan.slast)
    good = (qpos.cpu().numpy(), qlast.cpu().numpy(), slast.cpu().numpy())
    qsrc = plan.pairs.usid.cpu().numpy()[plan.qentry.cpu().numpy()]  # by query
    esrc = plan.pairs.usid.cpu().numpy()                             # by entry
    # a market outside the batch in the middle of source 0's chain: every query whose bisection probes it
    bad = bm.copy()
    mid = int(start[0] + (start[1] - start[0]) // 2)  # the first probe of every query of source 0
    for value in (len(e["outcome"]), -3):
        bad[mid] = value
        qpos, qlast, slast = _lag_queries(plan, e, _T(bad), plan.settle.start)
        with pytest.raises(N.BCEError):
            N.check_faults(_dev(), "corrupted bit_market")
        qpos, qlast, slast = qpos.cpu().numpy(), qlast.cpu().numpy(), slast.cpu().numpy()
        assert (qsrc == 0).sum() > 40 and (qpos[qsrc == 0] == 0).all() and (qlast[esrc == 0] == -1).all()
        assert np.array_equal(qpos[qsrc != 0], good[0][qsrc != 0])
        assert np.array_equal(qlast[esrc != 0], good[1][esrc != 0])
        assert np.array_equal(slast, good[2])  # the chain's last bit is intact
    # a start that is no range: source 2's chain ends before it begins, source 4's runs past the bits
    for s, (lo, hi) in ((2, (start[3], start[2])), (4, (start[4], len(bm) + 1))):
        st = start.copy()
        st[s], st[s + 1] = lo, hi
        assert lo > hi or hi > len(bm)
        qpos, qlast, slast = _lag_queries(plan, e, _T(bm), _T(st))
        with pytest.raises(N.BCEError):
            N.check_faults(_dev(), "start is no range")
        qpos, qlast, slast = qpos.cpu().numpy(), qlast.cpu().numpy(), slast.cpu().numpy()
        assert (qpos[qsrc == s] == 0).all() and (qlast[esrc == s] == -1).all() and slast[s] == -1
        assert (good[0][qsrc == s] > 0).any()
    N.check_faults(_dev(), "fault word is cleared")


def test_bad_arguments_are_refused_before_any_launch(edge):
    plan = _lagged(edge)
    pp, E, S, M = plan.pairs, plan.pairs.n_entries, edge["S"], len(edge["outcome"])
    bm = _T(_bit_market(edge))
    L = N.lib()
    full = [E, N.ptr(plan.qentry), N.ptr(pp.usid), N.ptr(pp.emarket), E, N.ptr(plan.settle.start), S, N.ptr(bm),
            bm.numel(), N.ptr(plan.forecast_time_us), N.ptr(plan.resolve_time_us), M, N.ptr(plan.qpos.clone()),
            N.ptr(plan.qlast.clone()), N.ptr(plan.slast.clone()), N.stream(_dev())]
    for at, value in ((0, -1), (0, E + 1), (6, 0), (8, -1), (11, 0), (5, None), (7, None), (1, None), (12, None),
                      (14, None)):
        args = list(full)
        args[at] = value
        assert L.bce_walk_lag_queries(*args) == -1, at
        assert b"walk_lag_queries" in L.bce_last_error()
    N.check_faults(_dev(), "argument errors launch nothing")


def test_out_of_range_sid_raises_and_is_clamped(edge):
    e = edge
    mk = np.repeat(np.arange(len(e["off"]) - 1), np.diff(e["off"]))
    for where in (int(np.flatnonzero(e["outcome"][mk] >= 0)[4]), int(np.flatnonzero(e["outcome"][mk] < 0)[1])):
        b = dict(e, sid=e["sid"].copy())
        b["sid"][where] = e["S"] + 5
        N.check_faults(_dev(), "clean slate")
        with pytest.raises(N.BCEError, match="sid"):
            _lagged(b)
        N.check_faults(_dev(), "fault word is cleared")
        plan = _lagged(b, check=False)
        got, relconf, final = _run(plan, b)
        with pytest.raises(N.BCEError, match="sid"):
            N.check_faults(_dev(), "walk_forward")
        exp, exp_state = _expected(b, True)  # the stray signal went to the clamped row
        _compare(got, relconf, plan, exp, b["off"], "clamped sid")
        _same_state(final, exp_state, "clamped sid")
    N.check_faults(_dev(), "clamped sid")


# ----------------------------------------------------------------------------- golden fixture
def _check_dicts(results, g):
    for m, (res, exp) in enumerate(zip(results, g["results"])):
        assert (None if res["consensus"] is None else repr(res["consensus"])) == exp["consensus"], m
        assert repr(res["confidence"]) == exp["confidence"], m
        assert repr(res["normalization"]["totalWeight"]) == exp["totalWeight"], m
        assert [[w["sourceId"], repr(w["weight"]), repr(w["normalizedWeight"])] for w in res["sourceWeights"]] == \
            exp["sourceWeights"], m
        assert res["diagnostics"]["uniqueSources"] == res["normalization"]["sourceCount"] == len(exp["read"])


def test_fixture_through_the_batch_call(golden_dir):
    from bayesian_engine.timeutil import iso_to_us

    g, (off, sid, prob, outcome, S), state, forecast, resolve = load_fixture(golden_dir)
    b = dict(off=off, sid=sid, prob=prob, outcome=outcome, S=S, forecast=forecast, resolve=resolve, state=state)
    plan = _lagged(b)
    for kw in PATHS:
        got, relconf, final = _run(plan, b, **kw)
        uoff = plan.pairs.uoffsets.cpu().numpy()
        for m, r in enumerate(g["results"]):  # the reference's own numbers
            null = r["consensus"] is None
            assert null == bool(got["total_weight"][m] == 0)
            assert null or repr(float(got["consensus"][m])) == r["consensus"], m
            assert repr(float(got["confidence"][m])) == r["confidence"], m
            assert repr(float(got["total_weight"][m])) == r["totalWeight"], m
            ent = slice(int(uoff[m]), int(uoff[m + 1]))
            assert [[repr(float(x)), repr(float(y))] for x, y in relconf[ent]] == [x[1:] for x in r["read"]], m
        rows = {n: (r, c, ts) for n, r, c, ts in g["final"]}
        for s, n in enumerate(g["names"]):
            assert (repr(float(final[0][s])), repr(float(final[1][s]))) == rows[n][:2], n
            assert got["total"][s] > 0 and final[2][s] == iso_to_us(rows[n][2]), n
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

    g = load_fixture(golden_dir)[0]
    store = NamespacedReliabilityStore(str(tmp_path / "lag.db"))
    _seed_store(store, g)
    before = _rows(store, g["scope"])
    kw = dict(domain=g["domain"], resolve_times=g["resolve_times"])
    dry, dsum = store.walk_forward(_fixture_markets(g), g["forecast_times"], dry_run=True, **kw)
    assert _rows(store, g["scope"]) == before  # dry run: the database is untouched
    wet, wsum = store.walk_forward(_fixture_markets(g), g["forecast_times"], **kw)
    assert dry == wet and dsum == wsum
    _check_dicts(wet, g)
    assert _rows(store, g["scope"]) == g["final"]  # updated_at: the resolve time of each source's last settling market
    assert {n: [repr(r.reliability), repr(r.confidence), r.updated_at] for n, r in wsum.records.items()} == \
        {row[0]: row[1:] for row in g["final"]}
    with pytest.raises(ValueError, match="resolve_times has 3 entries"):
        store.walk_forward(_fixture_markets(g), g["forecast_times"], domain=g["domain"], resolve_times=["", "", ""])
    late = list(g["resolve_times"])
    late[3] = g["forecast_times"][2]  # before its own forecast
    with pytest.raises(ValueError, match="market 3 resolves before"):
        store.walk_forward(_fixture_markets(g), g["forecast_times"], domain=g["domain"], resolve_times=late)
    scores = store.sweep_decay(_fixture_markets(g), g["forecast_times"], [30.0], [0.1], domain=g["domain"],
                               resolve_times=g["resolve_times"])
    assert int(scores.counts[0, 0, 0]) == sum(r["consensus"] is not None and mk["outcome"] is not None
                                              for r, mk in zip(g["results"], g["markets"]))
    store.close()
    N.check_faults(_dev(), "namespaced store")


def test_fixture_through_the_aggregator(golden_dir, tmp_path):
    from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    g = load_fixture(golden_dir)[0]
    insertion = [7, 2, 9, 0, 3, 5, 4, 1, 8, 6]  # not the time order; 3 and 4 tie, and 3 stands first as recorded
    assert insertion.index(3) < insertion.index(4)
    assert sorted(range(10), key=lambda i: (g["forecast_times_us"][i], insertion.index(i))) == list(range(10))

    def fill(swap=None):
        ms = MarketStore()
        for i in insertion:
            signals, outcome = _fixture_markets(g)[i]
            market = ms.create_market(MarketId(f"lag:m{i}"))
            for s in signals:
                market.add_signal(s)
            market.created_at = g["forecast_times"][i]
            if outcome is not None:
                market.resolve(outcome)
                market.resolved_at = g["resolve_times"][i] if i != swap else g["forecast_times"][0]
        ms.create_market(MarketId("lag:empty"))  # no signals: not part of the walk
        return ms

    store = NamespacedReliabilityStore(str(tmp_path / "agg.db"))
    _seed_store(store, g)
    before = _rows(store, g["scope"])
    agg = CrossMarketAggregator(fill())
    dry, dsum = agg.walk_forward(store, patterns=["lag:*"], domain=g["domain"], lagged=True, dry_run=True)
    assert _rows(store, g["scope"]) == before
    out, summary = agg.walk_forward(store, patterns=["lag:*"], domain=g["domain"], lagged=True)
    assert dry == out and dsum == summary
    assert list(out) == [f"lag:m{i}" for i in range(10)]  # (created_at, store position)
    assert all(out[k]["marketId"] == k for k in out)
    _check_dicts(list(out.values()), g)
    assert _rows(store, g["scope"]) == g["final"]
    # the unlagged walk of the same store orders and times the markets by resolved_at: another back-test
    plain, _ = agg.walk_forward(store, patterns=["lag:*"], domain=g["domain"], dry_run=True)
    assert list(plain) != list(out)
    with pytest.raises(ValueError, match="lag:m6.*earlier than created_at"):
        CrossMarketAggregator(fill(swap=6)).walk_forward(store, domain=g["domain"], lagged=True, dry_run=True)
    with pytest.raises(ValueError, match="domain_of"):
        agg.walk_forward(store, lagged=True, domain_of=lambda m: "d", dry_run=True)
    rows = agg.sweep_decay(store, [30.0], [0.1], domain=g["domain"], lagged=True)
    assert len(rows) == 1 and rows[0].params == {"half_life_days": 30.0, "min_rel": 0.1}
    store.close()
    N.check_faults(_dev(), "aggregator")
