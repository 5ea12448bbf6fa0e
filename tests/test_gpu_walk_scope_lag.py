"""GPU checks of the namespaced walk-forward with resolution lag and of the namespaced decay sweep
(batch.WalkScopePlan.build_lagged, bce_walk_scope_read_lag, batch.walk_sweep_scoped and the store
layers): every market's consensus, every slot's weight, every entry's scope and read state and the
final domain and global rows -- stamps included -- equal the event loop of
tests/walk_scope_lag_ref.py exactly (``==``; NaN-aware) and the fixture recorded from the
reference's NamespacedReliabilityStore; without lag the plan and the walk equal the ordinary ones
byte for byte; every point of a sweep equals that point run alone, bit for bit."""
import dataclasses

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM
from bayesian_engine.timeutil import iso_to_us
from oracle import oracle as orc
from test_gpu_score import _check as _check_score
from test_gpu_walk_scoped import (NS, _bytes, _check_dicts, _compare, _db_rows, _final_rows, _fixture_markets,
                                  _global_table, _pair_table, _same_rows, _seed_store)
from walk_scope_lag_ref import load_fixture, walk_scope_lag_ref
from walk_scope_ref import GLOBAL, scope_key, walk_scope_ref

pytestmark = pytest.mark.gpu

OFF = batch.SETTLE_LONG_OFF
PATHS = ({}, {"long_min": OFF}, {"long_min": 1, "chunk_bits": 64})
DAY = 86_400_000_000
HOUR = 3_600_000_000
T0 = 1_790_000_000_000_000
NOTS = int(orc.NO_TIMESTAMP)
R = lambda x: repr(float(x))  # noqa: E731
RESULT = ("consensus", "confidence", "total_weight", "n_unique", "usid", "weight", "nweight", "scope")


def _dev():
    return torch.device("cuda", 0)


def _T(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev())


def _args(b):
    off, sid, prob, outcome, md, D, S = b
    return (_T(off, np.int64), _T(sid, np.int32), _T(prob, np.float64), _T(outcome, np.int8), _T(md, np.int32), S, D)


def _lagged(b, forecast, resolve, update_global, **kw):
    return batch.WalkScopePlan.build_lagged(*_args(b), _T(forecast, np.int64), _T(resolve, np.int64),
                                            update_global=update_global, **kw)


def _tables(b, rows, market_scope=True):
    off, _, _, _, _, D, S = b
    return (_pair_table(rows, "d", D, S), *_global_table(rows, S),
            _pair_table(rows, "m", len(off) - 1, S) if market_scope else None)


def _run(b, rows, plan, mtime=None, **kw):
    """(result fields as numpy, relconf by entry, final domain + global rows); ``mtime`` for an
    ordinary plan only."""
    off, prob = _T(b[0], np.int64), _T(b[2], np.float64)
    mt = () if mtime is None else (_T(mtime, np.int64),)
    dt, gt, gh, pt = _tables(b, rows)
    res = batch.walk_forward_scoped(plan, dt, gt, *mt, pairs=pt, global_has=gh, offsets=off, prob=prob, **kw)
    torch.cuda.synchronize()
    out = {k: getattr(res, k).cpu().numpy() for k in RESULT}
    final = _final_rows(res, gt, gh)
    dt, gt, gh, pt = _tables(b, rows)  # the read states themselves: the trace alone on fresh tables
    tkw = {k: v for k, v in kw.items() if k in ("mark_cold", "long_min", "chunk_bits")}
    wt, scope = batch.walk_scope_trace(plan, dt, gt, *mt, pairs=pt, global_has=gh, **tkw)
    torch.cuda.synchronize()
    assert np.array_equal(scope.cpu().numpy(), out["scope"])
    return out, wt.relconf[:plan.pairs.n_entries].cpu().numpy(), final


def _slots(off, n_unique):
    return np.concatenate([np.arange(a, a + u) for a, u in zip(off[:-1], n_unique)] + [np.zeros(0, np.int64)])


def _same_bytes(a, b, off, what=""):
    """Two _run results: every written byte equal (slots past a market's unique sources are not written)."""
    slots = _slots(off, a[0]["n_unique"])
    for k in a[0]:
        pick = slots if k in ("usid", "weight", "nweight") else slice(None)
        assert a[0][k][pick].tobytes() == b[0][k][pick].tobytes(), (what, k)
    assert a[1].tobytes() == b[1].tobytes(), what
    assert a[2] == b[2], what


# ----------------------------------------------------------------------------- golden fixture
@pytest.mark.parametrize("update_global", [False, True])
def test_fixture_through_the_batch_call(golden_dir, update_global):
    g, b, rows, forecast, resolve = load_fixture(golden_dir)
    off = b[0]
    run = g["runs"]["true" if update_global else "false"]
    exp, exp_rows = walk_scope_lag_ref(*b[:5], b[6], rows, forecast, resolve, update_global=update_global)
    plan = _lagged(b, forecast, resolve, update_global)
    assert plan.lagged and plan.outcome is not None
    for kw in PATHS:
        got, relconf, final = _run(b, rows, plan, **kw)
        _compare(got, relconf, plan, exp, off, f"fixture {kw}")
        _same_rows(final, exp_rows, f"fixture {kw}")
        uoff = plan.pairs.uoffsets.cpu().numpy()
        for m, r in enumerate(run["results"]):  # the reference's own numbers
            null = r["consensus"] is None
            assert null == bool(got["total_weight"][m] == 0)
            assert null or R(got["consensus"][m]) == r["consensus"], m
            assert R(got["confidence"][m]) == r["confidence"] and R(got["total_weight"][m]) == r["totalWeight"], m
            ent = slice(int(uoff[m]), int(uoff[m + 1]))
            assert got["n_unique"][m] == len(r["read"]), m
            assert [[R(x), R(y), NS[int(sc)]] for (x, y), sc in zip(relconf[ent], got["scope"][ent])] == \
                [x[1:4] for x in r["read"]], m
            assert [int(sc) == 3 for sc in got["scope"][ent]] == [x[4] == "cold-start" for x in r["read"]], m
            a = int(off[m])
            assert [[R(x), R(y)] for x, y in zip(got["weight"][a:a + len(r["read"])],
                                                 got["nweight"][a:a + len(r["read"])])] == \
                [x[1:] for x in r["sourceWeights"]], m
        rec = {(n, k): (float(r), float(c), iso_to_us(ts), 1 if ts else 0) for n, k, r, c, ts in run["final"]}
        mine = {(g["names"][s], scope_key(g, sc)): v for (sc, s), v in final.items()}
        assert mine == {k: _bytes(v) for k, v in rec.items() if not k[1].startswith("walk:")}
    N.check_faults(_dev(), "fixture")


# ----------------------------------------------------------------------------- edge batch
def _edge_batch():
    """48 markets, 8 sources, 3 domains and 8 markets without one; market 20 is empty.  Source 0
    signals 11 times in every market of domain 0 (the chain of (domain 0, source 0) is longer than
    256 bits) and source 1 38 times in every market without a domain (its global chain is longer
    than 256 bits even without update_global); sources 2..6 signal 0..5 times per market.  Source 7
    is seen in the unresolved markets only.  Forecast times come in tied groups of 2 and 3; the
    lags are zero, an hour, exactly up to the forecast time of the next group, nine days, and past
    the last forecast.  Rows: (domain 0, source 2) and (global, source 3) exist without a stamp;
    the market row (4, source 4) has a stamp, (7, source 5) has none; sources 5 and 6 have no
    other row."""
    rng = np.random.default_rng(23)
    S, M, D = 8, 48, 3
    md = np.array([0, 0, 1, -1, 0, 2], np.int32)[np.arange(M) % 6]
    unresolved = (5, 17, 33)
    outcome = rng.integers(0, 2, M).astype(np.int8)
    outcome[list(unresolved)] = -1
    markets = []
    for m in range(M):
        if m == 20:
            markets.append([])
            continue
        sig = [(int(rng.integers(2, 7)), float(np.round(rng.random(), 3))) for _ in range(int(rng.integers(0, 6)))]
        if md[m] == 0:
            sig += [(0, float(np.round(rng.random(), 3))) for _ in range(11)]
        if md[m] == -1:
            sig += [(1, float(np.round(rng.random(), 3))) for _ in range(38)]
        if m in unresolved:
            sig += [(7, 0.9), (7, 0.2)]
        if m == 4:
            sig += [(4, 0.6), (2, 0.5)]  # the market row wins; 0.5 is exactly on the threshold: votes True
        if m == 7:
            sig += [(5, 0.3)]            # the market row without a stamp falls through
        order = rng.permutation(len(sig))
        markets.append([sig[i] for i in order])
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in markets])
    sid = np.array([s for x in markets for s, _ in x], np.int32)
    prob = np.array([p for x in markets for _, p in x], np.float64)
    group = np.repeat(np.arange(M), np.tile([2, 3], M)[:M])[:M]  # 0 0 1 1 1 2 2 3 3 3 ...
    gtime = T0 + np.arange(group.max() + 3) * 2 * DAY + 123
    forecast = gtime[group]
    kind = np.arange(M) % 5
    resolve = np.select([kind == 1, kind == 2, kind == 3, kind == 4],
                        [forecast + HOUR, gtime[group + 1], forecast + 9 * DAY + 7, gtime[-1] + DAY + np.arange(M)],
                        forecast)
    rows = {
        (("d", 0), 0): (0.9, 0.3, T0 - 3 * DAY, 1),
        (("d", 0), 2): (0.66, 0.41, NOTS, 0),       # exists, no stamp: skipped until a bit of its chain is visible
        (("d", 0), 3): (1.0, 1.0, T0 + DAY, 1),     # a stamp later than the first forecasts: read undecayed there
        (("d", 1), 2): (0.05, 0.99, T0 - 40 * DAY, 1),
        (("d", 2), 4): (0.37, 0.5, T0 - 90 * DAY, 1),
        (GLOBAL, 1): (0.8, 0.5, T0 - 2 * DAY, 1),
        (GLOBAL, 2): (0.3, 0.7, T0 - 30 * DAY, 1),
        (GLOBAL, 3): (0.9, 0.2, NOTS, 0),           # the same at global scope
        (GLOBAL, 4): (0.0, 0.6, T0 - 10 * DAY, 1),
        (("m", 4), 4): (0.77, 0.8, T0 - DAY, 1),
        (("m", 7), 5): (0.2, 0.2, NOTS, 0),
    }
    # what the batch is meant to hold
    res = np.flatnonzero(outcome >= 0)
    mk = np.repeat(np.arange(M), np.diff(off))
    assert ((sid == 0) & (outcome[mk] >= 0) & (md[mk] == 0)).sum() > 256
    assert ((sid == 1) & (outcome[mk] >= 0) & (md[mk] == -1)).sum() > 256
    assert set(np.bincount(group)[:-1].tolist()) == {2, 3} and set(md.tolist()) == {-1, 0, 1, 2}
    assert (np.diff(forecast) >= 0).all() and (resolve[res] >= forecast[res]).all()
    assert all(len({int(md[m]) for m in res if kind[m] == k}) >= 3 for k in range(5))  # every lag in most domains
    assert any(resolve[a] == forecast[b] and forecast[a] < forecast[b] for a in res for b in range(M))
    assert any(resolve[a] > resolve[b] for a in res for b in res if a < b)
    assert (resolve[res] > forecast[-1]).any()
    assert set(mk[sid == 7].tolist()) <= set(unresolved) and {5, 6} <= set(sid[outcome[mk] >= 0].tolist())
    assert 4 in sid[off[4]:off[5]] and 5 in sid[off[7]:off[8]] and off[21] == off[20]
    return dict(b=(off, sid, prob, outcome, md, D, S), rows=rows, forecast=forecast, resolve=resolve)


@pytest.fixture(scope="module")
def edge():
    e = _edge_batch()
    b = e["b"]
    e["exp"] = {ug: walk_scope_lag_ref(*b[:5], b[6], e["rows"], e["forecast"], e["resolve"], update_global=ug)
                for ug in (False, True)}
    return e


@pytest.mark.parametrize("update_global", [False, True])
def test_edge_batch(edge, update_global):
    b, rows, forecast, resolve = edge["b"], edge["rows"], edge["forecast"], edge["resolve"]
    exp, exp_rows = edge["exp"][update_global]
    written = exp["scope"][exp["scope"] != 255]
    assert {0, 1, 2, 3} == set(written.tolist())
    unlagged, _ = walk_scope_ref(*b[:5], b[6], rows, forecast, update_global=update_global)
    assert (unlagged["scope"] != exp["scope"]).any()  # the lag decides the scope of some read
    plan = _lagged(b, forecast, resolve, update_global)
    for sp in (plan.dsettle, plan.gsettle):  # both families take the long path at the defaults
        assert sp.chunks(batch.WALK_LONG_MIN, batch.WALK_CHUNK_BITS)[0] >= 1
    f00 = int(np.flatnonzero((plan.dplan.emarket.cpu().numpy() == 0) & (plan.dplan.usid.cpu().numpy() == 0))[0])
    assert plan.dsettle.total.cpu().numpy()[f00] > 256 and plan.gsettle.total.cpu().numpy()[1] > 256
    runs = [_run(b, rows, plan, **kw) for kw in PATHS]
    for kw, run in zip(PATHS, runs):
        _compare(run[0], run[1], plan, exp, b[0], f"edge {kw} {update_global}")
        _same_rows(run[2], exp_rows, f"edge {kw} {update_global}")
        _same_bytes(run, runs[0], b[0], f"edge {kw}")
    N.check_faults(_dev(), "edge batch")


# ----------------------------------------------------------------------------- degenerate lag
@pytest.mark.parametrize("update_global", [False, True])
def test_without_lag_the_plan_and_the_walk_are_the_ordinary_ones(edge, update_global):
    b, rows, f = edge["b"], edge["rows"], edge["forecast"]
    lag = _lagged(b, f, f, update_global)
    plain = batch.WalkScopePlan.build(*_args(b), update_global=update_global)
    assert torch.equal(lag.dentry, plain.dentry) and lag.dentry.dtype == plain.dentry.dtype
    for fam in ("dq", "gq"):
        for name in ("qstart", "qpos", "qentry", "qlast", "slast"):
            x, y = getattr(getattr(lag, fam), name), getattr(getattr(plain, fam), name)
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (fam, name)
    for fam in ("dsettle", "gsettle"):
        x, y = getattr(lag, fam), getattr(plain, fam)
        for name in ("bits", "start", "order", "total", "correct"):
            assert torch.equal(getattr(x, name), getattr(y, name)), (fam, name)
        assert x.n_bits == y.n_bits and x.n_sources == y.n_sources and np.array_equal(x.lens_desc, y.lens_desc)
    _same_bytes(_run(b, rows, lag), _run(b, rows, plain, mtime=f), b[0], "no lag")
    N.check_faults(_dev(), "no lag")


# ----------------------------------------------------------------------------- the kernel alone
def _read_args(plan, tr, gt, pt, times, out):
    """The argument list of bce_walk_scope_read / bce_walk_scope_read_lag behind ``times``."""
    pp = plan.pairs
    p = N.ptr
    return [pp.n_entries, p(pp.usid), p(pp.emarket), *[p(t) for t in times], pp.n_markets, pp.n_sources,
            p(pt.poffsets), *batch._pair_pointers(pt), pt.n_rows, p(plan.dentry), p(plan.dq.qlast), p(tr.dtrace),
            p(tr.raw.rel), p(tr.raw.conf), p(tr.raw.t_us), p(tr.dhas), plan.dplan.n_entries, p(plan.gq.qlast),
            p(tr.gtrace), p(gt.rel), p(gt.conf), p(gt.t_us), p(tr.global_has), DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM,
            0.5, 0.25, 0, 0, *[p(x) for x in out], N.stream(_dev())]


def _outputs(E):
    return (torch.full((E, 2), -7.0, dtype=torch.float64, device=_dev()),
            torch.full(((E + 31) // 32,), 0x5A5A5A5A, dtype=torch.int32, device=_dev()),
            torch.full((E,), 77, dtype=torch.uint8, device=_dev()))


def test_new_entry_with_one_array_twice_is_the_old_entry_and_refuses_bad_arguments(edge):
    b, rows, f = edge["b"], edge["rows"], edge["forecast"]
    plan = batch.WalkScopePlan.build(*_args(b), update_global=True)
    E = plan.pairs.n_entries
    dt, gt, gh, pt = _tables(b, rows)
    mt = _T(f, np.int64)
    gtrace = torch.empty((E, 2), dtype=torch.float64, device=_dev())
    tr = batch._walk_scope_traces(plan, dt, gt, mt, pt, gh, None, None, gtrace)
    assert tr.gtrace is gtrace and tr.dtrace is not None and pt.n_rows == 2
    L = N.lib()
    old, new = _outputs(E), _outputs(E)
    N.check(L.bce_walk_scope_read(*_read_args(plan, tr, gt, pt, (mt,), old)), "bce_walk_scope_read")
    N.check(L.bce_walk_scope_read_lag(*_read_args(plan, tr, gt, pt, (mt, mt), new)), "bce_walk_scope_read_lag")
    torch.cuda.synchronize()
    N.check_faults(_dev(), "both entries")
    for x, y in zip(old, new):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert set(old[2].cpu().numpy().tolist()) == {0, 1, 2, 3}
    # a NULL time array or a negative size: BCE_EINVAL, nothing launched
    untouched = _outputs(E)
    full = _read_args(plan, tr, gt, pt, (mt, mt), untouched)
    for at, value in ((3, None), (4, None), (0, -1), (5, -1), (13, -1), (21, -1)):
        args = list(full)
        args[at] = value
        assert L.bce_walk_scope_read_lag(*args) == -1, at
        assert b"walk_scope_read" in L.bce_last_error()
    torch.cuda.synchronize()
    for x, y in zip(untouched, _outputs(E)):
        assert torch.equal(x, y)
    N.check_faults(_dev(), "argument errors launch nothing")


@pytest.mark.parametrize("field", ["dqlast", "gqlast"])
def test_out_of_range_qlast_raises_and_the_other_entries_are_answered(edge, field):
    b, rows = edge["b"], edge["rows"]
    plan = _lagged(b, edge["forecast"], edge["resolve"], True)
    E, M = plan.pairs.n_entries, plan.pairs.n_markets

    def trace(p):
        dt, gt, gh, pt = _tables(b, rows)
        wt, scope = batch.walk_scope_trace(p, dt, gt, pairs=pt, global_has=gh)
        torch.cuda.synchronize()
        return wt.relconf[:E].cpu().numpy(), scope.cpu().numpy()

    N.check_faults(_dev(), "clean slate")
    good = trace(plan)
    N.check_faults(_dev(), "a valid plan raises nothing")
    e = int(np.flatnonzero(plan.dentry.cpu().numpy() >= 0)[5])
    q = plan.dq if field == "dqlast" else plan.gq
    for value in (M, M + 3, -2, -7):
        x = q.qlast.clone()
        x[e] = value
        bad = dataclasses.replace(plan, **{field[0] + "q": dataclasses.replace(q, qlast=x)})
        relconf, scope = trace(bad)
        with pytest.raises(N.BCEError):
            N.check_faults(_dev(), "walk_scope_read_lag")
        keep = np.arange(E) != e
        assert relconf[keep].tobytes() == good[0][keep].tobytes() and np.array_equal(scope[keep], good[1][keep])
        assert scope[e] in (0, 1, 2, 3) and np.isfinite(relconf[e]).all()  # answered from what can be read safely
        minus = q.qlast.clone()
        minus[e] = -1  # the bad value reads as -1: "no earlier bit"
        as_none = trace(dataclasses.replace(plan, **{field[0] + "q": dataclasses.replace(q, qlast=minus)}))
        N.check_faults(_dev(), "-1 is a valid qlast")
        assert relconf[e].tobytes() == as_none[0][e].tobytes() and scope[e] == as_none[1][e]
    N.check_faults(_dev(), "the fault word is cleared")


# ----------------------------------------------------------------------------- commit=False
def test_commit_false_leaves_every_input_untouched(edge):
    b, rows = edge["b"], edge["rows"]
    plan = _lagged(b, edge["forecast"], edge["resolve"], True)
    dt, gt, gh, pt = _tables(b, rows)
    o, p = _T(b[0], np.int64), _T(b[2], np.float64)
    inputs = [plan.forecast_time_us, plan.resolve_time_us, o, p, gt.rel, gt.conf, gt.t_us, gt.present, gh] + \
        [getattr(t, f) for t in (dt, pt) for f in ("poffsets", "psid", "rel", "conf", "t_us", "has")]
    before = [x.cpu().numpy().tobytes() for x in inputs]
    dry = batch.walk_forward_scoped(plan, dt, gt, offsets=o, prob=p, pairs=pt, global_has=gh, commit=False)
    torch.cuda.synchronize()
    assert dry.domains is dt and [x.cpu().numpy().tobytes() for x in inputs] == before
    wet = batch.walk_forward_scoped(plan, dt, gt, offsets=o, prob=p, pairs=pt, global_has=gh)
    torch.cuda.synchronize()
    for k in ("consensus", "confidence", "total_weight", "n_unique", "scope"):
        assert getattr(dry, k).cpu().numpy().tobytes() == getattr(wet, k).cpu().numpy().tobytes(), k
    # the committed call wrote the global table and a NEW domain table; the old one and the market rows stay
    after = [x.cpu().numpy().tobytes() for x in inputs]
    assert wet.domains is not dt and after[:4] == before[:4] and after[9:] == before[9:] and after[4:9] != before[4:9]
    N.check_faults(_dev(), "commit")


# ----------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("lagged", [False, True])
def test_walk_sweep_scoped_equals_every_point_run_alone(edge, lagged):
    b, rows, f = edge["b"], edge["rows"], edge["forecast"]
    off, prob, outcome = _T(b[0], np.int64), _T(b[2], np.float64), _T(b[3], np.int8)
    M = len(b[3])
    if lagged:
        plan, mt = _lagged(b, f, edge["resolve"], True), ()
    else:
        plan, mt = batch.WalkScopePlan.build(*_args(b), update_global=True), (_T(f, np.int64),)
    dt, gt, gh, pt = _tables(b, rows)
    inputs = [off, prob, gt.rel, gt.conf, gt.t_us, gt.present, gh] + \
        [getattr(t, k) for t in (dt, pt) for k in ("poffsets", "psid", "rel", "conf", "t_us", "has")]
    before = [x.cpu().numpy().tobytes() for x in inputs]
    hl, mr = [DECAY_HALF_LIFE_DAYS, 5.0, 90.0], [DECAY_MINIMUM, 0.4]
    scores, (cons, nulls) = batch.walk_sweep_scoped(plan, dt, gt, *mt, offsets=off, prob=prob, half_life_days=hl,
                                                    min_rel=mr, pairs=pt, global_has=gh, keep_consensus=True)
    torch.cuda.synchronize()
    N.check_faults(_dev(), "walk_sweep_scoped")
    assert [x.cpu().numpy().tobytes() for x in inputs] == before  # no input is written
    assert scores.counts.shape == (6, 1, 5) and cons.shape == (6, M) and nulls.shape == (6, M)
    whole = batch.ScorePlan.whole(M, device=_dev())
    k = 0
    for h in hl:
        for m in mr:
            wt, _ = batch.walk_scope_trace(plan, dt, gt, *mt, pairs=pt, global_has=gh, half_life_days=h, min_rel=m)
            res = batch.consensus(off, plan.pairs.esid, prob, wt)
            assert torch.equal(res.consensus.view(torch.int64), cons[k].view(torch.int64)), (h, m)
            assert torch.equal(res.is_null(off), nulls[k]), (h, m)
            alone = batch.score(whole, res.consensus, outcome, valid=~res.is_null(off))
            for name in ("counts", "sums", "bin_n", "bin_pos", "bin_psum"):
                x, y = getattr(alone, name), getattr(scores, name)[k]
                assert torch.equal(x.view(torch.int64), y.view(torch.int64)), (h, m, name)
            # and against the shaped CPU reference: Brier to the bit, log loss within 4 ulp per term
            fx = dict(goff=np.array([0, M], np.int64), pidx=np.arange(M, dtype=np.int64), value=cons[k].cpu().numpy(),
                      outcome=b[3], valid=(~nulls[k]).cpu().numpy().astype(np.uint8), B=10, eps=1e-15)
            _check_score({name: getattr(scores, name)[k].cpu().numpy()
                          for name in ("counts", "sums", "bin_n", "bin_pos", "bin_psum")}, fx, f"point {h} {m}")
            k += 1
    assert not torch.equal(cons[0], cons[2])  # the decay parameters do reach the consensus
    ref = batch.walk_forward_scoped(plan, dt, gt, *mt, offsets=off, prob=prob, pairs=pt, global_has=gh, commit=False)
    assert torch.equal(ref.consensus.view(torch.int64), cons[0].view(torch.int64))  # the default point
    assert torch.equal(ref.is_null(off), nulls[0])
    dry = batch.score_markets(ref, off, outcome)
    for name in ("counts", "sums", "bin_n", "bin_pos", "bin_psum"):
        assert torch.equal(getattr(dry, name).view(torch.int64), getattr(scores, name)[0].view(torch.int64)), name
    only, none = batch.walk_sweep_scoped(plan, dt, gt, *mt, offsets=off, prob=prob, half_life_days=[5.0],
                                         min_rel=[0.4], pairs=pt, global_has=gh)
    assert none is None and torch.equal(only.sums[0].view(torch.int64), scores.sums[3].view(torch.int64))
    assert [x.cpu().numpy().tobytes() for x in inputs] == before
    N.check_faults(_dev(), "walk_sweep_scoped")


# ----------------------------------------------------------------------------- store layers
def _scored(g, run):
    return sum(r["consensus"] is not None and mk["outcome"] is not None for r, mk in zip(run["results"], g["markets"]))


@pytest.mark.parametrize("update_global", [False, True])
def test_fixture_through_the_namespaced_store(golden_dir, tmp_path, update_global):
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    g = load_fixture(golden_dir)[0]
    run = g["runs"]["true" if update_global else "false"]
    store = NamespacedReliabilityStore(str(tmp_path / "lag.db"))
    _seed_store(store, g)
    before = _db_rows(store)
    kw = dict(domains=g["domains"], market_ids=g["market_ids"], update_global=update_global,
              resolve_times=g["resolve_times"])
    scores = store.sweep_decay_namespaced(_fixture_markets(g), g["forecast_times"], [DECAY_HALF_LIFE_DAYS],
                                          [DECAY_MINIMUM], **kw)
    assert scores.counts.shape == (1, 1, 5) and int(scores.counts[0, 0, 0]) == _scored(g, run)
    assert int(scores.counts[0, 0, 2]) == sum(mk["outcome"] is None for mk in g["markets"])
    dry, dsum = store.walk_forward_namespaced(_fixture_markets(g), g["forecast_times"], dry_run=True, **kw)
    assert _db_rows(store) == before  # the sweep and the dry run: the database is untouched
    wet, wsum = store.walk_forward_namespaced(_fixture_markets(g), g["forecast_times"], **kw)
    assert dry == wet and dsum == wsum
    _check_dicts(wet, g, run)
    assert _db_rows(store) == run["final"]  # updated_at: the resolve time of each row's last settling market
    final = {(n, k): [r, c, ts] for n, k, r, c, ts in run["final"]}
    for (name, dom), rec in wsum.records.items():
        key = f"__domain__:{dom}" if dom else "__global__"
        assert [repr(rec.reliability), repr(rec.confidence), rec.updated_at] == final[(name, key)], (name, dom)
    for name, rec in wsum.global_records.items():
        assert [repr(rec.reliability), repr(rec.confidence), rec.updated_at] == final[(name, "__global__")], name
    with pytest.raises(ValueError, match="resolve_times has 3 entries"):
        store.walk_forward_namespaced(_fixture_markets(g), g["forecast_times"], resolve_times=["", "", ""])
    late = list(g["resolve_times"])
    late[3] = g["forecast_times"][2]  # before its own forecast
    with pytest.raises(ValueError, match="market 3 resolves before"):
        store.walk_forward_namespaced(_fixture_markets(g), g["forecast_times"], domains=g["domains"],
                                      resolve_times=late)
    assert store.sweep_decay_namespaced([([], None)], g["forecast_times"][:1], [30.0], [0.1]) is None
    store.close()
    N.check_faults(_dev(), "namespaced store")


def test_fixture_through_the_aggregator(golden_dir, tmp_path):
    from bayesian_engine.market import BacktestScore, CrossMarketAggregator, MarketId, MarketStore
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    g = load_fixture(golden_dir)[0]
    run = g["runs"]["true"]
    dom = dict(zip(g["market_ids"], g["domains"]))
    domain_of = lambda m: dom[str(m.id)]  # noqa: E731
    insertion = [7, 2, 9, 0, 3, 11, 5, 4, 1, 10, 8, 6]  # not the time order; 3 stands before 4 and 9 before 10
    assert insertion.index(3) < insertion.index(4) and insertion.index(9) < insertion.index(10)
    assert sorted(range(12), key=lambda i: (g["forecast_times_us"][i], insertion.index(i))) == list(range(12))
    ms = MarketStore()
    for i in insertion:
        signals, outcome = _fixture_markets(g)[i]
        market = ms.create_market(MarketId(g["market_ids"][i]))
        for s in signals:
            market.add_signal(s)
        market.created_at = g["forecast_times"][i]
        if outcome is not None:
            market.resolve(outcome)
            market.resolved_at = g["resolve_times"][i]
    ms.create_market(MarketId("walk:empty"))  # no signals: not part of the walk
    store = NamespacedReliabilityStore(str(tmp_path / "agg.db"))
    _seed_store(store, g)
    before = _db_rows(store)
    agg = CrossMarketAggregator(ms)
    kw = dict(patterns=["walk:*"], update_global=True, market_scope=True)
    rows = agg.sweep_decay_namespaced(store, [DECAY_HALF_LIFE_DAYS, 5.0], [DECAY_MINIMUM, 0.4, 0.6], domain_of,
                                      lagged=True, **kw)
    assert len(rows) == 6 and all(isinstance(r, BacktestScore) for r in rows)
    assert [r.params for r in rows] == [{"half_life_days": h, "min_rel": m} for h in (DECAY_HALF_LIFE_DAYS, 5.0)
                                        for m in (DECAY_MINIMUM, 0.4, 0.6)]
    assert rows[0].n == _scored(g, run)
    dry, dsum = agg.walk_forward_namespaced(store, domain_of, lagged=True, dry_run=True, **kw)
    assert _db_rows(store) == before
    # the unlagged namespaced walk is walk_forward(domain_of=), and another back-test than the lagged one
    plain = agg.walk_forward_namespaced(store, domain_of, dry_run=True, **kw)
    assert plain == agg.walk_forward(store, domain_of=domain_of, dry_run=True, **kw)
    assert list(plain[0]) != list(dry)
    score = agg.score_walk(dry, sources=False)  # score_walk takes the dict; its sums run in another item order
    assert score.overall.n == rows[0].n and score.overall.accuracy == rows[0].accuracy
    out, summary = agg.walk_forward_namespaced(store, domain_of, lagged=True, **kw)
    assert dry == out and dsum == summary
    assert list(out) == g["market_ids"] and all(out[k]["marketId"] == k for k in out)  # (created_at, store position)
    _check_dicts(list(out.values()), g, run)
    assert _db_rows(store) == run["final"]
    with pytest.raises(ValueError, match="domain_of"):
        agg.walk_forward(store, lagged=True, domain_of=domain_of, dry_run=True)
    with pytest.raises(ValueError, match="domain_of is needed"):
        agg.walk_forward_namespaced(store, None, dry_run=True)
    store.close()
    N.check_faults(_dev(), "aggregator")
