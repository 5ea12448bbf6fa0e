"""GPU checks of the update-rule sweep (batch.walk_trace_grid / walk_sweep_update /
commit_update_point and the store layers), all bit-exact (``==``; NaN-aware): against the fixture
recorded from the reference under four update rules, against the plain-Python event loop of
tests/update_sweep_ref.py over random batches at every lane mapping and over a crafted long chain,
and against the existing single-rule path at the reference's own rule."""
import numpy as np
import pytest
import torch

from bayesian_engine import batch
from bayesian_engine.config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM
from oracle import oracle as orc
from update_sweep_ref import check_point, load_fixture, update_sweep_ref

pytestmark = pytest.mark.gpu

OFF = batch.SETTLE_LONG_OFF
MASK = 0x7FFFFFFF
DAY = 86_400_000_000
T0 = 1_790_000_000_000_000
POINTS = [(0.15, 0.10), (0.05, 0.10), (0.30, 0.20), (0.0, 0.10)]
LAG_POINTS = [(0.05, 0.10), (0.30, 0.20)]
RATES = [round(0.004 * (k + 1), 3) for k in range(64)]  # 64 distinct steps under a cap of 10
FIELDS = ("counts", "sums", "bin_n", "bin_pos", "bin_psum")


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _plan(csr, resolve=None, forecast=None):
    off, sid, prob, outcome, S = csr
    args = (_T(np.asarray(off, np.int64)), _T(np.asarray(sid, np.int32)), _T(np.asarray(prob, np.float64)),
            _T(np.asarray(outcome, np.int8)), S)
    if resolve is None:
        return batch.WalkPlan.build(*args)
    return batch.WalkPlan.build_lagged(*args, _T(np.asarray(forecast, np.int64)), _T(np.asarray(resolve, np.int64)))


def _table(state):
    rel, conf, t_us, present = state
    return batch.ReliabilityTable(_T(np.array(rel, np.float64)), _T(np.array(conf, np.float64)),
                                  _T(np.array(t_us, np.int64)), _T(np.array(present, np.uint8)), [""] * len(rel))


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _same_scores(a, b, what=""):
    for f in FIELDS:
        assert torch.equal(getattr(a, f).view(torch.int64), getattr(b, f).view(torch.int64)), (what, f)


def _read_slice(plan, table, mt, trace_k, csr):
    """Slice k of a grid trace through the unchanged read side: ``(relconf [E, 2], exists [E],
    consensus fields)`` of bce_walk_read_lag and :func:`batch.consensus` over the entries."""
    off, _, prob = csr[:3]
    E = plan.pairs.n_entries
    relconf, bits, exists = batch._walk_buffers(E, _dev())
    batch._walk_read(plan, table, mt, trace_k, relconf, bits, exists, False, DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM)
    wtable = batch.SourceTable(relconf, bits, range(E))
    res = batch.consensus(_T(np.asarray(off, np.int64)), plan.pairs.esid, _T(np.asarray(prob, np.float64)), wtable)
    torch.cuda.synchronize()
    got = {k: getattr(res, k).cpu().numpy() for k in ("consensus", "confidence", "total_weight", "n_unique")}
    return relconf[:E].cpu().numpy(), exists[:E].cpu().numpy(), got


def _check_slice(plan, table, mt, trace_k, csr, exp, what):
    """Every entry's read state and every market's consensus of slice k against the ref's."""
    off = csr[0]
    relconf, exists, got = _read_slice(plan, table, mt, trace_k, csr)
    for k in ("consensus", "confidence", "total_weight", "n_unique"):
        assert _eq(got[k], exp[k]), (what, k, np.flatnonzero(~(got[k] == exp[k]))[:8])
    esrc = plan.pairs.usid.cpu().numpy()
    uoff = plan.pairs.uoffsets.cpu().numpy()
    for m in range(len(off) - 1):
        a, u = int(off[m]), int(exp["n_unique"][m])
        ent = np.arange(uoff[m], uoff[m + 1])
        assert len(ent) == u, (what, m)
        assert np.array_equal(esrc[ent], exp["usid"][a:a + u] & MASK), (what, m)
        assert _eq(relconf[ent, 0], exp["rel_read"][a:a + u]), (what, m, "reliability read")
        assert _eq(relconf[ent, 1], exp["conf_read"][a:a + u]), (what, m, "confidence read")
        assert np.array_equal(exists[ent], exp["exists"][a:a + u]), (what, m)


def _check_grid(csr, state, times, points, resolve=None, what="", **kw):
    """walk_trace_grid(final=True) over ``points`` against one ref run per point; returns
    ``(plan, trace, final, refs)``."""
    plan = _plan(csr, resolve, times)
    table = _table(state)
    mt = None if resolve is not None else _T(np.asarray(times, np.int64))
    trace, fin = batch.walk_trace_grid(plan, table, mt, learning_rate=[r for r, _ in points],
                                       max_step=[c for _, c in points], final=True, **kw)
    torch.cuda.synchronize()
    E, S = plan.pairs.n_entries, csr[4]
    assert trace.shape == (len(points), E, 2) and fin.shape == (len(points), S, 2)
    fin_h = fin.cpu().numpy()
    refs = []
    for k, (rate, cap) in enumerate(points):
        exp, exp_state = update_sweep_ref(*csr, *state, times, rate, cap, resolve_time_us=resolve, all_present=False)
        _check_slice(plan, table, mt, trace[k], csr, exp, (what, k, rate, cap))
        assert _eq(fin_h[k, :, 0], exp_state[0]), (what, k, "final rel", np.flatnonzero(fin_h[k, :, 0] != exp_state[0]))
        assert _eq(fin_h[k, :, 1], exp_state[1]), (what, k, "final conf")
        refs.append((exp, exp_state))
    for name, x, x0 in zip(("rel", "conf", "t_us", "present"), (table.rel, table.conf, table.t_us, table.present), state):
        assert _eq(x.cpu().numpy(), np.asarray(x0)), (what, name, "the table was written")
    return plan, trace, fin, refs


# ----------------------------------------------------------------------------- the recorded fixture
def test_fixture_every_point(golden_dir):
    u, (g, csr, state, times), _ = load_fixture(golden_dir)
    for kw in ({}, {"long_min": 1, "chunk_bits": 64}):
        _, _, _, refs = _check_grid(csr, state, times, POINTS, what=f"fixture {kw}", **kw)
        for p, (exp, exp_state) in zip(u["points"], refs):  # the GPU equals the ref, the ref the reference
            check_point(p, g, csr, exp, exp_state)


def test_lagged_fixture(golden_dir):
    u, _, (g, csr, state, forecast, resolve) = load_fixture(golden_dir)
    _, _, _, refs = _check_grid(csr, state, forecast, LAG_POINTS, resolve=resolve, what="lagged fixture")
    for p, (exp, exp_state) in zip(u["lag_points"], refs):
        check_point(p, g, csr, exp, exp_state)


# ----------------------------------------------------------------------- identity with the old path
def _written(plan):
    return (plan.qlast >= 0).cpu().numpy()  # the entries a trace writes: those with an earlier bit


def test_default_point_is_the_existing_trace_and_sweep(golden_dir):
    _, (g, csr, state, times), _ = load_fixture(golden_dir)
    plan, table, mt = _plan(csr), _table(state), _T(times)
    off, prob = _T(csr[0]), _T(csr[2])
    E = plan.pairs.n_entries
    old = torch.empty((E, 2), dtype=torch.float64, device=_dev())
    batch._walk_settle_trace(plan, table, mt, old, None, None)
    trace = batch.walk_trace_grid(plan, table, mt, learning_rate=[0.05, 0.15, 0.3], max_step=[0.1, 0.1, 0.2])
    torch.cuda.synchronize()
    w = _written(plan)
    assert w.any() and _eq(trace[1].cpu().numpy()[w], old.cpu().numpy()[w])
    hl, mr = [DECAY_HALF_LIFE_DAYS, 3.0], [DECAY_MINIMUM, 0.45]
    base, bkept = batch.walk_sweep(plan, table, mt, offsets=off, prob=prob, half_life_days=hl, min_rel=mr,
                                   keep_consensus=True)
    got, kept = batch.walk_sweep_update(plan, table, mt, offsets=off, prob=prob, learning_rate=[0.05, 0.15, 0.3],
                                        max_step=[0.1, 0.1, 0.2], half_life_days=hl, min_rel=mr, keep_consensus=True)
    torch.cuda.synchronize()
    assert got.counts.shape[0] == 12 and kept[0].shape == (12, len(csr[0]) - 1)
    mid = batch.ScoreResult(*(getattr(got, f)[4:8] for f in FIELDS))
    _same_scores(mid, base, "rows of the default rule")
    assert torch.equal(kept[0][4:8].view(torch.int64), bkept[0].view(torch.int64)) and torch.equal(kept[1][4:8], bkept[1])
    assert not torch.equal(kept[0][0:4].view(torch.int64), bkept[0].view(torch.int64))  # another rule, another walk


# -------------------------------------------------------------------------------- the lane mapping
def _random_batch(seed, M=40, S=7, cover=False):
    """M markets over S sources: lengths 0..6, duplicate sources inside a market, one unresolved
    market, one absent row, one row at each end of [0, 1]; times a day apart with two equal."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 7, M)
    if cover:  # every source in some resolved market
        lens = np.maximum(lens, 4)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    if cover:
        assert n >= 2 * S
        sid[off[1]:off[1] + S] = rng.permutation(S)  # behind market 0, which stays resolved
    for m in range(0, M, 5):  # a duplicate
        if lens[m] >= 2 and not (cover and m < M // 2):
            sid[off[m] + 1] = sid[off[m]]
    prob = np.round(rng.random(n), 3)
    outcome = rng.integers(0, 2, M).astype(np.int8)
    outcome[M // 2] = -1
    rel, conf = rng.uniform(0.05, 0.95, S), rng.uniform(0.2, 0.9, S)
    present = np.ones(S, np.uint8)
    present[S - 1], rel[S - 1], conf[S - 1] = 0, 0.5, 0.25
    rel[0], rel[1] = 1.0, 0.0
    t_us = np.where(present != 0, T0 - rng.integers(1, 60, S) * DAY, orc.NO_TIMESTAMP).astype(np.int64)
    times = T0 + np.arange(M, dtype=np.int64) * DAY
    times[7] = times[6]
    return (off, sid, prob, outcome, S), (rel, conf, t_us, present), times


@pytest.mark.parametrize("K", [1, 3, 5, 8, 64])
def test_lane_mapping(K):
    csr, state, times = _random_batch(100 + K)
    points = [(0.15, 0.10)] if K == 1 else [(r, 10.0) for r in RATES[::64 // K][:K]]
    plan, _, _, _ = _check_grid(csr, state, times, points, what=f"K={K}")
    Kp = 1 << (K - 1).bit_length()
    assert 0 < plan.settle.n_touched and (Kp == 64 or plan.settle.n_touched % (64 // Kp))


def test_lane_mapping_last_wave_partly_empty():
    csr, state, times = _random_batch(7, S=70, cover=True)
    plan, _, _, _ = _check_grid(csr, state, times, [(0.15, 0.10), (0.03, 10.0), (0.5, 0.3)], what="70 chains")
    assert plan.settle.n_touched == 70  # 16 chains a wave: four full waves and one of six


# ----------------------------------------------------------------------------------- the long path
LONG_POINTS = [(0.25, 1.0), (0.1, 1.0), (0.02, 1.0), (0.01, 1.0), (0.0, 1.0), (1.0, 1.0)]


def _long_bits():
    """1,500 bits for chunks of 64: 200 alternating bits; runs of exactly sync_run - 1 and
    sync_run equal bits for the steps 0.1 (11) and 0.25 (5), each inside a chunk, ending on a
    chunk's last bit and straddling a boundary, the values alternating, every run fenced by the
    opposite bit; 120 ones at the end (a run of 51 inside a chunk: step 0.02; none of 101)."""
    bits = (np.arange(1500) % 2).astype(np.uint8)
    c, value = 4, 1
    for n in (10, 11, 4, 5):
        for start in (64 * c + 20, 64 * (c + 2) - n, 64 * (c + 3) - n // 2):
            bits[start:start + n] = value
            bits[start - 1] = bits[start + n] = 1 - value
            value = 1 - value
        c += 4
    assert 64 * c <= 1380
    bits[1379] = 0
    bits[1380:] = 1
    return bits


def _long_batch():
    rng = np.random.default_rng(5)
    bits = _long_bits()
    M, S = len(bits), 6
    off, sid, prob = [0], [], []
    for m in range(M):  # source 0 in every market: a query at every chain position
        row = [(0, 0.9 if bits[m] else 0.1)]
        if m % 37 == 0:
            row += [(int(s), float(np.round(rng.random(), 3))) for s in rng.integers(1, S, 2)]
        for s, p in row:
            sid.append(s)
            prob.append(p)
        off.append(len(sid))
    outcome = np.ones(M, np.int8)
    rel, conf = np.array([0.37, 0.9, 0.1, 0.5, 0.66, 0.2]), np.array([0.25, 0.3, 0.5, 0.7, 0.9, 0.99])
    present = np.ones(S, np.uint8)
    t_us = np.full(S, T0 - 3 * DAY, np.int64)
    times = T0 + np.arange(M, dtype=np.int64) * (DAY // 8)
    return (np.array(off, np.int64), np.array(sid, np.int32), np.array(prob), outcome, S), (rel, conf, t_us, present), \
        times


def test_long_chain_every_position():
    csr, state, times = _long_batch()
    d, s = batch.update_steps([r for r, _ in LONG_POINTS], 1.0)
    assert s.tolist() == [5, 11, 51, 101, 0, 2]
    plan, trace, fin, _ = _check_grid(csr, state, times, LONG_POINTS, what="long", long_min=64, chunk_bits=64)
    assert plan.settle.chunks(64, 64)[0] == 1 and plan.settle.chunks(64, 64)[2] == 24  # one long chain, 24 chunks
    flat, ffin = batch.walk_trace_grid(plan, _table(state), _T(times), learning_rate=[r for r, _ in LONG_POINTS],
                                       max_step=1.0, final=True, long_min=OFF)
    torch.cuda.synchronize()
    w = _written(plan)
    assert _eq(trace.cpu().numpy()[:, w], flat.cpu().numpy()[:, w]) and _eq(fin.cpu().numpy(), ffin.cpu().numpy())


# ------------------------------------------------------------------------------ blocking, committing
def test_blocks_of_two_points_equal_one_block():
    csr, state, times = _random_batch(31)
    plan, table, mt = _plan(csr), _table(state), _T(times)
    E = plan.pairs.n_entries
    kw = dict(offsets=_T(csr[0]), prob=_T(csr[2]), learning_rate=[0.15, 0.05, 0.3, 0.0, 0.6],
              max_step=[0.1, 0.1, 0.2, 0.1, 1.0], half_life_days=[30.0, 3.0], min_rel=[0.1], keep_consensus=True,
              final=True)
    one, kept1, fin1 = batch.walk_sweep_update(plan, table, mt, **kw)
    two, kept2, fin2 = batch.walk_sweep_update(plan, table, mt, max_trace_bytes=2 * 16 * E + 8, **kw)
    tiny, _, _ = batch.walk_sweep_update(plan, table, mt, max_trace_bytes=0, **kw)  # at least one point a block
    torch.cuda.synchronize()
    assert one.counts.shape[0] == 10
    _same_scores(one, two, "blocks of 2")
    _same_scores(one, tiny, "blocks of 1")
    assert torch.equal(kept1[0].view(torch.int64), kept2[0].view(torch.int64)) and torch.equal(kept1[1], kept2[1])
    assert torch.equal(fin1.view(torch.int64), fin2.view(torch.int64))


def test_commit_update_point():
    csr, state, times = _random_batch(47)
    plan, mt = _plan(csr), _T(times)
    points = [(0.15, 0.10), (0.3, 0.2)]
    _, fin = batch.walk_trace_grid(plan, _table(state), mt, learning_rate=[0.15, 0.3], max_step=[0.1, 0.2], final=True)
    now = int(times[-1]) + 9 * DAY
    for k, (rate, cap) in enumerate(points):
        table = _table(state)
        touched = batch.commit_update_point(plan, table, fin, k, mt)
        torch.cuda.synchronize()
        _, (rel, conf, t_us, present) = update_sweep_ref(*csr, *state, times, rate, cap)
        assert sorted(touched.cpu().numpy().tolist()) == sorted(np.flatnonzero(t_us != state[2]).tolist())
        for name, got, exp in zip(("rel", "conf", "t_us", "present"),
                                  (table.rel, table.conf, table.t_us, table.present), (rel, conf, t_us, present)):
            assert _eq(got.cpu().numpy(), exp), (k, name)
        assert _eq(table.view(now).cpu().numpy(), orc.decay_view(rel, t_us, present, now)), k
    walked = _table(state)  # the reference's own rule: what walk_forward itself commits
    batch.walk_forward(plan, walked, mt, offsets=_T(csr[0]), prob=_T(csr[2]))
    committed = _table(state)
    batch.commit_update_point(plan, committed, fin, 0, mt)
    torch.cuda.synchronize()
    for a, b in zip((walked.rel, walked.conf, walked.t_us, walked.present),
                    (committed.rel, committed.conf, committed.t_us, committed.present)):
        assert _eq(a.cpu().numpy(), b.cpu().numpy())
    with pytest.raises(ValueError):
        batch.commit_update_point(plan, committed, fin, 2, mt)


# ----------------------------------------------------------------------------- store and aggregator
def _history():
    from bayesian_engine.market import MarketId, MarketStore

    rng = np.random.default_rng(12)
    ms = MarketStore()
    for i in range(12):
        market = ms.create_market(MarketId(f"pol:{i}"))
        for _ in range(int(rng.integers(2, 6))):
            market.add_signal({"sourceId": f"src{int(rng.integers(0, 5))}", "probability": float(rng.random())})
        market.created_at = f"2024-01-{1 + 2 * i:02d}T00:00:00+00:00"
        if i != 5:
            market.resolve(bool(rng.integers(0, 2)))
            market.resolved_at = f"2024-01-{2 + 2 * i + (5 if i % 3 == 0 else 0):02d}T12:00:00+00:00"
    return ms


@pytest.mark.parametrize("lagged", [False, True])
def test_store_and_aggregator(tmp_path, lagged):
    from bayesian_engine.market import CrossMarketAggregator
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    agg = CrossMarketAggregator(_history())
    store = NamespacedReliabilityStore(str(tmp_path / "u.db"))
    lr, cap, hl, mr = [0.05, 0.15, 0.4], [0.1, 0.1, 0.25], [30.0, 3.0], [0.1]
    _, markets, stamps, rstamps = agg._walk_history(None, None, lagged)
    scores = store.sweep_update(markets, stamps, lr, cap, hl, mr, domain="d", resolve_times=rstamps)
    decay = store.sweep_decay(markets, stamps, hl, mr, domain="d", resolve_times=rstamps)
    assert scores.counts.shape[0] == 6 and int(scores.n_scored[0, 0]) > 0
    _same_scores(batch.ScoreResult(*(getattr(scores, f)[2:4] for f in FIELDS)), decay, "the default rule")
    rows = agg.sweep_update(store, lr, cap, hl, mr, domain="d", lagged=lagged)
    drows = agg.sweep_decay(store, hl, mr, domain="d", lagged=lagged)
    assert [r.params for r in rows] == [{"learning_rate": r, "max_step": c, "half_life_days": h, "min_rel": m}
                                        for r, c in zip(lr, cap) for h in hl for m in mr]
    for got, exp in zip(rows[2:4], drows):
        assert (got.n, got.brier, got.log_loss, got.accuracy) == (exp.n, exp.brier, exp.log_loss, exp.accuracy)
    assert len({r.brier for r in rows}) > 2  # the rule moves the score
    one = agg.sweep_update(store, 0.15, domain="d", lagged=lagged)  # a lone number, the default decay
    assert len(one) == 1 and one[0].params == {"learning_rate": 0.15, "max_step": 0.1,
                                               "half_life_days": DECAY_HALF_LIFE_DAYS, "min_rel": DECAY_MINIMUM}
    assert one[0].brier == rows[2].brier
    kw = dict(n_boot=16, seed=3, block=2)
    s1, b1 = store.compare_update(markets, stamps, lr, cap, hl, mr, domain="d", resolve_times=rstamps, **kw)
    s2, b2 = store.compare_update(markets, stamps, lr, cap, hl, mr, domain="d", resolve_times=rstamps, **kw)
    _same_scores(s1, scores, "compare_update's sweep")
    assert b1.counts.shape == (17, 1, 6, 2)
    assert torch.equal(b1.counts, b2.counts) and torch.equal(b1.sums.view(torch.int64), b2.sums.view(torch.int64))
    c1 = agg.compare_update(store, lr, cap, hl, mr, domain="d", lagged=lagged, **kw)
    c2 = agg.compare_update(store, lr, cap, hl, mr, domain="d", lagged=lagged, **kw)
    assert c1 == c2 and len(c1.rows) == 6 and [r.params for r in c1.rows] == [r.params for r in rows]
    assert c1.best == int(np.argmin(b1.point("brier")[0].cpu().numpy())) == c1.reference
    assert store._store.list_sources("__domain__:d") == []  # nothing was written
    store.close()
