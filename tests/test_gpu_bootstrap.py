"""GPU checks of the bootstrap of back-test scores (bce_score_bootstrap, batch.score_bootstrap,
the compare_decay methods) against tests/boot_ref.py: the counts and the brier / brier_base sums
of every replicate equal the shaped reference to the bit; the log-loss sums equal it to the bit
when the reference is fed the device's own per-item log terms (batch.score over one group per
item), and independently lie within 4 ulp per term times the weight, plus one rounding of each
product, plus the summation bound, of the reference over ``-math.log``."""
import math

import numpy as np
import pytest
import torch

import boot_ref as B
import score_ref as R
from bayesian_engine import _native as N
from bayesian_engine import batch

pytestmark = pytest.mark.gpu

NB = 256  # rows 0 .. 256: one full workgroup of replicates and one that holds a single lane
SEED = 5
LOG_ULP_CAP = 4  # tests/test_gpu_score.py: its stated cap on a log-loss term against -math.log


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _plan(fx, check=True):
    return batch.ScorePlan.groups(_T(fx["goff"]), _T(fx["pidx"]), _T(fx.get("oidx")), check=check)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def _boot(fx, values=None, valids=None, unit=None, n_boot=NB, seed=SEED, plan=None, faults=True, **kw):
    value = fx["value"] if values is None else np.stack(values)
    valid = fx.get("valid") if valids is None else np.stack(valids)
    r = batch.score_bootstrap(plan or _plan(fx), _T(value), _T(fx["outcome"]), valid=_T(valid), base=_T(fx.get("base")),
                              unit=_T(unit), n_boot=n_boot, seed=seed, eps=fx["eps"], **kw)
    if faults:
        N.check_faults(_dev(), "score_bootstrap")
    return r.counts.cpu().numpy(), r.sums.cpu().numpy(), r


def _device_log_terms(fx, value=None, valid=None):
    """The device's own log-loss term of every item: batch.score over one group per item."""
    items = R.per_item(fx)
    r = batch.score(_plan(items), _T(fx["value"] if value is None else value), _T(fx["outcome"]),
                    valid=_T(fx.get("valid") if valid is None else valid), base=_T(fx.get("base")), eps=fx["eps"])
    N.check_faults(_dev(), "score")
    return r.sums[:, 1].cpu().numpy()


def _log_bound(w, terms):
    """Of one group and replicate: weights w[n], the -math.log terms[n] of its scored items."""
    pairs = [(int(a), float(t)) for a, t in zip(w, terms) if a and t]
    per_term = sum(a * LOG_ULP_CAP * math.ulp(t) for a, t in pairs) * (1 + len(pairs) * 2.0 ** -52)
    product = sum(math.ulp(a * t) for a, t in pairs)  # w * t is rounded once on either side
    return per_term + product + R.sum_bound([a * t for a, t in pairs])


def _check(fx, counts, sums, what, unit=None, values=None, valids=None, seed=SEED):
    """Everything against the shaped reference; returns the reference over -math.log."""
    reps = np.arange(counts.shape[0])
    K = counts.shape[2]
    vals = [fx["value"]] if values is None else values
    vlds = [fx.get("valid")] * K if valids is None else valids
    own = [_device_log_terms(fx, vals[k], vlds[k]) for k in range(K)]
    ref = B.boot_ref(fx, seed, reps, values=values, valids=valids, unit=unit)
    dev = B.boot_ref(fx, seed, reps, values=values, valids=valids, unit=unit, log_terms=own)
    assert np.array_equal(counts, ref["counts"]), (what, "counts")
    assert _same_bits(sums[..., 0], ref["sums"][..., 0]), (what, "brier")
    assert _same_bits(sums[..., 2], ref["sums"][..., 2]), (what, "brier_base")
    assert _same_bits(sums[..., 1], dev["sums"][..., 1]), (what, "log loss over the device's own terms")
    for g, grp in enumerate(ref["groups"]):
        for k in range(K):
            t = grp["terms"][0, k, 1]  # replicate 0 has weight 1: the terms themselves
            if not np.isfinite(t).all():
                continue  # eps = 0: an infinite term; the bit comparison above covers it
            for r in (0, 1, 2, len(reps) - 1):
                bound = _log_bound(grp["w"][r], t)
                assert abs(sums[r, g, k, 1] - ref["sums"][r, g, k, 1]) <= bound, (what, g, k, r, "log loss")
    return ref


FIXTURES = B.all_fixtures()


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_every_replicate_against_the_reference(name):
    fx = FIXTURES[name]
    counts, sums, r = _boot(fx)
    G = len(fx["goff"]) - 1
    assert counts.shape == (NB + 1, G, 1, 2) and sums.shape == (NB + 1, G, 1, 3)
    _check(fx, counts, sums, name)
    # row 0 against batch.score: the same items, another summation shape
    s = batch.score(_plan(fx), _T(fx["value"]), _T(fx["outcome"]), valid=_T(fx.get("valid")), base=_T(fx.get("base")),
                    n_bins=fx["B"], eps=fx["eps"])
    N.check_faults(_dev(), "score")
    sc, ss = s.counts.cpu().numpy(), s.sums.cpu().numpy()
    assert np.array_equal(counts[0, :, 0, 0], sc[:, 0]) and np.array_equal(counts[0, :, 0, 1], sc[:, 1]), name
    own = _device_log_terms(fx)
    dev = B.boot_ref(fx, SEED, [0], log_terms=[own])
    for g in range(G):
        for c in range(3):
            t = dev["groups"][g]["terms"][0, 0, c]
            if np.isfinite(t).all():
                assert abs(sums[0, g, 0, c] - ss[g, c]) <= R.sum_bound(t), (name, g, c)
            else:
                assert sums[0, g, 0, c] == ss[g, c] == math.inf, (name, g, c)
    if name == "tile":
        assert np.diff(fx["goff"]).tolist() == [B.TILE - 1, B.TILE, B.TILE + 1, 3 * B.TILE + 1]
        assert batch.BOOT_TILE == B.TILE
    if name == "lengths":
        assert not counts[:, 0].any() and not sums[:, 0].any()  # the empty group, in every replicate
        assert len({int(x) for x in counts[1:, -1, 0, 0]}) > 50  # the replicates do differ
        again, again_s, _ = _boot(fx)
        assert np.array_equal(again, counts) and _same_bits(again_s, sums)  # two runs: every bit
        rev = R.fx_lengths(reverse=True)
        back, back_s, _ = _boot(rev)
        assert np.array_equal(back[:, ::-1], counts) and _same_bits(back_s[:, ::-1], sums)  # not the other groups


def _raw(fx, value, valid, rep0, n_rep, n_sets=1, seed=SEED, unit=None):
    """bce_score_bootstrap itself, for a replicate range."""
    L = N.require_gpu()
    plan = _plan(fx)
    G, M = plan.n_groups, len(fx["outcome"])
    value, valid = _T(np.ascontiguousarray(value)), _T(valid)
    counts = torch.zeros((n_rep, G, n_sets, 2), dtype=torch.int64, device=_dev())
    sums = torch.zeros((n_rep, G, n_sets, 3), dtype=torch.float64, device=_dev())
    sb = int(L.bce_boot_scratch_bytes(plan.n_segments, n_rep, n_sets))
    scratch = torch.empty(sb // 8, dtype=torch.int64, device=_dev())
    n_values = value.shape[-1]
    outcome, base, unit = _T(fx["outcome"]), _T(fx.get("base")), _T(unit)
    N.check(L.bce_score_bootstrap(N.ptr(plan.group_offsets), G, N.ptr(plan.seg_start), N.ptr(plan.seg_group),
                                  plan.n_segments, N.ptr(plan.pidx), N.ptr(plan.oidx), plan.n_items, N.ptr(value),
                                  n_values, n_values, n_sets, N.ptr(outcome), N.ptr(valid),
                                  M if valid is not None and valid.dim() == 2 else 0, N.ptr(base), N.ptr(unit), M,
                                  fx["eps"], seed, rep0, n_rep, N.ptr(scratch), sb, N.ptr(counts), N.ptr(sums),
                                  N.stream(_dev())), "bce_score_bootstrap")
    N.check_faults(_dev(), "bce_score_bootstrap")
    return counts.cpu().numpy(), sums.cpu().numpy()


def test_tiling_of_sets_and_replicates_changes_no_bit():
    fx = B.fx_tile()
    rng = np.random.default_rng(3)
    K = batch.BOOT_MAX_SETS + 1
    M = len(fx["outcome"])
    values = [rng.random(M) for _ in range(K)]
    valids = [(rng.random(M) < 0.8).astype(np.uint8) for _ in range(K)]
    counts, sums, _ = _boot(fx, values=values, valids=valids)
    assert counts.shape == (NB + 1, 4, K, 2)
    for k in range(K):  # every set alone
        c1, s1, _ = _boot(fx, values=[values[k]], valids=[valids[k]])
        assert np.array_equal(c1[:, :, 0], counts[:, :, k]) and _same_bits(s1[:, :, 0], sums[:, :, k]), k
    assert not np.array_equal(counts[:, :, 0], counts[:, :, 1])
    _check(fx, counts[:, :, 7:], sums[:, :, 7:], "sets 7 and 8", values=values[7:], valids=valids[7:])
    # one mask for all sets (valid_stride = 0)
    shared, shared_s, _ = _boot(fx, values=values[:3])
    c1, s1, _ = _boot(fx, values=[values[2]])
    assert np.array_equal(shared[:, :, 2], c1[:, :, 0]) and _same_bits(shared_s[:, :, 2], s1[:, :, 0])
    # replicate ranges
    whole = _raw(fx, values[0], valids[0], 0, NB + 1)
    assert np.array_equal(whole[0], counts[:, :, :1]) and _same_bits(whole[1], sums[:, :, :1])
    lo, hi = _raw(fx, values[0], valids[0], 0, 100), _raw(fx, values[0], valids[0], 100, NB + 1 - 100)
    assert np.array_equal(np.concatenate([lo[0], hi[0]]), whole[0])
    assert _same_bits(np.concatenate([lo[1], hi[1]]), whole[1])
    # a scratch budget that forces both tilings: 100 replicates of 8 sets at a time
    n_seg = _plan(fx).n_segments
    small, small_s, _ = _boot(fx, values=values, valids=valids, scratch_budget=n_seg * 8 * 40 * 100)
    assert np.array_equal(small, counts) and _same_bits(small_s, sums)


def test_resampling_units():
    fx = R.fx_random(10)
    M = len(fx["outcome"])
    blocks = np.arange(M, dtype=np.int64) // 7
    counts, sums, _ = _boot(fx, unit=blocks)
    _check(fx, counts, sums, "unit = m // 7", unit=blocks)
    rng = np.random.default_rng(9)
    ids = rng.integers(-2 ** 63, 2 ** 63 - 1, M, dtype=np.int64)
    ids[:4] = (-1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0)
    ids[10], ids[20] = ids[3], ids[3]
    counts, sums, _ = _boot(fx, unit=ids)
    _check(fx, counts, sums, "arbitrary ids", unit=ids)
    # one market per group: W is the weight itself; markets of one unit share it in every replicate
    scored = [m for m in range(M) if fx["outcome"][m] >= 0 and fx["valid"][m]]
    a, b, c = scored[0], scored[1], scored[2]
    ids[a] = ids[b] = 12345
    ids[c] = 12346
    each = dict(fx, goff=np.arange(M + 1, dtype=np.int64), pidx=np.arange(M, dtype=np.int64))
    counts, _, _ = _boot(each, unit=ids, n_boot=64)
    W = counts[:, :, 0, 0]
    assert np.array_equal(W[:, a], W[:, b]) and not np.array_equal(W[:, a], W[:, c])
    host = batch.boot_weights(SEED, np.arange(65), ids).numpy()
    assert np.array_equal(counts[:, scored, 0, 0], host[:, scored])
    assert (counts[0, scored, 0, 0] == 1).all() and not counts[:, [m for m in range(M) if m not in scored]].any()


def test_signals_of_a_market_share_its_weight_under_a_per_source_plan():
    fx = R.fx_sources_items()
    n = 3000
    items = dict(fx, goff=np.arange(n + 1, dtype=np.int64), pidx=fx["pidx"][:n], oidx=fx["oidx"][:n])
    counts, _, _ = _boot(items, n_boot=16)
    market = items["oidx"]
    host = batch.boot_weights(SEED, np.arange(17), market).numpy()
    scored = counts[0, :, 0, 0] == 1
    assert scored.sum() > 1000 and np.array_equal(counts[:, scored, 0, 0], host[:, scored])
    m = np.bincount(market[scored]).argmax()  # a market with many scored signals, of several sources
    rows = np.flatnonzero(scored & (market == m))
    assert len(rows) > 1 and (counts[:, rows, 0, 0] == counts[:, rows[:1], 0, 0]).all()


def test_bad_offsets_and_indices_raise_the_fault_word_and_spare_the_other_groups():
    good = R.fx_overlap()
    want, want_s, _ = _boot(good, n_boot=8)
    pidx = good["pidx"].copy()
    pidx[7] = 6   # outside the values
    pidx[8] = -1
    fx = dict(good, pidx=pidx)
    got, got_s, _ = _boot(fx, n_boot=8, faults=False)
    with pytest.raises(N.BCEError):
        N.check_faults(_dev(), "score_bootstrap")
    assert np.array_equal(got[:, 0], want[:, 0]) and _same_bits(got_s[:, 0], want_s[:, 0])
    ref = B.boot_ref(fx, SEED, np.arange(9))  # the reference leaves an item outside its arrays out
    assert np.array_equal(got[:, 1], ref["counts"][:, 1]) and _same_bits(got_s[:, 1, :, 0], ref["sums"][:, 1, :, 0])
    assert got[0, 1, 0, 0] == want[0, 1, 0, 0] - 1  # item 7 was scored, item 8 is unresolved either way
    # offsets that decrease: the group reads as empty
    fx = dict(good, goff=np.array([0, 7, 5, 10], np.int64))
    got, got_s, _ = _boot(fx, n_boot=8, plan=_plan(fx, check=False), faults=False)
    with pytest.raises(N.BCEError):
        N.check_faults(_dev(), "score_bootstrap")
    assert not got[:, 1].any() and not got_s[:, 1].any()
    first = B.boot_ref(dict(good, goff=np.array([0, 7], np.int64)), SEED, np.arange(9))
    assert np.array_equal(got[:, 0], first["counts"][:, 0]) and _same_bits(got_s[:, 0, :, 0], first["sums"][:, 0, :, 0])
    N.check_faults(_dev(), "cleared")  # the word was cleared: the next call is clean
    again, _, _ = _boot(good, n_boot=8)
    assert np.array_equal(again, want)


def test_planted_differences():
    rng = np.random.default_rng(17)
    M = 400
    outcome = rng.integers(0, 2, M).astype(np.int8)
    a = np.clip(outcome + rng.uniform(-0.05, 0.05, M), 0.0, 1.0)
    fx = dict(goff=np.array([0, M], np.int64), pidx=np.arange(M, dtype=np.int64), oidx=None, value=a, outcome=outcome,
              valid=None, base=None, B=10, eps=1e-15)
    _, _, r = _boot(fx, values=[a, np.full(M, 0.5), a.copy()])
    for metric in ("brier", "log_loss", "accuracy"):
        pb = r.p_better(metric, 1)[0].cpu().numpy()
        assert pb[0] == 1.0 and pb[2] == 1.0 and pb[1] == 0.0, metric
        d, lo, hi = r.diff(metric, 2)
        assert not d[:, 0, 0].any() and float(lo[0, 0]) == 0.0 == float(hi[0, 0]), metric  # A against its copy
        assert r.p_better(metric, 0)[0, 2] == 0.0 and r.p_better(metric, 2)[0, 0] == 0.0, metric
        best = r.p_best(metric)[0].cpu().numpy()
        assert best.sum() == 1.0 and best.tolist() == [1.0, 0.0, 0.0], metric  # the tie goes to the lower index
    lo, hi = r.interval("brier")
    assert float(lo[0, 0]) <= float(hi[0, 0]) < 0.01 and float(lo[0, 1]) == 0.25 == float(hi[0, 1])
    assert float(r.stderr("brier")[0, 1]) == 0.0 and float(r.stderr("brier")[0, 0]) > 0.0


# ------------------------------------------------------------------------------------ end to end
def _history():
    from bayesian_engine.market import MarketId, MarketStore

    rng = np.random.default_rng(61)
    ms = MarketStore()
    for i in range(60):
        market = ms.create_market(MarketId(f"{'pol' if i % 3 else 'spo'}:{i}"))
        for _ in range(int(rng.integers(1, 6))):
            market.add_signal({"sourceId": f"src{int(rng.integers(0, 6))}", "probability": float(rng.random())})
        market.created_at = f"2024-01-{1 + i % 28:02d}T00:00:00+00:00"
        if i % 6:
            market.resolve(bool(rng.integers(0, 2)))
            market.resolved_at = f"2024-0{2 + i % 2}-{1 + (7 * i) % 28:02d}T12:00:00+00:00"
    return ms


@pytest.mark.parametrize("walk", ["plain", "lagged", "namespaced"])
def test_compare_decay_end_to_end(tmp_path, monkeypatch, walk):
    from bayesian_engine.market import CrossMarketAggregator
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    agg = CrossMarketAggregator(_history())
    store = NamespacedReliabilityStore(str(tmp_path / "c.db"))
    hl, mr = [30.0, 3.0], [0.1, 0.45]
    seen = {}
    name = "walk_sweep_scoped" if walk == "namespaced" else "walk_sweep"
    real = getattr(batch, name)

    def spy(plan, *a, **kw):
        out = real(plan, *a, **kw)
        if kw.get("keep_consensus"):
            seen["kept"], seen["outcome"] = out[1], plan.outcome
        return out

    monkeypatch.setattr(batch, name, spy)
    kw = dict(n_boot=NB, seed=11, block=3)
    if walk == "namespaced":
        _, markets, stamps, rstamps, skw = agg._namespaced_history("category", None, False, False, True, None)
        scores, boot = store.compare_decay_namespaced(markets, stamps, hl, mr, resolve_times=rstamps, **skw, **kw)
        alone = store.sweep_decay_namespaced(markets, stamps, hl, mr, resolve_times=rstamps, **skw)
        cmp = agg.compare_decay_namespaced(store, hl, mr, "category", lagged=True, **kw)
    else:
        lagged = walk == "lagged"
        _, markets, stamps, rstamps = agg._walk_history(None, None, lagged)
        scores, boot = store.compare_decay(markets, stamps, hl, mr, domain="d", resolve_times=rstamps, **kw)
        alone = store.sweep_decay(markets, stamps, hl, mr, domain="d", resolve_times=rstamps)
        cmp = agg.compare_decay(store, hl, mr, domain="d", lagged=lagged, **kw)
    for f in ("counts", "sums", "bin_n", "bin_pos", "bin_psum"):  # the ScoreResult of the sweep itself
        assert torch.equal(getattr(scores, f).view(torch.int64), getattr(alone, f).view(torch.int64)), f
    cons, nulls = seen["kept"]
    outcome = seen["outcome"].cpu().numpy()
    M = len(outcome)
    assert cons.shape == (4, M) and boot.counts.shape == (NB + 1, 1, 4, 2)
    fx = dict(goff=np.array([0, M], np.int64), pidx=np.arange(M, dtype=np.int64), oidx=None, value=None, outcome=outcome,
              valid=None, base=None, B=10, eps=1e-15)
    values = list(cons.cpu().numpy())
    valids = list((~nulls).cpu().numpy().astype(np.uint8))
    _check(fx, boot.counts.cpu().numpy(), boot.sums.cpu().numpy(), walk, unit=np.arange(M, dtype=np.int64) // 3,
           values=values, valids=valids, seed=11)
    assert torch.equal(boot.counts[0, 0, :, 0], scores.n_scored[:, 0]) and int(boot.W[0, 0, 0]) > 20
    # the comparison is read off the same result
    point = boot.point("brier")[0].cpu().numpy()
    assert cmp.best == int(np.argmin(point)) == cmp.reference and cmp.metric == "brier" and len(cmp.rows) == 4
    assert [r.params for r in cmp.rows] == [{"half_life_days": h, "min_rel": m} for h in hl for m in mr]
    lo, hi = boot.interval("brier")
    d, dlo, dhi = boot.diff("brier", cmp.reference)
    for k, row in enumerate(cmp.rows):
        assert row.n == int(boot.W[0, 0, k]) and row.value == point[k]
        assert abs(row.value - float(scores.brier[k, 0])) <= 1e-12  # the same terms in another summation shape
        assert (row.lo, row.hi) == (float(lo[0, k]), float(hi[0, k])) and row.lo <= row.hi
        assert (row.diff, row.diff_lo, row.diff_hi) == (float(d[0, 0, k]), float(dlo[0, k]), float(dhi[0, k]))
        assert row.diff_lo <= row.diff_hi and row.diff >= 0.0  # no point estimate beats the best one
        assert row.p_better == float(boot.p_better("brier", cmp.reference)[0, k])
    ref = cmp.rows[cmp.reference]
    assert (ref.diff, ref.diff_lo, ref.diff_hi, ref.p_better) == (0.0, 0.0, 0.0, 0.0)
    assert abs(sum(r.p_best for r in cmp.rows) - 1.0) < 1e-12
    other = agg.compare_decay(store, hl, mr, domain="d", n_boot=8, reference=3, metric="accuracy") \
        if walk == "plain" else None
    if other is not None:
        assert other.reference == 3 and other.rows[3].diff == 0.0 and other.metric == "accuracy"
        acc = [r.value for r in other.rows]
        assert other.best == acc.index(max(acc))
    store.close()
