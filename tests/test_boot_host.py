"""CPU checks of the bootstrap (include/bce.h: bce_boot_weights_host, bce_score_bootstrap's
argument checks; batch.bootstrap): the committed threshold table against its ``decimal``
derivation, the host weights against the numpy restatement of tests/boot_ref.py, the sampler's
distribution, the reference against ``math.fsum`` and tests/score_ref.py, the statistics of
``BootstrapResult`` against plain numpy, and the argument errors.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import boot_ref as B
import score_ref as R
from bayesian_engine import _native as N
from bayesian_engine import batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def test_the_committed_threshold_table_is_the_decimal_derivation():
    src = open(os.path.join(ROOT, "bayesian-consensus-engine_amd", "csrc", "boot_weights.hpp")).read()
    body = re.search(r"constexpr uint64_t T\[kBootThresholds\] = \{(.*?)\};", src, flags=re.S).group(1)
    table = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{16})ull", body)]
    exp = B.thresholds()
    assert len(exp) == 21 and table == exp
    assert (exp[0], exp[1], exp[19], exp[20]) == (0x5e2d58d8b3bcdf1a, 0xbc5ab1b16779be35, 0xfffffffffffffffd,
                                                  0xffffffffffffffff)
    assert all(a < b for a, b in zip(exp, exp[1:]))
    # the numpy mixer is the plain statement of the header
    for z in (0, 1, B.GOLD, B.MASK, 0x0123456789ABCDEF):
        assert int(B.mix(np.array([z], np.uint64))[0]) == B.mix_int(z)
    h = np.array([0, exp[0] - 1, exp[0], exp[5], exp[6] - 1, exp[6], exp[19], B.MASK], np.uint64)
    assert B.count(h).tolist() == [0, 0, 1, 6, 6, 7, 20, 21]


def test_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "bce.h")).read()
    define = dict(re.findall(r"^#define[ \t]+(BCE_BOOT_[A-Z_]+)[ \t]+(\d+)", src, flags=re.M))
    assert int(define["BCE_BOOT_MAX_SETS"]) == N.BOOT_MAX_SETS == batch.BOOT_MAX_SETS == B.MAX_SETS
    assert int(define["BCE_BOOT_TILE"]) == N.BOOT_TILE == batch.BOOT_TILE == B.TILE
    assert B.SEG == batch.SCORE_SEG and B.SEG % B.TILE == 0


def test_host_weights_equal_the_numpy_restatement():
    reps = [0, 1, 2, 255, 2 ** 31, 2 ** 62]
    units = np.array([-2 ** 63, -1, 0, 1, 2 ** 40], np.int64)
    seen = set()
    for seed in (0, 1, 2 ** 64 - 1):
        got = batch.boot_weights(seed, reps, units)
        assert got.dtype == torch.int32 and tuple(got.shape) == (6, 5) and got.device.type == "cpu"
        assert np.array_equal(got.numpy(), B.weights(seed, reps, units)), seed
        assert (got[0] == 1).all()  # replicate 0 is the sample itself
        key = B.mix_int(seed + 2 * B.GOLD)
        h = B.mix_int(key ^ B.mix_int((2 ** 40 + B.GOLD) & B.MASK))  # one draw, on Python ints
        assert int(got[2, 4]) == sum(h >= t for t in B.thresholds())
        seen.add(tuple(got.numpy().ravel()))
    assert len(seen) == 3  # the seed matters
    assert np.array_equal(batch.boot_weights(-1, reps, units).numpy(), batch.boot_weights(2 ** 64 - 1, reps, units).numpy())
    assert tuple(batch.boot_weights(3, [], units).shape) == (0, 5) and tuple(batch.boot_weights(3, reps, []).shape) == (6, 0)


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_the_weights_are_poisson_one(seed):
    """The four limits are the issue's conditions on the sampler, not measurements of it."""
    reps, units = np.arange(1, 257), np.arange(4096)
    w = batch.boot_weights(seed, reps, units).numpy()
    assert np.array_equal(w, B.weights(seed, reps, units))  # 2^20 draws, the rare tail branch included
    assert w.min() == 0 and 7 <= w.max() <= 21
    x = w.astype(np.float64)
    print(f"seed {seed}: mean {x.mean():.5f} var {x.var():.5f} max {w.max()}")
    assert abs(x.mean() - 1.0) <= 0.005
    assert abs(x.var() - 1.0) <= 0.01
    for k in range(6):
        assert abs((w == k).mean() - B.poisson_mass(k)) <= 0.003, k
    c = np.corrcoef(x[:64])
    assert np.abs(c - np.eye(64)).max() <= 0.1


@pytest.mark.parametrize("name", sorted(B.all_fixtures()))
def test_reference_against_fsum_and_the_scoring_reference(name):
    fx = B.all_fixtures()[name]
    rows = [0, 1, 2, 255, 256]
    ref = B.boot_ref(fx, 5, rows)
    exact = B.fsum_sums(ref, range(len(rows)))
    base = R.score_ref(fx)
    assert np.array_equal(ref["counts"][0, :, 0, 0], base["counts"][:, 0])  # row 0: n_scored and n_hit
    assert np.array_equal(ref["counts"][0, :, 0, 1], base["counts"][:, 1])
    for g, grp in enumerate(ref["groups"]):
        wmax = int(grp["w"].max()) if grp["w"].size else 0
        for c in range(3):
            t = base["terms"][g][c]
            assert np.array_equal(grp["terms"][0, 0, c], t, equal_nan=True)  # weight 1: the terms of score_ref
            if not np.isfinite(t).all():
                continue
            for x in range(len(rows)):
                assert abs(ref["sums"][x, g, 0, c] - exact[x, g, 0, c]) <= R.sum_bound(t) * wmax, (name, g, c, x)
    assert (ref["counts"][..., 1] <= ref["counts"][..., 0]).all()


def _hand_built():
    """R = 6 replicates, G = 2 groups, K = 3 sets: ties, a NaN replicate, an empty group."""
    counts = np.zeros((7, 2, 3, 2), np.int64)
    sums = np.zeros((7, 2, 3, 3), np.float64)
    W = np.array([10, 8, 12, 0, 9, 10, 11])  # replicate 3 drew nothing: every metric is NaN there
    brier = np.array([[0.20, 0.25, 0.20], [0.10, 0.30, 0.10], [0.30, 0.20, 0.30], [0, 0, 0], [0.25, 0.25, 0.40],
                      [0.15, 0.10, 0.15], [0.50, 0.60, 0.40]])
    counts[:, 0, :, 0] = W[:, None]
    counts[:, 0, :, 1] = (W // 2)[:, None] + np.array([0, 1, 0])[None, :] * (W > 0)[:, None]
    sums[:, 0, :, 0] = brier * W[:, None]
    sums[:, 0, :, 1] = 2.0 * brier * W[:, None]
    sums[:, 0, :, 2] = 0.25 * W[:, None]
    return batch.BootstrapResult(torch.from_numpy(counts), torch.from_numpy(sums), has_base=True)


def test_bootstrap_result_statistics_against_numpy():
    r = _hand_built()
    assert r.n_boot == 6 and tuple(r.brier.shape) == (7, 2, 3)
    x = r.brier.numpy()
    assert np.isnan(x[3]).all() and np.isnan(x[:, 1]).all()  # W == 0: the NaN replicate, the empty group
    W = r.W.numpy()[:, 0, 0]
    exp = r.sums.numpy()[:, 0, :, 0] / np.where(W > 0, W, 1)[:, None]
    live = [1, 2, 4, 5, 6]  # the replicates that drew something
    assert np.array_equal(x[live, 0], exp[live]) and np.array_equal(r.point("brier").numpy()[0], exp[0])
    lo, hi = r.interval("brier", 0.9)
    assert np.allclose(lo.numpy()[0], np.quantile(exp[live], 0.05, axis=0), rtol=0, atol=1e-15)
    assert np.allclose(hi.numpy()[0], np.quantile(exp[live], 0.95, axis=0), rtol=0, atol=1e-15)
    assert np.isnan(lo.numpy()[1]).all() and np.isnan(hi.numpy()[1]).all()
    assert np.allclose(r.stderr("brier").numpy()[0], exp[live].std(axis=0, ddof=1), rtol=1e-14, atol=0)
    assert np.isnan(r.stderr("brier").numpy()[1]).all()
    d, dlo, dhi = r.diff("brier", 1, 0.9)
    dexp = exp - exp[:, 1:2]
    assert np.array_equal(d.numpy()[live, 0], dexp[live]) and not d.numpy()[:, 0, 1][live].any()
    assert np.allclose(dlo.numpy()[0], np.quantile(dexp[live], 0.05, axis=0), rtol=0, atol=1e-15)
    assert np.allclose(dhi.numpy()[0], np.quantile(dexp[live], 0.95, axis=0), rtol=0, atol=1e-15)
    # strictly better than set 1: replicate 4 ties for set 0 (0.25 == 0.25) and counts for neither
    pb = r.p_better("brier", 1).numpy()
    assert pb[0].tolist() == [(exp[live, k] < exp[live, 1]).mean() for k in range(3)] == [0.4, 0.0, 0.4]
    assert np.isnan(pb[1]).all()
    assert r.p_better("brier", 0).numpy()[0, 2] == 0.2  # equal in three replicates, better in one, worse in one
    # the best set: sets 0 and 2 tie in replicates 1 and the tie goes to set 0
    best = r.p_best("brier").numpy()
    first = np.bincount(np.argmin(exp[live], axis=1), minlength=3) / len(live)  # argmin: the first minimum
    assert best[0].tolist() == first.tolist() == [0.4, 0.4, 0.2] and best[0].sum() == 1.0
    assert np.isnan(best[1]).all()
    # accuracy: higher is better
    acc = r.accuracy.numpy()[:, 0]
    assert np.array_equal(acc[live], (r.counts.numpy()[live, 0, :, 1] / W[live, None]))
    assert r.p_better("accuracy", 0).numpy()[0].tolist() == [0.0, 1.0, 0.0]
    assert r.p_best("accuracy").numpy()[0].tolist() == [0.0, 1.0, 0.0]
    assert np.array_equal(r.log_loss.numpy()[live, 0], (r.sums.numpy()[live, 0, :, 1] / W[live, None]))
    assert np.array_equal(r.skill.numpy()[live, 0], x[live, 0] - r.brier_base.numpy()[live, 0])
    # a set that is NaN in one replicate only never wins it, and is left out of its own shares
    counts = r.counts.clone()
    counts[2, 0, 1] = 0
    one = batch.BootstrapResult(counts, r.sums, has_base=True)
    assert one.p_best("brier").numpy()[0].tolist() == [0.6, 0.2, 0.2]
    assert one.p_better("brier", 1).numpy()[0].tolist() == [0.5, 0.0, 0.5]
    with pytest.raises(ValueError):
        batch.BootstrapResult(r.counts, r.sums).skill
    for bad in (dict(metric="ece", ref=0), dict(metric="brier", ref=3), dict(metric="brier", ref=-1)):
        with pytest.raises(ValueError):
            r.p_better(**bad)
    with pytest.raises(TypeError):
        r.diff("brier", 1.0)
    with pytest.raises(ValueError):
        r.interval("brier", 1.0)
    empty = batch.BootstrapResult(r.counts[:1], r.sums[:1])  # n_boot = 0: no replicate, NaN limits
    assert np.isnan(empty.interval("brier")[0].numpy()).all() and empty.point("brier")[0, 0] == 0.2


def _call(**over):
    """bce_score_bootstrap with valid arguments over host buffers (never launched: every call here
    is refused by an argument check first), ``over`` replacing some."""
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    a = dict(group_offsets=p, n_groups=1, seg_start=p, seg_group=p, n_segments=1, pidx=p, oidx=None, n_items=4, value=p,
             n_values=4, value_stride=4, n_sets=1, outcome=p, valid=None, valid_stride=0, base=None, unit=None,
             n_markets=4, eps=1e-15, seed=0, rep0=0, n_rep=2, scratch=p, scratch_bytes=80, counts=p, sums=p,
             stream=None)
    a.update(over)
    return N.load_library().bce_score_bootstrap(*a.values()), buf


def test_argument_errors_need_no_gpu():
    lib = N.load_library()
    assert lib.bce_boot_scratch_bytes(3, 257, 8) == 3 * 257 * 8 * 40 and lib.bce_boot_scratch_bytes(1, 2, 1) == 80
    assert lib.bce_boot_scratch_bytes(1, 1, 0) == 0 and lib.bce_boot_scratch_bytes(1, 1, batch.BOOT_MAX_SETS + 1) == 0
    assert lib.bce_boot_scratch_bytes(-1, 1, 1) == 0 and lib.bce_boot_scratch_bytes(2 ** 40, 2 ** 40, 8) == 0
    bad = [dict(n_groups=-1), dict(n_items=-1), dict(n_values=-1), dict(n_markets=-1), dict(n_rep=-1),
           dict(n_segments=-1), dict(value_stride=-1), dict(valid_stride=-1), dict(n_sets=0),
           dict(n_sets=batch.BOOT_MAX_SETS + 1), dict(rep0=-1), dict(eps=-1e-9), dict(eps=math.nan),
           dict(group_offsets=None), dict(seg_start=None), dict(seg_group=None), dict(pidx=None), dict(value=None),
           dict(outcome=None), dict(counts=None), dict(sums=None), dict(scratch=None), dict(scratch_bytes=79),
           dict(n_segments=0)]
    for over in bad:
        rc, _ = _call(**over)
        assert rc == EINVAL and lib.bce_last_error(), over
    rc, buf = _call(scratch_bytes=88, scratch=None)
    assert rc == EINVAL
    rc, buf = _call(scratch=np.zeros(64, np.int64).ctypes.data + 4, scratch_bytes=200)  # misaligned
    assert rc == EINVAL and b"aligned" in lib.bce_last_error()
    assert _call(n_groups=0, group_offsets=None)[0] == 0 and _call(n_rep=0, counts=None)[0] == 0  # nothing to do
    # the host weights
    w = np.zeros(4, np.int32)
    reps, units = np.array([0, -1], np.int64), np.array([1, 2], np.int64)
    assert lib.bce_boot_weights_host(0, N.ptr(reps), 2, N.ptr(units), 2, N.ptr(w)) == EINVAL and not w.any()
    assert lib.bce_boot_weights_host(0, None, 2, N.ptr(units), 2, N.ptr(w)) == EINVAL
    assert lib.bce_boot_weights_host(0, N.ptr(reps), -1, N.ptr(units), 2, N.ptr(w)) == EINVAL
    assert lib.bce_boot_weights_host(0, N.ptr(reps), 1, N.ptr(units), 2, None) == EINVAL
    assert lib.bce_boot_weights_host(0, None, 0, None, 0, None) == 0
    with pytest.raises(ValueError):
        batch.boot_weights(0, [-1], [0])
    with pytest.raises(TypeError):
        batch.boot_weights(0.5, [1], [0])


def test_python_argument_checks_need_no_gpu(tmp_path):
    from bayesian_engine.market import CrossMarketAggregator, MarketStore
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    assert batch.boot_units(7, 3).tolist() == [0, 0, 0, 1, 1, 1, 2] and batch.boot_units(0).numel() == 0
    for bad in ((-1, 1), (3, 0)):
        with pytest.raises(ValueError):
            batch.boot_units(*bad)
    plan = batch.ScorePlan.whole(4)
    value, outcome = torch.rand(4, dtype=torch.float64), torch.tensor([0, 1, 1, -1], dtype=torch.int8)
    ok = dict(plan=plan, value=value, outcome=outcome)
    for over in (dict(n_boot=-1), dict(eps=-1.0), dict(eps=math.nan), dict(scratch_budget=0), dict(value=value.float()),
                 dict(value=value.reshape(1, 2, 2)), dict(outcome=outcome.long()), dict(valid=torch.ones(3)),
                 dict(valid=torch.ones(2, 4)), dict(base=torch.rand(4)), dict(base=torch.rand(5, dtype=torch.float64)),
                 dict(unit=torch.arange(4, dtype=torch.int32)), dict(unit=torch.arange(3))):
        with pytest.raises(ValueError):
            batch.score_bootstrap(**dict(ok, **over))
    for over in (dict(n_boot=2.5), dict(seed="x"), dict(n_boot=True)):
        with pytest.raises(TypeError):
            batch.score_bootstrap(**dict(ok, **over))
    store = NamespacedReliabilityStore(str(tmp_path / "a.db"))
    agg = CrossMarketAggregator(MarketStore())
    for over in (dict(n_boot=0), dict(block=0), dict(metric="ece"), dict(metric="skill"), dict(level=1.0),
                 dict(reference=4), dict(reference=-1), dict(half_life_days=[]), dict(half_life_days=[0.0]),
                 dict(min_rel=[1.5])):
        for fn, extra in ((agg.compare_decay, {}), (agg.compare_decay_namespaced, dict(domain_of="category"))):
            with pytest.raises(ValueError):
                fn(**dict(dict(store=store, half_life_days=[30.0, 3.0], min_rel=[0.1, 0.4]), **extra, **over))
    for over in (dict(n_boot=1.5), dict(block="2"), dict(reference=1.0), dict(store=object())):
        with pytest.raises(TypeError):
            agg.compare_decay(**dict(dict(store=store, half_life_days=[30.0], min_rel=[0.1]), **over))
    for bad in (dict(n_boot=0), dict(block=0)):
        with pytest.raises(ValueError):
            store.compare_decay([], [], [30.0], [0.1], **bad)
        with pytest.raises(ValueError):
            store.compare_decay_namespaced([], [], [30.0], [0.1], **bad)
    with pytest.raises(TypeError):
        store.compare_decay([], [], [30.0], [0.1], n_boot=1.5)
    # a history without signals needs no GPU either
    assert store.compare_decay([], [], [30.0], [0.1]) is None
    assert store.compare_decay_namespaced([], [], [30.0], [0.1]) is None
    cmp = agg.compare_decay(store, [30.0, 3.0], [0.1], n_boot=4)
    assert cmp.best is None and cmp.reference is None and [r.n for r in cmp.rows] == [0, 0]
    assert cmp.rows[1].params == {"half_life_days": 3.0, "min_rel": 0.1} and cmp.rows[0].value is None
    store.close()
