"""Scoring without a GPU: the integer half of batch.ScorePlan on CPU tensors, the shaped reference of
tests/score_ref.py against math.fsum on every fixture of the GPU tests, the BCE_EINVAL paths of
bce_score_groups, batch.ScoreResult's derived formulas and the argument checks of
CrossMarketAggregator.score_walk / sweep_decay."""
import math

import numpy as np
import pytest
import torch

import score_ref as R
from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore


def test_constants_match_the_header():
    assert (batch.SCORE_SEG, batch.SCORE_LANES, batch.SCORE_MAX_BINS) == (R.SEG, R.LANES, 32)
    import os
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "bce.h")).read()
    assert f"#define BCE_SCORE_SEG {R.SEG} " in text and f"#define BCE_SCORE_LANES {R.LANES} " in text
    assert "#define BCE_SCORE_MAX_BINS 32" in text


# ------------------------------------------------------------------------------- plan integers
def test_by_source_on_cpu_tensors_matches_a_dict_of_lists():
    offsets, sid, _, _, _, _ = R.fx_sources()
    plan = batch.ScorePlan.by_source(torch.from_numpy(offsets), torch.from_numpy(sid), 40)
    goff, pidx, oidx, clamped = R.by_source_ref(offsets, sid, 40)
    assert clamped == 0 and plan.n_clamped == 0
    assert np.array_equal(plan.group_offsets.numpy(), goff)
    assert np.array_equal(plan.pidx.numpy(), pidx) and np.array_equal(plan.oidx.numpy(), oidx)
    lens = np.diff(goff)
    assert lens[31] == 0 and lens.max() > R.SEG  # an empty source, and one of more than a segment
    nseg = np.maximum((lens + R.SEG - 1) // R.SEG, 1)
    assert np.array_equal(plan.seg_start.numpy(), np.concatenate([[0], np.cumsum(nseg)]))
    assert plan.n_segments == int(nseg.sum()) and plan.n_groups == 40 and plan.n_items == len(sid)


def test_by_source_clamps_and_counts():
    offsets = np.array([0, 3, 3, 6], np.int64)
    sid = np.array([2, -1, 0, 7, 2, 0], np.int32)
    plan = batch.ScorePlan.by_source(torch.from_numpy(offsets), torch.from_numpy(sid), 3)
    goff, pidx, oidx, clamped = R.by_source_ref(offsets, sid, 3)
    assert plan.n_clamped == clamped == 2
    assert np.array_equal(plan.group_offsets.numpy(), goff) and goff.tolist() == [0, 3, 3, 6]
    assert np.array_equal(plan.pidx.numpy(), pidx) and np.array_equal(plan.oidx.numpy(), oidx)
    for bad in (0, -1, 1 << 31, "x"):
        with pytest.raises(ValueError):
            batch.ScorePlan.by_source(torch.from_numpy(offsets), torch.from_numpy(sid), bad)
    with pytest.raises(ValueError):
        batch.ScorePlan.by_source(torch.tensor([0, 4, 3, 6]), torch.from_numpy(sid), 3)


def test_groups_and_whole():
    fx = R.fx_lengths()
    plan = batch.ScorePlan.groups(torch.from_numpy(fx["goff"]), torch.from_numpy(fx["pidx"]))
    assert plan.oidx is None and plan.n_groups == len(R.LENGTHS)
    assert np.diff(plan.seg_start.numpy()).tolist() == [1, 1, 1, 1, 1, 1, 1, 2, 3]
    whole = batch.ScorePlan.whole(5000)
    assert whole.group_offsets.tolist() == [0, 5000] and whole.n_segments == 3
    assert whole.pidx.tolist() == list(range(5000)) and whole.seg_group.tolist() == [0, 0, 0]
    assert plan.seg_group.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7, 8, 8, 8]
    assert batch.ScorePlan.whole(0).n_segments == 1
    with pytest.raises(ValueError):
        batch.ScorePlan.groups(torch.tensor([0, 5, 3]), torch.arange(5))
    with pytest.raises(ValueError):
        batch.ScorePlan.groups(torch.tensor([0, 6]), torch.arange(5))
    with pytest.raises(ValueError):
        batch.ScorePlan.whole(-1)
    loose = batch.ScorePlan.groups(torch.tensor([0, 5, 3]), torch.arange(5), check=False)  # left to the kernel
    assert loose.seg_start.tolist() == [0, 1, 2]


# ------------------------------------------------------------------------ the reference itself
def test_shaped_sum_is_the_documented_shape():
    x = np.arange(1, 2 * R.SEG + 4, dtype=np.float64) * 0.1
    # written out a second time, element by element
    total = 0.0
    for s in range(0, x.size, R.SEG):
        seg = x[s:s + R.SEG]
        p = [0.0] * R.LANES
        for i, v in enumerate(seg):
            p[i % R.LANES] = p[i % R.LANES] + float(v)
        o = R.LANES // 2
        while o:
            for lane in range(o):
                p[lane] = p[lane] + p[lane + o]
            o //= 2
        total = total + p[0]
    assert R.shaped_sum(x) == total
    assert R.shaped_sum([]) == 0.0 and R.shaped_sum([0.25]) == 0.25


@pytest.mark.parametrize("name", sorted(R.all_fixtures()))
def test_shaped_reference_within_the_summation_bound_of_fsum(name):
    fx = R.all_fixtures()[name]
    ref = R.score_ref(fx)
    G, B = len(fx["goff"]) - 1, fx["B"]
    assert (ref["counts"][:, [0, 2, 3, 4]].sum(1) == np.diff(fx["goff"])).all()
    for g in range(G):
        t = ref["terms"][g]
        cols = [(ref["sums"][g, c], t[c]) for c in range(3)] + [(ref["bin_psum"][g, b], t[3 + b]) for b in range(B)]
        for shaped, terms in cols:
            if not np.isfinite(terms).all():  # eps = 0 and q = 0: the term, and the sum, are +inf
                assert shaped == math.inf
                continue
            exact = math.fsum(float(v) for v in terms)
            assert abs(shaped - exact) <= R.sum_bound(terms), (name, g)


def test_item_rule_on_the_class_fixture():
    with_base, without = R.fx_classes()
    assert R.score_ref(with_base)["counts"][0].tolist() == [1, 1, 1, 1, 5]
    assert R.score_ref(without)["counts"][0].tolist() == [3, 2, 1, 1, 3]
    e = R.score_ref(R.fx_edges(8))
    assert e["bin_n"][0].tolist() == [2, 2, 2, 2, 2, 2, 2, 4]  # v = 1.0 in the last bin
    assert e["counts"][0, 1] == 9  # hits: v < 0.5 with o = 0 (4), v >= 0.5 with o = 1 (5)
    assert e["terms"][0][1].max() == -math.log(1e-15)  # v = 0, o = 1 clipped (and v = 1, o = 0)


# --------------------------------------------------------------------------- argument errors
def _call(lib, **kw):
    a = dict(goff=1, G=1, seg=1, sgroup=1, n_seg=1, pidx=1, oidx=None, n_items=1, value=1, n_values=1, outcome=1, valid=None,
             base=None, M=1, B=10, eps=1e-15, scratch=8, sbytes=1 << 20, counts=1)
    a.update(kw)
    p = lambda x: None if x is None else 4096 + 8 * x  # noqa: E731  never dereferenced: the checks come first
    return lib.bce_score_groups(p(a["goff"]), a["G"], p(a["seg"]), p(a["sgroup"]), a["n_seg"], p(a["pidx"]), p(a["oidx"]), a["n_items"],
                                p(a["value"]), a["n_values"], p(a["outcome"]), p(a["valid"]), p(a["base"]), a["M"],
                                a["B"], a["eps"], p(a["scratch"]), a["sbytes"], p(a["counts"]), None, None, None,
                                None, None)


@pytest.mark.parametrize("kw, word", [
    (dict(G=-1), "negative"), (dict(n_items=-1), "negative"), (dict(B=0), "n_bins"), (dict(B=33), "n_bins"),
    (dict(eps=-1e-300), "eps"), (dict(eps=math.nan), "eps"), (dict(goff=None), "NULL"), (dict(seg=None), "NULL"), (dict(sgroup=None), "NULL"),
    (dict(counts=None), "NULL"), (dict(pidx=None), "NULL"), (dict(value=None), "NULL"), (dict(outcome=None), "NULL"),
    (dict(scratch=None), "scratch"), (dict(sbytes=8), "scratch"), (dict(n_seg=0), "segment"),
])
def test_argument_errors_need_no_gpu(kw, word):
    lib = N.load_library()
    assert _call(lib, **kw) == -1
    assert word.encode() in lib.bce_last_error()


def test_scratch_bytes_and_empty_call():
    lib = N.load_library()
    assert lib.bce_score_scratch_bytes(3, 10) == 3 * (8 + 30) * 8
    assert lib.bce_score_scratch_bytes(1, 32) == (8 + 96) * 8
    assert lib.bce_score_scratch_bytes(1, 33) == 0 and lib.bce_score_scratch_bytes(-1, 10) == 0
    assert _call(lib, G=0, goff=None, seg=None, counts=None, scratch=None) == 0  # nothing to do


# --------------------------------------------------------------------------- derived formulas
def _result(fx):
    ref = R.score_ref(fx)
    t = torch.from_numpy
    return ref, batch.ScoreResult(t(ref["counts"]), t(ref["sums"]), t(ref["bin_n"]), t(ref["bin_pos"]),
                                  t(ref["bin_psum"]), has_base=fx.get("base") is not None)


def test_derived_scores_and_nan_where_nothing_is_scored():
    fx = R.fx_random(10)
    fx["goff"] = np.array([0, 233, 233, 700], np.int64)  # an empty group in the middle
    ref, r = _result(fx)
    exp = R.derived(ref["counts"], ref["sums"], ref["bin_n"], ref["bin_pos"], ref["bin_psum"])
    for g, e in enumerate(exp):
        assert int(r.n_scored[g]) == e["n"]
        for k, got in (("brier", r.brier), ("log_loss", r.log_loss), ("accuracy", r.accuracy),
                       ("brier_base", r.brier_base)):
            assert (math.isnan(e[k]) and math.isnan(float(got[g]))) or float(got[g]) == e[k], (g, k)
        assert (math.isnan(e["ece"]) and math.isnan(float(r.ece[g]))) or abs(float(r.ece[g]) - e["ece"]) < 1e-15
        assert math.isnan(float(r.skill[g])) if e["n"] == 0 else float(r.skill[g]) == e["brier"] - e["brier_base"]
    assert exp[1]["n"] == 0
    mean, obs = r.calibration
    empty = ref["bin_n"] == 0
    assert np.array_equal(np.isnan(mean.numpy()), empty) and np.array_equal(np.isnan(obs.numpy()), empty)
    k = ~empty
    assert np.array_equal(mean.numpy()[k], ref["bin_psum"][k] / ref["bin_n"][k])
    assert np.array_equal(obs.numpy()[k], ref["bin_pos"][k] / ref["bin_n"][k])
    assert int(r.n_hit[0]) == ref["counts"][0, 1] and int(r.n_unresolved[2]) == ref["counts"][2, 2]
    assert int(r.n_null[2]) == ref["counts"][2, 3] and int(r.n_bad[2]) == ref["counts"][2, 4]
    _, nobase = _result(dict(fx, base=None))
    with pytest.raises(ValueError):
        nobase.skill


def test_merge_adds_left_to_right_and_stack_adds_a_dimension():
    _, a = _result(R.fx_random(10, seed=1))
    _, b = _result(R.fx_random(10, seed=2))
    _, c = _result(R.fx_random(10, seed=3))
    m = batch.ScoreResult.merge([a, b, c])
    assert torch.equal(m.counts, a.counts + b.counts + c.counts)
    assert torch.equal(m.sums, (a.sums + b.sums) + c.sums) and torch.equal(m.bin_psum, (a.bin_psum + b.bin_psum) + c.bin_psum)
    assert torch.equal(a.sums, _result(R.fx_random(10, seed=1))[1].sums)  # the parts are not written
    s = batch.ScoreResult.stack([a, b])
    assert s.counts.shape == (2, 2, 5) and s.brier.shape == (2, 2) and s.ece.shape == (2, 2)
    assert torch.equal(s.brier[1], b.brier)
    _, other = _result(R.fx_random(32))
    with pytest.raises(ValueError):
        batch.ScoreResult.merge([a, other])
    with pytest.raises(ValueError):
        batch.ScoreResult.merge([])


# ------------------------------------------------------------------- market layer arguments
def _aggregator():
    ms = MarketStore()
    m = ms.create_market(MarketId("a:1"))
    m.add_signal({"sourceId": "s", "probability": 0.7})
    m.resolve(True)
    return CrossMarketAggregator(ms)


def test_score_walk_argument_validation():
    agg = _aggregator()
    res = {"a:1": {"consensus": 0.7}}
    with pytest.raises(TypeError):
        agg.score_walk([res])
    for bad in (0, 33):
        with pytest.raises(ValueError):
            agg.score_walk(res, n_bins=bad)
    with pytest.raises(TypeError):
        agg.score_walk(res, domain_of=3)
    with pytest.raises(TypeError):
        agg.score_walk(res, pattern_lists=["a:*"])  # a list of LISTS
    with pytest.raises(KeyError):
        agg.score_walk({"b:9": {"consensus": 0.5}})
    empty = agg.score_walk({}, pattern_lists=[["a:*"]])  # nothing to score: no GPU needed
    assert empty.overall.n == 0 and empty.overall.brier is None and len(empty.groups) == 1 and empty.sources == {}


def test_sweep_decay_argument_validation(tmp_path):
    from bayesian_engine.reliability import SQLiteReliabilityStore
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    agg = _aggregator()
    plain = SQLiteReliabilityStore(str(tmp_path / "plain.db"))
    with pytest.raises(TypeError):
        agg.sweep_decay(plain, [30.0], [0.1])
    store = NamespacedReliabilityStore(str(tmp_path / "ns.db"))
    for hl, mr in (([], [0.1]), ([30.0], []), ([0.0], [0.1]), ([-1.0], [0.1]), ([math.nan], [0.1]), ([30.0], [1.5]),
                   ([30.0], [-0.1])):
        with pytest.raises(ValueError):
            agg.sweep_decay(store, hl, mr)
    with pytest.raises(TypeError):
        agg.sweep_decay(store, 30.0, [0.1])
    with pytest.raises(ValueError):
        agg.sweep_decay(store, [30.0], [0.1], n_bins=40)
    empty = CrossMarketAggregator(MarketStore()).sweep_decay(store, [30.0, 60.0], [0.1])  # no history: no GPU
    assert [e.params for e in empty] == [{"half_life_days": 30.0, "min_rel": 0.1},
                                         {"half_life_days": 60.0, "min_rel": 0.1}]
    assert all(e.n == 0 and e.brier is None for e in empty)
    store.close()
