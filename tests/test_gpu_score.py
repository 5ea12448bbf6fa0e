"""GPU checks of back-test scoring (bce_score_groups, batch.score / score_markets / score_sources /
walk_sweep, CrossMarketAggregator.score_walk / sweep_decay) against tests/score_ref.py: counts and
every fp64 sum except the log loss equal the shaped reference to the bit; a log-loss term is
within 4 ulp of ``-math.log`` and a log-loss sum within that plus the summation bound.

Largest log distance seen on an MI355X (printed by test_log_loss_terms_and_sums): 1 ulp."""
import fnmatch
import math

import numpy as np
import pytest
import torch

import score_ref as R
from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM

pytestmark = pytest.mark.gpu

DAY = 86_400_000_000
T0 = 1_790_000_000_000_000
ECE_TOL = 32 * 2.0 ** -52  # <= 32 bin terms of at most 1 each, added in some order in torch and in Python
LOG_ULP_CAP = 4  # a cap, not a measurement: two implementations within 1 ulp of the truth differ by <= 2; doubled


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _plan(fx, check=True):
    return batch.ScorePlan.groups(_T(fx["goff"]), _T(fx["pidx"]), _T(fx.get("oidx")), check=check)


def _score(fx, plan=None, faults=True):
    r = batch.score(plan or _plan(fx), _T(fx["value"]), _T(fx["outcome"]), valid=_T(fx.get("valid")),
                    base=_T(fx.get("base")), n_bins=fx["B"], eps=fx["eps"])
    if faults:
        N.check_faults(_dev(), "score")
    return {k: getattr(r, k).cpu().numpy() for k in ("counts", "sums", "bin_n", "bin_pos", "bin_psum")}, r


def _log_bound(terms):
    """4 ulp per term plus the summation bound, over the math.log terms of one group."""
    finite = [float(t) for t in terms if math.isfinite(t)]
    return sum(LOG_ULP_CAP * math.ulp(t) for t in finite) * (1 + len(finite) * 2.0 ** -52) + R.sum_bound(finite)


def _check(got, fx, what=""):
    """Everything against the shaped reference; returns it."""
    ref = R.score_ref(fx)
    for k in ("counts", "bin_n", "bin_pos"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    assert (got["counts"][:, [0, 2, 3, 4]].sum(1) == np.diff(fx["goff"]).clip(min=0)).all(), what
    assert np.array_equal(_bits(got["sums"][:, 0]), _bits(ref["sums"][:, 0])), (what, "brier")
    assert np.array_equal(_bits(got["sums"][:, 2]), _bits(ref["sums"][:, 2])), (what, "brier_base")
    assert np.array_equal(_bits(got["bin_psum"]), _bits(ref["bin_psum"])), (what, "bin_psum")
    for g in range(len(fx["goff"]) - 1):
        terms = ref["terms"][g][1]
        if not np.isfinite(terms).all():
            assert got["sums"][g, 1] == math.inf, (what, g)
            continue
        assert abs(got["sums"][g, 1] - ref["sums"][g, 1]) <= _log_bound(terms), (what, g, "logloss")
    return ref


@pytest.fixture(scope="module")
def lengths():
    fx = R.fx_lengths()
    got, _ = _score(fx)
    return fx, got, _check(got, fx, "lengths")


def test_group_lengths_around_the_lane_stride_and_the_segment(lengths):
    fx, got, ref = lengths
    assert np.diff(fx["goff"]).tolist() == list(R.LENGTHS)
    assert not got["counts"][0].any() and not got["sums"][0].any() and not got["bin_psum"][0].any()  # empty group
    assert got["counts"][:, 0].sum() > 0 and got["counts"][:, 2].sum() > 0 and got["counts"][:, 3].sum() > 0
    again, _ = _score(fx)
    for k in got:  # two runs: every bit
        assert np.array_equal(again[k].view(np.uint64), got[k].view(np.uint64)), k


def test_outputs_do_not_depend_on_the_other_groups_of_the_call(lengths):
    _, got, _ = lengths
    rev = R.fx_lengths(reverse=True)
    back, _ = _score(rev)
    _check(back, rev, "reversed")
    for k in got:  # group g of the call is group G - 1 - g of the reversed call: log loss included
        assert np.array_equal(back[k][::-1].view(np.uint64), got[k].view(np.uint64)), k


def test_overlapping_groups_and_a_duplicated_member():
    fx = R.fx_overlap()
    got, _ = _score(fx)
    _check(got, fx, "overlap")
    assert got["counts"][0].tolist() == [5, 4, 0, 0, 0]  # market 1 counted twice
    assert got["counts"][1, 2] == 1


def test_every_class_is_counted_once():
    with_base, without = R.fx_classes()
    got, _ = _score(with_base)
    _check(got, with_base, "classes with base")
    assert got["counts"][0].tolist() == [1, 1, 1, 1, 5]
    got, _ = _score(without)
    _check(got, without, "classes")
    assert got["counts"][0].tolist() == [3, 2, 1, 1, 3]
    assert got["sums"][0, 2] == 0.0  # no base: brier_base stays zero


def test_zero_half_and_one_with_both_outcomes():
    fx = R.fx_edges(8)
    got, r = _score(fx)
    ref = _check(got, fx, "edges")
    assert got["bin_n"][0].tolist() == [2, 2, 2, 2, 2, 2, 2, 4]  # exact edges k / 8; v = 1.0 in the last bin
    assert got["bin_pos"][0].tolist() == [1, 1, 1, 1, 1, 1, 1, 2]
    assert got["counts"][0, 1] == 9  # v = 0.5 votes True: a hit with o = 1, a miss with o = 0
    items = R.per_item(fx)
    each, _ = _score(items)
    v, o = fx["value"], fx["outcome"]
    for i in range(len(v)):
        assert each["counts"][i, 1] == int((v[i] >= 0.5) == (o[i] == 1)), i
        if (v[i] == 0.0 and o[i] == 1) or (v[i] == 1.0 and o[i] == 0):
            assert abs(each["sums"][i, 1] - -math.log(1e-15)) <= LOG_ULP_CAP * math.ulp(-math.log(1e-15))  # clipped
        if (v[i] == 1.0 and o[i] == 1) or (v[i] == 0.0 and o[i] == 0):
            assert each["sums"][i, 1] == 0.0
    unclipped = R.fx_edges(8, eps=0.0)
    got0, _ = _score(unclipped)
    _check(got0, unclipped, "eps = 0")
    assert got0["sums"][0, 1] == math.inf and np.array_equal(_bits(got0["sums"][:, 0]), _bits(got["sums"][:, 0]))
    assert float(r.brier[0]) == ref["sums"][0, 0] / 18


@pytest.mark.parametrize("B", [1, 10, 32])
def test_random_forecasts_per_bin_count(B):
    fx = R.fx_random(B)
    got, r = _score(fx)
    ref = _check(got, fx, f"B = {B}")
    assert got["bin_n"].shape == (2, B) and (got["bin_n"].sum(1) == got["counts"][:, 0]).all()
    exp = R.derived(ref["counts"], got["sums"], ref["bin_n"], ref["bin_pos"], ref["bin_psum"])
    for g, e in enumerate(exp):
        assert float(r.brier[g]) == e["brier"] and float(r.accuracy[g]) == e["accuracy"]
        assert float(r.log_loss[g]) == e["log_loss"] and float(r.skill[g]) == e["brier"] - e["brier_base"]
        assert abs(float(r.ece[g]) - e["ece"]) <= ECE_TOL


def test_log_loss_terms_and_sums():
    worst = 0.0
    for fx in (R.fx_random(10), R.fx_edges(8), R.fx_lengths()):
        items = R.per_item(fx)
        if len(items["pidx"]) > 3000:
            items = dict(items, goff=items["goff"][:3001])
        got, _ = _score(items)  # one group per item: the group's sum is the item's term
        ref = R.score_ref(items)
        for i in range(len(items["goff"]) - 1):
            if ref["counts"][i, 0] == 0:
                assert got["sums"][i, 1] == 0.0
                continue
            exp = float(ref["terms"][i][1][0])  # -math.log(max(q, eps))
            dist = abs(got["sums"][i, 1] - exp) / math.ulp(exp)
            worst = max(worst, dist)
            assert dist <= LOG_ULP_CAP, (i, got["sums"][i, 1], exp)
        whole, _ = _score(fx)
        _check(whole, fx, "log sums")
    print(f"largest distance of a log-loss term from -math.log: {worst} ulp")


# ------------------------------------------------------------------------------------ per source
@pytest.fixture(scope="module")
def source_batch():
    return R.fx_sources()


def test_per_source_counts_equal_agreement_stats(source_batch):
    offsets, sid, prob, outcome, _, _ = source_batch
    S = 40
    plan = batch.ScorePlan.by_source(_T(offsets), _T(sid), S)
    goff, pidx, oidx, _ = R.by_source_ref(offsets, sid, S)
    assert np.array_equal(plan.group_offsets.cpu().numpy(), goff)
    assert np.array_equal(plan.pidx.cpu().numpy(), pidx) and np.array_equal(plan.oidx.cpu().numpy(), oidx)
    r = batch.score_sources(plan, _T(prob), _T(outcome))
    correct, total = batch.agreement_stats(_T(offsets), _T(sid), _T(prob), _T(outcome), S)
    N.check_faults(_dev(), "per source")
    assert np.array_equal(r.n_scored.cpu().numpy(), total.cpu().numpy())
    assert np.array_equal(r.n_hit.cpu().numpy(), correct.cpu().numpy())
    assert int(r.n_scored[31]) == 0 and math.isnan(float(r.brier[31]))


def test_per_source_sums_and_skill_against_the_consensus(source_batch):
    offsets, sid, prob, outcome, consensus, valid = source_batch
    fx = R.fx_sources_items()
    plan = batch.ScorePlan.by_source(_T(offsets), _T(sid), 40)
    assert int(np.diff(fx["goff"]).max()) > R.SEG and plan.n_segments > 40
    r = batch.score_sources(plan, _T(prob), _T(outcome), consensus=_T(consensus), valid=_T(valid))
    N.check_faults(_dev(), "per source")
    got = {k: getattr(r, k).cpu().numpy() for k in ("counts", "sums", "bin_n", "bin_pos", "bin_psum")}
    ref = _check(got, fx, "sources")
    skill = r.skill.cpu().numpy()
    for g in range(40):
        n = int(ref["counts"][g, 0])
        if n:
            assert skill[g] == ref["sums"][g, 0] / n - ref["sums"][g, 2] / n, g
        else:
            assert math.isnan(skill[g])


# ----------------------------------------------------------------------------------- walk-forward
def _walk_batch(seed=3, M=36, S=12):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 9, M)
    lens[[4, 17]] = 0  # empty markets: consensus None
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    outcome = rng.choice(np.array([-1, 0, 1], np.int8), M, p=[0.25, 0.35, 0.4])
    outcome[[4, 17]] = 1  # resolved, so they count as null and not as unresolved
    mtime = T0 + np.arange(M, dtype=np.int64) * 11 * DAY
    rel = rng.uniform(0.2, 0.95, S)
    rel[:2] = 0.0  # sources 0 and 1 start at weight 0: a market of theirs alone has no consensus
    conf = rng.random(S)
    t_us = np.full(S, T0 - 40 * DAY, np.int64)
    present = (rng.random(S) < 0.8).astype(np.uint8)
    present[:2] = 1
    return off, sid, prob, outcome, mtime, (rel, conf, t_us, present), S


def _table(state):
    rel, conf, t_us, present = state
    return batch.ReliabilityTable(_T(rel.copy()), _T(conf.copy()), _T(t_us.copy()), _T(present.copy()),
                                  [""] * len(rel))


def test_score_markets_on_a_walk_forward_result():
    off, sid, prob, outcome, mtime, state, S = _walk_batch()
    plan = batch.WalkPlan.build(_T(off), _T(sid), _T(prob), _T(outcome), S)
    res = batch.walk_forward(plan, _table(state), _T(mtime), offsets=_T(off), prob=_T(prob), commit=False)
    r = batch.score_markets(res, _T(off), _T(outcome))
    null = res.is_null(_T(off))
    alone = batch.score(batch.ScorePlan.whole(len(outcome), device=_dev()), res.consensus, _T(outcome), valid=~null)
    N.check_faults(_dev(), "score_markets")
    for k in ("counts", "sums", "bin_n", "bin_pos", "bin_psum"):
        assert torch.equal(getattr(r, k), getattr(alone, k)), k
    M = len(outcome)
    fx = dict(goff=np.array([0, M], np.int64), pidx=np.arange(M, dtype=np.int64), oidx=None,
              value=res.consensus.cpu().numpy(), outcome=outcome, valid=(~null).cpu().numpy().astype(np.uint8),
              base=None, B=10, eps=1e-15)
    got = {k: getattr(r, k).cpu().numpy() for k in ("counts", "sums", "bin_n", "bin_pos", "bin_psum")}
    _check(got, fx, "walk")
    assert got["counts"][0, 3] >= 2 and got["counts"][0, 2] > 0 and got["counts"][0, 0] > 10
    halves = batch.ScorePlan.groups(_T(np.array([0, M // 2, M], np.int64)), _T(np.arange(M, dtype=np.int64)))
    two = batch.score_markets(res, _T(off), _T(outcome), plan=halves, n_bins=5)
    assert int(two.n_scored.sum()) == got["counts"][0, 0] and two.bin_n.shape == (2, 5)


def test_walk_sweep_equals_every_point_run_alone():
    off, sid, prob, outcome, mtime, state, S = _walk_batch(seed=8)
    plan = batch.WalkPlan.build(_T(off), _T(sid), _T(prob), _T(outcome), S)
    table = _table(state)
    before = [x.clone() for x in (table.rel, table.conf, table.t_us, table.present)]
    hl, mr = [DECAY_HALF_LIFE_DAYS, 5.0, 90.0], [DECAY_MINIMUM, 0.4]
    scores, (cons, nulls) = batch.walk_sweep(plan, table, _T(mtime), offsets=_T(off), prob=_T(prob),
                                             half_life_days=hl, min_rel=mr, keep_consensus=True)
    N.check_faults(_dev(), "walk_sweep")
    assert scores.counts.shape == (6, 1, 5) and scores.brier.shape == (6, 1) and cons.shape == (6, len(outcome))
    for x, b in zip((table.rel, table.conf, table.t_us, table.present), before):
        assert torch.equal(x, b)  # never committed
    whole = batch.ScorePlan.whole(len(outcome), device=_dev())
    k = 0
    for h in hl:
        for m in mr:
            wt, _ = batch.walk_trace(plan, _table(state), _T(mtime), half_life_days=h, min_rel=m)
            res = batch.consensus(_T(off), plan.pairs.esid, _T(prob), wt)
            assert torch.equal(res.consensus.view(torch.int64), cons[k].view(torch.int64)), (h, m)
            assert torch.equal(res.is_null(_T(off)), nulls[k]), (h, m)
            alone = batch.score(whole, res.consensus, _T(outcome), valid=~res.is_null(_T(off)))
            for f in ("counts", "sums", "bin_n", "bin_pos", "bin_psum"):
                a, b = getattr(alone, f), getattr(scores, f)[k]
                assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (h, m, f)
            k += 1
    assert not torch.equal(cons[0], cons[2])  # the decay parameters do reach the consensus
    ref = batch.walk_forward(plan, _table(state), _T(mtime), offsets=_T(off), prob=_T(prob), commit=False)
    assert torch.equal(ref.consensus.view(torch.int64), cons[0].view(torch.int64))  # the default point
    assert torch.equal(ref.is_null(_T(off)), nulls[0])
    only, none = batch.walk_sweep(plan, table, _T(mtime), offsets=_T(off), prob=_T(prob), half_life_days=[5.0],
                                  min_rel=[0.4])
    assert none is None and torch.equal(only.sums[0].view(torch.int64), scores.sums[3].view(torch.int64))
    N.check_faults(_dev(), "walk_sweep")


# ----------------------------------------------------------------------------------- market layer
def _history():
    from bayesian_engine.market import MarketId, MarketStore

    rng = np.random.default_rng(41)
    ms = MarketStore()
    for i in range(30):
        market = ms.create_market(MarketId(f"{'pol' if i % 3 else 'spo'}:{i}"))
        for _ in range(int(rng.integers(1, 7))):
            market.add_signal({"sourceId": f"src{int(rng.integers(0, 9))}", "probability": float(rng.random())})
        market.created_at = f"2024-01-{1 + i % 28:02d}T00:00:00+00:00"
        if i % 5:
            market.resolve(bool(rng.integers(0, 2)))
            market.resolved_at = f"2024-03-{1 + (7 * i) % 28:02d}T12:00:00+00:00"
    ms.create_market(MarketId("pol:empty"))  # no signals: not part of the walk
    return ms


def _same_score(got, e, what):
    assert got.n == e["n"], what
    if e["n"] == 0:
        assert got.brier is None and got.log_loss is None and got.accuracy is None and got.ece is None, what
        return
    assert got.brier == e["brier"] and got.accuracy == e["accuracy"], what
    assert abs(got.log_loss - e["log_loss"]) <= 1e-12 * e["log_loss"] and abs(got.ece - e["ece"]) <= ECE_TOL, what


@pytest.mark.parametrize("device_match", [False, True])
def test_score_walk_against_the_reference(tmp_path, device_match):
    from bayesian_engine.market import CrossMarketAggregator
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    ms = _history()
    agg = CrossMarketAggregator(ms)
    store = NamespacedReliabilityStore(str(tmp_path / "h.db"))
    results, _ = agg.walk_forward(store, domain="d", dry_run=True)
    lists = [["pol:*"], ["spo:1*", "*:2?", "nothing*"]]
    ws = agg.score_walk(results, pattern_lists=lists, domain_of="category", device_match=device_match)
    keys = list(results)
    at = {k: i for i, k in enumerate(keys)}
    value = np.array([r["consensus"] if r["consensus"] is not None else 0.0 for r in results.values()])
    valid = np.array([r["consensus"] is not None for r in results.values()], np.uint8)
    outcome = np.array([-1 if ms._markets[k].outcome is None else int(ms._markets[k].outcome) for k in keys], np.int8)
    groups = [list(range(len(keys)))]
    for d in ("spo", "pol") if keys[0].startswith("spo") else ("pol", "spo"):
        groups.append([i for i, k in enumerate(keys) if k.startswith(d + ":")])
    for patterns in lists:
        groups.append([at[k] for p in patterns for k in ms._markets if fnmatch.fnmatch(k, p) and k in at])
    goff = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    fx = dict(goff=goff, pidx=np.array([i for g in groups for i in g], np.int64), oidx=None, value=value,
              outcome=outcome, valid=valid, base=None, B=10, eps=1e-15)
    ref = R.score_ref(fx)
    exp = R.derived(ref["counts"], ref["sums"], ref["bin_n"], ref["bin_pos"], ref["bin_psum"])
    _same_score(ws.overall, exp[0], "overall")
    assert ws.overall.n_unresolved == ref["counts"][0, 2] > 0 and ws.overall.n > 10
    assert list(ws.domains) == [keys[0].split(":")[0], "pol" if keys[0].startswith("spo") else "spo"]
    for j, d in enumerate(ws.domains):
        _same_score(ws.domains[d], exp[1 + j], d)
    assert len(ws.groups) == 2 and len(groups[4]) > 0
    for j, got in enumerate(ws.groups):
        _same_score(got, exp[3 + j], f"list {j}")
    rows = ws.overall.calibration
    assert [r["bin"] for r in rows] == [b for b in range(10) if ref["bin_n"][0, b]]
    assert all(r["n"] == ref["bin_n"][0, r["bin"]] and r["observed"] == ref["bin_pos"][0, r["bin"]] / r["n"] and
               r["mean_forecast"] == ref["bin_psum"][0, r["bin"]] / r["n"] for r in rows)
    # sources: first-seen order over the walk, every signal counted, the consensus as the base
    names, sig = [], []
    for m, k in enumerate(keys):
        for s in ms._markets[k].signals:
            if s["sourceId"] not in names:
                names.append(s["sourceId"])
            sig.append((names.index(s["sourceId"]), m, s["probability"]))
    assert list(ws.sources) == names
    order = sorted(range(len(sig)), key=lambda i: sig[i][0])  # stable
    sgoff = np.concatenate([[0], np.cumsum(np.bincount([s[0] for s in sig], minlength=len(names)))]).astype(np.int64)
    sfx = dict(goff=sgoff, pidx=np.array(order, np.int64), oidx=np.array([sig[i][1] for i in order], np.int64),
               value=np.array([s[2] for s in sig]), outcome=outcome, valid=valid, base=value, B=10, eps=1e-15)
    sref = R.score_ref(sfx)
    sexp = R.derived(sref["counts"], sref["sums"], sref["bin_n"], sref["bin_pos"], sref["bin_psum"])
    for name, e in zip(names, sexp):
        got = ws.sources[name]
        assert got.n == e["n"] and got.source_id == name
        if e["n"]:
            assert got.brier == e["brier"] and got.accuracy == e["accuracy"] and got.skill == e["brier"] - e["brier_base"]
            assert abs(got.log_loss - e["log_loss"]) <= 1e-12 * e["log_loss"]
        else:
            assert math.isnan(got.brier) and math.isnan(got.skill)
    assert agg.score_walk(results, sources=False).sources == {}
    store.close()


def test_sweep_decay_default_point_is_the_dry_run_walk(tmp_path):
    from bayesian_engine.market import CrossMarketAggregator
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    agg = CrossMarketAggregator(_history())
    store = NamespacedReliabilityStore(str(tmp_path / "s.db"))
    results, _ = agg.walk_forward(store, domain="d", dry_run=True)
    base = agg.score_walk(results, sources=False).overall
    grid = agg.sweep_decay(store, [DECAY_HALF_LIFE_DAYS, 3.0], [DECAY_MINIMUM, 0.45], domain="d")
    assert [g.params for g in grid] == [{"half_life_days": h, "min_rel": m} for h in (DECAY_HALF_LIFE_DAYS, 3.0)
                                        for m in (DECAY_MINIMUM, 0.45)]
    first = grid[0]
    assert (first.n, first.brier, first.log_loss, first.accuracy, first.ece, first.calibration, first.n_unresolved,
            first.n_null) == (base.n, base.brier, base.log_loss, base.accuracy, base.ece, base.calibration,
                              base.n_unresolved, base.n_null)
    assert all(g.n == base.n for g in grid) and len({g.brier for g in grid}) > 1  # the parameters matter
    assert store._store.list_sources("__domain__:d") == []  # a dry run by construction
    store.close()


# ------------------------------------------------------------------------------------------ faults
def test_bad_offsets_and_indices_raise_the_fault_word_and_spare_the_other_groups():
    good = R.fx_overlap()
    want, _ = _score(good)
    # group 1 leaves the item list; group 0 is untouched
    fx = dict(good, goff=np.array([0, 5, 12], np.int64))
    got, _ = _score(fx, plan=_plan(fx, check=False), faults=False)
    with pytest.raises(N.BCEError):
        N.check_faults(_dev(), "score")
    assert np.array_equal(got["counts"][0], want["counts"][0]) and np.array_equal(_bits(got["sums"][0]), _bits(want["sums"][0]))
    assert not got["counts"][1].any() and not got["sums"][1].any()  # read as empty
    # offsets that decrease
    fx = dict(good, goff=np.array([0, 7, 5, 10], np.int64))
    got, _ = _score(fx, plan=_plan(fx, check=False), faults=False)
    with pytest.raises(N.BCEError):
        N.check_faults(_dev(), "score")
    assert not got["counts"][1].any() and got["counts"][2, [0, 2, 3, 4]].sum() == 5
    # a member outside the markets, a forecast index outside the values: counted as bad
    pidx = good["pidx"].copy()
    pidx[7] = 6
    pidx[8] = -1
    fx = dict(good, pidx=pidx)
    got, _ = _score(fx, faults=False)
    with pytest.raises(N.BCEError):
        N.check_faults(_dev(), "score")
    assert np.array_equal(got["counts"][0], want["counts"][0]) and np.array_equal(_bits(got["sums"][0]), _bits(want["sums"][0]))
    assert got["counts"][1, 4] == 2 and got["counts"][1, [0, 2, 3, 4]].sum() == 5
    oidx = np.array([0, 1, 9, 3, 4, 5, 0, 1, 2, 3], np.int64)
    fx = dict(good, oidx=oidx)
    got, _ = _score(fx, faults=False)
    with pytest.raises(N.BCEError):
        N.check_faults(_dev(), "score")
    assert got["counts"][0, 4] == 1 and got["counts"][0, [0, 2, 3, 4]].sum() == 5
    N.check_faults(_dev(), "cleared")  # the word was cleared: the next call is clean
    again, _ = _score(good)
    assert np.array_equal(again["counts"], want["counts"])
