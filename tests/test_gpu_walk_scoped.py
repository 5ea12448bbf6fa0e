"""GPU checks of the namespaced walk-forward (batch.WalkScopePlan / batch.walk_forward_scoped and
the store layers): every entry's read state and scope code, every market's consensus, every slot's
weight, the new domain table and the global table equal the reference composition of
tests/walk_scope_ref.py exactly (``==``; NaN-aware) and the fixture recorded from the reference's
NamespacedReliabilityStore, with the chunked long-chain path forced, disabled and at its defaults."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.timeutil import iso_to_us
from oracle import oracle as orc
from walk_scope_ref import GLOBAL, fixture_batch, fixture_rows, scope_key, walk_scope_ref

pytestmark = pytest.mark.gpu

OFF = batch.SETTLE_LONG_OFF
KWS = [{}, {"long_min": OFF}, {"long_min": 1, "chunk_bits": 64}]
MASK = 0x7FFFFFFF
DAY = 86_400_000_000
T0 = 1_790_000_000_000_000
NOTS = int(orc.NO_TIMESTAMP)
NS = {0: "market", 1: "domain", 2: "global", 3: "global"}
R = lambda x: repr(float(x))  # noqa: E731


def _dev():
    return torch.device("cuda", 0)


def _T(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev())


def _pair_table(rows, kind, n, S):
    keys = sorted((sc[1], s) for (sc, s) in rows if sc != GLOBAL and sc[0] == kind)
    vals = [rows[((kind, k), s)] for k, s in keys]
    col = lambda i, dt: _T([v[i] for v in vals], dt)  # noqa: E731
    return batch.PairTable.from_rows(_T([k for k, _ in keys], np.int64), _T([s for _, s in keys], np.int32),
                                     col(0, np.float64), col(1, np.float64), col(2, np.int64), col(3, np.uint8), n, S)


def _global_table(rows, S):
    rel, conf = np.full(S, 0.5), np.full(S, 0.25)
    t_us, present, has = np.full(S, NOTS, np.int64), np.zeros(S, np.uint8), np.zeros(S, np.uint8)
    for (sc, s), (r, c, t, h) in rows.items():
        if sc == GLOBAL:
            rel[s], conf[s], t_us[s], present[s], has[s] = r, c, t, 1, h
    return batch.ReliabilityTable(_T(rel), _T(conf), _T(t_us), _T(present), [""] * S), _T(has)


def _plan(b, update_global, **kw):
    off, sid, prob, outcome, md, D, S = b
    return batch.WalkScopePlan.build(_T(off, np.int64), _T(sid, np.int32), _T(prob, np.float64), _T(outcome, np.int8),
                                     _T(md, np.int32), S, D, update_global=update_global, **kw)


def _bytes(x):
    return tuple(np.asarray(v, dt).tobytes() for v, dt in zip(x, (np.float64, np.float64, np.int64, np.uint8)))


def _final_rows(res, gtable, ghas):
    """The domain and global rows after the call, keyed as walk_scope_ref keys them."""
    d = res.domains
    po, ps = d.poffsets.cpu().numpy(), d.psid.cpu().numpy()
    cols = [x.cpu().numpy() for x in (d.rel, d.conf, d.t_us, d.has)]
    out = {}
    for k in range(d.n_markets):
        assert (np.diff(ps[po[k]:po[k + 1]]) > 0).all()
        for p in range(po[k], po[k + 1]):
            out[(("d", k), int(ps[p]))] = _bytes([c[p] for c in cols])
    g = [x.cpu().numpy() for x in (gtable.rel, gtable.conf, gtable.t_us, ghas, gtable.present)]
    for s in np.flatnonzero(g[4]):
        out[(GLOBAL, int(s))] = _bytes([c[s] for c in g[:4]])
    return out


def _run(b, rows, mtime, update_global, plan=None, market_scope=True, **kw):
    """(result fields as numpy, relconf by entry, final domain + global rows, plan)."""
    off, sid, prob, outcome, md, D, S = b
    M = len(off) - 1
    plan = plan or _plan(b, update_global)
    args = dict(offsets=_T(off, np.int64), prob=_T(prob, np.float64))
    tables = lambda: (_pair_table(rows, "d", D, S), *_global_table(rows, S),  # noqa: E731
                      _pair_table(rows, "m", M, S) if market_scope else None)
    dt, gt, gh, pt = tables()
    mt = _T(mtime, np.int64)
    res = batch.walk_forward_scoped(plan, dt, gt, mt, pairs=pt, global_has=gh, **args, **kw)
    torch.cuda.synchronize()
    out = {k: getattr(res, k).cpu().numpy() for k in ("consensus", "confidence", "total_weight", "n_unique", "usid",
                                                      "weight", "nweight", "scope")}
    final = _final_rows(res, gt, gh)
    # the read states themselves: the trace alone on fresh tables
    dt, gt, gh, pt = tables()
    tkw = {k: v for k, v in kw.items() if k in ("mark_cold", "long_min", "chunk_bits")}
    wt, scope = batch.walk_scope_trace(plan, dt, gt, mt, pairs=pt, global_has=gh, **tkw)
    torch.cuda.synchronize()
    assert np.array_equal(scope.cpu().numpy(), out["scope"])
    return out, wt.relconf[:plan.pairs.n_entries].cpu().numpy(), final, plan


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _compare(got, relconf, plan, exp, off, what=""):
    """Every market and every entry against walk_scope_ref's output."""
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
        assert np.array_equal(got["scope"][ent], exp["scope"][a:a + u]), (what, m, "scope")
        assert _eq(relconf[ent, 0], exp["rel_read"][a:a + u]), (what, m, "reliability read")
        assert _eq(relconf[ent, 1], exp["conf_read"][a:a + u]), (what, m, "confidence read")


def _same_rows(final, exp_rows, what=""):
    exp = {k: _bytes(v) for k, v in exp_rows.items() if k[0] == GLOBAL or k[0][0] == "d"}
    assert set(final) == set(exp), (what, sorted(set(final) ^ set(exp))[:8])
    bad = [k for k in exp if final[k] != exp[k]]
    assert not bad, (what, bad[:8])


# ----------------------------------------------------------------------------- golden fixture
def _fixture(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "walk_namespaced_small.json")))
    off, sid, prob, outcome, md, dnames, S = fixture_batch(g)
    return g, (off, sid, prob, outcome, md, len(dnames), S), fixture_rows(g, iso_to_us)


@pytest.mark.parametrize("update_global", [False, True])
def test_fixture_through_the_batch_call(golden_dir, update_global):
    g, b, rows = _fixture(golden_dir)
    off = b[0]
    run = g["runs"]["true" if update_global else "false"]
    exp, exp_rows = walk_scope_ref(*b[:5], b[6], rows, g["times_us"], update_global=update_global)
    for kw in KWS:
        got, relconf, final, plan = _run(b, rows, g["times_us"], update_global, **kw)
        _compare(got, relconf, plan, exp, off, f"fixture {kw}")
        _same_rows(final, exp_rows, f"fixture {kw}")
        uoff = plan.pairs.uoffsets.cpu().numpy()
        for m, r in enumerate(run["results"]):  # the reference's own numbers
            null = r["consensus"] is None
            assert null == bool(got["total_weight"][m] == 0)
            assert null or R(got["consensus"][m]) == r["consensus"], m
            assert R(got["confidence"][m]) == r["confidence"] and R(got["total_weight"][m]) == r["totalWeight"], m
            ent = slice(int(uoff[m]), int(uoff[m + 1]))
            assert [[R(x), R(y), NS[int(sc)]] for (x, y), sc in zip(relconf[ent], got["scope"][ent])] == \
                [x[1:4] for x in r["read"]], m
            assert [int(sc) == 3 for sc in got["scope"][ent]] == [x[4] == "cold-start" for x in r["read"]], m
        rec = {(n, k): (float(r), float(c), iso_to_us(ts), 1 if ts else 0) for n, k, r, c, ts in run["final"]}
        mine = {(g["names"][s], scope_key(g, sc)): v for (sc, s), v in final.items()}
        assert mine == {k: _bytes(v) for k, v in rec.items() if not k[1].startswith("walk:")}
    N.check_faults(_dev(), "fixture")


def _seed_store(store, g):
    for name, key, r, c, ts in g["seeds"]:
        store._store._conn.execute(
            "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
            (name, key, float(r), float(c), ts))


def _db_rows(store):
    return [[r.source_id, r.market_id, repr(r.reliability), repr(r.confidence), r.updated_at]
            for r in store._store.list_sources()]


def _fixture_markets(g):
    return [([{"sourceId": g["names"][s], "probability": float(p)} for s, p in mk["signals"]], mk["outcome"])
            for mk in g["markets"]]


def _check_dicts(results, g, run, first=None):
    for m, (res, exp) in enumerate(zip(results, run["results"][:first])):
        assert (None if res["consensus"] is None else repr(res["consensus"])) == exp["consensus"], m
        assert repr(res["confidence"]) == exp["confidence"], m
        assert repr(res["normalization"]["totalWeight"]) == exp["totalWeight"], m
        assert [[w["sourceId"], repr(w["weight"]), repr(w["normalizedWeight"])] for w in res["sourceWeights"]] == \
            exp["sourceWeights"], m
        assert res["diagnostics"]["coldStartSources"] == [] and res["diagnostics"]["status"] == "computed"
        assert res["diagnostics"]["sources"] == len(g["markets"][m]["signals"])
        assert res["diagnostics"]["uniqueSources"] == res["normalization"]["sourceCount"] == len(exp["read"])


@pytest.mark.parametrize("update_global", [False, True])
def test_fixture_through_the_namespaced_store(golden_dir, tmp_path, update_global):
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    g = json.load(open(os.path.join(golden_dir, "walk_namespaced_small.json")))
    run = g["runs"]["true" if update_global else "false"]
    store = NamespacedReliabilityStore(str(tmp_path / "walk.db"))
    _seed_store(store, g)
    before = _db_rows(store)
    args = dict(domains=g["domains"], market_ids=g["market_ids"], update_global=update_global)
    dry, dsum = store.walk_forward_namespaced(_fixture_markets(g), g["times"], dry_run=True, **args)
    assert _db_rows(store) == before  # dry run: the database is untouched
    wet, wsum = store.walk_forward_namespaced(_fixture_markets(g), g["times"], **args)
    assert dry == wet and dsum == wsum
    _check_dicts(wet, g, run)
    assert _db_rows(store) == run["final"]  # updated_at included: each row's last writing market
    final = {(n, k): [r, c, ts] for n, k, r, c, ts in run["final"]}
    for (name, dom), rec in wsum.records.items():
        key = f"__domain__:{dom}" if dom else "__global__"
        assert [repr(rec.reliability), repr(rec.confidence), rec.updated_at] == final[(name, key)], (name, dom)
        assert rec.namespace.value == ("domain" if dom else "global")
    for name, rec in wsum.global_records.items():
        assert [repr(rec.reliability), repr(rec.confidence), rec.updated_at] == final[(name, "__global__")], name
    touched_global = {n for (n, d) in wsum.total if update_global or d is None}
    assert set(wsum.global_records) == touched_global and set(wsum.total) == set(wsum.records)
    assert all(wsum.correct[k] <= wsum.total[k] for k in wsum.total)
    with pytest.raises(ValueError, match="domains"):
        store.walk_forward_namespaced(_fixture_markets(g), g["times"], domains=["crypto"])
    with pytest.raises(ValueError, match="market id"):
        store.walk_forward_namespaced(_fixture_markets(g), g["times"], market_ids=["x"] * 12)
    store.close()
    N.check_faults(_dev(), "namespaced store")


def test_aggregator_routes_domain_of_to_the_namespaced_walk(golden_dir, tmp_path):
    from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    g = json.load(open(os.path.join(golden_dir, "walk_namespaced_small.json")))
    dom = dict(zip(g["market_ids"], g["domains"]))
    domain_of = lambda m: dom[str(m.id)]  # noqa: E731

    def fill(n_markets):
        ms = MarketStore()
        for i, ((signals, outcome), t) in enumerate(list(zip(_fixture_markets(g), g["times"]))[:n_markets]):
            market = ms.create_market(MarketId(g["market_ids"][i]))
            for s in signals:
                market.add_signal(s)
            market.created_at = "2020-01-01T00:00:00+00:00" if outcome is not None else t
            if outcome is not None:
                market.resolve(outcome)
                market.resolved_at = t
        return ms

    # the first five markets are in time order (3 and 4 tie: store position decides): the fixture itself
    for update_global in (False, True):
        store = NamespacedReliabilityStore(str(tmp_path / f"agg5{update_global}.db"))
        _seed_store(store, g)
        out, _ = CrossMarketAggregator(fill(5)).walk_forward(store, domain_of=domain_of, market_scope=True,
                                                             update_global=update_global, dry_run=True)
        assert list(out) == g["market_ids"][:5] and all(out[k]["marketId"] == k for k in out)
        _check_dicts(list(out.values()), g, g["runs"]["true" if update_global else "false"], first=5)
        store.close()
    # all twelve: market 6 is earlier than market 5, so it is walked first
    order = sorted(range(12), key=lambda i: (g["times_us"][i], i))
    assert order.index(6) < order.index(5)
    agg = NamespacedReliabilityStore(str(tmp_path / "agg.db"))
    ref = NamespacedReliabilityStore(str(tmp_path / "ref.db"))
    for st in (agg, ref):
        _seed_store(st, g)
    out, summary = CrossMarketAggregator(fill(12)).walk_forward(agg, patterns=["walk:*"], domain_of=domain_of,
                                                                market_scope=True, update_global=True)
    mk = _fixture_markets(g)
    exp, esummary = ref.walk_forward_namespaced([mk[i] for i in order], [g["times"][i] for i in order],
                                                domains=[g["domains"][i] for i in order],
                                                market_ids=[g["market_ids"][i] for i in order], update_global=True)
    assert list(out) == [g["market_ids"][i] for i in order]
    for k, e in zip(out, exp):
        assert {x: v for x, v in out[k].items() if x != "marketId"} == e
    assert summary == esummary and _db_rows(agg) == _db_rows(ref)
    with pytest.raises(ValueError, match="exclude"):
        CrossMarketAggregator(fill(2)).walk_forward(agg, domain="crypto", domain_of=domain_of)
    for st in (agg, ref):
        st.close()
    N.check_faults(_dev(), "aggregator")


# ----------------------------------------------------------------------------- random batch
M_RND, S_RND, D_RND = 300, 24, 3


def _planted_bits(n):
    """Alternating bits with runs of 12 equal bits across the 64- and the 128-bit boundary."""
    bits = (np.arange(n) & 1).astype(np.uint8)
    for a in (58, 122):
        bits[a:a + 12] = bits[a]
    return bits


@pytest.fixture(scope="module")
def rnd():
    """300 markets, 24 sources, 3 domains and ~20% of markets without one, 15% unresolved.  Source
    0 signals twice in every market; (domain 1, source 1) is a constructed chain: two signals per
    market of domain 1, whose bits are those of _planted_bits."""
    rng = np.random.default_rng(20261020)
    M, S, D = M_RND, S_RND, D_RND
    md = rng.choice([-1, 0, 1, 2], M, p=[0.2, 0.35, 0.3, 0.15]).astype(np.int32)
    outcome = rng.integers(0, 2, M).astype(np.int8)
    outcome[rng.random(M) < 0.15] = -1
    n_planted = 2 * int(((md == 1) & (outcome >= 0)).sum())
    planted = _planted_bits(n_planted)
    assert n_planted > 140
    markets, k = [], 0
    for m in range(M):
        sig = [(0, float(np.round(rng.random(), 3))) for _ in range(2)]
        pool = np.arange(2 if md[m] == 1 else 1, S)
        for _ in range(int(rng.integers(0, 9))):
            sig.append((int(rng.choice(pool)), float(np.round(rng.random(), 3))))
        if md[m] == 1:
            for _ in range(2):
                if outcome[m] >= 0:
                    sig.append((1, 0.75 if planted[k] == outcome[m] else 0.25))  # (p >= 0.5) == outcome <=> bit
                    k += 1
                else:
                    sig.append((1, 0.6))
        order = rng.permutation(len(sig))
        ones = [i for i in order if sig[i][0] == 1]  # the planted signals keep their order
        it = iter(sorted(ones))
        markets.append([sig[next(it)] if sig[i][0] == 1 else sig[i] for i in order])
    assert k == n_planted and all(2 <= len(x) <= 12 for x in markets)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in markets])
    sid = np.array([s for x in markets for s, _ in x], np.int32)
    prob = np.array([p for x in markets for _, p in x], np.float64)
    gaps = rng.choice([0.0, 0.0, 0.25, 1.0, 3.0, 20.0, -0.5], M)
    mtime = (T0 + np.cumsum(gaps) * DAY).astype(np.int64) + 77
    rows = {}

    def seed(scope, s):
        has = rng.random() < 0.7
        t = int(T0 - rng.integers(0, 90) * DAY) if has and rng.random() < 0.9 else NOTS  # truthy, unparseable
        rows[(scope, s)] = (float(rng.choice([0.0, 1.0, rng.random()])), float(rng.random()), t if has else NOTS,
                            int(has))
    for d in range(D):
        for s in range(S):
            if rng.random() < 0.5:
                seed(("d", d), s)
    for s in range(S):
        if rng.random() < 0.6:
            seed(GLOBAL, s)
    for m in range(M):
        for s in set(sid[off[m]:off[m + 1]].tolist()):
            if rng.random() < 0.15:
                seed(("m", m), s)
    b = (off, sid, prob, outcome, md, D, S)
    exp = {ug: walk_scope_ref(off, sid, prob, outcome, md, S, rows, mtime, update_global=ug) for ug in (False, True)}
    return dict(b=b, rows=rows, mtime=mtime, exp=exp)


@pytest.mark.parametrize("update_global", [False, True])
def test_random_batch(rnd, update_global):
    b, rows, mtime = rnd["b"], rnd["rows"], rnd["mtime"]
    exp, exp_rows = rnd["exp"][update_global]
    assert {0, 1, 2, 3} <= set(exp["scope"][exp["scope"] != 255].tolist())
    plan = _plan(b, update_global)
    dtotal = plan.dsettle.total.cpu().numpy()
    f1 = int(np.flatnonzero((plan.dplan.emarket.cpu().numpy() == 1) & (plan.dplan.usid.cpu().numpy() == 1))[0])
    assert dtotal[f1] > 140 and dtotal[plan.dplan.usid.cpu().numpy() == 0].max() > 128
    assert plan.gsettle.total.cpu().numpy()[0] > (128 if update_global else 64)
    runs = []
    for kw in KWS:
        got, relconf, final, _ = _run(b, rows, mtime, update_global, plan=plan, **kw)
        _compare(got, relconf, plan, exp, b[0], f"random {kw}")
        _same_rows(final, exp_rows, f"random {kw}")
        runs.append((got, relconf, final))
    slots = np.concatenate([np.arange(a, a + u) for a, u in zip(b[0][:-1], exp["n_unique"])])
    for got, relconf, final in runs[1:]:  # and equal each other, byte for byte
        for k in got:  # the slots past a market's unique sources are not written
            pick = slots if k in ("usid", "weight", "nweight") else slice(None)
            assert got[k][pick].tobytes() == runs[0][0][k][pick].tobytes(), k
        assert relconf.tobytes() == runs[0][1].tobytes() and final == runs[0][2]
    N.check_faults(_dev(), "random batch")


def test_mark_cold_sets_the_cold_bit_where_the_read_ended_cold(rnd):
    b, rows, mtime = rnd["b"], rnd["rows"], rnd["mtime"]
    exp, exp_rows = walk_scope_ref(*b[:5], b[6], rows, mtime, update_global=True, mark_cold=True)
    got, relconf, final, plan = _run(b, rows, mtime, True, mark_cold=True)
    _compare(got, relconf, plan, exp, b[0], "mark_cold")
    _same_rows(final, exp_rows, "mark_cold")
    slots = np.concatenate([np.arange(a, a + u) for a, u in zip(b[0][:-1], exp["n_unique"])])
    ent = got["usid"][slots] & MASK
    assert np.array_equal(got["usid"][slots] < 0, got["scope"][ent] == batch.NS_COLD) and (got["usid"][slots] < 0).any()
    N.check_faults(_dev(), "mark_cold")


def test_commit_false_leaves_every_input_untouched(rnd):
    (off, sid, prob, outcome, md, D, S), rows, mtime = rnd["b"], rnd["rows"], rnd["mtime"]
    plan = _plan(rnd["b"], True)
    dt, (gt, gh), pt = _pair_table(rows, "d", D, S), _global_table(rows, S), _pair_table(rows, "m", len(off) - 1, S)
    mt, o, p = _T(mtime), _T(off), _T(prob)
    inputs = [mt, o, p, gt.rel, gt.conf, gt.t_us, gt.present, gh] + \
        [getattr(t, f) for t in (dt, pt) for f in ("poffsets", "psid", "rel", "conf", "t_us", "has")]
    before = [x.cpu().numpy().tobytes() for x in inputs]
    dry = batch.walk_forward_scoped(plan, dt, gt, mt, offsets=o, prob=p, pairs=pt, global_has=gh, commit=False)
    torch.cuda.synchronize()
    assert dry.domains is dt and [x.cpu().numpy().tobytes() for x in inputs] == before
    wet = batch.walk_forward_scoped(plan, dt, gt, mt, offsets=o, prob=p, pairs=pt, global_has=gh)
    torch.cuda.synchronize()
    for k in ("consensus", "confidence", "total_weight", "n_unique"):
        assert getattr(dry, k).cpu().numpy().tobytes() == getattr(wet, k).cpu().numpy().tobytes(), k
    assert dry.scope.cpu().numpy().tobytes() == wet.scope.cpu().numpy().tobytes()
    # the committed call wrote the global table and a NEW domain table; the old one and the market rows stay
    after = [x.cpu().numpy().tobytes() for x in inputs]
    assert wet.domains is not dt and after[:3] == before[:3] and after[8:] == before[8:] and after[3:8] != before[3:8]
    assert wet.domain_total is plan.dsettle.total and wet.global_correct is plan.gsettle.correct
    N.check_faults(_dev(), "commit")


# ----------------------------------------------------------------------------- cross-checks
def test_without_domains_it_is_walk_forward(rnd):
    off, sid, prob, outcome, _, _, S = rnd["b"]
    M = len(off) - 1
    rows = {k: (r, c, t, 1) for k, (r, c, t, h) in rnd["rows"].items() if k[0] == GLOBAL}  # has == present
    b = (off, sid, prob, outcome, np.full(M, -1, np.int32), 0, S)
    got, relconf, final, plan = _run(b, rows, rnd["mtime"], False, market_scope=False)
    wplan = batch.WalkPlan.build(_T(off), _T(sid), _T(prob), _T(outcome), S)
    table, _ = _global_table(rows, S)
    res = batch.walk_forward(wplan, table, _T(rnd["mtime"]), offsets=_T(off), prob=_T(prob))
    wt, exists = batch.walk_trace(wplan, _global_table(rows, S)[0], _T(rnd["mtime"]))
    torch.cuda.synchronize()
    slots = np.concatenate([np.arange(a, a + u) for a, u in zip(off[:-1], got["n_unique"])])
    for k in ("consensus", "confidence", "total_weight", "n_unique", "usid", "weight", "nweight"):
        pick = slots if k in ("usid", "weight", "nweight") else slice(None)
        assert got[k][pick].tobytes() == getattr(res, k).cpu().numpy()[pick].tobytes(), k
    E = plan.pairs.n_entries
    assert relconf.tobytes() == wt.relconf[:E].cpu().numpy().tobytes()
    assert np.array_equal(got["scope"] == batch.NS_GLOBAL, exists.cpu().numpy() != 0)
    assert set(got["scope"].tolist()) == {batch.NS_GLOBAL, batch.NS_COLD}
    present = table.present.cpu().numpy()
    mine = {s: v for (sc, s), v in final.items()}
    assert sorted(mine) == np.flatnonzero(present).tolist()
    cols = [x.cpu().numpy() for x in (table.rel, table.conf, table.t_us, table.present)]
    assert all(mine[s] == _bytes([c[s] for c in cols]) for s in mine)
    N.check_faults(_dev(), "no domains")


def test_no_resolved_market_is_consensus_pairs_per_market_time(rnd):
    off, sid, prob, _, md, D, S = rnd["b"]
    M = 40
    off, md = off[:M + 1], md[:M]
    sid, prob = sid[:off[-1]], prob[:off[-1]]
    rows = {k: v for k, v in rnd["rows"].items() if k[0] == GLOBAL or k[0][0] == "d" or k[0][1] < M}
    mtime = T0 + np.array([0, 3, 3, 40, 1], np.int64)[np.arange(M) % 5] * DAY
    b = (off, sid, prob, np.full(M, -1, np.int8), md, D, S)
    got, relconf, final, plan = _run(b, rows, mtime, True)
    assert plan.dsettle.n_touched == 0 and plan.gsettle.n_touched == 0
    _same_rows(final, rows, "nothing is settled")
    dt, (gt, gh), pt = _pair_table(rows, "d", D, S), _global_table(rows, S), _pair_table(rows, "m", M, S)
    uoff = plan.pairs.uoffsets.cpu().numpy()
    for now in np.unique(mtime):
        r = batch.consensus_pairs(_T(off), _T(sid), _T(prob), pt, int(now), plan=plan.pairs, namespaced=True,
                                  global_scope=batch.ScopeTable(gt.rel, gt.conf, gt.t_us, gh), domains=dt,
                                  market_domain=_T(md))
        torch.cuda.synchronize()
        scope = r.scope.cpu().numpy()
        for m in np.flatnonzero(mtime == now):
            a, u = int(off[m]), int(got["n_unique"][m])
            for k in ("consensus", "confidence", "total_weight", "n_unique"):
                assert _eq(getattr(r.result, k).cpu().numpy()[m], got[k][m]), (m, k)
            for k in ("usid", "weight", "nweight"):
                assert _eq(getattr(r.result, k).cpu().numpy()[a:a + u], got[k][a:a + u]), (m, k)
            assert np.array_equal(scope[uoff[m]:uoff[m + 1]], got["scope"][uoff[m]:uoff[m + 1]]), m
    N.check_faults(_dev(), "no resolved market")


# ----------------------------------------------------------------------------- bad inputs
@pytest.mark.parametrize("field", ["dentry", "dqlast", "gqlast"])
def test_out_of_range_index_raises_and_the_other_entries_are_answered(golden_dir, field):
    g, b, rows = _fixture(golden_dir)
    off, _, _, _, _, D, S = b
    plan = _plan(b, True)
    E, F, M = plan.pairs.n_entries, plan.dplan.n_entries, len(off) - 1
    tables = lambda: (_pair_table(rows, "d", D, S), *_global_table(rows, S), _pair_table(rows, "m", M, S))  # noqa: E731

    def trace(p):
        dt, gt, gh, pt = tables()
        wt, scope = batch.walk_scope_trace(p, dt, gt, _T(g["times_us"], np.int64), pairs=pt, global_has=gh)
        torch.cuda.synchronize()
        return wt.relconf[:E].cpu().numpy(), scope.cpu().numpy()

    N.check_faults(_dev(), "clean slate")
    good = trace(plan)
    N.check_faults(_dev(), "a valid plan raises nothing")
    dentry = plan.dentry.cpu().numpy()
    e = int(np.flatnonzero(dentry >= 0)[3])
    for value in ({"dentry": F + 5, "dqlast": M + 3, "gqlast": M}[field], -7):
        if field == "dentry":
            x = plan.dentry.clone()
            x[e] = value
            bad = dataclasses.replace(plan, dentry=x)
        else:
            q = plan.dq if field == "dqlast" else plan.gq
            x = q.qlast.clone()
            x[e] = value
            bad = dataclasses.replace(plan, **{field[0] + "q": dataclasses.replace(q, qlast=x)})
        relconf, scope = trace(bad)
        with pytest.raises(N.BCEError):
            N.check_faults(_dev(), "walk_scope_read")
        keep = np.arange(E) != e
        assert relconf[keep].tobytes() == good[0][keep].tobytes() and np.array_equal(scope[keep], good[1][keep])
        assert scope[e] in (0, 1, 2, 3) and np.isfinite(relconf[e]).all()  # answered from what can be read safely
    N.check_faults(_dev(), "the fault word is cleared")
