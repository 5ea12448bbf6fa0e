"""GPU checks of the market-scope pair table (batch.pair_resolve / consensus_pairs / settle_pairs
and the store layers): every output equals the oracle composition of tests/pair_ref.py exactly
(``np.array_equal``), and the golden fixture made by the reference is reproduced through the
stores."""
import itertools
import json
import os
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest
import torch

import pair_ref
from bayesian_engine import _native as N
from bayesian_engine import batch
from pair_ref import fixture_batch

pytestmark = pytest.mark.gpu

NOW = 1_790_000_000_000_000
NOTS = pair_ref.NOTS
DAY = 86_400_000_000
EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _table(t):
    return batch.PairTable(_T(t["poffsets"]), _T(t["psid"]), _T(t["rel"]), _T(t["conf"]), _T(t["t_us"]),
                           _T(t["has"]), t["n_markets"], t["n_sources"])


def _np_table(tab):
    return dict(poffsets=tab.poffsets.cpu().numpy(), psid=tab.psid.cpu().numpy(), rel=tab.rel.cpu().numpy(),
                conf=tab.conf.cpu().numpy(), t_us=tab.t_us.cpu().numpy(), has=tab.has.cpu().numpy(),
                n_markets=tab.n_markets, n_sources=tab.n_sources)


def _rand_row(rng):
    """(rel, conf, t_us, has): some rows without a timestamp, some with a falsy updated_at."""
    k = rng.random()
    t = NOTS if k < 0.2 else NOW - int(rng.integers(0, 90 * DAY))
    has = 0 if k < 0.1 else 1  # has = 0 implies NO_TIMESTAMP; an unparseable stamp is has = 1 without one
    return float(rng.uniform(0.0, 1.0)), float(rng.random()), int(t), has


def _dense(rng, S, p_has):
    rel, conf = rng.uniform(0.0, 1.0, S), rng.random(S)
    has = (rng.random(S) < p_has).astype(np.uint8)
    t = np.where(rng.random(S) < 0.2, NOTS, NOW - rng.integers(0, 90 * DAY, S)).astype(np.int64)
    return rel, conf, t, has


def _scope(sc):
    return None if sc is None else batch.ScopeTable(*(_T(a) for a in sc))


def _bits(flags):
    """u32 words of a flag per entry, bit e % 32 of word e // 32."""
    Q = len(flags)
    pad = np.zeros(max((Q + 31) // 32, 1) * 32, np.uint8)
    pad[:Q] = flags
    return np.packbits(pad.reshape(-1, 32), axis=1, bitorder="little").view("<u4").ravel()


def _check_resolve(t, qoff, qsid, *, emarket, dom=None, glob=None, skip=None):
    """Every mode, apply_decay on and off, mark_cold, against pair_ref; ``skip``: entries left out."""
    tab = _table(t)
    Q = len(qsid)
    keep = np.ones(Q, bool) if skip is None else ~skip
    dq, ds = _T(qoff), _T(qsid)
    de = None if emarket is None else _T(emarket)
    lb, matched, _ = pair_ref.lookup(qoff, np.clip(qsid, 0, t["n_sources"] - 1), t)
    for mode, decay, cold in itertools.product(("store", "namespaced", "raw"), (True, False), (False, True)):
        if mode == "raw" and (cold or not decay):
            continue
        kw = dict(domain=_scope(dom), global_scope=_scope(glob)) if mode == "namespaced" else {}
        r = batch.pair_resolve(dq, ds, tab, NOW, mode=mode, emarket=de, apply_decay=decay, mark_cold=cold, **kw)
        what = (mode, decay, cold, emarket is None)
        assert np.array_equal(r.lb.cpu().numpy()[keep], lb[keep]), what
        assert np.array_equal(r.matched.cpu().numpy()[keep], matched[keep]), what
        if skip is not None:
            continue  # the reference arrays below are taken over the clean entries by the caller
        if mode == "raw":
            exp = pair_ref.resolve("raw", qoff, qsid, t, NOW)
            for g, e in zip((r.rel, r.conf, r.t_us, r.present), exp):
                assert np.array_equal(g.cpu().numpy(), e), what
            continue
        rel, conf, scope = pair_ref.resolve(mode, qoff, qsid, t, NOW, dom, glob, decay)
        rc = r.table.relconf.cpu().numpy()[:Q]
        assert np.array_equal(rc[:, 0], rel) and np.array_equal(rc[:, 1], conf), what
        assert np.array_equal(r.scope.cpu().numpy(), scope), what
        flags = (scope != 3) if cold else np.ones(Q, bool)
        assert np.array_equal(r.table.bits.cpu().numpy().view(np.uint32), _bits(flags)), what
    return tab


# ---------------------------------------------------------------------------------------- lookup
SEG_LENS = (0, 1, 2, 63, 64, 65, 256, 257, 1500)


@pytest.fixture(scope="module")
def segments():
    """One table with a segment of every length in SEG_LENS (rows at the odd sids), queried below
    the first row, above the last, at every row and in every gap; between them a market with 64
    rows and no query, and one with queries and no rows."""
    rng = np.random.default_rng(2026)
    S = 2 * max(SEG_LENS) + 2
    rows, qoff, qsid = [], [0], []
    lens = []
    for n in SEG_LENS:
        lens += [n, 64]  # the 64-row market after each has an empty query range
    for m, n in enumerate(lens):
        rows += [(m, 2 * i + 1, *_rand_row(rng)) for i in range(n)]
        if m % 2 == 0:
            qsid += list(range(0, 2 * n + 1))
        qoff.append(len(qsid))
    t = pair_ref.make_table(rows, len(lens), S)
    qoff, qsid = np.array(qoff, np.int64), np.array(qsid, np.int32)
    emarket = np.repeat(np.arange(len(lens)), np.diff(qoff)).astype(np.int32)
    return dict(t=t, qoff=qoff, qsid=qsid, emarket=emarket, S=S, dom=_dense(rng, S, 0.5), glob=_dense(rng, S, 0.7))


@pytest.mark.parametrize("with_emarket", [True, False])
def test_lookup_every_segment_length(segments, with_emarket):
    s = segments
    t = s["t"]
    assert (t["has"] == 0).any() and ((t["t_us"] == NOTS) & (t["has"] == 1)).any()
    em = s["emarket"] if with_emarket else None
    for dom, glob in ((s["dom"], s["glob"]), (None, s["glob"]), (s["dom"], None), (None, None)):
        _check_resolve(t, s["qoff"], s["qsid"], emarket=em, dom=dom, glob=glob)
    # a has = 0 row is used at store scope and skipped by the namespaced fallback
    uoff, usid = s["qoff"], s["qsid"]
    _, matched, row = pair_ref.lookup(uoff, usid, t)
    e = int(np.flatnonzero((row >= 0) & (t["has"][np.maximum(row, 0)] == 0))[0])
    st = pair_ref.resolve("store", uoff, usid, t, NOW)
    ns = pair_ref.resolve("namespaced", uoff, usid, t, NOW, s["dom"], s["glob"])
    assert st[2][e] == 0 and ns[2][e] != 0 and st[0][e] == t["rel"][row[e]]
    N.check_faults(_dev(), "lookup")


@pytest.mark.parametrize("Q", [0, 31, 32, 33, 63, 64, 65])
def test_lookup_ballot_bits_and_tiny_shapes(Q):
    rng = np.random.default_rng(Q)
    S = 80
    rows = [(0, s, *_rand_row(rng)) for s in range(S) if rng.random() < 0.5]
    qoff, qsid = np.array([0, Q], np.int64), np.arange(Q, dtype=np.int32)
    dom = _dense(rng, S, 0.3)
    for t in (pair_ref.make_table(rows, 1, S), pair_ref.make_table([], 1, S)):  # M = 1, and P = 0
        _check_resolve(t, qoff, qsid, emarket=np.zeros(Q, np.int32), dom=dom)
        _check_resolve(t, qoff, qsid, emarket=None, dom=dom)
    N.check_faults(_dev(), "tiny shapes")


def test_lookup_out_of_range_sid_raises_and_is_clamped(segments):
    s = segments
    qsid = s["qsid"].copy()
    last = int(s["qoff"][9]) - 1  # the last entry of a queried market: still ascending
    first = int(s["qoff"][16])    # the first entry of the longest one
    qsid[last] = s["S"] + 5
    qsid[first] = -3
    skip = np.zeros(len(qsid), bool)
    skip[[last, first]] = True
    N.check_faults(_dev(), "clean slate")
    tab = _check_resolve(s["t"], s["qoff"], qsid, emarket=s["emarket"], skip=skip)
    with pytest.raises(N.BCEError, match="sid"):
        N.check_faults(_dev(), "pair_resolve")
    N.check_faults(_dev(), "fault word is cleared")
    r = batch.pair_resolve(_T(s["qoff"]), _T(qsid), tab, NOW, emarket=_T(s["emarket"]))
    with pytest.raises(N.BCEError, match="sid"):
        N.check_faults(_dev(), "pair_resolve")
    rel, conf, scope = pair_ref.resolve("store", s["qoff"], s["qsid"], s["t"], NOW)
    rc = r.table.relconf.cpu().numpy()[:len(qsid)]
    assert np.array_equal(rc[~skip, 0], rel[~skip]) and np.array_equal(rc[~skip, 1], conf[~skip])
    assert np.array_equal(r.scope.cpu().numpy()[~skip], scope[~skip])


def test_lookup_decreasing_offsets_raise():
    t = pair_ref.make_table([(0, 1, 0.5, 0.5, NOTS, 1), (1, 2, 0.5, 0.5, NOTS, 1)], 3, 4)
    tab = _table(t)
    N.check_faults(_dev(), "clean slate")
    batch.pair_resolve(_T(np.array([0, 2, 1, 3], np.int64)), _T(np.array([0, 1, 2], np.int32)), tab, NOW)
    with pytest.raises(N.BCEError, match="offsets"):
        N.check_faults(_dev(), "qoffsets")
    tab.poffsets = _T(np.array([0, 2, 1, 2], np.int64))
    batch.pair_resolve(_T(np.array([0, 1, 2, 3], np.int64)), _T(np.array([0, 1, 2], np.int32)), tab, NOW)
    with pytest.raises(N.BCEError, match="offsets"):
        N.check_faults(_dev(), "poffsets")
    N.check_faults(_dev(), "cleared")


# ------------------------------------------------------------------------------ consensus_pairs
@pytest.fixture(scope="module")
def cbatch():
    rng = np.random.default_rng(77)
    lens = np.array([0, 1, 8, 9, 32, 33, 64, 65, 300])
    S = 50  # fewer sources than the long markets have signals: duplicates
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    sid = rng.integers(0, S, off[-1]).astype(np.int32)
    prob = rng.random(off[-1])
    rows = [(m, s, *_rand_row(rng)) for m in range(len(lens)) for s in range(S) if rng.random() < 0.5]
    return dict(off=off, sid=sid, prob=prob, S=S, t=pair_ref.make_table(rows, len(lens), S),
                dom=_dense(rng, S, 0.4), glob=_dense(rng, S, 0.5))


def _same_consensus(res, exp, off, what):
    for k in ("consensus", "confidence", "total_weight", "n_unique"):
        assert np.array_equal(getattr(res, k).cpu().numpy(), exp[k], equal_nan=True), (what, k)
    usid, weight, nweight = res.usid.cpu().numpy(), res.weight.cpu().numpy(), res.nweight.cpu().numpy()
    for m in range(len(off) - 1):
        a, u = int(off[m]), int(exp["n_unique"][m])
        assert np.array_equal(usid[a:a + u], exp["usid"][a:a + u]), (what, m)
        assert np.array_equal(weight[a:a + u], exp["weight"][a:a + u]), (what, m)
        assert np.array_equal(nweight[a:a + u], exp["nweight"][a:a + u]), (what, m)


@pytest.mark.parametrize("route", ["planned", "max_len", "bins"])
def test_consensus_pairs_matches_the_helper(cbatch, route):
    c = cbatch
    tab = _table(c["t"])
    off, sid, prob = _T(c["off"]), _T(c["sid"]), _T(c["prob"])
    kw = {"planned": {}, "max_len": {"max_len": 300}, "bins": {"bins": batch.Plan.build(c["off"], _dev())}}[route]
    plan = batch.PairPlan.build(off, sid, prob, c["S"])
    exp, uoff, usid, scope = pair_ref.consensus(c["off"], c["sid"], c["prob"], c["t"], NOW)
    assert np.array_equal(plan.uoffsets.cpu().numpy(), uoff) and np.array_equal(plan.usid.cpu().numpy(), usid)
    for p in (None, plan):
        pc = batch.consensus_pairs(off, sid, prob, tab, NOW, plan=p, mode="exact", check=True, **dict(kw))
        _same_consensus(pc.result, exp, c["off"], (route, p is None))
        assert np.array_equal(pc.scope.cpu().numpy(), scope)
        assert np.array_equal(pc.matched.cpu().numpy(), (scope == 0).astype(np.uint8))
    # the namespaced fallback with cold sources marked
    exp, _, _, scope = pair_ref.consensus(c["off"], c["sid"], c["prob"], c["t"], NOW, namespaced=True,
                                          domain=c["dom"], glob=c["glob"], mark_cold=True)
    assert (scope == 3).any() and (scope == 1).any() and (scope == 2).any()
    pc = batch.consensus_pairs(off, sid, prob, tab, NOW, plan=plan, namespaced=True, mark_cold=True,
                               domain=_scope(c["dom"]), global_scope=_scope(c["glob"]), check=True, **dict(kw))
    _same_consensus(pc.result, exp, c["off"], (route, "namespaced"))
    assert np.array_equal(pc.scope.cpu().numpy(), scope)


# --------------------------------------------------------------------------------- settle_pairs
CHAINS = (1, 2, 11, 12, 255, 256, 257, 600)


@pytest.fixture(scope="module")
def sbatch():
    """Markets 0..7: one pair each with a chain of CHAINS[m] signals (even markets have the row,
    odd ones do not); market 8: many sources with duplicates, rows for every third source and for
    sources that do not signal; market 9: unresolved, with rows; market 10: empty."""
    rng = np.random.default_rng(99)
    S = 40
    sig, rows, outcome = [], [], []
    for m, n in enumerate(CHAINS):
        s = 3 + 4 * m
        sig.append([(s, float(p)) for p in rng.random(n)])
        outcome.append(int(rng.integers(0, 2)))
        rows += [(m, s - 1, *_rand_row(rng)), (m, s + 1, *_rand_row(rng))]
        if m % 2 == 0:
            rows.append((m, s, *_rand_row(rng)))
    mixed = [(int(s), float(p)) for s, p in zip(rng.integers(0, S, 120), rng.random(120))]
    sig.append(mixed)
    outcome.append(1)
    rows += [(8, s, *_rand_row(rng)) for s in range(S) if s % 3 == 0]
    sig.append([(int(s), float(p)) for s, p in zip(rng.integers(0, S, 30), rng.random(30))])
    outcome.append(-1)
    rows += [(9, s, *_rand_row(rng)) for s in range(S) if s % 2 == 0]
    sig.append([])
    outcome.append(0)
    off = np.zeros(len(sig) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in sig])
    sid = np.array([s for x in sig for s, _ in x], np.int32)
    prob = np.array([p for x in sig for _, p in x], np.float64)
    return dict(off=off, sid=sid, prob=prob, outcome=np.array(outcome, np.int8), S=S,
                t=pair_ref.make_table(rows, len(sig), S))


def _same_table(got, exp, what):
    for k in ("poffsets", "psid", "rel", "conf", "t_us", "has"):
        assert got[k].dtype == exp[k].dtype, (what, k)
        assert np.array_equal(got[k], exp[k]), (what, k, np.flatnonzero(got[k] != exp[k])[:8])


def test_settle_pairs_matches_the_helper(sbatch):
    b = sbatch
    t = b["t"]
    off, sid, prob, outcome = _T(b["off"]), _T(b["sid"]), _T(b["prob"]), _T(b["outcome"])
    plan = batch.PairPlan.build(off, sid, prob, b["S"])
    exp, total, correct = pair_ref.settle(b["off"], b["sid"], b["prob"], b["outcome"], t, NOW)
    got = {}
    for name, kw in (("default", {}), ("one lane", {"long_min": batch.SETTLE_LONG_OFF})):
        new, splan = batch.settle_pairs(plan, _table(t), off, prob, outcome, NOW, **kw)
        got[name] = _np_table(new)
        _same_table(got[name], exp, name)
        assert np.array_equal(splan.total.cpu().numpy()[:plan.n_entries], total)
        assert np.array_equal(splan.correct.cpu().numpy()[:plan.n_entries], correct)
    for k in got["default"]:
        if isinstance(got["default"][k], np.ndarray):
            assert got["default"][k].tobytes() == got["one lane"][k].tobytes(), k
    new_t = got["default"]
    assert sorted(total[total > 0].tolist())[-4:] == [255, 256, 257, 600]
    # sorted and unique inside every market
    for m in range(new_t["n_markets"]):
        seg = new_t["psid"][new_t["poffsets"][m]:new_t["poffsets"][m + 1]]
        assert (np.diff(seg) > 0).all(), m
    assert len(new_t["psid"]) > len(t["psid"])  # pairs without a row were inserted
    # the unresolved market's rows, and every row no signal touched: bit for bit
    old = {(m, s): r for m, s, *r in pair_ref.table_rows(t)}
    now = {(m, s): r for m, s, *r in pair_ref.table_rows(new_t)}
    uoff, usid, emarket, _ = pair_ref.entries(b["off"], b["sid"], b["S"])
    touched = {(int(emarket[e]), int(usid[e])) for e in np.flatnonzero(total > 0)}
    assert any(m == 9 for m, _ in old) and not any(m == 9 for m, _ in touched)
    for key, r in old.items():
        if key not in touched:
            assert now[key] == r, key
    for key in touched:
        assert now[key][2] == NOW and now[key][3] == 1
    # a second batch on the returned table equals the reference's two batches
    outcome2 = np.where(b["outcome"] >= 0, 1 - b["outcome"], 1).astype(np.int8)  # market 9 now resolves
    exp2, _, _ = pair_ref.settle(b["off"], b["sid"], b["prob"], outcome2, exp, NOW + DAY)
    new2, _ = batch.settle_pairs(plan, new, off, prob, _T(outcome2), NOW + DAY)
    _same_table(_np_table(new2), exp2, "second batch")
    N.check_faults(_dev(), "settle_pairs")


def test_settle_pairs_empty_table_and_empty_batch():
    S = 5
    off = np.array([0, 3, 3], np.int64)
    sid, prob = np.array([4, 0, 4], np.int32), np.array([0.9, 0.2, 0.4])
    outcome = np.array([1, 0], np.int8)
    t = pair_ref.make_table([], 2, S)
    plan = batch.PairPlan.build(_T(off), _T(sid), _T(prob), S)
    new, _ = batch.settle_pairs(plan, batch.PairTable.empty(2, S, _dev()), _T(off), _T(prob), _T(outcome), NOW)
    _same_table(_np_table(new), pair_ref.settle(off, sid, prob, outcome, t, NOW)[0], "empty table")
    none = batch.PairPlan.build(_T(np.zeros(3, np.int64)), _T(sid[:0]), _T(prob[:0]), S)
    same, _ = batch.settle_pairs(none, new, _T(np.zeros(3, np.int64)), _T(prob[:0]), _T(outcome), NOW)
    _same_table(_np_table(same), _np_table(new), "empty batch")
    N.check_faults(_dev(), "settle_pairs edge")


# ------------------------------------------------------------------------- fixture through stores
def _seed(conn, g):
    for row in g["seeds"]:
        conn.execute("INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) "
                     "VALUES (?, ?, ?, ?, ?)", tuple(row))


def test_fixture_through_settle_resolved(golden_dir, tmp_path):
    from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore
    with open(os.path.join(golden_dir, "pair_scope_small.json")) as f:
        g = json.load(f)
    ns = NamespacedReliabilityStore(str(tmp_path / "resolved.db"))
    _seed(ns._store._conn, g)
    ms = MarketStore()
    for mid, mk in zip(g["market_ids"], g["markets"]):
        market = ms.create_market(MarketId(mid))
        for s, p in mk["signals"]:
            market.add_signal({"sourceId": g["names"][s], "probability": p})
        if mk["outcome"] is not None:
            market.resolve(mk["outcome"])
    summary = CrossMarketAggregator(ms).settle_resolved(ns, update_global=True, market_scope=True)
    rows = [[r.source_id, r.market_id, r.reliability, r.confidence] for r in ns._store.list_sources()]
    assert rows == g["final"]
    assert all(m in g["market_ids"] for _, m in summary.records)
    ns.close()
    N.check_faults(_dev(), "settle_resolved")


def test_fixture_through_the_stores(golden_dir, tmp_path):
    import bayesian_engine.decay as dmod
    from bayesian_engine.market import MarketId, MarketStore
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore
    with open(os.path.join(golden_dir, "pair_scope_small.json")) as f:
        g = json.load(f)
    names, mids = g["names"], g["market_ids"]
    ns = NamespacedReliabilityStore(str(tmp_path / "pairs.db"))
    _seed(ns._store._conn, g)
    ms = MarketStore()
    for mid, mk in zip(mids, g["markets"]):
        market = ms.create_market(MarketId(mid))
        for s, p in mk["signals"]:
            market.add_signal({"sourceId": names[s], "probability": p})
    now = EPOCH + timedelta(microseconds=g["now_us"])

    class _Frozen(datetime):
        @classmethod
        def now(cls, tz=None):
            return now

    old = dmod.datetime
    dmod.datetime = _Frozen
    try:
        default = ms.compute_all_consensus(ns._store)
        paired = ms.compute_all_consensus(ns._store, pair_table=True)
    finally:
        dmod.datetime = old
    assert list(paired) == list(default) == list(g["consensus"])
    for k in default:
        assert list(paired[k]) == list(default[k])
        assert paired[k] == default[k] == g["consensus"][k], k
    # settlement at market scope, global rows as well
    markets = [([{"sourceId": names[s], "probability": p} for s, p in mk["signals"]], mk["outcome"])
               for mk in g["markets"]]
    dump = lambda: [[r.source_id, r.market_id, r.reliability, r.confidence, r.updated_at]  # noqa: E731
                    for r in ns._store.list_sources()]
    before = dump()
    dry = ns.settle_markets(markets, update_global=True, dry_run=True, now=now, market_ids=mids)
    assert dump() == before  # dry_run writes nothing
    summary = ns.settle_markets(markets, domain="ignored", update_global=True, now=now, market_ids=mids)
    assert [row[:4] for row in dump()] == g["final"]
    assert {k: (r.reliability, r.confidence) for k, r in dry.records.items()} == \
        {k: (r.reliability, r.confidence) for k, r in summary.records.items()}
    final = {(s, m): (r, c) for s, m, r, c in g["final"]}
    for (s, m), rec in summary.records.items():
        assert (rec.reliability, rec.confidence) == final[(s, m)] and rec.namespace.value == "market"
    for s, rec in summary.global_records.items():
        assert (rec.reliability, rec.confidence) == final[(s, "__global__")]
    off, sid, _, outcome = fixture_batch(g)
    assert sum(summary.total.values()) == int(np.diff(off)[outcome >= 0].sum())
    with pytest.raises(ValueError):
        ns.settle_markets(markets, market_ids=mids[:-1])
    with pytest.raises(ValueError):
        ns.settle_markets(markets, market_ids=[mids[0]] * len(mids))
    with pytest.raises(ValueError):
        ns.settle_markets(markets, market_ids=[""] + mids[1:])
    ns.close()
    N.check_faults(_dev(), "stores")
