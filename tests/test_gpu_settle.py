"""GPU checks of batch settlement (batch.SettlePlan / batch.settle and the store layers): every
reliability, confidence, timestamp and present flag equals the oracle composition of
tests/settle_ref.py exactly (``==``; NaN-aware), with the chunked long-chain path forced, disabled
and at its defaults."""
import json
import os
import sqlite3

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from oracle import oracle as orc
from settle_ref import apply_chains, chains, fixture_scope, settle_ref

pytestmark = pytest.mark.gpu

OFF = batch.SETTLE_LONG_OFF
NOW = 1_790_000_000_000_000


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _build(off, sid, prob, outcome, S, **kw):
    return batch.SettlePlan.build(_T(np.asarray(off, np.int64)), _T(np.asarray(sid, np.int32)),
                                  _T(np.asarray(prob, np.float64)), _T(np.asarray(outcome, np.int8)), S, **kw)


def _apply(plan, rel, conf, t_us, present, now=NOW, **kw):
    d = [_T(np.array(rel, np.float64)), _T(np.array(conf, np.float64)), _T(np.array(t_us, np.int64)),
         _T(np.array(present, np.uint8))]
    batch.settle(plan, *d, now, **kw)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in d)


def _same(got, exp, what=""):
    for name, g, e in zip(("rel", "conf", "t_us", "present"), got, exp):
        assert g.dtype == e.dtype, (what, name)
        assert np.array_equal(g, e, equal_nan=g.dtype == np.float64), (what, name, np.flatnonzero(g != e)[:8])


# ----------------------------------------------------------------------------- golden fixture
def test_fixture_both_scopes(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "settle_small.json")))
    prob = np.array([float(x) for x in g["prob"]])
    S = g["n_sources"]
    plan = _build(g["offsets"], g["sid"], prob, g["outcome"], S)
    assert plan.total.cpu().tolist() == g["total"] and plan.correct.cpu().tolist() == g["correct"]
    correct, total = batch.agreement_stats(_T(np.array(g["offsets"], np.int64)), _T(np.array(g["sid"], np.int32)),
                                           _T(prob), _T(np.array(g["outcome"], np.int8)), S)
    assert correct.cpu().tolist() == g["correct"] and total.cpu().tolist() == g["total"]
    for scope in ("domain", "global"):
        (rel, conf, present), (erel, econf, epresent) = fixture_scope(g, scope)
        t0 = np.where(present, 5, orc.NO_TIMESTAMP).astype(np.int64)
        for kw in ({}, {"long_min": OFF}, {"long_min": 11, "chunk_bits": 64}):
            r, c, t, p = _apply(plan, rel, conf, t0, present, **kw)
            assert [repr(float(x)) for x in r] == [repr(float(x)) for x in erel], (scope, kw)
            assert [repr(float(x)) for x in c] == [repr(float(x)) for x in econf], (scope, kw)
            assert p.tolist() == epresent.tolist(), (scope, kw)
            assert np.array_equal(t == NOW, np.array(g["total"]) > 0)
    N.check_faults(_dev(), "fixture")


# ----------------------------------------------------------------------------- edge batch
EDGE_LENS = (0, 1, 2, 10, 11, 12, 63, 64, 65, 127, 128, 129)  # chain length of sources 0..11


@pytest.fixture(scope="module")
def edge():
    rng = np.random.default_rng(23)
    S, M = 300, 70
    outcome = rng.integers(0, 2, M).astype(np.int8)
    outcome[[3, 20, 21, 40, 69]] = -1  # unresolved markets in between
    resolved = np.flatnonzero(outcome >= 0)
    trip = []  # (market, sid, prob)
    for s, ln in enumerate(EDGE_LENS):  # exact chain lengths, spread over the markets with duplicates
        trip += [(int(m), s, float(rng.random())) for m in rng.choice(resolved, ln)]
    trip += [(3, 0, 0.9), (20, 0, 0.1), (40, 5, 0.7)]  # source 0 signals in unresolved markets only
    for m in range(M):
        trip += [(m, int(s), float(rng.random())) for s in rng.integers(12, 290, int(rng.integers(8, 40)))]
    perm = rng.permutation(len(trip))
    trip = sorted((trip[i] for i in perm), key=lambda x: x[0])  # stable: a random position order per market
    mk = np.array([x[0] for x in trip])
    sid = np.array([x[1] for x in trip], np.int32)
    prob = np.array([x[2] for x in trip], np.float64)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(mk, minlength=M))
    live = np.flatnonzero((outcome[mk] >= 0) & (sid >= 12))
    prob[live[0]], prob[live[1]], prob[live[2]] = np.nan, 0.5, 1.5
    prob[np.flatnonzero((outcome[mk] >= 0) & (sid == 9))[:3]] = [np.nan, 0.5, -0.25]
    present = (rng.random(S) < 0.7).astype(np.uint8)
    rel = np.where(present, rng.random(S), 0.5)
    conf = np.where(present, rng.random(S), 0.25)
    t_us = np.where(present, rng.integers(1, 10**15, S), orc.NO_TIMESTAMP).astype(np.int64)
    special = {12: 1.0, 13: 0.0, 14: 1.7, 15: -0.3, 16: np.nan, 4: np.nan, 7: 1.7, 10: 0.0}
    for s, v in special.items():
        rel[s], present[s], t_us[s] = v, 1, 99
    conf[[17, 8, 11]] = 1.0
    conf[[18, 9]] = 0.0
    present[[17, 18, 8, 9, 11]] = 1
    present[[1, 3, 6]] = 0  # absent rows: cold start, whatever the arrays hold there
    rel[[1, 3, 6]], conf[[1, 3, 6]], t_us[[1, 3, 6]] = 0.5, 0.25, orc.NO_TIMESTAMP
    rel[299], conf[299], t_us[299], present[299] = 0.8125, 0.4, 12345, 1  # in no market at all
    state = (rel, conf, t_us, present)
    exp = settle_ref(off, sid, prob, outcome, S, *state, NOW)
    return dict(off=off, sid=sid, prob=prob, outcome=outcome, S=S, state=state, exp=exp)


@pytest.mark.parametrize("kw", [{}, {"long_min": OFF}, {"long_min": 64, "chunk_bits": 64},
                                {"long_min": 1, "chunk_bits": 64}], ids=["default", "off", "long64", "long1"])
def test_edge_batch(edge, kw):
    e = edge
    total = e["exp"][4]
    assert total[:12].tolist() == list(EDGE_LENS) and (total[12:19] > 0).all() and total[290:].sum() == 0
    plan = _build(e["off"], e["sid"], e["prob"], e["outcome"], e["S"])
    assert plan.total.cpu().tolist() == total.tolist() and plan.correct.cpu().tolist() == e["exp"][5].tolist()
    assert plan.n_touched == int((total > 0).sum()) and plan.n_bits == int(total.sum())
    got = _apply(plan, *e["state"], **kw)
    _same(got, e["exp"][:4], f"edge {kw}")
    for g, before in zip(got, e["state"]):  # sources without a chain: every array bit-identical
        idle = total == 0
        assert idle[0] and idle[299]
        assert g[idle].tobytes() == np.asarray(before, g.dtype)[idle].tobytes()
    assert (got[2][total > 0] == NOW).all() and (got[3][total > 0] == 1).all()
    N.check_faults(_dev(), "edge batch")


def test_out_of_range_sid_raises_and_is_clamped(edge):
    e = edge
    sid = e["sid"].copy()
    mk = np.repeat(np.arange(len(e["off"]) - 1), np.diff(e["off"]))
    j = int(np.flatnonzero((e["outcome"][mk] >= 0) & (sid >= 12))[5])
    sid[j] = e["S"] + 5
    N.check_faults(_dev(), "clean slate")
    with pytest.raises(N.BCEError, match="sid"):
        _build(e["off"], sid, e["prob"], e["outcome"], e["S"])
    N.check_faults(_dev(), "fault word is cleared")
    plan = _build(e["off"], sid, e["prob"], e["outcome"], e["S"], check=False)
    got = _apply(plan, *e["state"])
    with pytest.raises(N.BCEError, match="sid"):
        N.check_faults(_dev(), "settle")
    # the stray signal went to the clamped row; every row is what the reference gives for that
    exp = settle_ref(e["off"], sid, e["prob"], e["outcome"], e["S"], *e["state"], NOW)
    _same(got, exp[:4], "clamped sid")
    assert plan.total.cpu().tolist() == exp[4].tolist()


def test_two_builds_give_identical_bits(edge):
    e = edge
    runs = []
    for _ in range(2):
        plan = _build(e["off"], e["sid"], e["prob"], e["outcome"], e["S"])
        runs.append((plan, _apply(plan, *e["state"], long_min=32, chunk_bits=64)))
    (pa, a), (pb, b) = runs
    for name in ("bits", "start", "order", "total", "correct"):
        assert torch.equal(getattr(pa, name), getattr(pb, name)), name
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ----------------------------------------------------------------------------- long path forced
LONG_MIN = 128


def _long_chains():
    rng = np.random.default_rng(41)
    alt = lambda n: (np.arange(n) & 1).astype(np.uint8)  # noqa: E731
    ch = {}
    ch["alternating"] = alt(5000)                       # no sync run: worker 0 walks all of it
    ch["ones"] = np.ones(5000, np.uint8)
    ch["random50"] = (rng.random(20000) < 0.5).astype(np.uint8)
    ch["random90"] = (rng.random(20000) < 0.9).astype(np.uint8)
    ch["runs_of_10"] = np.tile(np.r_[np.ones(10, np.uint8), np.zeros(1, np.uint8)], 300)  # never 11 equal
    for C in (64, 256):  # runs of exactly 11 that just fit a chunk (53), straddle (54, 63), open one (64)
        b = alt(C * 16)
        for chunk, at in ((3, 53), (6, 54), (9, 63), (12, 64)):
            a = chunk * C + (at if C == 64 else C - 64 + at)
            b[a:a + 11] = b[a]
            assert b[a - 1] != b[a] and b[a + 11] != b[a]
        ch[f"runs_of_11_c{C}"] = b
    tail = alt(1500)
    tail[-11:] = tail[-11]
    ch["run_ends_on_last_bit"] = tail
    ch["exactly_long_min"] = (rng.random(LONG_MIN) < 0.5).astype(np.uint8)
    ch["long_min_minus_1"] = (rng.random(LONG_MIN - 1) < 0.5).astype(np.uint8)
    return ch


def _batch_from_chains(chain_list, n_markets=4, skip=2):
    """Every source's chain cut over the resolved markets (outcomes alternate), in order; market
    ``skip`` is unresolved and holds decoys."""
    off, sid, prob, outcome = [0], [], [], []
    live = [m for m in range(n_markets) if m != skip]
    for m in range(n_markets):
        o = -1 if m == skip else m & 1
        outcome.append(o)
        for s, b in enumerate(chain_list):
            if m == skip:
                seg = np.ones(3, np.uint8)
            else:
                k = live.index(m)
                seg = b[len(b) * k // len(live):len(b) * (k + 1) // len(live)]
            sid += [s] * len(seg)
            prob += np.where(seg == max(o, 0), 0.75, 0.25).tolist()  # (p >= 0.5) == outcome <=> bit
        off.append(len(sid))
    return np.array(off, np.int64), np.array(sid, np.int32), np.array(prob), np.array(outcome, np.int8)


@pytest.fixture(scope="module")
def forced():
    ch = _long_chains()
    names = list(ch)
    off, sid, prob, outcome = _batch_from_chains([ch[n] for n in names])
    S = len(names)
    packed = chains(off, sid, prob, outcome, S)
    for s, n in enumerate(names):  # the batch encodes the chains it was made from
        assert np.array_equal(packed.bits[packed.start[s]:packed.start[s + 1]], ch[n]), n
    exp = {}
    for label, r0 in (("0.37", 0.37), ("nan", np.nan), ("1.7", 1.7)):
        state = (np.full(S, r0), np.linspace(0.0, 1.0, S), np.full(S, 7, np.int64), np.ones(S, np.uint8))
        exp[label] = (state, apply_chains(packed, *state, NOW))
    return dict(names=names, args=(off, sid, prob, outcome, S), exp=exp)


@pytest.mark.parametrize("chunk_bits", [64, 256])
@pytest.mark.parametrize("start", ["0.37", "nan", "1.7"])
def test_long_path_forced(forced, start, chunk_bits):
    plan = _build(*forced["args"])
    n_long, _, n_chunks = plan.chunks(LONG_MIN, chunk_bits)
    assert n_long == len(forced["names"]) - 1  # every chain but the one of long_min - 1 bits
    assert n_chunks == sum(-(-int(x) // chunk_bits) for x in plan.lens_desc[:n_long])
    state, exp = forced["exp"][start]
    on = _apply(plan, *state, long_min=LONG_MIN, chunk_bits=chunk_bits)
    off = _apply(plan, *state, long_min=OFF)
    for x, y in zip(on, off):
        assert x.tobytes() == y.tobytes(), (start, chunk_bits)
    _same(on, exp, f"forced {start} {chunk_bits}")
    N.check_faults(_dev(), "forced long path")


# ----------------------------------------------------------------------------- store layers
def _dump(path):
    conn = sqlite3.connect(path)
    rows = conn.execute("SELECT source_id, market_id, reliability, confidence, updated_at FROM sources "
                        "ORDER BY source_id, market_id").fetchall()
    conn.close()
    return rows


def _seed(store, rows):
    for name, key, r, c in rows:
        store._store._conn.execute(
            "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
            (name, key, r, c, "2026-01-01T00:00:00+00:00"))


def test_settle_markets_reproduces_the_reference_fixture(golden_dir, tmp_path):
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    g = json.load(open(os.path.join(golden_dir, "settle_small.json")))
    names, off = g["names"], g["offsets"]
    markets = []
    for m, o in enumerate(g["outcome"]):
        sig = [{"sourceId": names[g["sid"][i]], "probability": float(g["prob"][i])} for i in range(off[m], off[m + 1])]
        markets.append((sig, None if o < 0 else bool(o)))
    store = NamespacedReliabilityStore(str(tmp_path / "fixture.db"))
    key = {"domain": f"__domain__:{g['domain']}", "global": store.GLOBAL_MARKET_ID}
    _seed(store, [(names[s["source"]], key[s["scope"]], float(s["reliability"]), float(s["confidence"]))
                  for s in g["seeds"]])
    res = store.settle_markets(markets, domain=g["domain"], update_global=True)
    for scope in ("domain", "global"):
        got = {r.source_id: [repr(r.reliability), repr(r.confidence)] for r in store._store.list_sources(key[scope])}
        assert got == g["final"][scope], scope
    touched = {n for n, t in zip(names, g["total"]) if t > 0}
    assert set(res.records) == touched and set(res.global_records) == touched
    assert res.total == {n: g["total"][names.index(n)] for n in touched}
    assert res.correct == {n: g["correct"][names.index(n)] for n in touched}
    for n in touched:
        assert [repr(res.records[n].reliability), repr(res.records[n].confidence)] == g["final"]["domain"][n]
        assert [repr(res.global_records[n].reliability), repr(res.global_records[n].confidence)] == g["final"]["global"][n]
    store.close()


def test_settle_markets_equals_the_per_signal_loop_and_dry_run_writes_nothing(tmp_path):
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

    rng = np.random.default_rng(9)
    names = [f"agent-{c}" for c in "abcdef"]
    markets = []
    for m in range(8):
        sig = [{"sourceId": names[int(j)], "probability": float(np.round(rng.random(), 3))}
               for j in rng.integers(0, len(names), int(rng.integers(2, 8)))]
        if m == 5:
            sig.append({"sourceId": names[0]})  # a missing probability reads as 0.5
        markets.append((sig, None if m == 3 else bool(rng.integers(0, 2))))
    seeds = [(names[0], "__domain__:x", 0.95, 0.3), (names[1], "__global__", 0.05, 0.99),
             (names[2], "__domain__:x", 1.0, 1.0)]
    batched = NamespacedReliabilityStore(str(tmp_path / "batched.db"))
    looped = NamespacedReliabilityStore(str(tmp_path / "looped.db"))
    for st in (batched, looped):
        _seed(st, seeds)
    before = _dump(str(tmp_path / "batched.db"))
    dry = batched.settle_markets(markets, domain="x", update_global=True, dry_run=True)
    assert _dump(str(tmp_path / "batched.db")) == before  # dry run: the database is untouched
    wet = batched.settle_markets(markets, domain="x", update_global=True)
    for signals, outcome in markets:
        if outcome is None:
            continue
        for s in signals:
            looped.update_reliability(s["sourceId"], (s.get("probability", 0.5) >= 0.5) == outcome, domain="x",
                                      update_global=True)
    strip = lambda rows: [r[:4] for r in rows]  # noqa: E731  -- updated_at differs by construction
    assert strip(_dump(str(tmp_path / "batched.db"))) == strip(_dump(str(tmp_path / "looped.db")))
    assert len(_dump(str(tmp_path / "batched.db"))) > len(before)
    for a, b in ((dry.records, wet.records), (dry.global_records, wet.global_records)):
        assert {k: (v.reliability, v.confidence) for k, v in a.items()} == \
               {k: (v.reliability, v.confidence) for k, v in b.items()}
    # global only: one plan, one scope
    only = NamespacedReliabilityStore(str(tmp_path / "global.db"))
    ref = NamespacedReliabilityStore(str(tmp_path / "global_ref.db"))
    res = only.settle_markets(markets, update_global=True)
    assert res.global_records == {}
    for signals, outcome in markets:
        if outcome is None:
            continue
        for s in signals:
            ref.update_reliability(s["sourceId"], (s.get("probability", 0.5) >= 0.5) == outcome, update_global=True)
    assert strip(_dump(str(tmp_path / "global.db"))) == strip(_dump(str(tmp_path / "global_ref.db")))
    for st in (batched, looped, only, ref):
        st.close()
