"""CPU checks of the market-scope pair table: the table builder and the plan's integer half on
CPU tensors, the merge's destination indices against a Python merge, the SQLite loader, the C
ABI's argument errors, and the expected-value helper against a fixture made by the reference."""
import json
import os

import numpy as np
import pytest
import torch

import pair_ref
from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.reliability import SQLiteReliabilityStore
from bayesian_engine.timeutil import NO_TIMESTAMP, iso_to_us
from pair_ref import fixture_batch, fixture_table

T = torch.from_numpy


def _fixture(golden_dir):
    with open(os.path.join(golden_dir, "pair_scope_small.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------ PairTable
def test_from_rows_sorts_and_rejects():
    rng = np.random.default_rng(3)
    M, S = 7, 11
    keys = rng.permutation(M * S)[:40]
    mk, sd = keys // S, keys % S
    rel, conf = rng.random(40), rng.random(40)
    t = rng.integers(0, 10**12, 40)
    has = rng.integers(0, 2, 40).astype(np.uint8)
    tab = batch.PairTable.from_rows(T(mk), T(sd.astype(np.int32)), T(rel), T(conf), T(t), T(has), M, S)
    exp = pair_ref.make_table(zip(mk, sd, rel, conf, t, has), M, S)
    for k in ("poffsets", "psid", "rel", "conf", "t_us", "has"):
        got = getattr(tab, k).numpy()
        assert got.dtype == exp[k].dtype and np.array_equal(got, exp[k]), k
    assert tab.n_rows == 40 and tab.n_markets == M and tab.n_sources == S
    with pytest.raises(ValueError, match="duplicate"):
        batch.PairTable.from_rows(T(np.array([1, 1])), T(np.array([2, 2], np.int32)), T(rel[:2]), T(conf[:2]),
                                  T(t[:2]), T(has[:2]), M, S)
    for bad_m, bad_s in ((M, 0), (-1, 0), (0, S), (0, -1)):
        with pytest.raises(ValueError, match="outside"):
            batch.PairTable.from_rows(T(np.array([bad_m])), T(np.array([bad_s], np.int32)), T(rel[:1]), T(conf[:1]),
                                      T(t[:1]), T(has[:1]), M, S)
    e = batch.PairTable.empty(3, 5, "cpu")
    assert e.n_rows == 0 and e.poffsets.tolist() == [0, 0, 0, 0]
    e2 = batch.PairTable.from_rows(*(T(np.zeros(0, dt)) for dt in (np.int64, np.int32, np.float64, np.float64,
                                                                  np.int64, np.uint8)), 3, 5)
    assert e2.n_rows == 0 and e2.poffsets.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------- PairPlan
def test_pair_plan_integer_half_matches_numpy():
    rng = np.random.default_rng(5)
    lens = np.array([0, 1, 5, 0, 9, 33, 2, 0])
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    S = 6  # few sources: many duplicates
    sid = rng.integers(0, S, off[-1]).astype(np.int32)
    prob = rng.random(off[-1])
    plan = batch.PairPlan.build(T(off), T(sid), T(prob), S)
    uoff, usid, emarket, esid = pair_ref.entries(off, sid, S)
    assert np.array_equal(plan.uoffsets.numpy(), uoff)
    assert np.array_equal(plan.usid.numpy(), usid) and plan.usid.dtype == torch.int32
    assert np.array_equal(plan.emarket.numpy(), emarket) and plan.emarket.dtype == torch.int32
    assert np.array_equal(plan.esid.numpy(), esid) and plan.esid.dtype == torch.int32
    assert (plan.n_markets, plan.n_entries, plan.n_sources) == (len(lens), len(usid), S)
    assert plan.n_entries < off[-1]  # the batch has duplicates
    with pytest.raises(ValueError, match="outside"):
        batch.PairPlan.build(T(off), T(np.where(np.arange(off[-1]) == 3, S, sid).astype(np.int32)), T(prob), S)
    empty = batch.PairPlan.build(T(np.zeros(3, np.int64)), T(np.zeros(0, np.int32)), T(np.zeros(0)), S)
    assert empty.n_entries == 0 and empty.uoffsets.tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------- merge
def _python_merge(t, uoffsets, usid, touched):
    """Final (market, sid, origin) rows: origin ("old", p) or ("entry", e), by a Python merge."""
    rows = {(m, s): ("old", p) for p, (m, s, *_) in enumerate(pair_ref.table_rows(t))}
    for m in range(len(uoffsets) - 1):
        for e in range(uoffsets[m], uoffsets[m + 1]):
            if touched[e]:
                rows[(m, int(usid[e]))] = ("entry", e)
    return [(m, s, rows[(m, s)]) for m, s in sorted(rows)]


@pytest.mark.parametrize("case", ["mixed", "empty_table", "nothing_touched"])
def test_merge_destinations_match_a_python_merge(case):
    S = 10
    #              market 0: rows 2 4 6     market 1: none      market 2: row 5     market 3: rows 0 9
    rows = [(0, 2), (0, 4), (0, 6), (2, 5), (3, 0), (3, 9)]
    if case == "empty_table":
        rows = []
    t = pair_ref.make_table([(m, s, 0.1 * i, 0.2, 7, 1) for i, (m, s) in enumerate(rows)], 5, S)
    # entries: front (0,1), match (0,2), middle (0,5), end (0,8); into the empty segment (1,3), (1,7);
    # untouched unmatched (2,1), end (2,6); match (3,0), untouched match (3,9); market 4 (empty, last): (4,4)
    ent = [(0, 1), (0, 2), (0, 5), (0, 8), (1, 3), (1, 7), (2, 1), (2, 6), (3, 0), (3, 9), (4, 4)]
    touched = np.array([1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 1], bool)
    if case == "nothing_touched":
        touched[:] = False
    emarket = np.array([m for m, _ in ent], np.int32)
    usid = np.array([s for _, s in ent], np.int32)
    uoffsets = np.zeros(6, np.int64)
    uoffsets[1:] = np.cumsum(np.bincount(emarket, minlength=5))
    lb, matched, _ = pair_ref.lookup(uoffsets, usid, t)
    dst_old, ins, dst_ins, upd, dst_upd, poff = batch._pair_merge_index(T(lb), T(matched), T(touched), T(emarket),
                                                                         T(t["poffsets"]))
    exp = _python_merge(t, uoffsets, usid, touched)
    origin = {}
    for p, d in enumerate(dst_old.tolist()):
        origin[d] = ("old", p)
    for e, d in zip(ins.tolist(), dst_ins.tolist()):
        assert d not in origin
        origin[d] = ("entry", e)
    for e, d in zip(upd.tolist(), dst_upd.tolist()):
        assert origin[d] == ("old", int(lb[e]))
        origin[d] = ("entry", e)
    assert sorted(origin) == list(range(len(exp)))
    assert [origin[d] for d in range(len(exp))] == [o for _, _, o in exp]
    exp_off = np.zeros(6, np.int64)
    exp_off[1:] = np.cumsum(np.bincount([m for m, _, _ in exp], minlength=5))
    assert np.array_equal(poff.numpy(), exp_off)


# ------------------------------------------------------------------------------------ SQLite
def test_load_pair_table_from_sqlite(tmp_path, monkeypatch):
    store = SQLiteReliabilityStore(str(tmp_path / "pairs.db"))
    names = [f"s{i:02d}" for i in range(9)]
    mids = [f"mk:{i}" for i in range(23)]
    rng = np.random.default_rng(11)
    exp_rows = []
    for mi, m in enumerate(mids):
        for si, s in enumerate(names + ["zz-not-ranked"]):
            if rng.random() < 0.4:
                ts = ["2026-02-01T00:00:00+00:00", "", "garbage"][int(rng.integers(0, 3))]
                r, c = float(rng.random()), float(rng.random())
                store._conn.execute("INSERT INTO sources VALUES (?,?,?,?,?)", (s, m, r, c, ts))
                if s in names:
                    exp_rows.append((mi, si, r, c, iso_to_us(ts), 1 if ts else 0))
    store._conn.execute("INSERT INTO sources VALUES (?,?,?,?,?)", ("s00", "other-market", 0.3, 0.3, ""))
    store._conn.execute("INSERT INTO sources VALUES (?,?,?,?,?)", ("s00", "__global__", 0.3, 0.3, ""))
    exp = pair_ref.make_table(exp_rows, len(mids), len(names))
    statements = []
    store._conn.set_trace_callback(statements.append)
    for chunk in (900, 5):  # 5: the 23 ids span five IN (...) statements
        monkeypatch.setattr(SQLiteReliabilityStore, "_IN_CHUNK", chunk)
        statements.clear()
        tab = store.load_pair_table(mids, names, device="cpu")
        assert len(statements) == -(-len(mids) // chunk)  # never one statement per market
        for k in ("poffsets", "psid", "rel", "conf", "t_us", "has"):
            assert np.array_equal(getattr(tab, k).numpy(), exp[k]), (chunk, k)
        assert tab.n_markets == len(mids) and tab.n_sources == len(names)
    assert (exp["t_us"] == NO_TIMESTAMP).any() and (exp["has"][exp["t_us"] == NO_TIMESTAMP] == 1).any()
    # more ids than one statement's host parameters: two statements at the default chunk
    monkeypatch.undo()
    assert SQLiteReliabilityStore._IN_CHUNK == 900
    statements.clear()
    many = [f"none:{i}" for i in range(1000)] + mids
    big = store.load_pair_table(many, names, device="cpu")
    assert len(statements) == 2 and big.n_markets == 1023
    assert np.array_equal(big.poffsets.numpy()[1000:], exp["poffsets"]) and not big.poffsets.numpy()[:1000].any()
    assert np.array_equal(big.rel.numpy(), exp["rel"])
    # row i of the batch is market_ids[i]
    rev = store.load_pair_table(mids[::-1], names, device="cpu")
    assert np.array_equal(np.diff(rev.poffsets.numpy()), np.diff(exp["poffsets"])[::-1])
    with pytest.raises(ValueError, match="duplicate"):
        store.load_pair_table([mids[0], mids[1], mids[0]], names, device="cpu")
    assert store.load_pair_table([], names, device="cpu").n_rows == 0
    store.close()


# --------------------------------------------------------------------------------------- C ABI
def test_pair_resolve_argument_errors_need_no_gpu():
    lib = N.load_library()
    assert "bce_pair_resolve" in N.EXPORTED

    def call(mode=0, qoff=1, M=2, qsid=1, Q=3, poff=1, tab=1, P=4, S=5, dense=(0, 0), apply_decay=1, relconf=0):
        p = lambda v: N.C.c_void_p(v * 64)  # noqa: E731  -- never dereferenced: the call fails first
        d = []
        for on in dense:
            d += [p(on)] * 4
        return lib.bce_pair_resolve(mode, p(qoff), M, p(qsid), None, Q, p(poff), p(tab), p(tab), p(tab), p(tab),
                                    p(tab), P, S, *d, apply_decay, 0, 30.0, 0.1, 0.5, 0.25, 0, None, None,
                                    N.C.c_void_p(relconf), None, None, None, None, None, None, None)

    for kw, word in ((dict(mode=7), b"mode"), (dict(M=-1), b"shape"), (dict(Q=-1), b"shape"), (dict(P=-1), b"shape"),
                     (dict(S=0), b"shape"), (dict(M=0), b"without markets"), (dict(qoff=0), b"offsets"),
                     (dict(poff=0), b"offsets"), (dict(qsid=0), b"qsid"), (dict(tab=0), b"table"),
                     (dict(dense=(1, 0)), b"BCE_PAIR_NAMESPACED"), (dict(mode=2, dense=(0, 1)), b"BCE_PAIR_NAMESPACED"),
                     (dict(relconf=8), b"aligned")):
        assert call(**kw) == -1, kw
        assert word in lib.bce_last_error(), (kw, lib.bce_last_error())
    # nothing to do: no markets, no entries, no rows
    assert call(M=0, Q=0, P=0) == 0


# ------------------------------------------------------------------- the helper vs the reference
def test_helper_reproduces_reference_fixture(golden_dir):
    g = _fixture(golden_dir)
    names, mids = g["names"], g["market_ids"]
    offsets, sid, prob, outcome = fixture_batch(g)
    assert len(mids) == 6 and len(names) == 5 and (outcome == -1).sum() == 1
    assert max(np.diff(offsets)) <= 8 and len(pair_ref.entries(offsets, sid, len(names))[1]) < len(sid)
    t = fixture_table(g)
    assert (t["t_us"] == NO_TIMESTAMP).sum() == 2 and (t["has"] == 0).sum() == 1
    # compute_all_consensus(SQLiteReliabilityStore): store mode, decay at the frozen clock
    exp, uoffsets, usid, _ = pair_ref.consensus(offsets, sid, prob, t, g["now_us"])
    for m, mid in enumerate(mids):
        ref = g["consensus"][mid]
        assert ref["consensus"] == exp["consensus"][m] and ref["confidence"] == exp["confidence"][m], mid
        assert ref["normalization"]["totalWeight"] == exp["total_weight"][m]
        a, u = int(offsets[m]), int(exp["n_unique"][m])
        assert [w["sourceId"] for w in ref["sourceWeights"]] == [names[s] for s in usid[uoffsets[m]:uoffsets[m + 1]]]
        assert [w["weight"] for w in ref["sourceWeights"]] == exp["weight"][a:a + u].tolist()
        assert [w["normalizedWeight"] for w in ref["sourceWeights"]] == exp["nweight"][a:a + u].tolist()
    # the per-signal update_reliability(market_id=m, update_global=True) loop
    new, total, correct = pair_ref.settle(offsets, sid, prob, outcome, t, g["now_us"])
    got = {(names[s], mids[m]): (r, c) for m, s, r, c, _, _ in pair_ref.table_rows(new)}
    ref = {(s, m): (r, c) for s, m, r, c in g["final"] if m != "__global__"}
    assert got == ref
    assert total.sum() == sum(np.diff(offsets)[outcome >= 0])
