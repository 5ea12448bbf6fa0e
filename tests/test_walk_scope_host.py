"""CPU checks of the namespaced walk-forward (no kernel): the oracle composition the GPU suite
compares against (tests/walk_scope_ref.py) reproduces the fixture recorded from the reference's
NamespacedReliabilityStore; batch.WalkScopePlan.order on CPU tensors against a brute-force count of
both chain families; the argument errors; the C ABI entry is declared and bound."""
import json
import os
import re

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.timeutil import iso_to_us, us_to_iso
from walk_scope_ref import fixture_batch, fixture_rows, scope_key, walk_scope_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = lambda x: repr(float(x))  # noqa: E731
NS = {0: "market", 1: "domain", 2: "global", 3: "global"}


def _fixture(golden_dir):
    return json.load(open(os.path.join(golden_dir, "walk_namespaced_small.json")))


def test_fixture_holds_the_cases_it_is_for(golden_dir):
    g = _fixture(golden_dir)
    off, sid, prob, outcome, md, dnames, S = fixture_batch(g)
    assert len(g["markets"]) == 12 and S == 6 and dnames == ["crypto", "sports"] and (md < 0).sum() == 2
    seeds = {(n, k): ts for n, k, _, _, ts in g["seeds"]}
    assert seeds[("src-2", "__domain__:crypto")] == "" and ("src-3", "__domain__:sports") not in seeds
    assert seeds[("src-0", "walk:m3")] and seeds[("src-1", "walk:m4")] == ""
    assert -1 in outcome and len(set(g["times_us"])) < 12 and (np.diff(g["times_us"]) < 0).any()
    assert any(len({s for s, _ in mk["signals"]}) < len(mk["signals"]) for mk in g["markets"])
    for run in g["runs"].values():
        reads = {(m, x[0]): x[3:] for m, r in enumerate(run["results"]) for x in r["read"]}
        assert reads[(0, "src-2")] == ["global", "global"] and reads[(3, "src-2")] == ["domain", "crypto"]
        assert reads[(1, "src-3")] == ["global", "cold-start"] and reads[(4, "src-3")] == ["domain", "sports"]
        assert reads[(3, "src-0")] == ["market", "walk:m3"] and reads[(4, "src-1")] == ["domain", "sports"]
        # src-4: its global row is written by market 2 (no domain), read by 4, 5 and 6, its crypto row by 6
        assert reads[(2, "src-4")] == ["global", "cold-start"] and reads[(6, "src-4")] == ["global", "global"]
        assert reads[(9, "src-4")] == ["domain", "crypto"]
        assert all(v == ["global", "cold-start"] for (m, n), v in reads.items() if n == "src-5")


@pytest.mark.parametrize("update_global", [False, True])
def test_oracle_composition_reproduces_the_reference_fixture(golden_dir, update_global):
    g = _fixture(golden_dir)
    names = g["names"]
    off, sid, prob, outcome, md, dnames, S = fixture_batch(g)
    run = g["runs"]["true" if update_global else "false"]
    exp, rows = walk_scope_ref(off, sid, prob, outcome, md, S, fixture_rows(g, iso_to_us), g["times_us"],
                               update_global=update_global)
    for m, r in enumerate(run["results"]):
        a, u = off[m], int(exp["n_unique"][m])
        assert R(exp["consensus"][m]) == r["consensus"] and R(exp["confidence"][m]) == r["confidence"], m
        assert R(exp["total_weight"][m]) == r["totalWeight"], m
        assert [[names[i & 0x7FFFFFFF], R(x), R(y), NS[int(sc)]] for i, x, y, sc in
                zip(exp["usid"][a:a + u], exp["rel_read"][a:a + u], exp["conf_read"][a:a + u],
                    exp["scope"][a:a + u])] == [x[:4] for x in r["read"]], m
        assert [int(sc) == 3 for sc in exp["scope"][a:a + u]] == [x[4] == "cold-start" for x in r["read"]], m
        assert [[names[i & 0x7FFFFFFF], R(x), R(y)] for i, x, y in
                zip(exp["usid"][a:a + u], exp["weight"][a:a + u], exp["nweight"][a:a + u])] == r["sourceWeights"], m
    got = sorted([names[s], scope_key(g, scope), R(r), R(c), us_to_iso(t) if has else ""]
                 for (scope, s), (r, c, t, has) in rows.items())
    assert got == sorted(run["final"])


# ----------------------------------------------------------------------------- the plan's integer half
def _restate(off, sid, outcome, md, S, update_global):
    """(usid, emarket, dentry, F, domain family, global family) by loops; a family is (qstart, qpos, qentry,
    qlast, slast)."""
    sid = np.clip(np.asarray(sid, np.int64), 0, S - 1)
    M = len(off) - 1
    usid, emarket = [], []
    for m in range(M):
        for s in sorted(set(sid[off[m]:off[m + 1]].tolist())):
            usid.append(s)
            emarket.append(m)
    E = len(usid)
    fkeys = sorted({(int(md[m]), s) for s, m in zip(usid, emarket) if md[m] >= 0})
    dentry = np.array([fkeys.index((int(md[m]), s)) if md[m] >= 0 else -1 for s, m in zip(usid, emarket)], np.int32)
    gout = [o if (update_global or md[m] < 0) else -1 for m, o in enumerate(outcome)]
    dout = [o if md[m] >= 0 else -1 for m, o in enumerate(outcome)]

    def family(chain, C, out):
        qstart, qpos, qentry = [0], [], []
        qlast, slast = np.full(E, -1, np.int32), np.full(C, -1, np.int64)
        for c in range(C):
            pos, last = 0, -1
            for e in range(E):  # entries ascend by market
                if chain[e] != c:
                    continue
                qpos.append(pos)
                qentry.append(e)
                qlast[e] = last
                m = emarket[e]
                if out[m] >= 0:
                    pos += int((sid[off[m]:off[m + 1]] == usid[e]).sum())
                    last = m
            qstart.append(len(qpos))
            slast[c] = last
        return (np.array(qstart, np.int64), np.array(qpos, np.int64), np.array(qentry, np.int32), qlast, slast)

    return (np.array(usid, np.int32), np.array(emarket, np.int32), dentry, len(fkeys),
            family(dentry, max(len(fkeys), 1), dout), family(usid, S, gout))


def _order(off, sid, prob, outcome, md, S, D, update_global=False):
    T = lambda a, dt: torch.tensor(np.asarray(a, dt))  # noqa: E731
    return batch.WalkScopePlan.order(T(off, np.int64), T(sid, np.int32), T(prob, np.float64), T(outcome, np.int8),
                                     T(md, np.int32), S, D, update_global)


def _check(off, sid, outcome, md, S, D, n_clamped=0):
    for update_global in (False, True):
        pairs, dplan, dentry, dq, gq, nc = _order(off, sid, np.full(len(sid), 0.5), outcome, md, S, D, update_global)
        usid, emarket, edentry, F, dfam, gfam = _restate(off, sid, outcome, md, S, update_global)
        E = len(usid)
        assert pairs.n_entries == E and dplan.n_entries == F and nc == n_clamped
        assert np.array_equal(pairs.usid[:E].numpy(), usid) and np.array_equal(pairs.emarket[:E].numpy(), emarket)
        assert dentry.dtype == torch.int32 and np.array_equal(dentry.numpy(), edentry)
        for fam, got, exp in (("domain", dq, dfam), ("global", gq, gfam)):
            for name, e in zip(("qstart", "qpos", "qentry", "qlast", "slast"), exp):
                x = getattr(got, name).numpy()
                assert x.dtype == e.dtype, (fam, name)
                assert np.array_equal(x, e), (fam, name, update_global)
        if not update_global and (np.asarray(md) >= 0).all():
            assert (gq.qlast.numpy() == -1).all() and (gq.slast.numpy() == -1).all()  # a family without bits
    # the single-family plan goes through the same code: its arrays are the global family's with every
    # market feeding it
    T = lambda a, dt: torch.tensor(np.asarray(a, dt))  # noqa: E731
    w = batch.WalkPlan.order(T(off, np.int64), T(sid, np.int32), T(np.full(len(sid), 0.5), np.float64),
                             T(outcome, np.int8), S)
    for got, exp in zip(w[1:6], (gq.qstart, gq.qpos, gq.qentry, gq.qlast, gq.slast)):
        assert got.numpy().tobytes() == exp.numpy().tobytes()


def test_small_batch_by_hand():
    off = [0, 3, 5, 5, 8]
    sid = [2, 0, 2, 1, 2, 0, 0, 2]
    md = [0, -1, 1, 0]
    pairs, dplan, dentry, dq, gq, _ = _order(off, sid, [0.5] * 8, [1, 1, 0, 1], md, 4, 2)
    # entries: (m0: 0, 2), (m1: 1, 2), (m3: 0, 2); the chains of domain 0: (0, 0) and (0, 2)
    assert dentry.tolist() == [0, 1, -1, -1, 0, 1]
    assert dq.qpos.tolist() == [0, 1, 0, 2] and dq.qentry.tolist() == [0, 4, 1, 5]
    assert dq.qlast.tolist() == [-1, -1, -1, -1, 0, 0] and dq.slast.tolist() == [3, 3]
    # global: only market 1 (no domain) leaves bits
    assert gq.qlast.tolist() == [-1, -1, -1, -1, -1, 1] and gq.slast.tolist() == [-1, 1, 1, -1]
    _check(off, sid, [1, 1, 0, 1], md, 4, 2)


def test_plans_hold_the_queries_order_returns():
    """4 markets, 3 sources, 2 domains: market 0 sees source 0 twice, market 1 has no domain, market 2 is
    unresolved.  A WalkPlan holds order()'s arrays as its ``q*`` fields and offers the very tensors as
    ``queries``; a WalkScopePlan holds order()'s ``dq`` / ``gq``."""
    off, sid = [0, 3, 5, 7, 10], [0, 2, 0, 1, 2, 0, 1, 0, 1, 2]
    outcome, md = [1, 0, -1, 1], [0, -1, 1, 0]
    fields = ("qstart", "qpos", "qentry", "qlast", "slast")
    T = lambda a, dt: torch.tensor(np.asarray(a, dt))  # noqa: E731
    args = (T(off, np.int64), T(sid, np.int32), T([0.5] * 10, np.float64), T(outcome, np.int8))
    pairs, *q, nc = batch.WalkPlan.order(*args, 3)
    # entries: (m0: 0, 2), (m1: 1, 2), (m2: 0, 1), (m3: 0, 1, 2); market 0 leaves two bits of source 0, market 2 none
    assert [x.tolist() for x in q] == [[0, 3, 6, 9], [0, 2, 2, 0, 1, 1, 0, 1, 2], [0, 4, 6, 2, 5, 7, 1, 3, 8],
                                       [-1, -1, -1, 0, 0, 1, 0, 1, 1], [3, 3, 3]]
    plan = batch.WalkPlan(None, pairs, *q, nc, args[3])
    assert not plan.lagged and plan.outcome is args[3] and isinstance(plan.queries, batch.WalkQueries)
    for name, x in zip(fields, q):
        assert getattr(plan.queries, name) is x and getattr(plan, name) is x, name
    pairs, dplan, dentry, dq, gq, nc = batch.WalkScopePlan.order(*args, T(md, np.int32), 3, 2)
    scoped = batch.WalkScopePlan(pairs, dplan, dentry, None, None, dq, gq, False, nc, args[3])
    assert scoped.dq is dq and scoped.gq is gq and not scoped.lagged and scoped.outcome is args[3]
    assert dentry.tolist() == [0, 2, -1, -1, 3, 4, 0, 1, 2]  # chains: (0, 0), (0, 1), (0, 2), (1, 0), (1, 1)
    _, _, _, F, dfam, gfam = _restate(off, sid, outcome, md, 3, False)
    assert F == dplan.n_entries == 5
    for fam, got, exp in (("domain", scoped.dq, dfam), ("global", scoped.gq, gfam)):
        for name, e in zip(fields, exp):
            assert np.array_equal(getattr(got, name).numpy(), e), (fam, name)
    assert scoped.gq.slast.tolist() == [-1, 1, 1] and scoped.dq.slast.tolist() == [3, 3, 3, -1, -1]
    # with update_global every resolved market feeds the global family: the single-scope plan's queries
    everything = batch.WalkScopePlan.order(*args, T(md, np.int32), 3, 2, True)[4]
    for name, x in zip(fields, q):
        assert torch.equal(getattr(everything, name), x) and getattr(everything, name).dtype == x.dtype, name


@pytest.mark.parametrize("seed", range(6))
def test_random_batches(seed):
    rng = np.random.default_rng(seed)
    M, S, D = int(rng.integers(1, 61)), int(rng.integers(1, 11)), int(rng.integers(1, 4))
    lens = rng.integers(0, 9, M)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    sid = rng.integers(0, S, int(off[-1]))
    _check(off.tolist(), sid, rng.integers(-1, 2, M), rng.integers(-1, D, M), S, D)


def test_degenerate_batches():
    off, sid = [0, 2, 3, 3, 6], [1, 0, 1, 2, 1, 1]
    _check(off, sid, [1, 0, 1, -1], [-1] * 4, 3, 0)          # D = 0: no domain family at all
    _check(off, sid, [1, 0, 1, 1], [0] * 4, 3, 1)            # every market in one domain
    _check(off, sid, [-1] * 4, [0, 1, -1, 1], 3, 2)          # no resolved market
    _check([0, 0, 0], [], [1, 0], [0, -1], 2, 1)             # empty markets
    _check([0], [], [], [], 2, 1)                            # M = 0
    _check([0, 2, 4], [0, 7, -3, 1], [1, -1], [0, -1], 2, 1, n_clamped=2)  # clamped and counted


def test_argument_errors():
    ok = dict(off=[0, 2, 3], sid=[0, 1, 0], prob=[0.5, 0.5, 0.5], outcome=[1, -1], md=[0, -1], S=2, D=1)

    def run(**kw):
        a = {**ok, **kw}
        return _order(a["off"], a["sid"], a["prob"], a["outcome"], a["md"], a["S"], a["D"])

    run()
    for bad in (0, -1, 1 << 31, "x"):
        with pytest.raises(ValueError, match="n_sources"):
            run(S=bad)
    for md in ([0, 1], [-2, 0]):
        with pytest.raises(ValueError, match="outside"):
            run(md=md)
    with pytest.raises(ValueError, match="one entry per market"):
        run(md=[0])
    with pytest.raises(ValueError, match="one entry per market"):
        run(outcome=[1])
    with pytest.raises(ValueError, match="offsets"):
        run(off=[0, 2, 4])
    with pytest.raises(ValueError, match="int8"):
        batch.WalkScopePlan.order(torch.tensor([0, 1]), torch.tensor([0], dtype=torch.int32),
                                  torch.tensor([0.5], dtype=torch.float64), torch.tensor([1], dtype=torch.int64),
                                  torch.tensor([0], dtype=torch.int32), 1, 1)


def test_abi_entry_is_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "bce.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bce_walk_scope_read\s*\(", src)
    assert "bce_walk_scope_read" in N.EXPORTED
    lib = N.load_library()
    assert lib.bce_abi_version() == 3
    # argument errors need no GPU: entries without markets, and a misaligned table
    assert lib.bce_walk_scope_read(4, *([None] * 3), 0, 1, *([None] * 6), 0, *([None] * 7), 0, *([None] * 6),
                                   30.0, 0.1, 0.5, 0.25, 0, 0, None, None, None, None) == -1
    assert b"walk_scope_read" in lib.bce_last_error()
