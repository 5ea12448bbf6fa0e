"""CPU checks of the per-market domain scope: the expected-value helper (tests/domain_ref.py)
against the fixture made by the reference, ``DomainPlan.build`` on CPU tensors, the domain rows
through ``load_pair_table``, the C ABI's argument errors and the ``ValueError`` / ``TypeError`` /
``NativeUnavailable`` cases of the public layers."""
import json
import os

import numpy as np
import pytest
import torch

import domain_ref
import pair_ref
from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore
from bayesian_engine.reliability import SQLiteReliabilityStore
from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore
from bayesian_engine.timeutil import NO_TIMESTAMP
from pair_ref import fixture_batch, fixture_table

T = torch.from_numpy


def _fixture(golden_dir):
    with open(os.path.join(golden_dir, "domain_scope_small.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------- the helper vs the reference
def test_helper_reproduces_reference_fixture(golden_dir):
    g = _fixture(golden_dir)
    names, mids = g["names"], g["market_ids"]
    offsets, sid, prob, outcome = fixture_batch(g)
    dnames, md = domain_ref.fixture_domains(g)
    assert len(mids) == 7 and len(names) == 5 and len(dnames) == 3 and (md == -1).sum() == 1
    assert (outcome == -1).sum() == 1 and 0.5 in prob.tolist()
    assert len(pair_ref.entries(offsets, sid, len(names))[1]) < len(sid)  # duplicates in a market
    t, dt, glob = fixture_table(g), domain_ref.fixture_domain_table(g), fixture_table(g, key="__global__")
    assert (t["has"] == 0).sum() == 1 and (dt["has"] == 0).sum() == 1
    assert ((dt["t_us"] == NO_TIMESTAMP) & (dt["has"] == 1)).sum() == 1  # the unparseable stamp
    exp, uoffsets, usid, scope = domain_ref.consensus(offsets, sid, prob, t, dt, md, g["now_us"], glob)
    assert set(scope.tolist()) == {0, 1, 2, 3}
    # the seeded corner rows resolve as the generator says
    emarket = domain_ref.entry_markets(uoffsets)
    at = {(int(m), int(s)): int(c) for m, s, c in zip(emarket, usid, scope)}
    assert at[(1, 4)] == 1   # market row with an empty stamp -> the sports domain row
    assert at[(0, 3)] == 1   # the crypto domain row with an unparseable stamp is used
    assert at[(4, 2)] == 2   # the politics domain row with an empty stamp -> global
    assert at[(3, 1)] == 0 and at[(3, 4)] == 3  # the market without a domain: its row, or the cold start
    for m, mid in enumerate(mids):
        ref = g["consensus"][mid]
        assert ref["consensus"] == exp["consensus"][m] and ref["confidence"] == exp["confidence"][m], mid
        assert ref["normalization"]["totalWeight"] == exp["total_weight"][m]
        a, u = int(offsets[m]), int(exp["n_unique"][m])
        assert [w["sourceId"] for w in ref["sourceWeights"]] == [names[s] for s in usid[uoffsets[m]:uoffsets[m + 1]]]
        assert [w["weight"] for w in ref["sourceWeights"]] == exp["weight"][a:a + u].tolist()
        assert [w["normalizedWeight"] for w in ref["sourceWeights"]] == exp["nweight"][a:a + u].tolist()
        assert ref["diagnostics"]["coldStartSources"] == []
    # the per-signal update_reliability(domain=d, update_global=...) loops: every row of the database
    for update_global in (True, False):
        assert domain_ref.fixture_settle(g, update_global) == domain_ref.fixture_final(g, update_global)
    assert domain_ref.fixture_final(g, True) != domain_ref.fixture_final(g, False)


# ----------------------------------------------------------------------------------- DomainPlan
def _plan_case(md, D, seed=5):
    rng = np.random.default_rng(seed)
    lens = np.array([0, 1, 5, 0, 9, 33, 2, 0])
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    S = 6  # few sources: a source in several domains, many duplicates
    sid = rng.integers(0, S, off[-1]).astype(np.int32)
    return off, sid, np.asarray(md, np.int32), S, D


@pytest.mark.parametrize("md, D", [([2, 0, 3, -1, 0, 3, -1, 2], 5),      # domains 1 and 4 have no market
                                   ([-1] * 8, 3),                        # no market has a domain
                                   ([-1] * 8, 0),
                                   ([0] * 8, 1)])
def test_domain_plan_matches_the_helper(md, D):
    off, sid, md, S, D = _plan_case(md, D)
    plan = batch.DomainPlan.build(T(off), T(sid), T(md), S, D)
    uoff, usid, edom, esid = domain_ref.domain_entries(off, sid, md, S, D)
    assert np.array_equal(plan.uoffsets.numpy(), uoff) and plan.uoffsets.dtype == torch.int64
    assert np.array_equal(plan.usid.numpy(), usid) and plan.usid.dtype == torch.int32
    assert np.array_equal(plan.emarket.numpy(), edom) and plan.emarket.dtype == torch.int32
    assert np.array_equal(plan.esid.numpy(), esid) and plan.esid.dtype == torch.int32
    assert (plan.n_markets, plan.n_entries, plan.n_sources) == (D, len(usid), S)
    assert isinstance(plan, batch.PairPlan) and np.array_equal(plan.market_domain.numpy(), md)
    live = np.repeat(md, np.diff(off)) >= 0
    assert (esid[~live] == 0).all() and (not live.any() or esid[live].max() == len(usid) - 1)
    if D == 5:
        assert len(set(usid.tolist())) < len(usid)  # a source in several domains
        assert np.diff(uoff)[[1, 4]].tolist() == [0, 0]


def test_domain_plan_rejects():
    off, sid, md, S, D = _plan_case([2, 0, 3, -1, 0, 3, -1, 2], 5)
    build = batch.DomainPlan.build
    with pytest.raises(ValueError, match="sid"):
        build(T(off), T(np.where(np.arange(len(sid)) == 3, S, sid).astype(np.int32)), T(md), S, D)
    with pytest.raises(ValueError, match="sid"):
        build(T(off), T(np.where(np.arange(len(sid)) == 3, -1, sid).astype(np.int32)), T(md), S, D)
    for bad in (D, -2):
        with pytest.raises(ValueError, match="market_domain"):
            build(T(off), T(sid), T(np.where(np.arange(len(md)) == 1, bad, md).astype(np.int32)), S, D)
    with pytest.raises(ValueError, match="market_domain"):
        build(T(off), T(sid), T(md[:-1]), S, D)
    with pytest.raises(ValueError, match="offsets"):
        build(T(off[::-1].copy()), T(sid), T(md), S, D)
    with pytest.raises(ValueError, match="offsets"):
        build(T(off), T(sid[:-1]), T(md), S, D)
    with pytest.raises(ValueError, match="n_sources"):
        build(T(off), T(sid), T(md), 0, D)
    with pytest.raises(ValueError, match="n_domains"):
        build(T(off), T(sid), T(md), S, -1)
    empty = build(T(np.zeros(3, np.int64)), T(np.zeros(0, np.int32)), T(np.array([0, -1], np.int32)), S, 2)
    assert empty.n_entries == 0 and empty.uoffsets.tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------ SQLite
def test_domain_rows_load_as_a_pair_table(golden_dir, tmp_path):
    g = _fixture(golden_dir)
    store = SQLiteReliabilityStore(str(tmp_path / "domains.db"))
    for row in g["seeds"]:
        store._conn.execute("INSERT INTO sources VALUES (?,?,?,?,?)", tuple(row))
    dnames, _ = domain_ref.fixture_domains(g)
    tab = store.load_pair_table([f"__domain__:{d}" for d in dnames], g["names"], device="cpu")
    exp = domain_ref.fixture_domain_table(g)
    for k in ("poffsets", "psid", "rel", "conf", "t_us", "has"):
        assert np.array_equal(getattr(tab, k).numpy(), exp[k]), k
    assert tab.n_markets == len(dnames) == 3 and tab.n_sources == len(g["names"])
    for d in range(3):  # strictly ascending inside a domain
        assert (np.diff(exp["psid"][exp["poffsets"][d]:exp["poffsets"][d + 1]]) > 0).all()
    store.close()


# --------------------------------------------------------------------------------------- C ABI
def test_scope_resolve_argument_errors_need_no_gpu():
    lib = N.load_library()
    assert "bce_scope_resolve" in N.EXPORTED

    def call(qoff=1, M=2, qsid=1, Q=3, poff=1, tab=1, P=4, mdom=1, doff=1, D=2, dtab=1, R=4, S=5, glob=0,
             apply_decay=1, relconf=0):
        p = lambda v: N.C.c_void_p(v * 64)  # noqa: E731  -- never dereferenced: the call fails first
        return lib.bce_scope_resolve(p(qoff), M, p(qsid), None, Q, p(poff), p(tab), p(tab), p(tab), p(tab), p(tab), P,
                                     p(mdom), p(doff), D, p(dtab), p(dtab), p(dtab), p(dtab), p(dtab), R, S,
                                     p(glob), None, None, None, apply_decay, 0, 30.0, 0.1, 0.5, 0.25, 0, None, None,
                                     None, None, N.C.c_void_p(relconf), None, None, None)

    for kw, word in ((dict(M=-1), b"shape"), (dict(Q=-1), b"shape"), (dict(P=-1), b"shape"), (dict(D=-1), b"shape"),
                     (dict(R=-1), b"shape"), (dict(S=0), b"shape"), (dict(M=0), b"without markets"),
                     (dict(D=0), b"without domains"), (dict(qoff=0), b"qoffsets"), (dict(mdom=0), b"market_domain"),
                     (dict(qsid=0), b"qsid"), (dict(poff=0), b"poffsets"), (dict(tab=0), b"market table"),
                     (dict(doff=0), b"doffsets"), (dict(dtab=0), b"domain table"), (dict(glob=1), b"global"),
                     (dict(relconf=8), b"aligned")):
        assert call(**kw) == -1, kw
        assert word in lib.bce_last_error(), (kw, lib.bce_last_error())
    # nothing to do: no markets, no entries, no rows
    assert call(M=0, Q=0, P=0) == 0


# ------------------------------------------------------------------------------ public layers
def _tiny():
    S = 3
    off, sid, prob = T(np.array([0, 2, 3], np.int64)), T(np.array([0, 2, 1], np.int32)), T(np.array([0.2, 0.7, 0.5]))
    dense = batch.ScopeTable(torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64),
                             torch.zeros(S, dtype=torch.int64), torch.zeros(S, dtype=torch.uint8))
    return off, sid, prob, batch.PairTable.empty(2, S, "cpu"), batch.PairTable.empty(1, S, "cpu"), \
        T(np.array([0, -1], np.int32)), dense


def test_consensus_pairs_rejects_mixed_domain_arguments():
    off, sid, prob, pairs, domains, md, dense = _tiny()
    with pytest.raises(ValueError, match="exclude"):
        batch.consensus_pairs(off, sid, prob, pairs, 0, namespaced=True, domain=dense, domains=domains,
                              market_domain=md)
    with pytest.raises(ValueError, match="namespaced"):
        batch.consensus_pairs(off, sid, prob, pairs, 0, domains=domains, market_domain=md)
    with pytest.raises(ValueError, match="together"):
        batch.consensus_pairs(off, sid, prob, pairs, 0, namespaced=True, domains=domains)
    with pytest.raises(ValueError, match="together"):
        batch.consensus_pairs(off, sid, prob, pairs, 0, namespaced=True, market_domain=md)


def _markets():
    return [([{"sourceId": "a", "probability": 0.7}, {"sourceId": "b", "probability": 0.2}], True),
            ([{"sourceId": "a", "probability": 0.4}], False)]


def test_settle_markets_rejects_and_needs_the_gpu():
    ns = NamespacedReliabilityStore()
    with pytest.raises(ValueError, match="exclude"):
        ns.settle_markets(_markets(), domain="crypto", domains=["crypto", None])
    with pytest.raises(ValueError, match="entries"):
        ns.settle_markets(_markets(), domains=["crypto"])
    assert ns.settle_markets([], domains=[]).records == {}
    if not torch.cuda.is_available():
        with pytest.raises(N.NativeUnavailable):
            ns.settle_markets(_markets(), domains=["crypto", None])
        with pytest.raises(N.NativeUnavailable):
            ns.settle_markets(_markets(), domains=[None, ""], update_global=True)
    ns.close()


def test_market_layer_rejects():
    ms = MarketStore()
    ms.create_market(MarketId("crypto:btc")).add_signal({"sourceId": "a", "probability": 0.7})
    plain = SQLiteReliabilityStore()
    for store in (plain, None):
        with pytest.raises(TypeError, match="NamespacedReliabilityStore"):
            ms.compute_all_consensus(store, domain_of="category")
    ns = NamespacedReliabilityStore()
    with pytest.raises(TypeError, match="callable"):
        ms.compute_all_consensus(ns, domain_of="no-such-rule")
    agg = CrossMarketAggregator(ms)
    with pytest.raises(ValueError, match="exclude"):
        agg.settle_resolved(ns, domain="crypto", domain_of="category")
    with pytest.raises(TypeError, match="callable"):
        agg.settle_resolved(ns, domain_of=3)
    assert MarketId("crypto:btc").category == "crypto" and MarketId("plain").category is None
    if not torch.cuda.is_available():
        with pytest.raises(N.NativeUnavailable):
            ms.compute_all_consensus(ns, domain_of="category")
    plain.close()
    ns.close()
