"""GPU checks of the per-market domain scope (batch.scope_resolve / consensus_pairs(domains=) /
settle_domains and the store layers): every output equals the oracle composition of
tests/domain_ref.py exactly (``np.array_equal`` / ``tobytes``), and the golden fixture made by the
reference is reproduced through the stores."""
import itertools
import json
import os
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest
import torch

import domain_ref
import pair_ref
from bayesian_engine import _native as N
from bayesian_engine import batch

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


def _emarket(qoff):
    return domain_ref.entry_markets(qoff).astype(np.int32)


def _check_scope_resolve(t, dt, md, qoff, qsid, glob, *, with_emarket=(True, False), keep=None, md_ref=None,
                         dt_ref=None):
    """scope_resolve with and without the market table / the global scope, apply_decay and
    mark_cold both ways: every output against domain_ref.  ``keep``: the entries compared (all);
    ``md_ref`` / ``dt_ref``: the market_domain and the domain table the helper sees (``md``, ``dt``)."""
    S = dt["n_sources"]
    Q = len(qsid)
    keep = np.ones(Q, bool) if keep is None else keep
    md_ref = md if md_ref is None else md_ref
    tab, dtab = _table(t), _table(dt)
    dt = dt if dt_ref is None else dt_ref
    dq, ds, dm = _T(qoff), _T(qsid), _T(md)
    qclean = np.clip(qsid, 0, S - 1)
    lb, matched, _ = pair_ref.lookup(qoff, qclean, t)
    dlb, dmatched, _ = domain_ref.lookup_domain(qoff, qclean, md_ref, dt)
    for with_table, with_glob, decay in itertools.product((True, False), (True, False), (True, False)):
        rel, conf, scope = domain_ref.resolve(qoff, qclean, t if with_table else None, dt, md_ref, NOW,
                                              glob if with_glob else None, decay)
        for em, cold in itertools.product(with_emarket, (False, True)):
            what = (with_table, with_glob, decay, em, cold)
            got = batch.scope_resolve(dq, ds, tab if with_table else None, dtab, dm, NOW,
                                      emarket=_T(_emarket(qoff)) if em else None,
                                      global_scope=_scope(glob) if with_glob else None, apply_decay=decay,
                                      mark_cold=cold)
            g_lb, g_matched, g_dlb, g_dmatched, table, g_scope = got
            if with_table:
                assert np.array_equal(g_lb.cpu().numpy()[keep], lb[keep]), what
                assert np.array_equal(g_matched.cpu().numpy()[keep], matched[keep]), what
            else:
                assert not g_lb.cpu().numpy().any() and not g_matched.cpu().numpy().any(), what
            assert np.array_equal(g_dlb.cpu().numpy()[keep], dlb[keep]), what
            assert np.array_equal(g_dmatched.cpu().numpy()[keep], dmatched[keep]), what
            rc = table.relconf.cpu().numpy()[:Q]
            assert rc[keep, 0].tobytes() == rel[keep].tobytes() and rc[keep, 1].tobytes() == conf[keep].tobytes(), what
            assert np.array_equal(g_scope.cpu().numpy()[keep], scope[keep]), what
            if keep.all():
                words = table.bits.cpu().numpy().view(np.uint32)
                assert np.array_equal(words, domain_ref.present_words(scope, cold)), what
            if with_table and with_glob and decay and not cold:  # index=False: the same table, no index outputs
                bare = batch.scope_resolve(dq, ds, tab, dtab, dm, NOW, index=False, global_scope=_scope(glob))
                assert bare[:4] == (None, None, None, None)
                assert bare[4].relconf.cpu().numpy()[:Q][keep].tobytes() == rc[keep].tobytes(), what


# ---------------------------------------------------------------------------------------- lookup
DOM_LENS = (0, 1, 2, 63, 64, 65, 257, 1500)
MKT_LENS = (0, 1, 16)


@pytest.fixture(scope="module")
def segments():
    """Domain d has DOM_LENS[d] rows at the odd sids; one more domain of 64 rows that no market
    uses sits in the middle.  Every domain has a market that queries every row, every gap, below
    the first row and above the last; the markets' own segments cycle through MKT_LENS (rows at
    the lowest queried sids).  Between them: markets without a domain, one with rows and no
    query."""
    rng = np.random.default_rng(2027)
    S = 2 * max(DOM_LENS) + 2
    dom_lens = list(DOM_LENS[:4]) + [64] + list(DOM_LENS[4:])
    unused = 4
    drows = [(d, 2 * i + 1, *_rand_row(rng)) for d, n in enumerate(dom_lens) for i in range(n)]
    dt = pair_ref.make_table(drows, len(dom_lens), S)
    rows, qoff, qsid, md = [], [0], [], []
    for d, n in enumerate(dom_lens):
        if d == unused:
            continue
        for k, domain in enumerate((d, -1)):
            m = len(md)
            q = list(range(0, 2 * n + 1)) if domain >= 0 else list(range(0, min(2 * n + 1, 40)))
            L = MKT_LENS[(d + k) % 3]
            rows += [(m, s, *_rand_row(rng)) for s in range(min(L, S))]
            qsid += q
            qoff.append(len(qsid))
            md.append(domain)
    m = len(md)  # rows and no query
    rows += [(m, s, *_rand_row(rng)) for s in range(0, 64, 2)]
    qoff.append(len(qsid))
    md.append(1)
    t = pair_ref.make_table(rows, len(md), S)
    return dict(t=t, dt=dt, md=np.array(md, np.int32), qoff=np.array(qoff, np.int64), qsid=np.array(qsid, np.int32),
                S=S, glob=_dense(rng, S, 0.6), unused=unused)


@pytest.mark.parametrize("with_emarket", [True, False])
def test_lookup_every_segment_length(segments, with_emarket):
    s = segments
    dt, md = s["dt"], s["md"]
    assert (dt["has"] == 0).any() and ((dt["t_us"] == NOTS) & (dt["has"] == 1)).any()
    assert sorted(set(np.diff(dt["poffsets"]).tolist())) == sorted(DOM_LENS)
    assert sorted(set(np.diff(s["t"]["poffsets"]).tolist()) - {32}) == sorted(MKT_LENS)
    assert (md == -1).any() and s["unused"] not in md.tolist()
    rel, conf, scope = domain_ref.resolve(s["qoff"], s["qsid"], s["t"], dt, md, NOW, s["glob"])
    assert set(scope.tolist()) == {0, 1, 2, 3}
    N.check_faults(_dev(), "clean slate")
    _check_scope_resolve(s["t"], dt, md, s["qoff"], s["qsid"], s["glob"], with_emarket=(with_emarket,))
    N.check_faults(_dev(), "lookup")


@pytest.mark.parametrize("Q", [0, 31, 32, 33, 63, 64, 65])
def test_lookup_ballot_bits_and_tiny_shapes(Q):
    rng = np.random.default_rng(Q)
    S = 80
    drows = [(0, s, *_rand_row(rng)) for s in range(S) if rng.random() < 0.5]
    rows = [(0, s, *_rand_row(rng)) for s in range(S) if rng.random() < 0.3]
    qoff, qsid = np.array([0, Q], np.int64), np.arange(Q, dtype=np.int32)
    glob = _dense(rng, S, 0.3)
    N.check_faults(_dev(), "clean slate")
    for dt in (pair_ref.make_table(drows, 1, S), pair_ref.make_table([], 1, S)):  # D = 1, and R = 0
        for t in (pair_ref.make_table(rows, 1, S), pair_ref.make_table([], 1, S)):
            _check_scope_resolve(t, dt, np.zeros(1, np.int32), qoff, qsid, glob)
    N.check_faults(_dev(), "tiny shapes")


def test_lookup_more_domains_than_entries_and_markets():
    """D = 300 > Q = 5 > M = 3: the domain offsets are checked by lanes beyond the entries (two
    workgroups), a bad pair there is seen, and D = 0 works."""
    rng = np.random.default_rng(300)
    S, D = 50, 300
    drows = [(d, s, *_rand_row(rng)) for d in range(D) for s in range(S) if rng.random() < 0.05]
    dt = pair_ref.make_table(drows + [(299, 7, 0.3, 0.4, NOTS, 1), (17, 9, 0.6, 0.1, NOW - DAY, 1)], D, S)
    t = pair_ref.make_table([(1, 9, 0.2, 0.2, NOW - 3 * DAY, 1)], 3, S)
    md = np.array([299, 17, -1], np.int32)
    qoff, qsid = np.array([0, 2, 4, 5], np.int64), np.array([3, 7, 9, 11, 9], np.int32)
    glob = _dense(rng, S, 0.5)
    N.check_faults(_dev(), "clean slate")
    _check_scope_resolve(t, dt, md, qoff, qsid, glob)
    N.check_faults(_dev(), "D > Q")
    bad = dict(dt)
    bad["poffsets"] = dt["poffsets"].copy()
    bad["poffsets"][280] = bad["poffsets"][279] - 1  # domains 279 and 280: no market uses them
    assert 279 not in md and 280 not in md and bad["poffsets"][280] >= 0
    _check_scope_resolve(t, bad, md, qoff, qsid, glob, with_emarket=(True,), dt_ref=dt)
    with pytest.raises(N.BCEError, match="offsets"):
        N.check_faults(_dev(), "doffsets beyond the entries")
    none = pair_ref.make_table([], 0, S)
    _check_scope_resolve(t, none, np.full(3, -1, np.int32), qoff, qsid, glob)
    N.check_faults(_dev(), "D = 0")


def test_one_domain_equals_the_dense_namespaced_lookup():
    """Every market in one domain, the same rows given dense to pair_resolve: bit for bit."""
    rng = np.random.default_rng(41)
    S, M = 300, 40
    dense = _dense(rng, S, 0.5)
    stored = rng.random(S) < 0.6  # a dense row that does not exist has has = 0
    rel, conf, tus, has = (np.where(stored, a, f) for a, f in zip(dense, (0.5, 0.25, NOTS, 0)))
    has = has.astype(np.uint8)
    dt = pair_ref.make_table([(0, s, rel[s], conf[s], tus[s], has[s]) for s in np.flatnonzero(stored)], 1, S)
    assert (dt["has"] == 0).any()
    lens = rng.integers(0, 30, M)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    sid = rng.integers(0, S, off[-1]).astype(np.int32)
    rows = [(m, s, *_rand_row(rng)) for m in range(M) for s in range(S) if rng.random() < 0.03]
    t = pair_ref.make_table(rows, M, S)
    glob = _dense(rng, S, 0.5)
    qoff, qsid, emarket, _ = pair_ref.entries(off, sid, S)
    tab, dtab, md = _table(t), _table(dt), _T(np.zeros(M, np.int32))
    dscope = batch.ScopeTable(_T(rel), _T(conf), _T(tus.astype(np.int64)), _T(has))
    seen = set()
    for em, g, decay, cold in itertools.product((True, False), (glob, None), (True, False), (False, True)):
        kw = dict(emarket=_T(emarket) if em else None, global_scope=_scope(g), apply_decay=decay, mark_cold=cold)
        a = batch.pair_resolve(_T(qoff), _T(qsid), tab, NOW, mode="namespaced", domain=dscope, **kw)
        lb, matched, _, dmatched, table, scope = batch.scope_resolve(_T(qoff), _T(qsid), tab, dtab, md, NOW, **kw)
        what = (em, g is None, decay, cold)
        assert table.relconf.cpu().numpy().tobytes() == a.table.relconf.cpu().numpy().tobytes(), what
        assert table.bits.cpu().numpy().tobytes() == a.table.bits.cpu().numpy().tobytes(), what
        assert scope.cpu().numpy().tobytes() == a.scope.cpu().numpy().tobytes(), what
        assert lb.cpu().numpy().tobytes() == a.lb.cpu().numpy().tobytes(), what
        assert matched.cpu().numpy().tobytes() == a.matched.cpu().numpy().tobytes(), what
        assert np.array_equal(dmatched.cpu().numpy(), stored[qsid].astype(np.uint8)), what
        seen |= set(scope.cpu().numpy().tolist())
    assert seen == {0, 1, 2, 3}
    N.check_faults(_dev(), "equivalence")


# ------------------------------------------------------------------------------- rejected inputs
@pytest.fixture(scope="module")
def small():
    """4 markets in domains (0, 1, 2, -1), three sids queried in each; rows at all scopes."""
    rng = np.random.default_rng(8)
    S, D = 12, 3
    dt = pair_ref.make_table([(d, s, *_rand_row(rng)) for d in range(D) for s in (1, 3, 4, 7, 9)], D, S)
    t = pair_ref.make_table([(m, s, *_rand_row(rng)) for m in range(4) for s in (3, 5)], 4, S)
    qoff = np.array([0, 3, 6, 9, 12], np.int64)
    qsid = np.array([1, 3, 8] * 4, np.int32)
    return dict(t=t, dt=dt, md=np.array([0, 1, 2, -1], np.int32), qoff=qoff, qsid=qsid, glob=_dense(rng, S, 0.5), S=S)


@pytest.mark.parametrize("bad", [3, -2])
def test_market_domain_out_of_range_raises_and_reads_as_no_domain(small, bad):
    s = small
    md = s["md"].copy()
    md[1] = bad
    as_none = s["md"].copy()
    as_none[1] = -1
    N.check_faults(_dev(), "clean slate")
    _check_scope_resolve(s["t"], s["dt"], md, s["qoff"], s["qsid"], s["glob"], md_ref=as_none)
    with pytest.raises(N.BCEError, match="offsets"):
        N.check_faults(_dev(), "market_domain")
    N.check_faults(_dev(), "fault word is cleared")


@pytest.mark.parametrize("case", ["decreasing", "beyond"])
def test_bad_domain_offsets_raise_and_search_as_empty(small, case):
    s = small
    dt = dict(s["dt"])
    R = len(dt["psid"])
    assert dt["poffsets"].tolist() == [0, 5, 10, 15] and R == 15
    # decreasing: domain 1 = [5, 4) is no segment; domain 2 = [4, 15) is one, but not of its own rows.
    # beyond: domain 1 = [5, R + 6) and domain 2 = [R + 6, R) are no segments.
    dt["poffsets"] = np.array([0, 5, 4, 15] if case == "decreasing" else [0, 5, R + 6, R], np.int64)
    emarket = _emarket(s["qoff"])
    empty = [1] if case == "decreasing" else [1, 2]  # the markets whose domain is searched as empty
    N.check_faults(_dev(), "clean slate")
    # the entries not concerned (domain 0, and the market without a domain): every output
    _check_scope_resolve(s["t"], dt, s["md"], s["qoff"], s["qsid"], s["glob"], keep=np.isin(emarket, [0, 3]),
                         dt_ref=s["dt"])
    with pytest.raises(N.BCEError, match="offsets"):
        N.check_faults(_dev(), "doffsets")
    N.check_faults(_dev(), "fault word is cleared")
    # the entries of a broken segment resolve as if their domain had no rows
    rows = [r for r in pair_ref.table_rows(s["dt"]) if r[0] == 0]
    rel, conf, scope = domain_ref.resolve(s["qoff"], s["qsid"], s["t"], pair_ref.make_table(rows, 3, s["S"]), s["md"],
                                          NOW, s["glob"])
    _, _, _, dmatched, table, got = batch.scope_resolve(_T(s["qoff"]), _T(s["qsid"]), _table(s["t"]), _table(dt),
                                                        _T(s["md"]), NOW, global_scope=_scope(s["glob"]))
    sel = np.isin(emarket, empty)
    rc = table.relconf.cpu().numpy()[:len(sel)]
    assert rc[sel, 0].tobytes() == rel[sel].tobytes() and rc[sel, 1].tobytes() == conf[sel].tobytes()
    assert np.array_equal(got.cpu().numpy()[sel], scope[sel]) and not (scope[sel] == 1).any()
    assert not dmatched.cpu().numpy()[sel].any()
    with pytest.raises(N.BCEError, match="offsets"):
        N.check_faults(_dev(), "doffsets")
    N.check_faults(_dev(), "fault word is cleared")


def test_out_of_range_sid_raises_and_is_clamped(small):
    s = small
    qsid = s["qsid"].copy()
    qsid[2] = s["S"] + 5   # the last entry of market 0: still ascending
    qsid[3] = -3           # the first entry of market 1
    keep = np.ones(len(qsid), bool)
    keep[[2, 3]] = False
    N.check_faults(_dev(), "clean slate")
    _check_scope_resolve(s["t"], s["dt"], s["md"], s["qoff"], qsid, s["glob"], keep=keep)
    with pytest.raises(N.BCEError, match="sid"):
        N.check_faults(_dev(), "scope_resolve")
    # clamped: the two entries read sid S - 1 and sid 0
    clamped = np.clip(qsid, 0, s["S"] - 1)
    rel, conf, scope = domain_ref.resolve(s["qoff"], clamped, s["t"], s["dt"], s["md"], NOW, s["glob"])
    got = batch.scope_resolve(_T(s["qoff"]), _T(qsid), _table(s["t"]), _table(s["dt"]), _T(s["md"]), NOW,
                              global_scope=_scope(s["glob"]))
    assert got[4].relconf.cpu().numpy()[:12, 0].tobytes() == rel.tobytes()
    assert np.array_equal(got[5].cpu().numpy(), scope)
    with pytest.raises(N.BCEError, match="sid"):
        N.check_faults(_dev(), "scope_resolve")
    N.check_faults(_dev(), "fault word is cleared")


# ------------------------------------------------------------------------------ consensus_pairs
@pytest.fixture(scope="module")
def cbatch():
    """300 ragged markets of 0..40 signals over S = 97 sources (duplicates in the long ones), 5
    domains and some markets without one; half of the rows present at every scope."""
    rng = np.random.default_rng(78)
    M, S, D = 300, 97, 5
    lens = rng.integers(0, 41, M)
    lens[:4] = (0, 40, 1, 0)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    sid = rng.integers(0, S, off[-1]).astype(np.int32)
    sid[off[1]:off[1] + 20] = sid[off[1] + 20:off[1] + 40]  # market 1: every source twice
    prob = rng.random(off[-1])
    md = rng.integers(-1, D, M).astype(np.int32)
    uoff, usid, emarket, _ = pair_ref.entries(off, sid, S)
    rows = [(int(m), int(s), *_rand_row(rng)) for m, s in zip(emarket, usid) if rng.random() < 0.5]
    drows = [(d, s, *_rand_row(rng)) for d in range(D) for s in range(S) if rng.random() < 0.5]
    return dict(off=off, sid=sid, prob=prob, S=S, md=md, t=pair_ref.make_table(rows, M, S),
                dt=pair_ref.make_table(drows, D, S), glob=_dense(rng, S, 0.5))


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
def test_consensus_pairs_with_domains_matches_the_helper(cbatch, route):
    c = cbatch
    tab, dtab, md = _table(c["t"]), _table(c["dt"]), _T(c["md"])
    off, sid, prob = _T(c["off"]), _T(c["sid"]), _T(c["prob"])
    kw = {"planned": {}, "max_len": {"max_len": 40}, "bins": {"bins": batch.Plan.build(c["off"], _dev())}}[route]
    plan = batch.PairPlan.build(off, sid, prob, c["S"])
    assert len(set(c["md"].tolist())) == 6 and int(np.diff(c["off"]).max()) == 40
    for cold in (False, True):
        exp, uoff, usid, scope = domain_ref.consensus(c["off"], c["sid"], c["prob"], c["t"], c["dt"], c["md"], NOW,
                                                      c["glob"], mark_cold=cold)
        assert set(scope.tolist()) == {0, 1, 2, 3}
        dlb, dmatched, _ = domain_ref.lookup_domain(uoff, usid, c["md"], c["dt"])
        for p in (None, plan):
            pc = batch.consensus_pairs(off, sid, prob, tab, NOW, plan=p, namespaced=True, domains=dtab,
                                       market_domain=md, global_scope=_scope(c["glob"]), mark_cold=cold, check=True,
                                       **dict(kw))
            _same_consensus(pc.result, exp, c["off"], (route, cold, p is None))
            assert np.array_equal(pc.scope.cpu().numpy(), scope)
            assert np.array_equal(pc.dlb.cpu().numpy(), dlb) and np.array_equal(pc.dmatched.cpu().numpy(), dmatched)
    # the defaults are today's lookup
    old = batch.consensus_pairs(off, sid, prob, tab, NOW, plan=plan, check=True, **dict(kw))
    assert old.dlb is None and old.dmatched is None
    _same_consensus(old.result, pair_ref.consensus(c["off"], c["sid"], c["prob"], c["t"], NOW)[0], c["off"], route)


# ------------------------------------------------------------------------------- settle_domains
CHAINS = (1, 2, 11, 12, 255, 256, 257, 600)


@pytest.fixture(scope="module")
def sbatch():
    """Chain k is the pair (domain k % 3, source 3 + 4k) with CHAINS[k] signals cut over three
    markets of its domain (even k have the row, odd ones do not).  The markets are interleaved
    with those of the other domains, with markets without a domain and an unresolved one that
    carry the same sources, and with mixed markets over the even sources.  Domain 3 has rows and
    no market."""
    rng = np.random.default_rng(101)
    S, D = 40, 4
    markets, drows = [], []   # (domain, outcome, signals)
    for k, n in enumerate(CHAINS):
        d, s = k % 3, 3 + 4 * k
        cuts = sorted(rng.integers(0, n + 1, 2).tolist())
        for a, b in zip([0] + cuts, cuts + [n]):
            markets.append((d, int(rng.integers(0, 2)), [(s, float(p)) for p in rng.random(b - a)]))
        markets.append((-1, 1, [(s, float(p)) for p in rng.random(3)]))   # no domain: not in the chain
        drows += [(d, s - 1, *_rand_row(rng)), ((d + 1) % 3, s, *_rand_row(rng))]
        if k % 2 == 0:
            drows.append((d, s, *_rand_row(rng)))
    markets.append((0, -1, [(3, 0.9), (7, 0.1), (2, 0.4)]))                # unresolved
    for d in (0, 1, 2, -1):
        markets.append((d, 1, [(int(s) * 2, float(p)) for s, p in zip(rng.integers(0, S // 2, 60), rng.random(60))]))
    markets.append((1, 0, []))
    order = rng.permutation(len(markets))
    markets = [markets[i] for i in order]
    drows += [(3, s, *_rand_row(rng)) for s in range(0, S, 3)]
    drows = list({(d, s): (d, s, *r) for d, s, *r in drows}.values())
    off = np.zeros(len(markets) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for _, _, x in markets])
    sid = np.array([s for _, _, x in markets for s, _ in x], np.int32)
    prob = np.array([p for _, _, x in markets for _, p in x], np.float64)
    return dict(off=off, sid=sid, prob=prob, outcome=np.array([o for _, o, _ in markets], np.int8),
                md=np.array([d for d, _, _ in markets], np.int32), S=S, D=D, dt=pair_ref.make_table(drows, D, S))


def _same_table(got, exp, what):
    for k in ("poffsets", "psid", "rel", "conf", "t_us", "has"):
        assert got[k].dtype == exp[k].dtype, (what, k)
        assert np.array_equal(got[k], exp[k]), (what, k, np.flatnonzero(got[k] != exp[k])[:8])


def test_settle_domains_matches_the_helper(sbatch):
    b = sbatch
    dt = b["dt"]
    off, sid, prob, outcome, md = _T(b["off"]), _T(b["sid"]), _T(b["prob"]), _T(b["outcome"]), _T(b["md"])
    plan = batch.DomainPlan.build(off, sid, md, b["S"], b["D"])
    uoff, usid, edom, esid = domain_ref.domain_entries(b["off"], b["sid"], b["md"], b["S"], b["D"])
    assert np.array_equal(plan.uoffsets.cpu().numpy(), uoff) and np.array_equal(plan.usid.cpu().numpy(), usid)
    assert np.array_equal(plan.emarket.cpu().numpy(), edom) and np.array_equal(plan.esid.cpu().numpy(), esid)
    exp, total, correct = domain_ref.settle(b["off"], b["sid"], b["prob"], b["outcome"], b["md"], dt, NOW)
    chain = {(int(edom[e]), int(usid[e])): int(total[e]) for e in range(len(usid))}
    assert [chain[(k % 3, 3 + 4 * k)] for k in range(len(CHAINS))] == list(CHAINS)
    assert batch.SETTLE_LONG_MIN == 256
    got = {}
    for name, kw in (("default", {}), ("one lane", {"long_min": batch.SETTLE_LONG_OFF})):
        new, splan = batch.settle_domains(plan, _table(dt), off, prob, outcome, NOW, **kw)
        got[name] = _np_table(new)
        _same_table(got[name], exp, name)
        assert np.array_equal(splan.total.cpu().numpy()[:plan.n_entries], total)
        assert np.array_equal(splan.correct.cpu().numpy()[:plan.n_entries], correct)
    for k in got["default"]:
        if isinstance(got["default"][k], np.ndarray):
            assert got["default"][k].tobytes() == got["one lane"][k].tobytes(), k
    new_t = got["default"]
    for d in range(b["D"]):  # sorted and unique inside every domain
        seg = new_t["psid"][new_t["poffsets"][d]:new_t["poffsets"][d + 1]]
        assert (np.diff(seg) > 0).all(), d
    assert len(new_t["psid"]) > len(dt["psid"])  # pairs without a row were inserted
    # rows no signal touched -- domain 3's among them -- bit for bit
    old = {(d, s): r for d, s, *r in pair_ref.table_rows(dt)}
    now = {(d, s): r for d, s, *r in pair_ref.table_rows(new_t)}
    touched = {(int(edom[e]), int(usid[e])) for e in np.flatnonzero(total > 0)}
    assert any(d == 3 for d, _ in old) and not any(d == 3 for d, _ in touched)
    assert any(key not in touched for key in old)
    for key, r in old.items():
        if key not in touched:
            assert now[key] == r, key
    for key in touched:
        assert now[key][2] == NOW and now[key][3] == 1
    # a second batch on the returned table equals the reference's two batches
    outcome2 = np.where(b["outcome"] >= 0, 1 - b["outcome"], 1).astype(np.int8)  # the unresolved market resolves
    exp2, _, _ = domain_ref.settle(b["off"], b["sid"], b["prob"], outcome2, b["md"], exp, NOW + DAY)
    new2, _ = batch.settle_domains(plan, new, off, prob, _T(outcome2), NOW + DAY)
    _same_table(_np_table(new2), exp2, "second batch")
    N.check_faults(_dev(), "settle_domains")


def test_settle_domains_empty_table_and_empty_batch():
    S, D = 5, 2
    off = np.array([0, 3, 3, 5], np.int64)
    sid, prob = np.array([4, 0, 4, 1, 1], np.int32), np.array([0.9, 0.2, 0.4, 0.5, 0.1])
    outcome, md = np.array([1, 0, 1], np.int8), np.array([1, 0, -1], np.int32)
    dt = pair_ref.make_table([], D, S)
    plan = batch.DomainPlan.build(_T(off), _T(sid), _T(md), S, D)
    new, _ = batch.settle_domains(plan, batch.PairTable.empty(D, S, _dev()), _T(off), _T(prob), _T(outcome), NOW)
    exp = domain_ref.settle(off, sid, prob, outcome, md, dt, NOW)[0]
    _same_table(_np_table(new), exp, "empty table")
    assert exp["poffsets"].tolist() == [0, 0, 2]  # the market without a domain wrote nothing
    zero = np.zeros(4, np.int64)
    none = batch.DomainPlan.build(_T(zero), _T(sid[:0]), _T(md), S, D)
    same, _ = batch.settle_domains(none, new, _T(zero), _T(prob[:0]), _T(outcome), NOW)
    _same_table(_np_table(same), _np_table(new), "empty batch")
    nodom = batch.DomainPlan.build(_T(off), _T(sid), _T(np.full(3, -1, np.int32)), S, D)
    same, _ = batch.settle_domains(nodom, new, _T(off), _T(prob), _T(outcome), NOW)
    _same_table(_np_table(same), _np_table(new), "no market has a domain")
    N.check_faults(_dev(), "settle_domains edge")


# ------------------------------------------------------------------------- fixture through stores
def _store_with_fixture(g, path, resolve=False):
    from bayesian_engine.market import MarketId, MarketStore
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore
    ns = NamespacedReliabilityStore(str(path))
    for row in g["seeds"]:
        ns._store._conn.execute("INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) "
                                "VALUES (?, ?, ?, ?, ?)", tuple(row))
    ms = MarketStore()
    for mid, mk in zip(g["market_ids"], g["markets"]):
        market = ms.create_market(MarketId(mid))
        for s, p in mk["signals"]:
            market.add_signal({"sourceId": g["names"][s], "probability": p})
        if resolve and mk["outcome"] is not None:
            market.resolve(mk["outcome"])
    return ns, ms


def _fixture(golden_dir):
    with open(os.path.join(golden_dir, "domain_scope_small.json")) as f:
        return json.load(f)


def test_fixture_consensus_through_the_stores(golden_dir, tmp_path):
    import bayesian_engine.decay as dmod
    g = _fixture(golden_dir)
    ns, ms = _store_with_fixture(g, tmp_path / "consensus.db")
    now = EPOCH + timedelta(microseconds=g["now_us"])

    class _Frozen(datetime):
        @classmethod
        def now(cls, tz=None):
            return now

    old = dmod.datetime
    dmod.datetime = _Frozen
    try:
        by_name = ms.compute_all_consensus(ns, domain_of="category")
        by_call = ms.compute_all_consensus(ns, domain_of=lambda m: m.id.category)
        per_source = {}
        for market in ms.list_markets():
            rel = {}
            for s in market.signals:
                r = ns.get_reliability(s["sourceId"], market_id=str(market.id), domain=market.id.category,
                                       apply_decay=True)
                rel[s["sourceId"]] = {"reliability": r.reliability, "confidence": r.confidence}
            per_source[str(market.id)] = rel
    finally:
        dmod.datetime = old
    assert list(by_name) == list(g["consensus"])
    for k in by_name:
        assert list(by_name[k]) == list(g["consensus"][k])
        assert by_name[k] == by_call[k] == g["consensus"][k], k
    # the per-source API of the same store falls through the same rows
    assert per_source["sports:m1"]["src-4"]["confidence"] == 0.7  # empty market stamp -> the sports row
    assert per_source["crypto:m0"]["src-3"] == {"reliability": 0.66, "confidence": 0.41}  # unparseable: no decay
    ns.close()
    N.check_faults(_dev(), "compute_all_consensus")


@pytest.mark.parametrize("update_global", [True, False])
def test_fixture_settlement_through_the_stores(golden_dir, tmp_path, update_global):
    from bayesian_engine.market import CrossMarketAggregator
    g = _fixture(golden_dir)
    ns, ms = _store_with_fixture(g, tmp_path / "settle.db", resolve=True)
    agg = CrossMarketAggregator(ms)
    dump = lambda: [[r.source_id, r.market_id, r.reliability, r.confidence, r.updated_at]  # noqa: E731
                    for r in ns._store.list_sources()]
    before = dump()
    dry = agg.settle_resolved(ns, domain_of="category", update_global=update_global, dry_run=True)
    assert dump() == before  # dry_run writes nothing
    summary = agg.settle_resolved(ns, domain_of="category", update_global=update_global)
    final = g["final_update_global" if update_global else "final"]
    assert [row[:4] for row in dump()] == final
    assert {k: (r.reliability, r.confidence) for k, r in dry.records.items()} == \
        {k: (r.reliability, r.confidence) for k, r in summary.records.items()}
    rows = {(s, k): (r, c) for s, k, r, c in final}
    assert {d for _, d in summary.records} == {"crypto", "sports", "politics", None}
    for (s, d), rec in summary.records.items():
        key = "__global__" if d is None else f"__domain__:{d}"
        assert (rec.reliability, rec.confidence) == rows[(s, key)], (s, d)
        assert rec.namespace.value == ("global" if d is None else "domain")
    for s, rec in summary.global_records.items():
        assert (rec.reliability, rec.confidence) == rows[(s, "__global__")]
    off, sid, prob, outcome = pair_ref.fixture_batch(g)
    assert sum(summary.total.values()) == int(np.diff(off)[outcome >= 0].sum())
    assert set(summary.total) == set(summary.correct) == set(summary.records)
    # the sources of the market without a domain always reach __global__; the others with update_global only
    _, md = domain_ref.fixture_domains(g)
    direct = {g["names"][s] for m in np.flatnonzero((md < 0) & (outcome >= 0)) for s in sid[off[m]:off[m + 1]]}
    every = {g["names"][s] for m in np.flatnonzero(outcome >= 0) for s in sid[off[m]:off[m + 1]]}
    assert set(summary.global_records) == (every if update_global else direct) and direct < every
    with pytest.raises(ValueError):
        agg.settle_resolved(ns, domain="crypto", domain_of="category")
    ns.close()
    N.check_faults(_dev(), "settle_resolved")
