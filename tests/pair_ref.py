"""Expected values of the market-scope pair table (test infrastructure only).

A table is a dict of numpy arrays ``poffsets, psid, rel, conf, t_us, has`` plus ``n_markets`` and
``n_sources`` (the layout of ``batch.PairTable``).  The per-entry lookup is a host dict keyed by
(market, sid); fallback and decay go through ``oracle.namespace_resolve`` on the gathered rows,
consensus through ``oracle.consensus_csr`` with entry ranks, settlement through
``settle_ref.settle_ref`` over the entry space followed by a Python merge."""
from __future__ import annotations

import numpy as np

from bayesian_engine.timeutil import NO_TIMESTAMP, iso_to_us
from oracle import oracle as orc
from settle_ref import settle_ref

NOTS = orc.NO_TIMESTAMP


def make_table(rows, n_markets, n_sources):
    """rows: iterable of (market, sid, rel, conf, t_us, has) in any order, unique pairs."""
    rows = sorted(rows, key=lambda r: (r[0], r[1]))
    assert len({(r[0], r[1]) for r in rows}) == len(rows)
    col = lambda k, dt: np.array([r[k] for r in rows], dt)  # noqa: E731
    poffsets = np.zeros(n_markets + 1, np.int64)
    poffsets[1:] = np.cumsum(np.bincount(col(0, np.int64), minlength=n_markets))
    return dict(poffsets=poffsets, psid=col(1, np.int32), rel=col(2, np.float64), conf=col(3, np.float64),
                t_us=col(4, np.int64), has=col(5, np.uint8), n_markets=n_markets, n_sources=n_sources)


def table_rows(t):
    market = np.repeat(np.arange(t["n_markets"]), np.diff(t["poffsets"]))
    return [(int(m), int(s), float(r), float(c), int(ts), int(h))
            for m, s, r, c, ts, h in zip(market, t["psid"], t["rel"], t["conf"], t["t_us"], t["has"])]


def entries(offsets, sid, n_sources):
    """The unique (market, sid) pairs of a CSR batch in (market, sid) order:
    (uoffsets, usid, emarket, esid)."""
    offsets = np.asarray(offsets, np.int64)
    M = len(offsets) - 1
    market = np.repeat(np.arange(M, dtype=np.int64), np.diff(offsets))
    key = market * int(n_sources) + np.asarray(sid, np.int64)
    ukey, esid = np.unique(key, return_inverse=True)
    emarket = ukey // int(n_sources)
    uoffsets = np.zeros(M + 1, np.int64)
    uoffsets[1:] = np.cumsum(np.bincount(emarket, minlength=M))
    return uoffsets, (ukey % int(n_sources)).astype(np.int32), emarket.astype(np.int32), esid.astype(np.int32)


def lookup(qoffsets, qsid, t):
    """(lb, matched, row) per entry: the lower bound inside the market's segment (global row
    index), whether it is the entry's pair, and the row index from the host dict (-1: none)."""
    where = {(m, s): i for i, (m, s, *_) in enumerate(table_rows(t))}
    Q = len(qsid)
    lb, matched, row = np.zeros(Q, np.int64), np.zeros(Q, np.uint8), np.full(Q, -1, np.int64)
    for m in range(len(qoffsets) - 1):
        p0, p1 = int(t["poffsets"][m]), int(t["poffsets"][m + 1])
        for e in range(int(qoffsets[m]), int(qoffsets[m + 1])):
            s = int(qsid[e])
            lb[e] = p0 + np.searchsorted(t["psid"][p0:p1], s, side="left")
            row[e] = where.get((m, s), -1)
            matched[e] = row[e] >= 0
            assert not matched[e] or row[e] == lb[e]
    return lb, matched, row


def _gather(t, row):
    at = np.maximum(row, 0)
    pick = lambda a, fill: np.where(row >= 0, a[at], fill) if len(a) else np.full(len(row), fill)  # noqa: E731
    return (pick(t["rel"], 0.5).astype(np.float64), pick(t["conf"], 0.25).astype(np.float64),
            pick(t["t_us"], NOTS).astype(np.int64), pick(t["has"], 0).astype(np.uint8))


def resolve(mode, qoffsets, qsid, t, now_us, domain=None, glob=None, apply_decay=True):
    """mode "store" / "namespaced": (rel, conf, scope); "raw": (rel, conf, t_us, present).
    ``domain`` / ``glob``: None or dense (rel, conf, t_us, has) over the source ranks."""
    _, matched, row = lookup(qoffsets, qsid, t)
    g_rel, g_conf, g_t, g_has = _gather(t, row)
    if mode == "raw":
        return g_rel, g_conf, g_t, matched
    if len(qsid) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, np.uint8)
    if mode == "store":  # a row that exists is used whatever its updated_at
        return orc.namespace_resolve([(g_rel, g_conf, g_t, matched), None, None], apply_decay, now_us)
    dense = [None if sc is None else tuple(np.asarray(a)[np.asarray(qsid, np.int64)] for a in sc)
             for sc in (domain, glob)]
    return orc.namespace_resolve([(g_rel, g_conf, g_t, g_has & matched), *dense], apply_decay, now_us)


def consensus(offsets, sid, prob, t, now_us, namespaced=False, domain=None, glob=None, apply_decay=True,
              mark_cold=False):
    """oracle.consensus_csr over the entry ranks; also returns (uoffsets, usid, scope)."""
    uoffsets, usid, _, esid = entries(offsets, sid, t["n_sources"])
    rel, conf, scope = resolve("namespaced" if namespaced else "store", uoffsets, usid, t, now_us, domain, glob,
                               apply_decay)
    present = (scope != 3).astype(np.uint8) if mark_cold else np.ones(len(usid), np.uint8)
    if len(usid) == 0:
        rel, conf, present = np.full(1, 0.5), np.full(1, 0.25), np.zeros(1, np.uint8)
    return orc.consensus_csr(offsets, esid, prob, rel, conf, present), uoffsets, usid, scope


def settle(offsets, sid, prob, outcome, t, now_us):
    """The table after update_reliability(sid, correct, market_id=m) per signal of every market
    with outcome >= 0; also (total, correct) per entry."""
    uoffsets, usid, emarket, esid = entries(offsets, sid, t["n_sources"])
    E = len(usid)
    if E == 0:
        return t, np.zeros(0, np.int64), np.zeros(0, np.int64)
    rel, conf, t_us, present = resolve("raw", uoffsets, usid, t, now_us)
    rel, conf, t_us, present, total, correct = settle_ref(offsets, esid, prob, outcome, E, rel, conf, t_us, present,
                                                         now_us)
    rows = {(m, s): (m, s, r, c, ts, h) for m, s, r, c, ts, h in table_rows(t)}
    for e in np.flatnonzero(total > 0):
        m, s = int(emarket[e]), int(usid[e])
        assert t_us[e] == now_us and present[e] == 1
        rows[(m, s)] = (m, s, float(rel[e]), float(conf[e]), int(now_us), 1)
    return make_table(rows.values(), t["n_markets"], t["n_sources"]), total, correct


# ------------------------------------------------------------------ the golden fixture as arrays
def fixture_batch(g):
    """(offsets, sid, prob, outcome) of the fixture's markets, ranks over g["names"]."""
    offsets, sid, prob, outcome = [0], [], [], []
    for mk in g["markets"]:
        for s, p in mk["signals"]:
            sid.append(s)
            prob.append(p)
        offsets.append(len(sid))
        outcome.append(-1 if mk["outcome"] is None else int(mk["outcome"]))
    return (np.array(offsets, np.int64), np.array(sid, np.int32), np.array(prob, np.float64),
            np.array(outcome, np.int8))


def fixture_table(g, key=None):
    """The seeded market-scope rows as a pair_ref table, or the dense scope of one key."""
    names, mids = g["names"], g["market_ids"]
    if key is None:
        rows = [(mids.index(m), names.index(s), r, c, iso_to_us(ts), 1 if ts else 0)
                for s, m, r, c, ts in g["seeds"] if m in mids]
        return make_table(rows, len(mids), len(names))
    S = len(names)
    rel, conf, t, has = np.full(S, 0.5), np.full(S, 0.25), np.full(S, NO_TIMESTAMP, np.int64), np.zeros(S, np.uint8)
    for s, m, r, c, ts in g["seeds"]:
        if m == key:
            i = names.index(s)
            rel[i], conf[i], t[i], has[i] = r, c, iso_to_us(ts), 1 if ts else 0
    return rel, conf, t, has
