"""Expected values of the per-market domain scope (test infrastructure only).

The domain rows are a ``pair_ref`` table whose "market" index is the domain index (the layout of
``batch.PairTable`` with ``n_markets = D``); ``market_domain`` int32[M] names the domain of every
market, -1 = none.  Per entry the market row comes from ``pair_ref.lookup``, the domain row from
a host dict keyed (domain, sid), the global row from the dense arrays; fallback and decay go
through ``oracle.namespace_resolve`` on the gathered rows, consensus through
``oracle.consensus_csr`` with entry ranks, settlement through ``settle_ref.settle_ref`` over the
(domain, sid) entry space followed by a Python merge."""
from __future__ import annotations

import numpy as np

import pair_ref
from bayesian_engine.timeutil import iso_to_us
from oracle import oracle as orc
from pair_ref import _gather, make_table, table_rows
from settle_ref import settle_ref

GLOBAL = "__global__"


def entry_markets(qoffsets):
    return np.repeat(np.arange(len(qoffsets) - 1, dtype=np.int64), np.diff(np.asarray(qoffsets, np.int64)))


def lookup_domain(qoffsets, qsid, market_domain, dt):
    """(dlb, dmatched, drow) per entry: the lower bound inside the segment of the market's domain
    (a row index of the domain table; 0 without a domain), whether it is the entry's (domain,
    sid), and the row index from the host dict (-1: none)."""
    where = {(d, s): i for i, (d, s, *_) in enumerate(table_rows(dt))}
    Q = len(qsid)
    dlb, dmatched, drow = np.zeros(Q, np.int64), np.zeros(Q, np.uint8), np.full(Q, -1, np.int64)
    for e, m in enumerate(entry_markets(qoffsets)):
        d, s = int(market_domain[m]), int(qsid[e])
        if d < 0:
            continue
        d0, d1 = int(dt["poffsets"][d]), int(dt["poffsets"][d + 1])
        dlb[e] = d0 + np.searchsorted(dt["psid"][d0:d1], s, side="left")
        drow[e] = where.get((d, s), -1)
        dmatched[e] = drow[e] >= 0
        assert not dmatched[e] or drow[e] == dlb[e]
    return dlb, dmatched, drow


def resolve(qoffsets, qsid, t, dt, market_domain, now_us, glob=None, apply_decay=True):
    """(rel, conf, scope) per entry; ``t`` None = no market scope, ``glob`` None or dense
    (rel, conf, t_us, has) over the source ranks."""
    Q = len(qsid)
    if Q == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, np.uint8)
    scopes = [None, None, None]
    if t is not None:
        _, matched, row = pair_ref.lookup(qoffsets, qsid, t)
        g_rel, g_conf, g_t, g_has = _gather(t, row)
        scopes[0] = (g_rel, g_conf, g_t, g_has & matched)
    _, dmatched, drow = lookup_domain(qoffsets, qsid, market_domain, dt)
    d_rel, d_conf, d_t, d_has = _gather(dt, drow)
    scopes[1] = (d_rel, d_conf, d_t, d_has & dmatched)
    if glob is not None:
        scopes[2] = tuple(np.asarray(a)[np.asarray(qsid, np.int64)] for a in glob)
    return orc.namespace_resolve(scopes, apply_decay, now_us)


def present_words(scope, mark_cold):
    """The present-bit words of a lookup: bit e % 32 of word e // 32."""
    Q = len(scope)
    on = (np.asarray(scope) != 3) if mark_cold else np.ones(Q, bool)
    words = np.zeros(max((Q + 31) // 32, 1), np.uint32)
    for e in np.flatnonzero(on):
        words[e >> 5] |= np.uint32(1) << np.uint32(e & 31)
    return words


def consensus(offsets, sid, prob, t, dt, market_domain, now_us, glob=None, apply_decay=True, mark_cold=False):
    """oracle.consensus_csr over the entry ranks; also returns (uoffsets, usid, scope)."""
    uoffsets, usid, _, esid = pair_ref.entries(offsets, sid, dt["n_sources"])
    rel, conf, scope = resolve(uoffsets, usid, t, dt, market_domain, now_us, glob, apply_decay)
    present = (scope != 3).astype(np.uint8) if mark_cold else np.ones(len(usid), np.uint8)
    if len(usid) == 0:
        rel, conf, present = np.full(1, 0.5), np.full(1, 0.25), np.zeros(1, np.uint8)
    return orc.consensus_csr(offsets, esid, prob, rel, conf, present), uoffsets, usid, scope


def domain_entries(offsets, sid, market_domain, n_sources, n_domains):
    """The unique (domain, sid) pairs over the signals of markets with a domain, in (domain, sid)
    order: (uoffsets[D + 1], usid, edomain, esid); esid is 0 for the other signals."""
    offsets = np.asarray(offsets, np.int64)
    dom = np.repeat(np.asarray(market_domain, np.int64), np.diff(offsets))
    live = np.flatnonzero(dom >= 0)
    key = dom[live] * int(n_sources) + np.asarray(sid, np.int64)[live]
    ukey, inv = np.unique(key, return_inverse=True)
    edom = ukey // int(n_sources)
    uoffsets = np.zeros(int(n_domains) + 1, np.int64)
    uoffsets[1:] = np.cumsum(np.bincount(edom, minlength=int(n_domains)))
    esid = np.zeros(len(dom), np.int32)
    esid[live] = inv
    return uoffsets, (ukey % int(n_sources)).astype(np.int32), edom.astype(np.int32), esid


def settle(offsets, sid, prob, outcome, market_domain, dt, now_us):
    """The domain table after update_reliability(sid, correct, domain=domain_of(m)) per signal of
    every market with outcome >= 0 and a domain; also (total, correct) per (domain, sid) entry."""
    D = dt["n_markets"]
    uoffsets, usid, edom, esid = domain_entries(offsets, sid, market_domain, dt["n_sources"], D)
    F = len(usid)
    if F == 0:
        return dt, np.zeros(0, np.int64), np.zeros(0, np.int64)
    masked = np.where(np.asarray(market_domain) >= 0, np.asarray(outcome, np.int8), np.int8(-1)).astype(np.int8)
    rel, conf, t_us, present = pair_ref.resolve("raw", uoffsets, usid, dt, now_us)
    rel, conf, t_us, present, total, correct = settle_ref(offsets, esid, prob, masked, F, rel, conf, t_us, present,
                                                         now_us)
    rows = {(d, s): (d, s, r, c, ts, h) for d, s, r, c, ts, h in table_rows(dt)}
    for e in np.flatnonzero(total > 0):
        d, s = int(edom[e]), int(usid[e])
        assert t_us[e] == now_us and present[e] == 1
        rows[(d, s)] = (d, s, float(rel[e]), float(conf[e]), int(now_us), 1)
    return make_table(rows.values(), D, dt["n_sources"]), total, correct


# ------------------------------------------------------------------ the golden fixture as arrays
def fixture_domains(g):
    """(domain names in first-seen order, market_domain int32[M])."""
    names = list(dict.fromkeys(d for d in g["domains"] if d))
    return names, np.array([names.index(d) if d else -1 for d in g["domains"]], np.int32)


def fixture_domain_table(g):
    dnames, _ = fixture_domains(g)
    keys = [f"__domain__:{d}" for d in dnames]
    rows = [(keys.index(k), g["names"].index(s), r, c, iso_to_us(ts), 1 if ts else 0)
            for s, k, r, c, ts in g["seeds"] if k in keys]
    return make_table(rows, len(dnames), len(g["names"]))


def fixture_final(g, update_global):
    """The reference's final rows as {(source_id, key): (rel, conf)}."""
    return {(s, k): (r, c) for s, k, r, c in g["final_update_global" if update_global else "final"]}


def fixture_settle(g, update_global):
    """The final rows through this helper: the domain rows by :func:`settle`, the global rows by
    one settle_ref chain per source (the no-domain markets' signals, or every resolved signal
    with update_global), every other seeded row carried over."""
    offsets, sid, prob, outcome = pair_ref.fixture_batch(g)
    dnames, md = fixture_domains(g)
    now_us, names = g["now_us"], g["names"]
    out = {(s, k): (r, c) for s, k, r, c, _ in g["seeds"]}
    dt, total, _ = settle(offsets, sid, prob, outcome, md, fixture_domain_table(g), now_us)
    _, usid, edom, _ = domain_entries(offsets, sid, md, len(names), len(dnames))
    new = {(d, s): (r, c) for d, s, r, c, *_ in table_rows(dt)}
    for e in np.flatnonzero(total > 0):
        d, s = int(edom[e]), int(usid[e])
        out[(names[s], f"__domain__:{dnames[d]}")] = new[(d, s)]
    gout = outcome if update_global else np.where(md < 0, outcome, np.int8(-1)).astype(np.int8)
    rel, conf, t_us, has = pair_ref.fixture_table(g, key=GLOBAL)
    present = np.array([(n, GLOBAL) in out for n in names], np.uint8)  # a row exists, whatever its stamp
    rel, conf, _, _, gtotal, _ = settle_ref(offsets, sid, prob, gout, len(names), rel, conf, t_us, present, now_us)
    for s in np.flatnonzero(gtotal > 0):
        out[(names[s], GLOBAL)] = (float(rel[s]), float(conf[s]))
    return out
