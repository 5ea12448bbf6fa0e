"""Expected values of the namespaced walk-forward: NamespacedReliabilityStore run online, composed
from the CPU oracle one market at a time over a dict of rows (test infrastructure only).

``rows`` maps ``(scope, source rank)`` to ``(rel, conf, t_us, has)``; the scope is ``("m", market
index)``, ``("d", domain index)`` or ``"g"``.  A key that is present is a row that exists; ``has``
is "updated_at is truthy".  For m = 0..M-1: every unique source of the market is gathered at the
three scopes (a missing row has ``has = 0``) and resolved by ``orc.namespace_resolve`` with the
clock at the market's time, ``orc.consensus_csr`` scores the one-market CSR against that, and a
resolved market is then settled by ``settle_ref.apply_chains`` on its own slice, at its domain (or
the global scope without one) and, with ``update_global``, at the global scope as well; settled
rows get ``t_us`` = the market's time and ``has = 1``.  Market rows are never written."""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc
from settle_ref import apply_chains, chains

COLD = np.int32(-2**31)
GLOBAL = "g"


def _gather(rows, scope, srcs):
    n = len(srcs)
    rel, conf = np.full(n, 0.5), np.full(n, 0.25)
    t_us, has = np.full(n, orc.NO_TIMESTAMP, np.int64), np.zeros(n, np.uint8)
    for i, s in enumerate(srcs):
        row = rows.get((scope, int(s)))
        if row is not None:
            rel[i], conf[i], t_us[i], has[i] = row
    return rel, conf, t_us, has


def _settle_scope(rows, scope, sid, prob, outcome, S, now):
    """update_reliability for every signal of one resolved market at one scope."""
    rel, conf = np.full(S, 0.5), np.full(S, 0.25)
    t_us, present = np.full(S, orc.NO_TIMESTAMP, np.int64), np.zeros(S, np.uint8)
    for s in range(S):
        row = rows.get((scope, s))
        if row is not None:
            rel[s], conf[s], t_us[s], present[s] = row[0], row[1], row[2], 1
    ch = chains(np.array([0, len(sid)], np.int64), sid, prob, np.array([outcome], np.int8), S)
    rel, conf, t_us, present = apply_chains(ch, rel, conf, t_us, present, now)
    for s in np.flatnonzero(ch.total > 0):
        assert t_us[s] == now and present[s] == 1
        rows[(scope, int(s))] = (float(rel[s]), float(conf[s]), int(now), 1)


def walk_scope_ref(offsets, sid, prob, outcome, market_domain, n_sources, rows, market_time_us,
                   update_global=False, mark_cold=False, market_scope=True, global_scope=True):
    """Returns ``(out, rows)``: ``out`` the consensus_csr fields over the whole batch (per market
    and per signal slot; ``usid`` holds the SOURCE rank | cold << 31) plus, per slot, ``scope``
    (0 market / 1 domain / 2 global / 3 cold start) and ``rel_read`` / ``conf_read``; ``rows`` the
    final rows (a copy; the argument is left alone)."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    S = int(n_sources)
    sid = np.clip(np.ascontiguousarray(sid, np.int64), 0, S - 1).astype(np.int32)  # as the builder clamps
    prob = np.ascontiguousarray(prob, np.float64)
    outcome = np.ascontiguousarray(outcome, np.int8)
    rows = dict(rows)
    M, Nsig = len(offsets) - 1, len(sid)
    out = dict(consensus=np.zeros(M), confidence=np.zeros(M), total_weight=np.zeros(M),
               n_unique=np.zeros(M, np.int32), err_idx=np.zeros(M, np.int32), usid=np.full(Nsig, -1, np.int32),
               weight=np.zeros(Nsig), nweight=np.zeros(Nsig), scope=np.full(Nsig, 255, np.uint8),
               rel_read=np.zeros(Nsig), conf_read=np.zeros(Nsig))
    for m in range(M):
        a, b = int(offsets[m]), int(offsets[m + 1])
        now, d = int(market_time_us[m]), int(market_domain[m])
        srcs = np.unique(sid[a:b])
        if len(srcs):
            scopes = [_gather(rows, ("m", m), srcs) if market_scope else None,
                      _gather(rows, ("d", d), srcs) if d >= 0 else None,
                      _gather(rows, GLOBAL, srcs) if global_scope else None]
            if all(x is None for x in scopes):  # nothing to fall back through: every source is cold
                rel, conf, scope = np.full(len(srcs), 0.5), np.full(len(srcs), 0.25), np.full(len(srcs), 3, np.uint8)
            else:
                rel, conf, scope = orc.namespace_resolve(scopes, True, now)
            seen = (scope != 3).astype(np.uint8) if mark_cold else np.ones(len(srcs), np.uint8)
            local = np.searchsorted(srcs, sid[a:b]).astype(np.int32)
            one = orc.consensus_csr(np.array([0, b - a], np.int64), local, prob[a:b], rel, conf, seen)
        else:
            one = orc.consensus_csr(np.array([0, 0], np.int64), np.zeros(0, np.int32), np.zeros(0), np.full(1, 0.5),
                                    np.full(1, 0.25), np.ones(1, np.uint8))
        for k in ("consensus", "confidence", "total_weight", "n_unique", "err_idx"):
            out[k][m] = one[k][0]
        nu = int(one["n_unique"][0])
        assert nu == len(srcs)
        for k in ("weight", "nweight"):
            out[k][a:b] = one[k]
        if nu:
            lr = one["usid"][:nu] & ~COLD
            out["usid"][a:a + nu] = srcs[lr].astype(np.int32) | (one["usid"][:nu] & COLD)
            out["scope"][a:a + nu] = scope[lr]
            out["rel_read"][a:a + nu] = rel[lr]
            out["conf_read"][a:a + nu] = conf[lr]
        if outcome[m] >= 0 and b > a:
            target = ("d", d) if d >= 0 else GLOBAL
            _settle_scope(rows, target, sid[a:b], prob[a:b], outcome[m], S, now)
            if update_global and target != GLOBAL:
                _settle_scope(rows, GLOBAL, sid[a:b], prob[a:b], outcome[m], S, now)
    return out, rows


# ------------------------------------------------------------------ the golden fixture as arrays
def fixture_batch(g):
    """(offsets, sid, prob, outcome, market_domain, domain names, S) of walk_namespaced_small.json."""
    off, sid, prob, outcome = [0], [], [], []
    for mk in g["markets"]:
        for s, p in mk["signals"]:
            sid.append(s)
            prob.append(float(p))
        off.append(len(sid))
        outcome.append(-1 if mk["outcome"] is None else int(mk["outcome"]))
    dnames = list(dict.fromkeys(d for d in g["domains"] if d))
    md = np.array([dnames.index(d) if d else -1 for d in g["domains"]], np.int32)
    return (np.array(off, np.int64), np.array(sid, np.int32), np.array(prob), np.array(outcome, np.int8), md,
            dnames, len(g["names"]))


def fixture_rows(g, iso_to_us):
    """The seeded rows of the fixture keyed as :func:`walk_scope_ref` keys them."""
    dnames = list(dict.fromkeys(d for d in g["domains"] if d))
    rows = {}
    for name, key, r, c, ts in g["seeds"]:
        s = g["names"].index(name)
        if key == "__global__":
            scope = GLOBAL
        elif key.startswith("__domain__:"):
            scope = ("d", dnames.index(key[len("__domain__:"):]))
        else:
            scope = ("m", g["market_ids"].index(key))
        rows[(scope, s)] = (float(r), float(c), int(iso_to_us(ts)), 1 if ts else 0)
    return rows


def scope_key(g, scope):
    """The store key of a ref scope of the fixture."""
    dnames = list(dict.fromkeys(d for d in g["domains"] if d))
    if scope == GLOBAL:
        return "__global__"
    return f"__domain__:{dnames[scope[1]]}" if scope[0] == "d" else g["market_ids"][scope[1]]
