"""Expected values of the namespaced walk-forward with resolution lag: NamespacedReliabilityStore
run as an event loop, composed from the CPU oracle one event at a time over the dict of rows of
tests/walk_scope_ref.py (test infrastructure only).

The events are ``F_m = (forecast_time_us[m], m, 0)`` for every market and ``R_m =
(resolve_time_us[m], m, 1)`` for every resolved one, sorted ascending.  At ``F_m`` every unique
source of the market is gathered at the three scopes as the rows stand AT THAT EVENT and resolved
by ``orc.namespace_resolve`` with the clock at the forecast time; ``orc.consensus_csr`` scores the
one-market CSR against that.  At ``R_m`` the market is settled by ``_settle_scope`` on its own
slice with ``now = resolve_time_us[m]``, at its domain (or the global scope without one) and, with
``update_global``, at the global scope as well.  Market rows are never written.  Nothing here
knows about chains, prefixes or ranks: the order of the events is the whole model."""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import oracle as orc
from walk_scope_ref import COLD, GLOBAL, _gather, _settle_scope


def walk_scope_lag_ref(offsets, sid, prob, outcome, market_domain, n_sources, rows, forecast_time_us,
                       resolve_time_us, update_global=False, mark_cold=False, market_scope=True, global_scope=True):
    """Returns ``(out, rows)`` as ``walk_scope_ref.walk_scope_ref`` does: ``out`` the consensus_csr
    fields over the whole batch plus, per slot, ``scope`` / ``rel_read`` / ``conf_read``; ``rows``
    the rows after every event (a copy; the argument is left alone)."""
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
    events = [(int(forecast_time_us[m]), m, 0) for m in range(M)]
    events += [(int(resolve_time_us[m]), m, 1) for m in range(M) if outcome[m] >= 0]
    for now, m, kind in sorted(events):
        a, b = int(offsets[m]), int(offsets[m + 1])
        d = int(market_domain[m])
        if kind == 1:
            if b > a:
                target = ("d", d) if d >= 0 else GLOBAL
                _settle_scope(rows, target, sid[a:b], prob[a:b], outcome[m], S, now)
                if update_global and target != GLOBAL:
                    _settle_scope(rows, GLOBAL, sid[a:b], prob[a:b], outcome[m], S, now)
            continue
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
    return out, rows


def load_fixture(golden_dir):
    """tests/golden/walk_scope_lag_small.json as ``(g, (offsets, sid, prob, outcome, market_domain, D,
    S), rows, forecast_us, resolve_us)``; the resolve time of an unresolved market is 0 (it is never
    read).  ``g`` has the keys ``walk_scope_ref.fixture_batch`` / ``fixture_rows`` read."""
    from bayesian_engine.timeutil import iso_to_us
    from walk_scope_ref import fixture_batch, fixture_rows

    g = json.load(open(os.path.join(golden_dir, "walk_scope_lag_small.json")))
    off, sid, prob, outcome, md, dnames, S = fixture_batch(g)
    forecast = np.array(g["forecast_times_us"], np.int64)
    resolve = np.array([0 if t is None else t for t in g["resolve_times_us"]], np.int64)
    return g, (off, sid, prob, outcome, md, len(dnames), S), fixture_rows(g, iso_to_us), forecast, resolve
