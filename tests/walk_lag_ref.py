"""Expected values of walk-forward consensus with resolution lag: the reference run as an event
loop, composed from the CPU oracle one event at a time (test infrastructure only).

The events are ``F_m = (forecast_time_us[m], m, 0)`` for every market and ``R_m =
(resolve_time_us[m], m, 1)`` for every resolved one, sorted ascending.  At ``F_m`` the table is
read through ``orc.decay_view`` with the clock at the forecast time and ``orc.consensus_csr``
scores the one-market CSR against it; at ``R_m`` the market is settled by
``settle_ref.apply_chains`` on its own slice with ``now = resolve_time_us[m]``
(update_reliability per signal, in position order).  Nothing here knows about chains, prefixes or
ranks: the order of the events is the whole model."""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc
from settle_ref import apply_chains, chains

COLD = np.int32(-2**31)


def walk_lag_ref(offsets, sid, prob, outcome, n_sources, rel, conf, t_us, present, forecast_time_us,
                 resolve_time_us, all_present=True):
    """Returns ``(out, state)`` as ``walk_ref.walk_ref`` does: ``out`` the consensus_csr fields
    over the whole batch plus ``exists`` / ``rel_read`` / ``conf_read`` per slot, ``state`` the
    final ``(rel, conf, t_us, present)`` after every event."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    S = int(n_sources)
    sid = np.clip(np.ascontiguousarray(sid, np.int64), 0, S - 1).astype(np.int32)  # as the builder clamps
    prob = np.ascontiguousarray(prob, np.float64)
    outcome = np.ascontiguousarray(outcome, np.int8)
    rel, conf = np.array(rel, np.float64), np.array(conf, np.float64)
    t_us, present = np.array(t_us, np.int64), np.array(present, np.uint8)
    M, Nsig = len(offsets) - 1, len(sid)
    out = dict(consensus=np.zeros(M), confidence=np.zeros(M), total_weight=np.zeros(M),
               n_unique=np.zeros(M, np.int32), err_idx=np.zeros(M, np.int32), usid=np.full(Nsig, -1, np.int32),
               weight=np.zeros(Nsig), nweight=np.zeros(Nsig), exists=np.zeros(Nsig, np.uint8),
               rel_read=np.zeros(Nsig), conf_read=np.zeros(Nsig))
    events = [(int(forecast_time_us[m]), m, 0) for m in range(M)]
    events += [(int(resolve_time_us[m]), m, 1) for m in range(M) if outcome[m] >= 0]
    for now, m, kind in sorted(events):
        a, b = int(offsets[m]), int(offsets[m + 1])
        if kind == 1:
            ch = chains(np.array([0, b - a], np.int64), sid[a:b], prob[a:b], outcome[m:m + 1], S)
            rel, conf, t_us, present = apply_chains(ch, rel, conf, t_us, present, now)
            continue
        view = orc.decay_view(rel, t_us, present, now)            # absent rows read 0.5
        cview = np.where(present != 0, conf, 0.25)
        seen = np.ones(S, np.uint8) if all_present else present
        one = orc.consensus_csr(np.array([0, b - a], np.int64), sid[a:b], prob[a:b], view, cview, seen)
        for k in ("consensus", "confidence", "total_weight", "n_unique", "err_idx"):
            out[k][m] = one[k][0]
        for k in ("usid", "weight", "nweight"):
            out[k][a:b] = one[k]
        nu = int(one["n_unique"][0])
        src = one["usid"][:nu] & ~COLD
        out["exists"][a:a + nu] = present[src]
        out["rel_read"][a:a + nu] = view[src]
        out["conf_read"][a:a + nu] = cview[src]
    return out, (rel, conf, t_us, present)


def load_fixture(golden_dir):
    """tests/golden/walk_lag_small.json as ``(g, (offsets, sid, prob, outcome, S), state, forecast_us,
    resolve_us)``; the resolve time of the unresolved market is 0 (it is never read)."""
    import json
    import os

    from bayesian_engine.timeutil import iso_to_us

    g = json.load(open(os.path.join(golden_dir, "walk_lag_small.json")))
    names = g["names"]
    S = len(names)
    off, sid, prob, outcome = [0], [], [], []
    for mk in g["markets"]:
        for s, p in mk["signals"]:
            sid.append(s)
            prob.append(float(p))
        off.append(len(sid))
        outcome.append(-1 if mk["outcome"] is None else int(mk["outcome"]))
    rel, conf = np.full(S, 0.5), np.full(S, 0.25)
    t_us, present = np.full(S, orc.NO_TIMESTAMP, np.int64), np.zeros(S, np.uint8)
    for name, r, c, ts in g["seeds"]:
        s = names.index(name)
        rel[s], conf[s], t_us[s], present[s] = float(r), float(c), iso_to_us(ts), 1
    forecast = np.array(g["forecast_times_us"], np.int64)
    resolve = np.array([0 if t is None else t for t in g["resolve_times_us"]], np.int64)
    return (g, (np.array(off, np.int64), np.array(sid, np.int32), np.array(prob), np.array(outcome, np.int8), S),
            (rel, conf, t_us, present), forecast, resolve)
