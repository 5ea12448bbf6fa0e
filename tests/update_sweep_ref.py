"""Expected values of a walk-forward under another update rule: the reference run as an event
loop with ``_BASE_LEARNING_RATE`` / ``MAX_UPDATE_STEP`` as parameters (test infrastructure only).

Reads go through ``orc.decay_view`` and ``orc.consensus_csr`` as in walk_ref.py / walk_lag_ref.py;
the update is restated here from reliability.py:163-173 in plain Python floats, because the
oracle's ``outcome_update`` has the reference's constants compiled in.  Nothing here knows about
chains, steps or pin runs: one signal is one update, in event order."""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc

COLD = np.int32(-2**31)


def update_one(r: float, c: float, correct: bool, rate: float, cap: float):
    """reliability.py:163-173 with the two module constants as arguments."""
    direction = 1.0 if correct else -1.0
    raw_delta = rate * direction
    capped_delta = max(-cap, min(cap, raw_delta))
    new_reliability = max(0.0, min(1.0, r + capped_delta))
    new_confidence = c + (1.0 - c) * 0.10
    new_confidence = min(1.0, new_confidence)
    return new_reliability, new_confidence


def update_sweep_ref(offsets, sid, prob, outcome, n_sources, rel, conf, t_us, present, time_us, rate, cap,
                     resolve_time_us=None, all_present=True):
    """One update point.  Without ``resolve_time_us`` market m is scored and then settled at
    ``time_us[m]``, in market order (walk_ref.py); with it the events ``(time_us[m], m, 0)`` and
    ``(resolve_time_us[m], m, 1)`` run sorted (walk_lag_ref.py).  Returns ``(out, state)`` as those
    do: the consensus_csr fields over the batch plus ``exists`` / ``rel_read`` / ``conf_read`` per
    slot, and the final ``(rel, conf, t_us, present)``."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    S = int(n_sources)
    sid = np.clip(np.ascontiguousarray(sid, np.int64), 0, S - 1).astype(np.int32)  # as the builder clamps
    prob = np.ascontiguousarray(prob, np.float64)
    outcome = np.ascontiguousarray(outcome, np.int8)
    rel, conf = np.array(rel, np.float64), np.array(conf, np.float64)
    t_us, present = np.array(t_us, np.int64), np.array(present, np.uint8)
    rate, cap = float(rate), float(cap)
    M, Nsig = len(offsets) - 1, len(sid)
    out = dict(consensus=np.zeros(M), confidence=np.zeros(M), total_weight=np.zeros(M),
               n_unique=np.zeros(M, np.int32), usid=np.full(Nsig, -1, np.int32), exists=np.zeros(Nsig, np.uint8),
               rel_read=np.zeros(Nsig), conf_read=np.zeros(Nsig))
    if resolve_time_us is None:
        events = [(int(time_us[m]), m, kind) for m in range(M) for kind in ((0, 1) if outcome[m] >= 0 else (0,))]
    else:
        events = sorted([(int(time_us[m]), m, 0) for m in range(M)] +
                        [(int(resolve_time_us[m]), m, 1) for m in range(M) if outcome[m] >= 0])
    for now, m, kind in events:
        a, b = int(offsets[m]), int(offsets[m + 1])
        if kind == 1:
            for i in range(a, b):  # update_reliability per signal, in position order (market.py:298-301)
                s = int(sid[i])
                r, c = (float(rel[s]), float(conf[s])) if present[s] else (0.5, 0.25)  # reliability.py:133-140
                rel[s], conf[s] = update_one(r, c, bool(prob[i] >= 0.5) == bool(outcome[m]), rate, cap)
                t_us[s], present[s] = now, 1
            continue
        view = orc.decay_view(rel, t_us, present, now)            # absent rows read 0.5
        cview = np.where(present != 0, conf, 0.25)
        seen = np.ones(S, np.uint8) if all_present else present
        one = orc.consensus_csr(np.array([0, b - a], np.int64), sid[a:b], prob[a:b], view, cview, seen)
        for k in ("consensus", "confidence", "total_weight", "n_unique"):
            out[k][m] = one[k][0]
        out["usid"][a:b] = one["usid"]
        nu = int(one["n_unique"][0])
        src = one["usid"][:nu] & ~COLD
        out["exists"][a:a + nu] = present[src]
        out["rel_read"][a:a + nu] = view[src]
        out["conf_read"][a:a + nu] = cview[src]
    return out, (rel, conf, t_us, present)


def load_fixture(golden_dir):
    """tests/golden/update_sweep_small.json with the two batches it was recorded over:
    ``(u, walk, lag)`` -- ``walk`` = ``(g, (offsets, sid, prob, outcome, S), state, times_us)`` of
    walk_forward_small.json, ``lag`` = what ``walk_lag_ref.load_fixture`` returns."""
    import json
    import os

    from bayesian_engine.timeutil import iso_to_us
    from walk_lag_ref import load_fixture as load_lag

    u = json.load(open(os.path.join(golden_dir, "update_sweep_small.json")))
    g = json.load(open(os.path.join(golden_dir, u["walk_fixture"])))
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
    walk = (g, (np.array(off, np.int64), np.array(sid, np.int32), np.array(prob), np.array(outcome, np.int8), S),
            (rel, conf, t_us, present), np.array(g["times_us"], np.int64))
    return u, walk, load_lag(golden_dir)


def check_point(point, g, csr, out, state):
    """One recorded update point against ``(out, state)`` computed for it: every market's reads
    and consensus and the store's final rows, ``==`` on every float (through ``repr``)."""
    from bayesian_engine.timeutil import us_to_iso

    off, names = csr[0], g["names"]
    for m, exp in enumerate(point["results"]):
        a, nu = int(off[m]), int(out["n_unique"][m])
        src = out["usid"][a:a + nu] & ~COLD
        got = [[names[int(s)], repr(float(r)), repr(float(c))]
               for s, r, c in zip(src, out["rel_read"][a:a + nu], out["conf_read"][a:a + nu])]
        assert got == exp["read"], (point["learning_rate"], point["max_step"], m, got, exp["read"])
        tw = float(out["total_weight"][m])
        assert repr(tw) == exp["totalWeight"], (m, tw, exp["totalWeight"])
        cons = None if tw == 0 else repr(float(out["consensus"][m]))
        assert cons == exp["consensus"], (m, cons, exp["consensus"])
        assert repr(float(out["confidence"][m])) == exp["confidence"], m
    rel, conf, t_us, present = state
    rows = [[names[s], repr(float(rel[s])), repr(float(conf[s])), us_to_iso(int(t_us[s]))]
            for s in range(len(names)) if present[s]]
    assert sorted(rows) == sorted(point["final"]), (rows, point["final"])
