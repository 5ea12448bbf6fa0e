"""Expected values of the live consensus history (batch.walk_history_live): the
reference run as an event loop at arrival granularity, composed from the CPU oracle one event at a
time (test infrastructure only).

The events are ``(arrival_us[i], m, 0, k)`` for signal k of market m and ``(resolve_time_us[m], m,
1, 0)`` for every resolved market, sorted ascending.  At an arrival the table is read through
``orc.decay_view`` with the clock at the arrival and ``orc.consensus_csr`` scores the one-market CSR
of the market's first k + 1 signals against it; at a resolution the market is settled by
``settle_ref.apply_chains`` on its own slice with ``now = resolve_time_us[m]``.  Nothing here knows
about chains, prefixes or ranks: the order of the events is the whole model."""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc
from settle_ref import apply_chains, chains

FIELDS = ("consensus", "confidence", "total_weight", "n_unique")


def history_live_ref(offsets, sid, prob, outcome, n_sources, rel, conf, t_us, present, arrival_us,
                     resolve_time_us, half_life=30.0, min_rel=0.10):
    """Returns ``(out, state)``: ``out`` the four per-signal arrays of a HistoryResult (0.0 where
    null), ``state`` the final ``(rel, conf, t_us, present)`` after every event."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    S = int(n_sources)
    sid = np.clip(np.ascontiguousarray(sid, np.int64), 0, S - 1).astype(np.int32)  # as the builder clamps
    prob = np.ascontiguousarray(prob, np.float64)
    outcome = np.ascontiguousarray(outcome, np.int8)
    rel, conf = np.array(rel, np.float64), np.array(conf, np.float64)
    t_us, present = np.array(t_us, np.int64), np.array(present, np.uint8)
    M, Nsig = len(offsets) - 1, len(sid)
    out = dict(consensus=np.zeros(Nsig), confidence=np.zeros(Nsig), total_weight=np.zeros(Nsig),
               n_unique=np.zeros(Nsig, np.int32))
    events = [(int(arrival_us[i]), m, 0, i - int(offsets[m])) for m in range(M)
              for i in range(int(offsets[m]), int(offsets[m + 1]))]
    events += [(int(resolve_time_us[m]), m, 1, 0) for m in range(M) if outcome[m] >= 0]
    seen = np.ones(S, np.uint8)
    for now, m, kind, k in sorted(events):
        a, b = int(offsets[m]), int(offsets[m + 1])
        if kind == 1:
            ch = chains(np.array([0, b - a], np.int64), sid[a:b], prob[a:b], outcome[m:m + 1], S)
            rel, conf, t_us, present = apply_chains(ch, rel, conf, t_us, present, now)
            continue
        view = orc.decay_view(rel, t_us, present, now, half_life, min_rel)  # absent rows read 0.5
        cview = np.where(present != 0, conf, 0.25)
        one = orc.consensus_csr(np.array([0, k + 1], np.int64), sid[a:a + k + 1], prob[a:a + k + 1], view, cview, seen)
        for f in FIELDS:
            out[f][a + k] = one[f][0]
    return out, (rel, conf, t_us, present)


def expand_prefixes(offsets, sid, prob, outcome, arrival_us, resolve_time_us):
    """The batch expanded into its prefixes for the lagged walk (``walk_lag_ref`` / ``walk_forward``
    on ``WalkPlan.build_lagged``), in (arrival, market, position) order so that the forecast times
    ascend: prefix (m, k) is forecast at the arrival of signal k and never resolves, and every
    resolved market is appended ONCE more as a settling market that is forecast and resolved at
    its resolve time.  Returns ``(off, sid, prob, outcome, forecast, resolve, point)`` with
    ``point[i]`` the CSR position of the signal that expanded market i is the history point of (-1
    for a settling market).

    Ties are the live walk's: a prefix of market j sees resolved market m iff (resolve[m], m) <
    (arrival, j).  The lagged walk compares (resolve, index) < (forecast, index) over the expanded
    indices, so the expanded markets are ordered by (time, original market, settling after
    prefixes) -- a settling market's index then compares with a prefix's as the originals do."""
    offsets = np.asarray(offsets, np.int64)
    sid, prob, outcome = np.asarray(sid, np.int32), np.asarray(prob, np.float64), np.asarray(outcome, np.int8)
    M, Nsig = len(offsets) - 1, len(sid)
    lens = np.diff(offsets)
    res = np.flatnonzero(outcome >= 0)
    # the items (time, market, kind, k): every signal, then every resolved market
    market = np.concatenate([np.repeat(np.arange(M), lens), res])
    time = np.concatenate([np.asarray(arrival_us, np.int64), np.asarray(resolve_time_us, np.int64)[res]])
    kind = np.concatenate([np.zeros(Nsig, np.int64), np.ones(len(res), np.int64)])
    k = np.concatenate([np.arange(Nsig) - offsets[:-1][market[:Nsig]], np.zeros(len(res), np.int64)])
    order = np.lexsort((k, kind, market, time))
    market, time, kind, k = market[order], time[order], kind[order], k[order]
    n = np.where(kind == 1, lens[market], k + 1)
    off = np.zeros(len(n) + 1, np.int64)
    off[1:] = np.cumsum(n)
    src = np.repeat(offsets[:-1][market], n) + (np.arange(int(off[-1])) - np.repeat(off[:-1], n))
    return (off, sid[src], prob[src], np.where(kind == 1, outcome[market], -1).astype(np.int8), time,
            np.where(kind == 1, time, 0), np.where(kind == 1, -1, offsets[:-1][market] + k))


def load_fixture(golden_dir):
    """tests/golden/history_live_small.json as ``(g, (offsets, sid, prob, outcome, S), state,
    arrival_us, resolve_us)``; the resolve time of an unresolved market is 0 (it is never read)."""
    import json
    import os

    from bayesian_engine.timeutil import iso_to_us

    g = json.load(open(os.path.join(golden_dir, "history_live_small.json")))
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
    arrival = np.array([t for mk in g["arrival_times_us"] for t in mk], np.int64)
    resolve = np.array([0 if t is None else t for t in g["resolve_times_us"]], np.int64)
    return (g, (np.array(off, np.int64), np.array(sid, np.int32), np.array(prob), np.array(outcome, np.int8), S),
            (rel, conf, t_us, present), arrival, resolve)
