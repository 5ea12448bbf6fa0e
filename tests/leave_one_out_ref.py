"""Reference for bce_consensus_leave_one_out (include/bce.h): plain Python floats.

``loo_ref`` follows core.py:103-144 on the reduced signal list of every (market, source): the
sources that are left, in sorted order; per source the probabilities added in arrival order and
divided by their count; ``total += rel``; then the ordered sums ``avg * rel`` and ``conf * rel``
and the two divisions.  ``expand`` turns a batch into one reduced market per signal, so the same
values can be computed by anything that computes a consensus per market (the oracle,
``batch.consensus``).
"""
from __future__ import annotations

import json
import os

import numpy as np

FIELDS = ("consensus", "confidence", "total_weight", "n_unique")


def _consensus(sids, probs, rel, conf):
    """(consensus, confidence, total_weight, n_unique) of one signal list; 0.0 where None."""
    total = 0.0
    data = []
    for s in sorted(set(sids)):  # core.py:103
        mine = [p for x, p in zip(sids, probs) if x == s]  # core.py:115
        avg = sum(mine) / len(mine)  # core.py:116
        w = float(rel[s])
        total += w  # core.py:120
        data.append((avg, float(conf[s]), w))
    if total == 0:  # core.py:131 (an empty list too)
        return 0.0, 0.0, total, len(data)
    ws = sum(avg * w for avg, _, w in data)  # core.py:135-138
    cs = sum(c * w for _, c, w in data)  # core.py:141-144
    return ws / total, cs / total, total, len(data)


def loo_ref(offsets, sid, prob, rel, conf):
    """``(per_signal, full)``: the four arrays [N] of the leave-outs and the four arrays [M] of the
    markets' own consensus; ``rel`` / ``conf`` are indexed by sid (cold-start defaults baked in)."""
    N, M = len(sid), len(offsets) - 1
    new = lambda n: dict(consensus=np.zeros(n), confidence=np.zeros(n), total_weight=np.zeros(n),  # noqa: E731
                         n_unique=np.zeros(n, np.int32))
    out, full = new(N), new(M)
    for m in range(M):
        a, b = int(offsets[m]), int(offsets[m + 1])
        sids = [int(s) for s in sid[a:b]]
        probs = [float(p) for p in prob[a:b]]
        for k, v in zip(FIELDS, _consensus(sids, probs, rel, conf)):
            full[k][m] = v
        done = {}
        for i, x in enumerate(sids):
            if x not in done:
                keep = [q for q, s in enumerate(sids) if s != x]
                done[x] = _consensus([sids[q] for q in keep], [probs[q] for q in keep], rel, conf)
            for k, v in zip(FIELDS, done[x]):
                out[k][a + i] = v
    return out, full


def expand(offsets, sid, prob):
    """The batch of reduced markets: market p of the returned ``(offsets, sid, prob)`` holds the
    signals of p's market whose sid differs from ``sid[p]``, in CSR order."""
    offsets = np.asarray(offsets, np.int64)
    sid, prob = np.asarray(sid), np.asarray(prob)
    N = int(offsets[-1])
    lens = np.zeros(N, np.int64)
    idx = []
    for m in range(len(offsets) - 1):
        a, b = int(offsets[m]), int(offsets[m + 1])
        if a == b:
            continue
        s = sid[a:b]
        keep = s[None, :] != s[:, None]  # row p: the signals that stay when p's source leaves
        lens[a:b] = keep.sum(1)
        idx.append(np.nonzero(keep)[1] + a)
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    off2 = np.zeros(N + 1, np.int64)
    off2[1:] = np.cumsum(lens)
    return off2, sid[idx], prob[idx]


def load_fixture(golden_dir):
    """tests/golden/leave_one_out_small.json as ``(g, offsets, sid, prob, rel, conf, present)`` over
    the ranks of ``g["names"]`` (sorted() order); a source without a row is cold (0.5 / 0.25)."""
    g = json.load(open(os.path.join(golden_dir, "leave_one_out_small.json")))
    names = g["names"]
    S = len(names)
    rel, conf, present = np.full(S, 0.5), np.full(S, 0.25), np.zeros(S, np.uint8)
    for name, row in g["table"].items():
        s = names.index(name)
        rel[s], conf[s], present[s] = float(row["reliability"]), float(row["confidence"]), 1
    off, sid, prob = [0], [], []
    for mk in g["markets"]:
        for name, p in mk["signals"]:
            sid.append(names.index(name))
            prob.append(float(p))
        off.append(len(sid))
    return g, np.array(off, np.int64), np.array(sid, np.int32), np.array(prob, np.float64), rel, conf, present


def fixture_table(g):
    """The fixture's table as the ``source_reliability`` dict compute_consensus takes."""
    return {n: {"reliability": float(r["reliability"]), "confidence": float(r["confidence"])}
            for n, r in g["table"].items()}
