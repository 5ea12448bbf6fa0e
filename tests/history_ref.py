"""Reference for bce_consensus_history (include/bce.h): plain Python floats.

``history_ref`` is the restatement the kernels follow: sort a market ONCE by (sid, position); for
prefix k walk the sorted elements and skip those with position > k, adding a source's
probabilities in position order; where the sid changes close the run (``avg = s / cnt``, ``total
+= rel``, ``ws += avg * rel``, ``cs += conf * rel``); finish as compute_consensus does (core.py:
131-144).  ``expand`` turns a batch into its prefix markets, so the same points can be computed by
anything that computes a consensus per market (the oracle, ``batch.consensus``).
"""
from __future__ import annotations

import json
import os

import numpy as np

FIELDS = ("consensus", "confidence", "total_weight", "n_unique")


def history_ref(offsets, sid, prob, rel, conf):
    """The four arrays [N] of a history; ``rel`` / ``conf`` are indexed by sid (cold-start
    defaults baked in, as in the engine's source table)."""
    N = len(sid)
    out = dict(consensus=np.zeros(N), confidence=np.zeros(N), total_weight=np.zeros(N),
               n_unique=np.zeros(N, np.int32))
    for m in range(len(offsets) - 1):
        a, b = int(offsets[m]), int(offsets[m + 1])
        order = sorted(range(b - a), key=lambda i: (int(sid[a + i]), i))
        for k in range(b - a):
            total = ws = cs = 0.0
            j = 0
            cur, s, cnt = None, 0.0, 0
            for i in order + [None]:
                src = None if i is None else int(sid[a + i])
                if cur is not None and src != cur and cnt:
                    avg = s / cnt
                    r = float(rel[cur])
                    total += r
                    ws += avg * r
                    cs += float(conf[cur]) * r
                    j += 1
                    s, cnt = 0.0, 0
                cur = src
                if i is not None and i <= k:
                    s += float(prob[a + i])
                    cnt += 1
            null = total == 0.0
            out["consensus"][a + k] = 0.0 if null else ws / total
            out["confidence"][a + k] = 0.0 if null else cs / total
            out["total_weight"][a + k] = total
            out["n_unique"][a + k] = j
    return out


def expand(offsets, sid, prob):
    """The batch of prefix markets: point p of the history (CSR position p) is market p of the
    returned ``(offsets, sid, prob)``, which holds the signals of p's market up to and including p."""
    offsets = np.asarray(offsets, np.int64)
    N = int(offsets[-1])
    lens = np.diff(offsets)
    start = np.repeat(offsets[:-1], lens)          # by point: its market's first signal
    plen = np.arange(N, dtype=np.int64) - start + 1
    off2 = np.zeros(N + 1, np.int64)
    off2[1:] = np.cumsum(plen)
    idx = np.arange(int(off2[-1]), dtype=np.int64) - np.repeat(off2[:-1], plen) + np.repeat(start, plen)
    return off2, np.asarray(sid)[idx], np.asarray(prob)[idx]


def load_fixture(golden_dir):
    """tests/golden/history_small.json as ``(g, offsets, sid, prob, rel, conf, present)`` over the
    ranks of ``g["names"]`` (sorted() order); a source without a row is cold (0.5 / 0.25)."""
    g = json.load(open(os.path.join(golden_dir, "history_small.json")))
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


def fixture_points(g):
    """The recorded points in CSR order: (consensus repr or None, confidence, totalWeight, sourceCount)."""
    return [(p["consensus"], p["confidence"], p["totalWeight"], p["sourceCount"])
            for mk in g["markets"] for p in mk["history"]]
