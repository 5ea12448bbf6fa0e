#!/usr/bin/env python3
"""Generate history_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_history.py

A dozen small markets over 9 sources; for every market and every k the reference's own
``compute_consensus(signals[:k + 1], table)`` (core.py:63-180) is recorded: what a ``Market`` used
online returns after ``add_signal`` number k + 1.  The table has two sources of reliability 0.0,
one of 1.0, and leaves two sources out (cold start: 0.5 / 0.25).  The markets: an empty one, single
signals, repeated sources (a source signalling three times with others in between), an opening of
zero-weight sources only (consensus None until a weighted source arrives), a market of zero-weight
sources alone (None throughout), sources arriving in descending and in ascending order, one source
throughout, probabilities of 1.25 (compute_consensus does not range-check), and two random markets
of 31 and 33 signals.  Floats are stored as ``repr``; the fixture holds data only.
"""
from __future__ import annotations

import json
import os
import random

from bayesian_engine.core import compute_consensus

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [f"src-{i}" for i in range(9)]  # sorted() order == rank order
TABLE = {
    "src-0": {"reliability": 0.9, "confidence": 0.6},
    "src-1": {"reliability": 0.0, "confidence": 0.3},
    "src-2": {"reliability": 0.66, "confidence": 0.41},
    "src-3": {"reliability": 1.0, "confidence": 0.9999},
    "src-5": {"reliability": 0.0, "confidence": 0.8},
    "src-6": {"reliability": 0.37, "confidence": 0.5},
    "src-8": {"reliability": 0.123456789, "confidence": 0.05},
}  # src-4 and src-7 have no row


def make_markets():
    rng = random.Random(20261021)
    rnd = lambda: round(rng.random(), 3)  # noqa: E731
    markets = [
        [],
        [(4, 0.7)],
        [(1, 0.2)],                                              # zero weight alone: None
        [(1, 0.2), (5, 0.9), (1, 0.4), (3, 0.6), (0, 0.1)],      # zero-weight opening
        [(5, 0.3), (1, 0.8), (5, 0.5), (1, 0.1)],                # None throughout
        [(2, 0.1), (7, 0.9), (2, 0.2), (0, 0.5), (2, 0.3), (7, 0.4), (2, 0.6)],
        [(s, rnd()) for s in range(8, -1, -1)],                  # every arrival sorts first
        [(s, rnd()) for s in range(9)],                          # every arrival sorts last
        [(6, rnd()) for _ in range(6)],                          # one source throughout
        [(3, 1.25), (0, 0.4), (3, 0.2), (8, 1.25), (4, 0.0), (0, 1.0)],
        [(rng.randrange(9), rnd()) for _ in range(31)],
        [(rng.randrange(9), rnd()) for _ in range(33)],
    ]
    return markets


def main() -> None:
    doc = {"names": NAMES, "table": {k: {f: repr(v) for f, v in row.items()} for k, row in TABLE.items()},
           "markets": []}
    for sig in make_markets():
        signals = [{"sourceId": NAMES[s], "probability": p} for s, p in sig]
        history = []
        for k in range(len(signals)):
            res = compute_consensus(signals[:k + 1], TABLE)
            history.append({
                "consensus": None if res["consensus"] is None else repr(res["consensus"]),
                "confidence": repr(res["confidence"]),
                "totalWeight": repr(res["normalization"]["totalWeight"]),
                "sourceCount": res["normalization"]["sourceCount"],
            })
        doc["markets"].append({"signals": [[NAMES[s], repr(p)] for s, p in sig], "history": history})
    with open(os.path.join(HERE, "history_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
