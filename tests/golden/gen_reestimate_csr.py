#!/usr/bin/env python3
"""Generate reestimate_csr_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_reestimate_csr.py

A small ragged batch (12 markets x 8 sources, duplicate signals per source, one empty market,
one market with an out-of-range probability, one market whose only source has weight 0) is
iterated for 4 rounds with the reference's own functions: validate_input_payload and
compute_consensus with ``source_reliability = {sid: {"reliability": w}}`` (core.py:24-179) give
every market's consensus; the count loop of summarize_sources (market.py:293-304, restated
here because its outcome is the consensus vote rather than a resolved market's) and
``correct / total`` (market.py:309-310) give the next weights.  Floats are stored as their
repr, so a comparison is exact.  The fixture holds data only.
"""
from __future__ import annotations

import json
import os
import random

from bayesian_engine.config import SCHEMA_VERSION
from bayesian_engine.core import ValidationError, compute_consensus, validate_input_payload

HERE = os.path.dirname(os.path.abspath(__file__))
ROUNDS = 4
N_SOURCES = 8
NAMES = [f"src-{i}" for i in range(N_SOURCES)]  # sorted() order == rank order


def make_batch():
    rng = random.Random(20260301)
    markets = []
    for m in range(12):
        if m == 3:
            markets.append([])  # the empty market: consensus None
            continue
        if m == 7:
            markets.append([(7, 0.8), (7, 0.3)])  # only the zero-weight source: total weight 0
            continue
        n = rng.randint(1, 9)
        sig = [(rng.randrange(N_SOURCES - 1), round(rng.random(), 3)) for _ in range(n)]
        if m % 3 == 0 and sig:  # duplicates: a source signals again, with another vote
            s, p = sig[0]
            sig.append((s, round(1.0 - p, 3)))
            sig.append((s, rng.random()))
        if m == 5:
            sig[0] = (sig[0][0], 1.5)  # fails validate_input_payload: the market is skipped
        if m == 9:
            sig.append((2, 0.5))  # exactly on the vote threshold
        markets.append(sig)
    return markets


def main() -> None:
    markets = make_batch()
    w = [0.5] * N_SOURCES
    w[7] = 0.0
    w[1] = 0.9
    w_init = list(w)
    payloads = [
        {"schemaVersion": SCHEMA_VERSION, "marketId": f"m-{m}",
         "signals": [{"sourceId": NAMES[s], "probability": p} for s, p in sig]}
        for m, sig in enumerate(markets)
    ]
    rounds = []
    for _ in range(ROUNDS):
        rel = {NAMES[s]: {"reliability": w[s]} for s in range(N_SOURCES)}
        cons, null, outcome = [], [], []
        correct, total = [0] * N_SOURCES, [0] * N_SOURCES
        for payload in payloads:
            c = compute_consensus(payload["signals"], rel)["consensus"]
            try:
                validate_input_payload(payload)
                valid = True
            except ValidationError:
                valid = False
            cons.append(0.0 if c is None else c)
            null.append(int(c is None))
            if c is None or not valid:
                outcome.append(-1)
                continue
            out = c >= 0.5
            outcome.append(int(out))
            for signal in payload["signals"]:  # market.py:283-304
                s = NAMES.index(signal["sourceId"])
                total[s] += 1
                predicted_true = signal.get("probability", 0.5) >= 0.5
                if predicted_true == out:
                    correct[s] += 1
        w = [correct[s] / total[s] if total[s] > 0 else 0.5 for s in range(N_SOURCES)]  # market.py:310
        rounds.append({"cons": [repr(x) for x in cons], "null": null, "outcome": outcome,
                       "correct": correct, "total": total, "w": [repr(x) for x in w]})
    offsets = [0]
    for sig in markets:
        offsets.append(offsets[-1] + len(sig))
    doc = {
        "n_sources": N_SOURCES,
        "offsets": offsets,
        "sid": [s for sig in markets for s, _ in sig],
        "prob": [repr(p) for sig in markets for _, p in sig],
        "w_init": [repr(x) for x in w_init],
        "rounds": rounds,
    }
    with open(os.path.join(HERE, "reestimate_csr_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
