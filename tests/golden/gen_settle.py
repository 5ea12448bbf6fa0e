#!/usr/bin/env python3
"""Generate settle_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_settle.py

12 markets x 8 sources on a temp-file SQLite database: some domain and global rows pre-seeded
(one at reliability 1.0, one at 0.0, one with confidence already 1.0), duplicate signals of one
source in a market, an unresolved market, a probability of exactly 0.5, and one source (src-0)
with 27 signals -- 12 correct, then 15 wrong -- so both clamps are hit.  Every signal of every
resolved market is settled with the reference's own
``NamespacedReliabilityStore.update_reliability(sid, correct, domain="d", update_global=True)``,
``correct = (probability >= 0.5) == outcome`` as summarize_sources reads it (market.py:298-301).
The final (reliability, confidence) of every domain and global row is stored as repr, so a
comparison is exact; updated_at is not stored, only which rows exist.  The fixture holds data only.
"""
from __future__ import annotations

import json
import os
import random
import tempfile

from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

HERE = os.path.dirname(os.path.abspath(__file__))
N_SOURCES = 8
NAMES = [f"src-{i}" for i in range(N_SOURCES)]  # sorted() order == rank order
DOMAIN = "d"
STAMP = "2026-01-01T00:00:00+00:00"
# (scope, source, reliability, confidence)
SEEDS = [
    ("domain", 1, 1.0, 0.6),
    ("domain", 2, 0.0, 0.3),
    ("domain", 3, 0.42, 1.0),
    ("domain", 6, 0.95, 0.9999),
    ("global", 1, 0.0, 0.25),
    ("global", 4, 1.0, 1.0),
    ("global", 5, 0.77, 0.5),
    ("global", 7, 0.31, 0.8),  # src-7 only signals in the unresolved market: the row stays as it is
]


def make_batch():
    rng = random.Random(20261019)
    markets = []
    for m in range(12):
        outcome = None if m == 4 else (rng.random() < 0.5)
        sig = []
        if m <= 3 or 5 <= m <= 9:  # src-0: three signals per market, right in 0..3, wrong in 5..9
            right = m <= 3
            for _ in range(3):
                hi = outcome if right else not outcome
                sig.append((0, round(rng.uniform(0.55, 0.99) if hi else rng.uniform(0.01, 0.45), 3)))
        for _ in range(rng.randint(2, 7)):
            sig.append((rng.randrange(1, 7), round(rng.random(), 3)))
        if m % 3 == 1:  # a source signals again in the same market, with the opposite vote
            s, p = sig[-1]
            sig.append((s, round(1.0 - p, 3)))
        if m == 2:
            sig.append((3, 0.5))  # exactly on the threshold: votes True
        if m == 4:
            sig.append((7, 0.9))
            sig.append((7, 0.2))
        rng.shuffle(sig)
        markets.append((sig, outcome))
    return markets


def rows(store, key):
    return {r.source_id: [repr(r.reliability), repr(r.confidence)] for r in store._store.list_sources(key)}


def main() -> None:
    markets = make_batch()
    total, correct = [0] * N_SOURCES, [0] * N_SOURCES
    with tempfile.TemporaryDirectory() as tmp:
        store = NamespacedReliabilityStore(os.path.join(tmp, "settle.db"))
        for scope, s, r, c in SEEDS:
            key = f"__domain__:{DOMAIN}" if scope == "domain" else store.GLOBAL_MARKET_ID
            store._store._conn.execute(
                "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
                (NAMES[s], key, r, c, STAMP))
        for sig, outcome in markets:
            if outcome is None:
                continue
            for s, p in sig:
                ok = (p >= 0.5) == outcome
                total[s] += 1
                correct[s] += int(ok)
                store.update_reliability(NAMES[s], ok, domain=DOMAIN, update_global=True)
        final = {"domain": rows(store, f"__domain__:{DOMAIN}"), "global": rows(store, store.GLOBAL_MARKET_ID)}
        store.close()
    offsets = [0]
    for sig, _ in markets:
        offsets.append(offsets[-1] + len(sig))
    doc = {
        "n_sources": N_SOURCES,
        "names": NAMES,
        "domain": DOMAIN,
        "offsets": offsets,
        "sid": [s for sig, _ in markets for s, _ in sig],
        "prob": [repr(p) for sig, _ in markets for _, p in sig],
        "outcome": [-1 if o is None else int(o) for _, o in markets],
        "seeds": [{"scope": scope, "source": s, "reliability": repr(r), "confidence": repr(c), "updated_at": STAMP}
                  for scope, s, r, c in SEEDS],
        "total": total,
        "correct": correct,
        "final": final,
    }
    with open(os.path.join(HERE, "settle_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
