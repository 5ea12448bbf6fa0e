#!/usr/bin/env python3
"""Generate walk_namespaced_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_walk_namespaced.py

12 markets x 6 sources on a temp-file SQLite database behind the reference's
``NamespacedReliabilityStore``, run the way the reference runs online, the clock frozen at every
market's own time: per market, every unique source is fetched with ``get_reliability(sid,
market_id=<id>, domain=<domain or None>, apply_decay=True)`` into the dict
``compute_consensus(signals, dict)`` takes; a resolved market then calls ``update_reliability(sid,
(probability >= 0.5) == outcome, domain=<domain or None>, update_global=<flag>)`` for every signal
in position order.  The whole batch runs twice on fresh databases, ``update_global`` False / True.

Two domains (crypto, sports) and two markets without one.  Seeds: (src-2, crypto) has an EMPTY
``updated_at`` (skipped by the first read, yet the start of its chain; read at domain scope after
market 0 updated it); (src-3, sports) and (src-4, crypto) have no row and gain one mid-batch;
src-4's global row is created by market 2 (no domain) before its first crypto update in market 6;
(src-3, global) has an empty stamp too; the market row (src-0, walk:m3) has a stamp and wins,
(src-1, walk:m4) has an empty one and falls through.  Markets 1 and 6 hold a source twice, market
5 is unresolved, markets 3/4 and 9/10 share a time, market 6 is earlier than market 5; src-5 is
cold at every read.  Floats are stored as ``repr``; the fixture holds data only.
"""
from __future__ import annotations

import json
import os
import tempfile
from datetime import datetime, timedelta, timezone

import bayesian_engine.decay as ref_decay
import bayesian_engine.reliability as ref_rel
from bayesian_engine.core import compute_consensus
from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [f"src-{i}" for i in range(6)]  # sorted() order == rank order
T0 = datetime(2026, 3, 1, 12, 0, 0, 250000, tzinfo=timezone.utc)
EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)
DAYS = [0.0, 0.5, 3.0, 10.0, 10.0, 40.0, 38.5, 45.0, 135.0, 136.25, 136.25, 200.0]
CLOCK = [T0]
GLOBAL = "__global__"
CRYPTO, SPORTS = "__domain__:crypto", "__domain__:sports"


class _FrozenDT(datetime):
    @classmethod
    def now(cls, tz=None):
        return CLOCK[0] if tz is None else CLOCK[0].astimezone(tz)


def stamp(days: float) -> str:
    return (T0 - timedelta(days=days)).isoformat()


# (source, scope key, reliability, confidence, updated_at)
SEEDS = [
    (0, GLOBAL, 0.8, 0.5, stamp(3.0)),
    (1, GLOBAL, 0.3, 0.7, stamp(30.0)),
    (2, GLOBAL, 0.55, 0.35, stamp(1.0)),
    (3, GLOBAL, 0.9, 0.2, ""),            # exists, never read; the start of src-3's global chain
    (0, CRYPTO, 1.0, 0.6, stamp(2.0)),
    (1, CRYPTO, 0.0, 0.3, stamp(20.0)),
    (2, CRYPTO, 0.66, 0.41, ""),          # skipped by market 0's read, updated by market 0
    (0, SPORTS, 0.95, 0.25, stamp(75.0)),
    (1, SPORTS, 0.42, 0.9999, stamp(0.5)),
    (0, "walk:m3", 0.77, 0.8, stamp(1.0)),  # a market row with a stamp wins
    (1, "walk:m4", 0.2, 0.2, ""),           # one without falls through to the domain
]

# (domain, outcome, [(source, probability), ...])
MARKETS = [
    ("crypto", True, [(0, 0.81), (1, 0.35), (2, 0.7)]),
    ("sports", False, [(0, 0.2), (3, 0.64), (1, 0.5), (3, 0.31)]),
    (None, True, [(4, 0.9), (0, 0.45), (2, 0.66)]),
    ("crypto", True, [(0, 0.58), (2, 0.12), (1, 0.93)]),
    ("sports", True, [(1, 0.77), (3, 0.83), (4, 0.4)]),
    ("crypto", None, [(5, 0.8), (2, 0.3), (0, 0.6), (4, 0.55)]),
    ("crypto", False, [(4, 0.7), (2, 0.25), (4, 0.1), (1, 0.61)]),
    ("", False, [(1, 0.05), (3, 0.95), (0, 0.5)]),
    ("sports", True, [(0, 0.71), (2, 0.49), (3, 0.88)]),
    ("crypto", True, [(4, 0.52), (0, 0.97), (2, 0.63), (1, 0.18)]),
    ("sports", False, [(3, 0.27), (1, 0.74), (4, 0.36)]),
    ("crypto", True, [(5, 0.44), (2, 0.91), (0, 0.08)]),
]


def us(t: datetime) -> int:
    d = t - EPOCH
    return (d.days * 86400 + d.seconds) * 1_000_000 + d.microseconds


def run(update_global: bool, times):
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        store = NamespacedReliabilityStore(os.path.join(tmp, "walk.db"))
        for s, key, r, c, ts in SEEDS:
            store._store._conn.execute(
                "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
                (NAMES[s], key, r, c, ts))
        for m, ((domain, outcome, sig), t) in enumerate(zip(MARKETS, times)):
            CLOCK[0] = t
            signals = [{"sourceId": NAMES[s], "probability": p} for s, p in sig]
            table, read = {}, []
            for name in sorted({x["sourceId"] for x in signals}):
                rec = store.get_reliability(name, market_id=f"walk:m{m}", domain=domain or None, apply_decay=True)
                table[name] = {"reliability": rec.reliability, "confidence": rec.confidence}
                read.append([name, repr(rec.reliability), repr(rec.confidence), rec.namespace.value,
                             rec.namespace_value])
            res = compute_consensus(signals, table)
            results.append({
                "consensus": None if res["consensus"] is None else repr(res["consensus"]),
                "confidence": repr(res["confidence"]),
                "totalWeight": repr(res["normalization"]["totalWeight"]),
                "sourceWeights": [[w["sourceId"], repr(w["weight"]), repr(w["normalizedWeight"])]
                                  for w in res["sourceWeights"]],
                "read": read,
            })
            if outcome is None:
                continue
            for s, p in sig:
                store.update_reliability(NAMES[s], (p >= 0.5) == outcome, domain=domain or None,
                                         update_global=update_global)
        final = [[r.source_id, r.market_id, repr(r.reliability), repr(r.confidence), r.updated_at]
                 for r in store._store.list_sources()]
        store.close()
    return {"results": results, "final": final}


def main() -> None:
    ref_decay.datetime = _FrozenDT
    ref_rel.datetime = _FrozenDT
    times = [T0 + timedelta(days=d) for d in DAYS]
    doc = {
        "names": NAMES,
        "domains": [d for d, _, _ in MARKETS],
        "market_ids": [f"walk:m{m}" for m in range(len(MARKETS))],
        "times": [t.isoformat() for t in times],
        "times_us": [us(t) for t in times],
        "markets": [{"signals": [[s, repr(p)] for s, p in sig], "outcome": o} for _, o, sig in MARKETS],
        "seeds": [[NAMES[s], key, repr(r), repr(c), ts] for s, key, r, c, ts in SEEDS],
        "runs": {"false": run(False, times), "true": run(True, times)},
    }
    with open(os.path.join(HERE, "walk_namespaced_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
