#!/usr/bin/env python3
"""Generate walk_lag_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_walk_lag.py

10 markets x 6 sources on a temp-file SQLite database, at one domain scope, run as an event loop
with the clock frozen at every event's own time.  Every market has a forecast event ``(forecast
time, market, 0)`` and, if it is resolved, a resolution event ``(resolve time, market, 1)``; the
events run in ascending order.  At a forecast every unique source of the market is fetched with
``SQLiteReliabilityStore.get_reliability(sid, scope, apply_decay=True)`` into the dict
``compute_consensus(signals, dict)`` takes; at a resolution ``update_reliability(sid, scope,
(probability >= 0.5) == outcome)`` runs for every signal in position order (market.py:298-301).

Seeded rows: one at reliability 1.0, one at 0.0, one with an empty ``updated_at`` (used, never
decayed); src-5 has no row.  The batch has a duplicate source inside a market, an unresolved
market, two markets forecast at the same time (one of them resolving at that very time: the other
does not see it), a market that resolves after a later-forecast one has, two resolve times equal
to a later market's forecast time (which sees them), and a market that resolves after the last
forecast.  Floats are stored as ``repr``; the fixture holds data only.
"""
from __future__ import annotations

import json
import os
import random
import tempfile
from datetime import datetime, timedelta, timezone

import bayesian_engine.decay as ref_decay
import bayesian_engine.reliability as ref_rel
from bayesian_engine.core import compute_consensus
from bayesian_engine.reliability import SQLiteReliabilityStore

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [f"src-{i}" for i in range(6)]  # sorted() order == rank order
SCOPE = "__domain__:d"
T0 = datetime(2026, 3, 1, 12, 0, 0, 250000, tzinfo=timezone.utc)
EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)
# days from T0 of markets 0..9.  Forecasts ascend, 3 and 4 tie.
FORECAST = [0.0, 0.5, 3.0, 10.0, 10.0, 20.0, 21.0, 30.0, 45.0, 60.0]
# 1 resolves exactly when 3 and 4 are forecast (both see it); 4 resolves at its own forecast time
# (3 does not see it); 2 resolves after 3 and 4 have; 5 is unresolved; 6 resolves exactly when 7 is
# forecast; 8 resolves after the last forecast; 9 has no lag.
RESOLVE = [0.25, 10.0, 25.0, 12.0, 10.0, None, 30.0, 44.0, 90.0, 60.0]
CLOCK = [T0]


class _FrozenDT(datetime):
    @classmethod
    def now(cls, tz=None):
        return CLOCK[0] if tz is None else CLOCK[0].astimezone(tz)


def stamp(days: float) -> str:
    return (T0 - timedelta(days=days)).isoformat()


# (source, reliability, confidence, updated_at)
SEEDS = [
    (0, 1.0, 0.6, stamp(2.0)),
    (1, 0.0, 0.3, stamp(20.0)),
    (2, 0.66, 0.41, ""),          # falsy: the row supplies (rel, conf), never decayed
    (3, 0.42, 0.9999, stamp(0.5)),
    (4, 0.95, 0.25, stamp(75.0)),
]


def make_batch():
    rng = random.Random(20261020)
    markets = []
    for m in range(10):
        outcome = None if RESOLVE[m] is None else (rng.random() < 0.5)
        sig = [(rng.randrange(0, 6), round(rng.random(), 3)) for _ in range(rng.randint(3, 5))]
        if m in (1, 7):  # a source signals again in the same market, with the opposite vote
            s, p = sig[0]
            sig.append((s, round(1.0 - p, 3)))
        if m == 2:
            sig.append((4, 0.5))  # exactly on the threshold: votes True
        if m == 5:
            sig.append((5, 0.8))  # seen in the unresolved market
        rng.shuffle(sig)
        markets.append((sig, outcome))
    return markets


def us(t: datetime) -> int:
    d = t - EPOCH
    return (d.days * 86400 + d.seconds) * 1_000_000 + d.microseconds


def main() -> None:
    ref_decay.datetime = _FrozenDT
    ref_rel.datetime = _FrozenDT
    batch = make_batch()
    forecast = [T0 + timedelta(days=d) for d in FORECAST]
    resolve = [None if d is None else T0 + timedelta(days=d) for d in RESOLVE]
    events = [(t, m, 0) for m, t in enumerate(forecast)]
    events += [(t, m, 1) for m, t in enumerate(resolve) if t is not None]
    events.sort()
    results = [None] * len(batch)
    with tempfile.TemporaryDirectory() as tmp:
        store = SQLiteReliabilityStore(os.path.join(tmp, "walk.db"))
        for s, r, c, ts in SEEDS:
            store._conn.execute(
                "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
                (NAMES[s], SCOPE, r, c, ts))
        for t, m, kind in events:
            CLOCK[0] = t
            sig, outcome = batch[m]
            if kind == 1:
                for s, p in sig:
                    store.update_reliability(NAMES[s], SCOPE, (p >= 0.5) == outcome)
                continue
            signals = [{"sourceId": NAMES[s], "probability": p} for s, p in sig]
            table = {}
            for name in sorted({x["sourceId"] for x in signals}):
                rec = store.get_reliability(name, SCOPE, apply_decay=True)
                table[name] = {"reliability": rec.reliability, "confidence": rec.confidence}
            res = compute_consensus(signals, table)
            results[m] = {
                "consensus": None if res["consensus"] is None else repr(res["consensus"]),
                "confidence": repr(res["confidence"]),
                "totalWeight": repr(res["normalization"]["totalWeight"]),
                "sourceWeights": [[w["sourceId"], repr(w["weight"]), repr(w["normalizedWeight"])]
                                  for w in res["sourceWeights"]],
                "read": [[name, repr(table[name]["reliability"]), repr(table[name]["confidence"])]
                         for name in sorted(table)],
            }
        final = [[r.source_id, repr(r.reliability), repr(r.confidence), r.updated_at]
                 for r in store.list_sources(SCOPE)]
        store.close()
    doc = {
        "names": NAMES,
        "scope": SCOPE,
        "domain": "d",
        "forecast_times": [t.isoformat() for t in forecast],
        "forecast_times_us": [us(t) for t in forecast],
        "resolve_times": [None if t is None else t.isoformat() for t in resolve],
        "resolve_times_us": [None if t is None else us(t) for t in resolve],
        "events": [[m, kind] for _, m, kind in events],
        "markets": [{"signals": [[s, repr(p)] for s, p in sig], "outcome": None if o is None else bool(o)}
                    for sig, o in batch],
        "seeds": [[NAMES[s], repr(r), repr(c), ts] for s, r, c, ts in SEEDS],
        "results": results,
        "final": final,
    }
    with open(os.path.join(HERE, "walk_lag_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
