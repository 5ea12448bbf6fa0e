#!/usr/bin/env python3
"""Generate walk_scope_lag_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_walk_scope_lag.py

12 markets x 6 sources on a temp-file SQLite database behind the reference's
``NamespacedReliabilityStore``, run as an event loop with the clock frozen at every event's own
time.  Every market has a forecast event ``(forecast time, market, 0)`` and, if it is resolved, a
resolution event ``(resolve time, market, 1)``; the events run in ascending order.  At a forecast
every unique source of the market is fetched with ``get_reliability(sid, market_id=<id>,
domain=<domain or None>, apply_decay=True)`` into the dict ``compute_consensus(signals, dict)``
takes; at a resolution ``update_reliability(sid, (probability >= 0.5) == outcome, domain=<domain or
None>, update_global=<flag>)`` runs for every signal in position order.  The whole batch runs twice
on fresh databases, ``update_global`` False / True.

Two domains (crypto, sports) and two markets without one.  What the batch holds:

* (src-2, crypto) has an EMPTY ``updated_at``; its first update is market 0's, which resolves at
  day 12 -- after market 3 (crypto) is forecast at day 10, so market 3 still skips the row and
  falls to the global one; market 5 (crypto, day 20) reads it at domain scope.
* src-4 has no global row; market 2 (no domain) creates it when it resolves at day 10.5, between
  the forecasts of day 10 (market 4 reads src-4 cold) and day 20 (market 5 reads it at global).
* market 1 (sports) resolves at day 10.0, exactly when markets 3 and 4 are forecast: market 4
  (sports) sees it.  Market 6 resolves exactly when market 7 is forecast.
* markets 3 / 4 and 9 / 10 tie on their forecast; 4 and 10 resolve at that very time, which their
  tie-mates 3 and 9 do not see (9 and 10 share the crypto domain).
* the market row (src-0, walk:m3) has a stamp and wins; (src-1, walk:m4) has an empty one and
  falls through to the domain.  (src-3, global) has an empty stamp too, until market 7 updates it.
* market 5 is unresolved; markets 1 and 6 hold a source twice; market 8 resolves after the last
  forecast; market 11 has no lag; src-5 is cold at every read.

Floats are stored as ``repr``; the fixture holds data only.
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
# days from T0 of markets 0..11.  Forecasts ascend; 3 / 4 and 9 / 10 tie.
FORECAST = [0.0, 0.5, 3.0, 10.0, 10.0, 20.0, 21.0, 30.0, 45.0, 60.0, 60.0, 75.0]
RESOLVE = [12.0, 10.0, 10.5, 25.0, 10.0, None, 30.0, 44.0, 90.0, 61.0, 60.0, 75.0]
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
    (3, GLOBAL, 0.9, 0.2, ""),            # exists, not read until market 7 has stamped it
    (0, CRYPTO, 1.0, 0.6, stamp(2.0)),
    (1, CRYPTO, 0.0, 0.3, stamp(20.0)),
    (2, CRYPTO, 0.66, 0.41, ""),          # skipped until market 0 resolves at day 12
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
    ("crypto", True, [(0, 0.58), (2, 0.12), (1, 0.93), (4, 0.3)]),
    ("sports", True, [(1, 0.77), (3, 0.83), (4, 0.4)]),
    ("crypto", None, [(5, 0.8), (2, 0.3), (0, 0.6), (4, 0.55)]),
    ("crypto", False, [(4, 0.7), (2, 0.25), (4, 0.1), (1, 0.61)]),
    ("", False, [(1, 0.05), (3, 0.95), (0, 0.5)]),
    ("sports", True, [(0, 0.71), (2, 0.49), (3, 0.88)]),
    ("crypto", True, [(4, 0.52), (0, 0.97), (2, 0.63), (1, 0.18)]),
    ("crypto", False, [(3, 0.27), (1, 0.74), (4, 0.36)]),
    ("crypto", True, [(5, 0.44), (2, 0.91), (0, 0.08)]),
]


def us(t: datetime) -> int:
    d = t - EPOCH
    return (d.days * 86400 + d.seconds) * 1_000_000 + d.microseconds


def run(update_global: bool, events):
    results = [None] * len(MARKETS)
    with tempfile.TemporaryDirectory() as tmp:
        store = NamespacedReliabilityStore(os.path.join(tmp, "walk.db"))
        for s, key, r, c, ts in SEEDS:
            store._store._conn.execute(
                "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
                (NAMES[s], key, r, c, ts))
        for t, m, kind in events:
            CLOCK[0] = t
            domain, outcome, sig = MARKETS[m]
            if kind == 1:
                for s, p in sig:
                    store.update_reliability(NAMES[s], (p >= 0.5) == outcome, domain=domain or None,
                                             update_global=update_global)
                continue
            signals = [{"sourceId": NAMES[s], "probability": p} for s, p in sig]
            table, read = {}, []
            for name in sorted({x["sourceId"] for x in signals}):
                rec = store.get_reliability(name, market_id=f"walk:m{m}", domain=domain or None, apply_decay=True)
                table[name] = {"reliability": rec.reliability, "confidence": rec.confidence}
                read.append([name, repr(rec.reliability), repr(rec.confidence), rec.namespace.value,
                             rec.namespace_value])
            res = compute_consensus(signals, table)
            results[m] = {
                "consensus": None if res["consensus"] is None else repr(res["consensus"]),
                "confidence": repr(res["confidence"]),
                "totalWeight": repr(res["normalization"]["totalWeight"]),
                "sourceWeights": [[w["sourceId"], repr(w["weight"]), repr(w["normalizedWeight"])]
                                  for w in res["sourceWeights"]],
                "read": read,
            }
        final = [[r.source_id, r.market_id, repr(r.reliability), repr(r.confidence), r.updated_at]
                 for r in store._store.list_sources()]
        store.close()
    return {"results": results, "final": final}


def main() -> None:
    ref_decay.datetime = _FrozenDT
    ref_rel.datetime = _FrozenDT
    forecast = [T0 + timedelta(days=d) for d in FORECAST]
    resolve = [None if d is None else T0 + timedelta(days=d) for d in RESOLVE]
    events = [(t, m, 0) for m, t in enumerate(forecast)]
    events += [(t, m, 1) for m, t in enumerate(resolve) if t is not None]
    events.sort()
    doc = {
        "names": NAMES,
        "domains": [d for d, _, _ in MARKETS],
        "market_ids": [f"walk:m{m}" for m in range(len(MARKETS))],
        "forecast_times": [t.isoformat() for t in forecast],
        "forecast_times_us": [us(t) for t in forecast],
        "resolve_times": [None if t is None else t.isoformat() for t in resolve],
        "resolve_times_us": [None if t is None else us(t) for t in resolve],
        "events": [[m, kind] for _, m, kind in events],
        "markets": [{"signals": [[s, repr(p)] for s, p in sig], "outcome": o} for _, o, sig in MARKETS],
        "seeds": [[NAMES[s], key, repr(r), repr(c), ts] for s, key, r, c, ts in SEEDS],
        "runs": {"false": run(False, events), "true": run(True, events)},
    }
    with open(os.path.join(HERE, "walk_scope_lag_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
