#!/usr/bin/env python3
"""Generate history_live_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_history_live.py

10 markets x 6 sources on a temp-file SQLite database, at one domain scope, run as an event loop at
ARRIVAL granularity with the clock frozen at every event's own time.  Signal k of market m is the
event ``(arrival time, m, 0, k)`` and every resolved market the event ``(resolve time, m, 1)``; the
events run in ascending order.  At an arrival every unique source of the market's first k + 1
signals is fetched with ``SQLiteReliabilityStore.get_reliability(sid, scope, apply_decay=True)``
into the dict ``compute_consensus(signals[:k + 1], dict)`` takes -- a ``Market`` used online; at a
resolution ``update_reliability(sid, scope, (probability >= 0.5) == outcome)`` runs for every signal
in position order (market.py:298-301).

Seeded rows: one at reliability 1.0, one at 0.0, one with an empty ``updated_at`` (used, never
decayed); src-5 has no row.  What the batch holds is asserted in ``check_batch``: a market that
resolves between two arrivals of another one they share a source with, a resolve time equal to an
arrival of a lower-indexed and of a higher-indexed market, two signals of one market at one time,
a source signalling twice in a market with opposite votes, a source that is cold at a market's
first points and has a row at its later ones, an unresolved market, a market that resolves exactly
at its last arrival, and markets that are not in time order.  Floats are stored as ``repr``; the
fixture holds data only.
"""
from __future__ import annotations

import json
import os
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
CLOCK = [T0]

# (signals as (source, probability, arrival in days from T0), outcome, resolve in days from T0)
MARKETS = [
    ([(0, 0.8, 0.0), (5, 0.7, 0.5), (1, 0.3, 1.0)], True, 2.0),
    # long-lived: src-5 is cold at its first two points and has a row (market 0, at day 2.0: the
    # lower index is seen at the tie) from the third; two signals at day 2.0; src-5 votes both ways;
    # its day-6.0 point does not see market 3 resolve at 6.0 (higher index); market 4 resolves
    # between its last two arrivals; it resolves exactly at its last arrival
    ([(5, 0.6, 0.25), (0, 0.4, 1.5), (2, 0.55, 2.0), (5, 0.35, 2.0), (3, 0.9, 6.0), (1, 0.2, 12.0)], False, 12.0),
    ([(4, 0.5, 1.0), (2, 0.1, 3.0), (5, 0.8, 7.0)], None, None),
    ([(3, 0.65, 3.0), (0, 0.2, 4.0), (4, 0.5, 5.0)], True, 6.0),
    ([(1, 0.9, 4.5), (1, 0.1, 4.5), (2, 0.7, 5.5)], True, 9.0),
    ([(3, 0.3, 6.0), (0, 0.6, 8.0), (4, 0.45, 10.0), (5, 0.5, 20.0)], False, 25.0),  # its day-6.0 point sees market 3
    ([(2, 0.4, 9.0)], True, 9.0),
    ([(0, 0.95, 30.0), (1, 0.05, 30.0), (2, 0.5, 31.0), (3, 0.5, 40.0), (4, 0.6, 45.0), (5, 0.4, 60.0)], True, 90.0),
    ([(5, 0.7, 0.125), (5, 0.2, 50.0)], False, 50.0),
    ([(4, 0.3, 13.0), (3, 0.8, 14.0)], False, 14.0),
]


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


def check_batch() -> None:
    """What the batch is meant to hold."""
    res = [(m, r) for m, (_, o, r) in enumerate(MARKETS) if o is not None]
    arr = [(m, k, s, t) for m, (sig, _, _) in enumerate(MARKETS) for k, (s, _, t) in enumerate(sig)]
    src = lambda m: {s for s, _, _ in MARKETS[m][0]}  # noqa: E731
    # a market resolving strictly between two arrivals of another market, a source of it arriving later there
    assert any(a != m and t0 < r < t1 and s1 in src(m)
               for m, r in res for a, k0, _, t0 in arr for b, k1, s1, t1 in arr if a == b and k1 == k0 + 1)
    # a resolve time equal to an arrival of a lower-indexed and of a higher-indexed market, with a shared source
    assert any(any(a < m and t == r and s in src(m) for a, _, s, t in arr) and
               any(a > m and t == r and s in src(m) for a, _, s, t in arr) for m, r in res)
    assert any(a == b and k1 == k0 + 1 and t0 == t1 for a, k0, _, t0 in arr for b, k1, _, t1 in arr)
    assert any(s0 == s1 and (p0 >= 0.5) != (p1 >= 0.5)
               for sig, _, _ in MARKETS for i, (s0, p0, _) in enumerate(sig) for s1, p1, _ in sig[i + 1:])
    # src-5 has no row: cold at market 1's first points, settled by market 0 before its later ones
    assert 5 not in {s for s, *_ in SEEDS} and MARKETS[1][0][0][0] == 5 and MARKETS[1][0][0][2] < MARKETS[0][2] \
        and 5 in src(0) and MARKETS[1][0][3][0] == 5 and MARKETS[1][0][3][2] >= MARKETS[0][2]
    assert any(o is None for _, o, _ in MARKETS)
    assert any(o is not None and r == sig[-1][2] for sig, o, r in MARKETS)
    assert all(o is None or r >= sig[-1][2] for sig, o, r in MARKETS)
    assert all(sig[i][2] <= sig[i + 1][2] for sig, _, _ in MARKETS for i in range(len(sig) - 1))
    assert any(MARKETS[m + 1][0][0][2] < MARKETS[m][0][0][2] for m in range(len(MARKETS) - 1))  # not in time order


def us(t: datetime) -> int:
    d = t - EPOCH
    return (d.days * 86400 + d.seconds) * 1_000_000 + d.microseconds


def main() -> None:
    check_batch()
    ref_decay.datetime = _FrozenDT
    ref_rel.datetime = _FrozenDT
    at = lambda days: T0 + timedelta(days=days)  # noqa: E731
    events = [(at(t), m, 0, k) for m, (sig, _, _) in enumerate(MARKETS) for k, (_, _, t) in enumerate(sig)]
    events += [(at(r), m, 1, 0) for m, (_, o, r) in enumerate(MARKETS) if o is not None]
    events.sort()
    results = [[None] * len(sig) for sig, _, _ in MARKETS]
    with tempfile.TemporaryDirectory() as tmp:
        store = SQLiteReliabilityStore(os.path.join(tmp, "live.db"))
        for s, r, c, ts in SEEDS:
            store._conn.execute(
                "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
                (NAMES[s], SCOPE, r, c, ts))
        for t, m, kind, k in events:
            CLOCK[0] = t
            sig, outcome, _ = MARKETS[m]
            if kind == 1:
                for s, p, _ in sig:
                    store.update_reliability(NAMES[s], SCOPE, (p >= 0.5) == outcome)
                continue
            signals = [{"sourceId": NAMES[s], "probability": p} for s, p, _ in sig[:k + 1]]
            table = {}
            for name in sorted({x["sourceId"] for x in signals}):
                rec = store.get_reliability(name, SCOPE, apply_decay=True)
                table[name] = {"reliability": rec.reliability, "confidence": rec.confidence}
            res = compute_consensus(signals, table)
            results[m][k] = {
                "consensus": None if res["consensus"] is None else repr(res["consensus"]),
                "confidence": repr(res["confidence"]),
                "totalWeight": repr(res["normalization"]["totalWeight"]),
                "sourceCount": res["normalization"]["sourceCount"],
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
        "arrival_times": [[at(t).isoformat() for _, _, t in sig] for sig, _, _ in MARKETS],
        "arrival_times_us": [[us(at(t)) for _, _, t in sig] for sig, _, _ in MARKETS],
        "resolve_times": [None if o is None else at(r).isoformat() for _, o, r in MARKETS],
        "resolve_times_us": [None if o is None else us(at(r)) for _, o, r in MARKETS],
        "markets": [{"signals": [[s, repr(p)] for s, p, _ in sig], "outcome": None if o is None else bool(o)}
                    for sig, o, _ in MARKETS],
        "seeds": [[NAMES[s], repr(r), repr(c), ts] for s, r, c, ts in SEEDS],
        "results": results,
        "final": final,
    }
    with open(os.path.join(HERE, "history_live_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
