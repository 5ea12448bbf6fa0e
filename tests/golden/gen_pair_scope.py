#!/usr/bin/env python3
"""Generate pair_scope_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_pair_scope.py

6 markets x 5 sources on a temp-file SQLite database, at MARKET scope: some (source, market) rows
and some ``__global__`` rows pre-seeded (one market row with an unparseable ``updated_at``, one
with an empty one), duplicate signals of one source in a market, one unresolved market, a
probability of exactly 0.5.  Under a frozen clock the fixture records

* ``consensus``: ``MarketStore.compute_all_consensus(SQLiteReliabilityStore)`` over all six
  markets (market.py:200-221: ``get_reliability(sid, str(market.id), apply_decay=True)`` per pair);
* ``final``: every row of the database after the reference's own per-signal loop
  ``NamespacedReliabilityStore.update_reliability(sid, correct, market_id=m, update_global=True)``
  over the resolved markets, ``correct = (probability >= 0.5) == outcome`` (market.py:298-301).

Floats are stored through ``json`` (``repr``: exact); ``updated_at`` of the final rows is not
stored.  The fixture holds data only.
"""
from __future__ import annotations

import json
import os
import random
import tempfile
from datetime import datetime, timedelta, timezone

import bayesian_engine.decay as ref_decay
import bayesian_engine.reliability as ref_rel
from bayesian_engine.market import MarketId, MarketStore
from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [f"src-{i}" for i in range(5)]  # sorted() order == rank order
MARKETS = [f"pair:m{i}" for i in range(6)]
NOW = datetime(2026, 3, 1, 12, 0, 0, tzinfo=timezone.utc)
EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)
GLOBAL = "__global__"


class _FrozenDT(datetime):
    @classmethod
    def now(cls, tz=None):
        return NOW if tz is None else NOW.astimezone(tz)


def stamp(days: float) -> str:
    return (NOW - timedelta(days=days)).isoformat()


# (source, market id, reliability, confidence, updated_at)
SEEDS = [
    (0, MARKETS[0], 0.9, 0.6, stamp(3.5)),
    (1, MARKETS[0], 0.2, 0.3, stamp(40.0)),
    (3, MARKETS[0], 0.66, 0.41, "not-a-date"),  # unparseable: used, never decayed
    (0, MARKETS[1], 1.0, 1.0, stamp(0.25)),
    (2, MARKETS[1], 0.0, 0.9999, stamp(12.0)),
    (4, MARKETS[2], 0.55, 0.5, ""),              # falsy: the row still supplies (rel, conf) at store scope
    (1, MARKETS[3], 0.31, 0.8, stamp(7.0)),      # the unresolved market: stays as it is
    (2, MARKETS[4], 0.95, 0.25, stamp(100.0)),
    (4, MARKETS[5], 0.12, 0.7, stamp(1.0)),
    (0, GLOBAL, 0.77, 0.5, stamp(2.0)),
    (2, GLOBAL, 0.0, 0.25, stamp(9.0)),
    (3, GLOBAL, 1.0, 1.0, stamp(30.0)),
]


def make_batch():
    rng = random.Random(20261019)
    markets = []
    for m in range(6):
        outcome = None if m == 3 else (rng.random() < 0.5)
        sig = [(rng.randrange(0, 5), round(rng.random(), 3)) for _ in range(rng.randint(2, 6))]
        if m in (0, 4):  # a source signals again in the same market, with the opposite vote
            s, p = sig[0]
            sig.append((s, round(1.0 - p, 3)))
            sig.append((s, p))
        if m == 2:
            sig.append((4, 0.5))  # exactly on the threshold: votes True
        rng.shuffle(sig)
        assert len(sig) <= 8
        markets.append((sig, outcome))
    return markets


def main() -> None:
    ref_decay.datetime = _FrozenDT
    ref_rel.datetime = _FrozenDT
    batch = make_batch()
    with tempfile.TemporaryDirectory() as tmp:
        store = NamespacedReliabilityStore(os.path.join(tmp, "pairs.db"))
        for s, mid, r, c, ts in SEEDS:
            store._store._conn.execute(
                "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
                (NAMES[s], mid, r, c, ts))
        ms = MarketStore()
        for mid, (sig, _) in zip(MARKETS, batch):
            market = ms.create_market(MarketId(mid))
            for s, p in sig:
                market.add_signal({"sourceId": NAMES[s], "probability": p})
        consensus = ms.compute_all_consensus(store._store)
        for mid, (sig, outcome) in zip(MARKETS, batch):
            if outcome is None:
                continue
            for s, p in sig:
                store.update_reliability(NAMES[s], (p >= 0.5) == outcome, market_id=mid, update_global=True)
        final = [[r.source_id, r.market_id, r.reliability, r.confidence] for r in store._store.list_sources()]
        store.close()
    d = NOW - EPOCH
    doc = {
        "names": NAMES,
        "market_ids": MARKETS,
        "now_us": (d.days * 86400 + d.seconds) * 1_000_000 + d.microseconds,
        "markets": [{"signals": [[s, p] for s, p in sig], "outcome": None if o is None else bool(o)}
                    for sig, o in batch],
        "seeds": [[NAMES[s], mid, r, c, ts] for s, mid, r, c, ts in SEEDS],
        "consensus": consensus,
        "final": final,
    }
    with open(os.path.join(HERE, "pair_scope_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
