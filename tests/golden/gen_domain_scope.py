#!/usr/bin/env python3
"""Generate domain_scope_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_domain_scope.py

7 markets x 5 sources on a temp-file SQLite database; the domain of a market is its
``MarketId.category`` (three domains, and one market without a category).  Rows are pre-seeded at
all three scopes: a market row with an empty ``updated_at`` (falls through to the domain), a
domain row with an unparseable stamp (used, never decayed), a domain row with an empty stamp
(falls through to global).  Duplicate signals of one source in a market, one unresolved market, a
probability of exactly 0.5.  Under a frozen clock the fixture records

* ``consensus``: per market, ``market.compute_consensus(source_rel)`` with ``source_rel`` built
  from ``NamespacedReliabilityStore.get_reliability(sid, market_id=str(market.id),
  domain=market.id.category, apply_decay=True)`` per unique source (the loop of market.py:206-220
  with the namespaced store's arguments);
* ``final_update_global`` / ``final``: every row of the database after the reference's own
  per-signal loop ``update_reliability(sid, correct, domain=d, update_global=True / False)`` over
  the resolved markets, ``correct = (probability >= 0.5) == outcome`` (market.py:298-301), each on
  a freshly seeded database.

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
MARKETS = ["crypto:m0", "sports:m1", "crypto:m2", "plain-m3", "politics:m4", "sports:m5", "crypto:m6"]
NOW = datetime(2026, 3, 1, 12, 0, 0, tzinfo=timezone.utc)
EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)
GLOBAL = "__global__"
UNRESOLVED = 5


class _FrozenDT(datetime):
    @classmethod
    def now(cls, tz=None):
        return NOW if tz is None else NOW.astimezone(tz)


def stamp(days: float) -> str:
    return (NOW - timedelta(days=days)).isoformat()


def dom(d: str) -> str:
    return f"__domain__:{d}"


# (source, store key, reliability, confidence, updated_at)
SEEDS = [
    (0, MARKETS[0], 0.9, 0.6, stamp(3.5)),
    (1, MARKETS[0], 0.2, 0.3, stamp(40.0)),
    (4, MARKETS[1], 0.55, 0.5, ""),                 # falsy: falls through to the sports domain row
    (2, MARKETS[2], 0.0, 0.9999, stamp(12.0)),
    (1, MARKETS[3], 0.31, 0.8, stamp(7.0)),         # the market without a domain
    (0, MARKETS[5], 1.0, 1.0, stamp(0.25)),         # the unresolved market
    (3, dom("crypto"), 0.66, 0.41, "not-a-date"),   # unparseable: used, never decayed
    (0, dom("crypto"), 0.81, 0.35, stamp(20.0)),
    (2, dom("crypto"), 0.4, 0.7, stamp(1.5)),
    (4, dom("sports"), 0.12, 0.7, stamp(1.0)),
    (1, dom("sports"), 0.95, 0.25, stamp(100.0)),
    (2, dom("politics"), 0.3, 0.3, ""),             # falsy: falls through to global
    (3, dom("politics"), 0.58, 0.9, stamp(60.0)),
    (0, GLOBAL, 0.77, 0.5, stamp(2.0)),
    (2, GLOBAL, 0.0, 0.25, stamp(9.0)),
    (3, GLOBAL, 1.0, 1.0, stamp(30.0)),
]
# signals that make the seeded rows above count: (market, source, probability)
PINNED = [(0, 3, 0.61), (1, 4, 0.5), (4, 2, 0.7), (4, 3, 0.2), (3, 1, 0.9), (3, 4, 0.35), (6, 3, 0.45), (6, 1, 0.8)]


def make_batch():
    rng = random.Random(20261019)
    markets = []
    for m in range(len(MARKETS)):
        outcome = None if m == UNRESOLVED else (rng.random() < 0.5)
        sig = [(rng.randrange(0, 5), round(rng.random(), 3)) for _ in range(rng.randint(2, 5))]
        if m in (0, 5):  # a source signals again in the same market, with the opposite vote
            s, p = sig[0]
            sig.append((s, round(1.0 - p, 3)))
            sig.append((s, p))
        sig += [(s, p) for mk, s, p in PINNED if mk == m]
        rng.shuffle(sig)
        markets.append((sig, outcome))
    return markets


def seeded_store(path):
    store = NamespacedReliabilityStore(path)
    for s, key, r, c, ts in SEEDS:
        store._store._conn.execute(
            "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
            (NAMES[s], key, r, c, ts))
    return store


def settle(store, batch, update_global):
    for mid, (sig, outcome) in zip(MARKETS, batch):
        if outcome is None:
            continue
        for s, p in sig:
            store.update_reliability(NAMES[s], (p >= 0.5) == outcome, domain=MarketId(mid).category,
                                     update_global=update_global)
    return [[r.source_id, r.market_id, r.reliability, r.confidence] for r in store._store.list_sources()]


def main() -> None:
    ref_decay.datetime = _FrozenDT
    ref_rel.datetime = _FrozenDT
    batch = make_batch()
    with tempfile.TemporaryDirectory() as tmp:
        store = seeded_store(os.path.join(tmp, "a.db"))
        ms = MarketStore()
        consensus = {}
        for mid, (sig, _) in zip(MARKETS, batch):
            market = ms.create_market(MarketId(mid))
            for s, p in sig:
                market.add_signal({"sourceId": NAMES[s], "probability": p})
            source_rel = {}
            for signal in market.signals:
                sid = signal["sourceId"]
                if sid not in source_rel:
                    rec = store.get_reliability(sid, market_id=str(market.id), domain=market.id.category,
                                                apply_decay=True)
                    source_rel[sid] = {"reliability": rec.reliability, "confidence": rec.confidence}
            consensus[mid] = market.compute_consensus(source_rel)
        final_g = settle(store, batch, True)
        store.close()
        store = seeded_store(os.path.join(tmp, "b.db"))
        final = settle(store, batch, False)
        store.close()
    d = NOW - EPOCH
    doc = {
        "names": NAMES,
        "market_ids": MARKETS,
        "domains": [MarketId(m).category for m in MARKETS],
        "now_us": (d.days * 86400 + d.seconds) * 1_000_000 + d.microseconds,
        "markets": [{"signals": [[s, p] for s, p in sig], "outcome": None if o is None else bool(o)}
                    for sig, o in batch],
        "seeds": [[NAMES[s], key, r, c, ts] for s, key, r, c, ts in SEEDS],
        "consensus": consensus,
        "final_update_global": final_g,
        "final": final,
    }
    with open(os.path.join(HERE, "domain_scope_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
