#!/usr/bin/env python3
"""Generate update_sweep_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_update_sweep.py

The online loop of gen_walk_forward.py (its batch, seeds, times and frozen clock) run once per
update point ``(learning rate, step cap)`` with the reference's two module constants
``bayesian_engine.reliability._BASE_LEARNING_RATE`` / ``.MAX_UPDATE_STEP`` patched to the point,
and the event loop of gen_walk_lag.py likewise for two of the points.  ``(0.15, 0.10)`` is the
reference's own rule, ``(0.0, 0.10)`` a rule that never moves a reliability.  Per point the
fixture holds every market's reads and consensus and the store's final rows.  Floats are stored
as ``repr``; the fixture holds data only.
"""
from __future__ import annotations

import json
import os
import tempfile
from datetime import datetime, timedelta

import bayesian_engine.decay as ref_decay
import bayesian_engine.reliability as ref_rel
from bayesian_engine.core import compute_consensus
from bayesian_engine.reliability import SQLiteReliabilityStore

import gen_walk_forward as gwf
import gen_walk_lag as gwl

HERE = os.path.dirname(os.path.abspath(__file__))
POINTS = [(0.15, 0.10), (0.05, 0.10), (0.30, 0.20), (0.0, 0.10)]
LAG_POINTS = [(0.05, 0.10), (0.30, 0.20)]
CLOCK = [gwf.T0]


class _FrozenDT(datetime):
    @classmethod
    def now(cls, tz=None):
        return CLOCK[0] if tz is None else CLOCK[0].astimezone(tz)


def run_events(mod, batch, events):
    """``(results by market, final rows)`` of one event loop on a fresh store seeded as ``mod``
    seeds it: kind 0 scores the market, kind 1 settles it."""
    results = [None] * len(batch)
    with tempfile.TemporaryDirectory() as tmp:
        store = SQLiteReliabilityStore(os.path.join(tmp, "walk.db"))
        for s, r, c, ts in mod.SEEDS:
            store._conn.execute(
                "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) VALUES (?, ?, ?, ?, ?)",
                (mod.NAMES[s], mod.SCOPE, r, c, ts))
        for t, m, kind in events:
            CLOCK[0] = t
            sig, outcome = batch[m]
            if kind == 1:
                for s, p in sig:
                    store.update_reliability(mod.NAMES[s], mod.SCOPE, (p >= 0.5) == outcome)
                continue
            signals = [{"sourceId": mod.NAMES[s], "probability": p} for s, p in sig]
            table = {}
            for name in sorted({x["sourceId"] for x in signals}):
                rec = store.get_reliability(name, mod.SCOPE, apply_decay=True)
                table[name] = {"reliability": rec.reliability, "confidence": rec.confidence}
            res = compute_consensus(signals, table)
            results[m] = {
                "consensus": None if res["consensus"] is None else repr(res["consensus"]),
                "confidence": repr(res["confidence"]),
                "totalWeight": repr(res["normalization"]["totalWeight"]),
                "read": [[name, repr(table[name]["reliability"]), repr(table[name]["confidence"])]
                         for name in sorted(table)],
            }
        final = [[r.source_id, repr(r.reliability), repr(r.confidence), r.updated_at]
                 for r in store.list_sources(mod.SCOPE)]
        store.close()
    return results, final


def run_point(mod, batch, events, rate, cap):
    ref_rel._BASE_LEARNING_RATE = rate
    ref_rel.MAX_UPDATE_STEP = cap
    results, final = run_events(mod, batch, events)
    return {"learning_rate": repr(rate), "max_step": repr(cap), "results": results, "final": final}


def main() -> None:
    ref_decay.datetime = _FrozenDT
    ref_rel.datetime = _FrozenDT
    keep = ref_rel._BASE_LEARNING_RATE, ref_rel.MAX_UPDATE_STEP
    batch = gwf.make_batch()
    times = [gwf.T0 + timedelta(days=d) for d in gwf.DAYS]
    # a market is scored, then settled, at its own time, in market order (times need not ascend)
    events = [(t, m, kind) for m, t in enumerate(times) for kind in ((0, 1) if batch[m][1] is not None else (0,))]
    points = [run_point(gwf, batch, events, rate, cap) for rate, cap in POINTS]
    lbatch = gwl.make_batch()
    forecast = [gwl.T0 + timedelta(days=d) for d in gwl.FORECAST]
    resolve = [None if d is None else gwl.T0 + timedelta(days=d) for d in gwl.RESOLVE]
    levents = sorted([(t, m, 0) for m, t in enumerate(forecast)] +
                     [(t, m, 1) for m, t in enumerate(resolve) if t is not None])
    lag_points = [run_point(gwl, lbatch, levents, rate, cap) for rate, cap in LAG_POINTS]
    ref_rel._BASE_LEARNING_RATE, ref_rel.MAX_UPDATE_STEP = keep
    doc = {"walk_fixture": "walk_forward_small.json", "lag_fixture": "walk_lag_small.json",
           "points": points, "lag_points": lag_points}
    with open(os.path.join(HERE, "update_sweep_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
