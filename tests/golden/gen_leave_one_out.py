#!/usr/bin/env python3
"""Generate leave_one_out_small.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_leave_one_out.py

The markets and the table of gen_history.py (an empty market, single signals, zero-weight sources
alone and in front, repeated sources, descending and ascending arrival, one source throughout,
probabilities of 1.25, two random markets of 31 and 33 signals).  For every market and every
source x of it, in sorted() order, the reference's own ``compute_consensus([s for s in signals if
s["sourceId"] != x], table)`` (core.py:63-180) is recorded; dropping the only source of a market
leaves no signals (core.py:88-96).  ``full`` is the call on all signals (None for the empty
market's consensus as well).  Floats are stored as ``repr``; the fixture holds data only.
"""
from __future__ import annotations

import json
import os

from bayesian_engine.core import compute_consensus

from gen_history import NAMES, TABLE, make_markets

HERE = os.path.dirname(os.path.abspath(__file__))


def record(res):
    return {"consensus": None if res["consensus"] is None else repr(res["consensus"]),
            "confidence": repr(res["confidence"]),
            "totalWeight": repr(res["normalization"]["totalWeight"]),
            "sourceCount": res["normalization"]["sourceCount"]}


def main() -> None:
    doc = {"names": NAMES, "table": {k: {f: repr(v) for f, v in row.items()} for k, row in TABLE.items()},
           "markets": []}
    for sig in make_markets():
        signals = [{"sourceId": NAMES[s], "probability": p} for s, p in sig]
        leave_out = []
        for x in sorted({s["sourceId"] for s in signals}):
            rest = [s for s in signals if s["sourceId"] != x]
            leave_out.append(dict(sourceId=x, **record(compute_consensus(rest, TABLE))))
        doc["markets"].append({"signals": [[NAMES[s], repr(p)] for s, p in sig], "leave_out": leave_out,
                               "full": record(compute_consensus(signals, TABLE))})
    with open(os.path.join(HERE, "leave_one_out_small.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
