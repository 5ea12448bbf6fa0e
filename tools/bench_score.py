#!/usr/bin/env python3
"""Time back-test scoring (batch.score, bce_score_groups) with HIP events.

  (a) market groups: one group of ``--markets`` markets (batch.ScorePlan.whole), the consensus
      scored against random outcomes, 10 bins;
  (b) the same markets cut into groups of 1000 members (the aggregate shape);
  (c) per source: the config-3 batch (ragged markets, Zipf(1.1) sources; bench_extra.make_c3_full)
      through ScorePlan.by_source, base = a consensus per market.

Every timing is ``--calls`` back-to-back calls of batch.score between two HIP events on the
stream, plans and scratch built beforehand; ``--reps`` repetitions, all printed.  The fraction is
model bytes / time / 8 TB/s with the byte model of DESIGN §4.20: per item one 8-byte index (two per
source), one 8-byte forecast gather, one outcome byte.

    python tools/bench_score.py [--markets M] [--signals N] [--sources S] [--out measurements/score.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bayesian-consensus-engine_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_engine import _native as N  # noqa: E402
from bayesian_engine import batch  # noqa: E402

HBM = 8e12


def event_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markets", type=int, default=1_000_000)
    ap.add_argument("--signals", type=int, default=100_000_000)
    ap.add_argument("--sources", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    T = batch.to_device(dev)

    def run(label, plan, value, outcome, item_bytes, **kw):
        sb = int(N.lib().bce_score_scratch_bytes(plan.n_segments, 10))
        scratch = torch.empty(max(sb // 8, 1), dtype=torch.int64, device=dev)
        fn = lambda: batch.score(plan, value, outcome, scratch=scratch, **kw)  # noqa: E731
        r = fn()
        N.check_faults(dev, label)
        ts = [event_ms(fn, args.calls) for _ in range(args.reps)]
        again = fn()
        same = all(torch.equal(getattr(r, k).view(torch.int64), getattr(again, k).view(torch.int64))
                   for k in ("counts", "sums", "bin_n", "bin_pos", "bin_psum"))
        model = plan.n_items * item_bytes
        best = min(ts)
        say(f"{label}: {plan.n_groups} groups, {plan.n_items} items, {plan.n_segments} segments; ms per call: "
            + " ".join(f"{t:.4f}" for t in ts) + f"; model {model / 1e6:.1f} MB, min {best:.4f} ms = "
            f"{model / (best * 1e-3) / 1e9:.0f} GB/s = {100 * model / (best * 1e-3) / HBM:.1f}% of 8 TB/s; "
            f"repeat bit-identical: {same}; scored {int(r.n_scored.sum())}")

    M = args.markets
    cons = T(rng.random(M))
    outcome = T(rng.choice(np.array([-1, 0, 1], np.int8), M, p=[0.1, 0.45, 0.45]))
    valid = T((rng.random(M) < 0.98).astype(np.uint8))
    run("(a) one group of all markets", batch.ScorePlan.whole(M, device=dev), cons, outcome, 17, valid=valid)
    goff = torch.arange(0, M + 1, 1000, dtype=torch.int64, device=dev)
    if int(goff[-1]) != M:
        goff = torch.cat([goff, torch.tensor([M], dtype=torch.int64, device=dev)])
    members = T(rng.integers(0, M, M).astype(np.int64))
    run("(b) groups of 1000 members", batch.ScorePlan.groups(goff, members), cons, outcome, 17, valid=valid)
    del members

    from bench_extra import make_c3_full
    off_h, sid_h, prob_h, _ = make_c3_full(args.signals, args.sources)
    Mc = len(off_h) - 1
    off, sid, prob = T(off_h), T(sid_h), T(prob_h)
    plan = batch.ScorePlan.by_source(off, sid, args.sources)
    lens = (plan.group_offsets[1:] - plan.group_offsets[:-1])
    say(f"config 3: {Mc} markets, {len(sid_h)} signals, {args.sources} sources; longest source "
        f"{int(lens.max())} signals, {int((lens == 0).sum())} sources without a signal")
    del sid
    outcome3 = T(rng.choice(np.array([-1, 0, 1], np.int8), Mc, p=[0.1, 0.45, 0.45]))
    cons3 = T(rng.random(Mc))
    run("(c) per source, base = consensus", plan, prob, outcome3, 25, base=cons3)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
