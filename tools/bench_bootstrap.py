#!/usr/bin/env python3
"""Time the bootstrap of back-test scores (batch.score_bootstrap, bce_score_bootstrap) with HIP
events.

  (a) one group of ``--markets`` markets (batch.ScorePlan.whole), K = 8 forecast sets, ``--boot``
      replicates;
  (b) the same with K = 1;
  (c) the only alternative that needs no new kernel: one batch.score call per replicate over a
      resampled member list (torch.multinomial indices, built beforehand and not timed), 16 calls
      timed and scaled to ``--boot`` + 1 calls for ONE set.

Every timing is one call between two HIP events on the stream after a warm-up call; ``--reps``
repetitions, all printed, the median reported.  Pairs = (replicates + 1) x items.

    python tools/bench_bootstrap.py [--markets M] [--boot R] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bayesian-consensus-engine_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_engine import _native as N  # noqa: E402
from bayesian_engine import batch  # noqa: E402


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markets", type=int, default=1_000_000)
    ap.add_argument("--boot", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sets", type=int, nargs="*", default=[8, 1])
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    T = batch.to_device(dev)
    M, R1 = args.markets, args.boot + 1
    outcome = T(rng.choice(np.array([-1, 0, 1], np.int8), M, p=[0.1, 0.45, 0.45]))
    plan = batch.ScorePlan.whole(M, device=dev)
    unit = batch.boot_units(M, 1, device=dev)
    for K in args.sets:
        value = T(rng.random((K, M)))
        valid = T((rng.random((K, M)) < 0.98).astype(np.uint8))
        fn = lambda: batch.score_bootstrap(plan, value, outcome, valid=valid, unit=unit, n_boot=args.boot)  # noqa: E731
        r = fn()
        N.check_faults(dev, "score_bootstrap")
        ts = [event_ms(fn) for _ in range(args.reps)]
        again = fn()
        same = torch.equal(r.counts, again.counts) and torch.equal(r.sums.view(torch.int64), again.sums.view(torch.int64))
        med = statistics.median(ts)
        pairs = R1 * M
        lo, hi = r.interval("brier")
        say(f"K = {K}: {M} markets, {plan.n_segments} segments, {R1} rows; ms per call: "
            + " ".join(f"{t:.3f}" for t in ts) + f"; median {med:.3f} ms = {pairs / (med * 1e-3) / 1e9:.1f} G pairs/s "
            f"= {pairs * K / (med * 1e-3) / 1e9:.1f} G (pair, set)/s; repeat bit-identical: {same}; "
            f"brier of set 0: {float(r.point('brier')[0, 0]):.6f} in [{float(lo[0, 0]):.6f}, {float(hi[0, 0]):.6f}]")
        del value, valid, r, again
    if not args.no_baseline:
        value = T(rng.random(M))
        valid = T((rng.random(M) < 0.98).astype(np.uint8))
        calls = 16
        p = torch.ones(M, dtype=torch.float32, device=dev)
        plans = [batch.ScorePlan.groups(plan.group_offsets, torch.multinomial(p, M, replacement=True), check=False)
                 for _ in range(calls)]
        scratch = torch.empty(max(int(N.lib().bce_score_scratch_bytes(plan.n_segments, 10)) // 8, 1), dtype=torch.int64,
                              device=dev)

        def baseline():
            for q in plans:
                batch.score(q, value, outcome, valid=valid, scratch=scratch)

        baseline()
        N.check_faults(dev, "baseline")
        ts = [event_ms(baseline) for _ in range(args.reps)]
        med = statistics.median(ts)
        say(f"baseline, one set: {calls} batch.score calls over resampled member lists (lists not timed); ms: "
            + " ".join(f"{t:.3f}" for t in ts) + f"; median {med / calls:.4f} ms per replicate, scaled to {R1} "
            f"replicates: {med / calls * R1:.1f} ms per set")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
