#!/usr/bin/env python3
"""Time the consensus history (batch.consensus_history, bce_consensus_history) with HIP events.

  (a) ``--markets`` markets of 32 signals, contiguous (max_len=32: one launch);
  (b) the same number of markets of 1..32 signals (max_len=32: one launch);
  (c) ``--long`` markets of 4096 signals (one workgroup each, the quadratic walk);
  (d) a ``--slice`` x 32 slice three ways, interleaved: the history kernel, batch.consensus over
      the batch expanded into its prefix markets (compact outputs, the expansion done beforehand),
      and the same with the expansion (a torch gather on the device) inside the timed window --
      the only route to these numbers without the kernel.

Every timing is ``--calls`` back-to-back calls between two HIP events on the stream, outputs
allocated beforehand; ``--reps`` repetitions taken in turn over the variants of a part, all
printed, with the minimum and the spread (max / min - 1).  The byte model of DESIGN §4.23: 12 B
read and one 16-B row gather per signal, 28 B written per signal.  The (d) outputs are compared
bit for bit before anything is timed.

    python tools/bench_history.py [--markets M] [--slice K] [--long L] [--out measurements/history.txt]
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
BYTES_PER_SIGNAL = 12 + 16 + 28


def event_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def expand_device(off, sid, prob):
    """The batch of prefix markets, built with torch on the device (tests/history_ref.expand)."""
    n = sid.numel()
    lens = off[1:] - off[:-1]
    start = torch.repeat_interleave(off[:-1], lens, output_size=n)
    plen = torch.arange(n, dtype=torch.int64, device=off.device) - start + 1
    off2 = torch.zeros(n + 1, dtype=torch.int64, device=off.device)
    torch.cumsum(plen, 0, out=off2[1:])
    total = int(off2[-1])
    idx = (torch.arange(total, dtype=torch.int64, device=off.device)
           - torch.repeat_interleave(off2[:-1], plen, output_size=total)
           + torch.repeat_interleave(start, plen, output_size=total))
    return off2, sid[idx], prob[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markets", type=int, default=1_000_000)
    ap.add_argument("--slice", type=int, default=65_536)
    ap.add_argument("--long", type=int, default=8)
    ap.add_argument("--sources", type=int, default=10_000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    T = batch.to_device(dev)
    S = args.sources
    table = batch.SourceTable.from_arrays(T(rng.uniform(0.1, 1.0, S)), T(rng.random(S)), None)

    def make(lens):
        off = np.zeros(len(lens) + 1, np.int64)
        off[1:] = np.cumsum(lens)
        n = int(off[-1])
        return T(off), T(rng.integers(0, S, n).astype(np.int32)), T(rng.random(n))

    def report(label, variants, n_signals, calls):
        """variants: {name: fn}; the repetitions go round the variants in turn."""
        for fn in variants.values():
            fn()
        N.check_faults(dev, label)
        ts = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                ts[k].append(event_ms(fn, calls))
        for k, t in ts.items():
            best = min(t)
            model = n_signals * BYTES_PER_SIGNAL
            say(f"{label} {k}: {n_signals} signals; ms per call: " + " ".join(f"{x:.4f}" for x in t)
                + f"; min {best:.4f} ms, spread {100 * (max(t) / best - 1):.1f}%; {n_signals / best / 1e6:.2f} "
                f"G points/s; model {model / 1e6:.1f} MB = {100 * model / (best * 1e-3) / HBM:.1f}% of 8 TB/s")
        return {k: min(t) for k, t in ts.items()}

    def history(csr, max_len):
        out = batch.HistoryResult.alloc(csr[1].numel(), dev)
        return lambda: batch.consensus_history(*csr, table, max_len=max_len, out=out)

    M = args.markets
    csr = make(np.full(M, 32))
    report("(a) markets x 32", {"history": history(csr, 32)}, csr[1].numel(), args.calls)
    del csr
    csr = make(rng.integers(1, 33, M))
    report("(b) markets of 1..32", {"history": history(csr, 32)}, csr[1].numel(), args.calls)
    del csr
    csr = make(np.full(args.long, 4096))
    plan = batch.Plan.build(csr[0].cpu().numpy(), dev)
    out = batch.HistoryResult.alloc(csr[1].numel(), dev)
    report(f"(c) {args.long} markets x 4096", {"history": lambda: batch.consensus_history(*csr, table, plan=plan,
                                                                                        out=out)},
           csr[1].numel(), 1)
    del csr, out

    K = args.slice
    csr = make(np.full(K, 32))
    n = csr[1].numel()
    ex = expand_device(*csr)
    n_ex = ex[1].numel()
    res = batch._alloc(n, n_ex, dev, False, False)
    plan_ex = batch.Plan.build_device(ex[0])

    def expanded():
        return batch.consensus(*ex, table, plan=plan_ex, unique_outputs=False, validate=False, out=res)

    def expanded_with_expansion():
        e = expand_device(*csr)
        return batch.consensus(*e, table, plan=plan_ex, unique_outputs=False, validate=False, out=res)

    h = batch.consensus_history(*csr, table, max_len=32)
    r = expanded()
    same = all(torch.equal(getattr(h, k), getattr(r, k))
               for k in ("consensus", "confidence", "total_weight", "n_unique"))
    say(f"(d) {K} x 32 slice: {n} signals expand to {n_ex} ({n_ex / n:.1f}x); history == expanded consensus, bit "
        f"for bit: {same}")
    best = report("(d) slice", {"history": history(csr, 32), "expanded, expansion not timed": expanded,
                                "expanded, expansion timed": expanded_with_expansion}, n, args.calls)
    hk = best["history"]
    say("(d) ratio of minima: expanded / history = "
        f"{best['expanded, expansion not timed'] / hk:.2f}x without the expansion, "
        f"{best['expanded, expansion timed'] / hk:.2f}x with it ({args.reps} interleaved repetitions)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
