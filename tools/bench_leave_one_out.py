#!/usr/bin/env python3
"""Time the leave-one-source-out consensus (batch.leave_one_out, bce_consensus_leave_one_out) with
HIP events, against the only other route to the same numbers: batch.consensus on the batch
expanded into one reduced market per signal.

  (a) ``--markets`` markets of 32 signals, contiguous (max_len=32: one launch);
  (b) a ragged batch of ``--ragged`` markets, lengths log-uniform in 1..4096 with one of 4096
      (a length-bin Plan built beforehand: one launch per bin).

For each shape the kernel runs on the WHOLE batch, the expanded route on a slice of it
(``--slice`` markets of (a), ``--ragged-slice`` of (b): the expanded batch of the whole would not
fit), the expansion done beforehand with torch on the device and not counted; its time is scaled
by (expanded signals of the whole) / (expanded signals of the slice).  On the slice the two
routes' outputs are compared bit for bit before anything is timed.

Every timing is ``--calls`` back-to-back calls between two HIP events on the stream, outputs
allocated beforehand; ``--reps`` repetitions taken in turn over the variants, all printed, with
the minimum and the spread (max / min - 1).  The byte model of DESIGN §4.25: 12 B read and one
16-B row gather per signal, 28 B written per signal, 28 B per market for the full outputs.

    python tools/bench_leave_one_out.py [--markets M] [--slice K] [--out measurements/leave_one_out.txt]
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
FIELDS = ("consensus", "confidence", "total_weight", "n_unique")


def event_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def expanded_sizes(off, sid):
    """int64[N]: the signals of every reduced market (tests/leave_one_out_ref.expand's lengths)."""
    n = sid.numel()
    lens = off[1:] - off[:-1]
    M = lens.numel()
    market = torch.repeat_interleave(torch.arange(M, dtype=torch.int64, device=off.device), lens, output_size=n)
    S = int(sid.max()) + 1 if n else 1
    key = market * S + sid.to(torch.int64)
    _, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    return lens[market] - cnt[inv]


def expand_device(off, sid, prob):
    """The batch of reduced markets, built with torch on the device: market p holds the signals of
    p's market whose sid differs from sid[p], in CSR order."""
    n = sid.numel()
    lens = off[1:] - off[:-1]
    M = lens.numel()
    dev = off.device
    market = torch.repeat_interleave(torch.arange(M, dtype=torch.int64, device=dev), lens, output_size=n)
    per_point = lens[market]  # candidates of every point: its market's signals
    cstart = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(per_point, 0, out=cstart[1:])
    total = int(cstart[-1])
    point = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), per_point, output_size=total)
    cand = torch.arange(total, dtype=torch.int64, device=dev) - cstart[:-1][point] + off[:-1][market][point]
    keep = sid[cand] != sid[point]
    del point
    off2 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(expanded_sizes(off, sid), 0, out=off2[1:])
    cand = cand[keep]
    return off2, sid[cand].contiguous(), prob[cand].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markets", type=int, default=1_000_000)
    ap.add_argument("--slice", type=int, default=65_536)
    ap.add_argument("--ragged", type=int, default=4096)
    ap.add_argument("--ragged-slice", type=int, default=96)
    ap.add_argument("--sources", type=int, default=10_000)
    ap.add_argument("--calls", type=int, default=3)
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
        return off, (T(off), T(rng.integers(0, S, n).astype(np.int32)), T(rng.random(n)))

    def report(label, variants, calls):
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
            say(f"{label} {k}: ms per call: " + " ".join(f"{x:.4f}" for x in t)
                + f"; min {best:.4f} ms, spread {100 * (max(t) / best - 1):.1f}%")
        return {k: min(t) for k, t in ts.items()}

    def shape(label, lens, n_slice, kw_of):
        off_h, csr = make(lens)
        M, n = len(lens), csr[1].numel()
        ex_total = int(expanded_sizes(csr[0], csr[1]).sum())
        out = batch.LeaveOneOutResult.alloc(n, dev, n_markets=M)
        kw = kw_of(off_h)
        # the slice: its first markets (the lengths are in random order)
        a = int(off_h[n_slice])
        off_s = csr[0][:n_slice + 1].contiguous()
        sl = (off_s, csr[1][:a].contiguous(), csr[2][:a].contiguous())
        ex = expand_device(*sl)
        n_ex = ex[1].numel()
        res = batch._alloc(a, n_ex, dev, False, False)
        plan_ex = batch.Plan.build_device(ex[0])

        def expanded():
            return batch.consensus(*ex, table, plan=plan_ex, unique_outputs=False, validate=False, out=res)

        got = batch.leave_one_out(*sl, table, full=False, **kw_of(off_h[:n_slice + 1]))
        ref = expanded()
        same = all(torch.equal(getattr(got, k), getattr(ref, k)) for k in FIELDS)
        say(f"{label}: {M} markets, {n} signals; the expanded batch would hold {ex_total} signals "
            f"({ex_total / max(n, 1):.1f}x); slice of {n_slice} markets: {a} signals expand to {n_ex}; "
            f"leave_one_out == expanded consensus on the slice, bit for bit: {same}")
        best = report(label, {"leave_one_out, whole batch": lambda: batch.leave_one_out(*csr, table, out=out, **kw),
                              "expanded consensus, slice": expanded}, args.calls)
        loo = best["leave_one_out, whole batch"]
        scaled = best["expanded consensus, slice"] * ex_total / max(n_ex, 1)
        model = n * (12 + 16 + 28) + M * 28
        say(f"{label}: leave_one_out {loo:.4f} ms = {n / loo / 1e6:.2f} G signals/s; byte model {model / 1e6:.1f} MB "
            f"= {100 * model / (loo * 1e-3) / HBM:.1f}% of 8 TB/s; expanded route scaled to the whole batch "
            f"{scaled:.2f} ms; ratio expanded / leave_one_out = {scaled / loo:.1f}x")

    shape("(a) markets x 32", np.full(args.markets, 32), args.slice, lambda off_h: dict(max_len=32))
    lens = np.exp(rng.uniform(0.0, np.log(4096.0), args.ragged)).astype(np.int64).clip(1, 4096)
    lens[args.ragged_slice // 2] = 4096
    shape("(b) ragged 1..4096", lens, args.ragged_slice, lambda off_h: dict(plan=batch.Plan.build(off_h, dev)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
