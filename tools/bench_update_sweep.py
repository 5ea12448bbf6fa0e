#!/usr/bin/env python3
"""Time the update-rule grid trace (bce_settle_trace_grid) against K single-rule traces, with HIP
events, on a C3-like walk plan: ``--signals`` signals in markets of log-uniform length on
[1, 4096], Zipf(1.1) sources, every market resolved (the head sources have chains of hundreds of
thousands of bits: the long path carries most of the work).

  (a) one bce_settle_trace_grid call at K = 4, 16, 64 rules, the steps spread evenly over each
      range of ``--step-ranges``: by default [0.004, 0.256] (pin runs of 251 down to 5 bits: the
      small steps all but never pin inside a 256-bit chunk of random bits, so the first worker of
      a chain walks nearly all of it) and [0.1, 0.352] (pin runs of 11 down to 4, the reference's
      own at the slow end), so the rules sync at different run lengths and the lanes of a chunk
      diverge;
  (b) K back-to-back bce_settle_trace calls into the K slices of the same buffer -- the only
      route to a K-rule trace without the kernel.  Their cost does not depend on the step, so
      the compiled-in rule stands for every rule.  ``--baseline-lib`` names a libbce_hip.so built
      from the commit before the grid trace; without it the current library's own
      bce_settle_trace is timed (the same device code).

Every timing is ``--calls`` back-to-back calls between two HIP events on the stream, buffers and
the step arrays allocated beforehand; ``--reps`` repetitions taken in turn over (a) and (b) at
one K, all printed, with the minimum and the spread (max / min - 1).  Before anything is timed,
slice k of (a) at the reference's own rule is compared bit for bit with (b)'s trace.

    python tools/bench_update_sweep.py [--signals N] [--baseline-lib PATH] [--out measurements/update_sweep.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
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
from bayesian_engine.config import DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY  # noqa: E402


def event_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def c3_like(total, S, seed):
    """The C3 law: log-uniform market lengths on [1, 4096], Zipf(1.1) sources."""
    rng = np.random.default_rng(seed)
    lens = np.floor(np.exp(rng.uniform(0, np.log(4097), size=total // 300 + 10))).astype(np.int64)
    cs = np.cumsum(lens)
    M = int(np.searchsorted(cs, total) + 1)
    lens = lens[:M]
    lens[-1] -= int(cs[M - 1] - total)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    z = rng.zipf(1.1, size=total)
    bad = np.nonzero(z > S)[0]
    while bad.size:
        z[bad] = rng.zipf(1.1, size=bad.size)
        bad = bad[z[bad] > S]
    sid = rng.permutation(S).astype(np.int32)[z - 1]
    return off, sid, rng.random(total), rng.integers(0, 2, M).astype(np.int8), rng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--signals", type=int, default=3_000_000)
    ap.add_argument("--sources", type=int, default=1_000_000)
    ap.add_argument("--points", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--step-ranges", nargs="+", default=["0.004:0.256", "0.1:0.352"])
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    T = batch.to_device(dev)
    L = N.require_gpu()
    base = L
    if args.baseline_lib:
        base = C.CDLL(args.baseline_lib)
        base.bce_settle_trace.restype, base.bce_settle_trace.argtypes = N._SIGS["bce_settle_trace"]
    off, sid, prob, outcome, rng = c3_like(args.signals, args.sources, 5)
    S = args.sources
    plan = batch.WalkPlan.build(T(off), T(sid), T(prob), T(outcome), S)
    rel, conf = T(rng.uniform(0.1, 1.0, S)), T(rng.random(S))
    present = T((rng.random(S) < 0.9).astype(np.uint8))
    sp, q, E = plan.settle, plan.queries, plan.pairs.n_entries
    n_long, chunk_start, n_chunks = sp.chunks(batch.SETTLE_LONG_MIN, batch.SETTLE_CHUNK_BITS)
    st = N.stream(dev)
    say(f"plan: {args.signals} signals, {len(off) - 1} markets, {S} sources, {sp.n_touched} touched chains "
        f"({n_long} long, {n_chunks} chunks of {batch.SETTLE_CHUNK_BITS} bits, longest {int(sp.lens_desc[0])} bits), "
        f"{E} entries; baseline library: {args.baseline_lib or 'the current one'}")
    head = (N.ptr(sp.bits), sp.n_bits, N.ptr(sp.start), N.ptr(sp.order), sp.n_touched, n_long, N.ptr(chunk_start),
            n_chunks, batch.SETTLE_CHUNK_BITS, S, N.ptr(rel), N.ptr(conf), N.ptr(present), DEFAULT_RELIABILITY,
            DEFAULT_CONFIDENCE, N.ptr(q.qstart), N.ptr(q.qpos), N.ptr(q.qentry), E)
    Kmax = max(args.points)
    trace = torch.empty((Kmax, E, 2), dtype=torch.float64, device=dev)
    trace_b = torch.empty((Kmax, E, 2), dtype=torch.float64, device=dev)

    def single(k):
        N.check(base.bce_settle_trace(*head, N.ptr(trace_b[k]), st), "bce_settle_trace")

    def grid_fn(K, step, sync):
        return lambda: N.check(L.bce_settle_trace_grid(*head, N.ptr(step), N.ptr(sync), K, N.ptr(trace), None, st),
                               "bce_settle_trace_grid")

    # slice 0 under the reference's own rule == the single-rule trace, on the rows a trace writes
    d, s = batch.update_steps([0.15, 0.05], 0.10)
    grid_fn(2, T(d), T(s))()
    single(0)
    N.check_faults(dev, "identity")
    w = plan.qlast >= 0
    say(f"grid slice at (0.15, 0.10) == bce_settle_trace, bit for bit, on the {int(w.sum())} written rows: "
        f"{torch.equal(trace[0][w].view(torch.int64), trace_b[0][w].view(torch.int64))}")

    for rng_text, K in ((r, K) for r in args.step_ranges for K in args.points):
        lo, hi = (float(x) for x in rng_text.split(":"))
        d, s = batch.update_steps([lo + (hi - lo) * k / max(K - 1, 1) for k in range(K)], 10.0)
        say(f"steps [{lo}, {hi}], K={K}: pin runs {int(s.max())} .. {int(s.min())} bits")
        variants = {"(a) grid, 1 call": grid_fn(K, T(d), T(s)),
                    f"(b) {K} single-rule calls": lambda K=K: [single(k) for k in range(K)]}
        for fn in variants.values():
            fn()
        N.check_faults(dev, f"K={K}")
        ts = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                ts[k].append(event_ms(fn, args.calls))
        for k, t in ts.items():
            best = min(t)
            say(f"K={K} {k}: ms per K-rule trace: " + " ".join(f"{x:.3f}" for x in t)
                + f"; min {best:.3f} ms, spread {100 * (max(t) / best - 1):.1f}%; {best / K:.3f} ms per rule; "
                f"{K * E * 16 / best / 1e6:.1f} GB/s of trace written")
        a, b = (min(t) for t in ts.values())
        say(f"K={K} ratio of minima: (b) / (a) = {b / a:.2f}x ({args.reps} interleaved repetitions)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
