#!/usr/bin/env python3
"""Time batch settlement (batch.SettlePlan / batch.settle) on about 10M signals.

Batches: ``c3`` -- the config-3 shape (ragged markets with log-uniform lengths on [1, 4096],
Zipf(1.1) sources), reduced to ``--signals``; ``uniform`` -- the same markets with sources drawn
uniformly.  Every market has a random outcome; a source agrees with it at a rate of its own,
drawn once from [0.3, 0.9].

  (a) SettlePlan.build: the compile, once per batch;
  (b) batch.settle with the long path disabled (one lane walks every chain);
  (c) batch.settle with it enabled, over a grid of ``long_min`` x ``chunk_bits``;
  (d) on a ``--slice``-signal prefix of the uniform batch only: what existed before --
      batch.outcome_update called once per chain step, the flags of every step prepared
      beforehand and not timed.

Every timing is ``--calls`` back-to-back calls between two device synchronises on the host
clock, each call preceded by a reset of the table from a pristine copy (timed on its own, and
part of every variant alike); the variants run interleaved, ``--reps`` times each.  All variants
must leave identical tables.  A grid point is proposed as the default only when each of its
repetitions is more than 4% below every repetition of (b).

The byte model of an apply, every array moved once: n_bits / 8 (the bit stream) +
T * (4 order + 16 start + 8+8 rel + 8+8 conf + 8 t_us + 1+1 present).

    python tools/bench_settle.py [--signals N] [--sources S] [--out measurements/settle.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bayesian-consensus-engine_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_engine import _native as N  # noqa: E402
from bayesian_engine import batch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, the MI355X's specified HBM3E rate
NOW = 1_790_000_000_000_000


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def outcomes_and_probs(off_h, sid_h, S, seed):
    """Random outcomes; prob on the outcome's side of 0.5 at the source's own hit rate."""
    rng = np.random.default_rng(seed)
    M = len(off_h) - 1
    outcome = rng.integers(0, 2, M).astype(np.int8)
    hit_rate = rng.uniform(0.3, 0.9, S)
    market = np.repeat(np.arange(M), np.diff(off_h))
    hit = rng.random(len(sid_h)) < hit_rate[sid_h]
    says_true = hit == (outcome[market] != 0)
    prob = np.where(says_true, rng.uniform(0.5, 1.0, len(sid_h)), rng.uniform(0.0, 0.5, len(sid_h)))
    return outcome, prob


class Table:
    def __init__(self, S, dev, seed=3):
        rng = np.random.default_rng(seed)
        present = (rng.random(S) < 0.8).astype(np.uint8)
        T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        self.pristine = (T(np.where(present, rng.random(S), 0.5)), T(np.where(present, rng.random(S), 0.25)),
                         T(np.where(present, 1_700_000_000_000_000, N.NO_TIMESTAMP).astype(np.int64)), T(present))
        self.live = tuple(x.clone() for x in self.pristine)

    def reset(self):
        for a, b in zip(self.live, self.pristine):
            a.copy_(b)

    def snapshot(self):
        return tuple(x.clone() for x in self.live)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def run_shape(name, off_h, sid_h, S, args, say):
    dev = torch.device("cuda", 0)
    outcome_h, prob_h = outcomes_and_probs(off_h, sid_h, S, seed=17)
    off, sid, prob, outcome = (torch.from_numpy(x).to(dev) for x in (off_h, sid_h, prob_h, outcome_h))
    M, Nsig = len(off_h) - 1, len(sid_h)
    calls = args.calls
    batch.SettlePlan.build(off, sid, prob, outcome, S)  # warm-up: code objects, torch sort workspaces
    tc = [timed(lambda: batch.SettlePlan.build(off, sid, prob, outcome, S)) for _ in range(3)]
    plan = tc[-1][1]
    ld = plan.lens_desc
    say(f"== {name}: {M} markets, {Nsig} signals, {S} sources ({plan.n_touched} touched); chain lengths: longest "
        f"{int(ld[0])}, 10th {int(ld[min(9, len(ld) - 1)])}, median {int(np.median(ld))}; {calls} calls per timing")
    say("(a) compile ms: " + " ".join(f"{t * 1e3:.2f}" for t, _ in tc))
    nbytes = plan.n_bits // 8 + plan.n_touched * 62
    table = Table(S, dev)

    def variant(long_min, chunk_bits):
        def run():
            for _ in range(calls):
                table.reset()
                batch.settle(plan, *table.live, NOW, long_min=long_min, chunk_bits=chunk_bits)
        return run

    def reset_only():
        for _ in range(calls):
            table.reset()

    grid = [(lm, cb) for lm in args.long_min for cb in args.chunk_bits if cb <= lm]
    variants = [("(b) long path off", variant(batch.SETTLE_LONG_OFF, 64))]
    variants += [(f"(c) long_min {lm:>6} chunk_bits {cb:>5}", variant(lm, cb)) for lm, cb in grid]
    ok = True
    base = None
    for label, run in variants:  # warm-up and the result check
        run()
        torch.cuda.synchronize()
        snap = table.snapshot()
        base = base or snap
        ok = ok and same(base, snap)
    say(f"all {len(variants)} variants leave identical tables: {ok}")
    times = {label: [] for label, _ in variants}
    t_reset = []
    for _ in range(max(args.reps, 3)):
        t_reset.append(timed(reset_only)[0] / calls)
        for label, run in variants:
            times[label].append(timed(run)[0] / calls)
    fmt = lambda ts: " ".join(f"{t * 1e3:.3f}" for t in ts)  # noqa: E731
    say(f"table reset alone           ms/call: {fmt(t_reset)}")
    tb = times[variants[0][0]]
    best = None
    for label, _ in variants:
        ts = times[label]
        note = ""
        if label.startswith("(c)"):
            clear = max(ts) < 0.96 * min(tb)
            note = f"   {min(tb) / min(ts):.2f}x of (b) by minima; {'clear of' if clear else 'inside'} (b)'s spread + 4%"
            if clear and (best is None or min(ts) < min(times[best])):
                best = label
        say(f"{label:<40} ms/call: {fmt(ts)}   (min {min(ts) * 1e3:.3f}){note}")
    say(f"best (c) clear of (b) in every repetition: {best or 'none'}")
    say(f"byte model of an apply: {nbytes / 1e6:.2f} MB -> (b) {100 * nbytes / min(tb) / HBM_PEAK:.3f}% of 8 TB/s: "
        f"the chains' dependent fp64 steps, not bytes, set the time")
    return ok, plan, (off_h, sid_h, prob_h, outcome_h)


def run_slice(off_h, sid_h, prob_h, outcome_h, S, args, say):
    """(d): a prefix of whole markets holding about --slice signals, settled by outcome_update looped
    once per chain step against batch.settle."""
    dev = torch.device("cuda", 0)
    m = int(np.searchsorted(off_h, args.slice, side="right")) - 1
    n = int(off_h[m])
    off_h, sid_h, prob_h, outcome_h = off_h[:m + 1], sid_h[:n], prob_h[:n], outcome_h[:m]
    off, sid, prob, outcome = (torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                               for x in (off_h, sid_h, prob_h, outcome_h))
    plan = batch.SettlePlan.build(off, sid, prob, outcome, S)
    steps = int(plan.lens_desc[0])
    # flags of step k: bit0 the source has a k-th signal, bit1 that signal agreed (prepared, not timed)
    order = np.argsort(sid_h, kind="stable")
    bit = ((prob_h >= 0.5) == (outcome_h[np.repeat(np.arange(m), np.diff(off_h))] != 0))[order]
    total = np.bincount(sid_h, minlength=S)
    start = np.concatenate([[0], np.cumsum(total)])
    flags_h = np.zeros((steps, S), np.uint8)
    for k in range(steps):
        live = np.flatnonzero(total > k)
        flags_h[k, live] = 1 | (bit[start[live] + k].astype(np.uint8) << 1)
    flags = torch.from_numpy(flags_h).to(dev)
    table = Table(S, dev)
    calls = args.calls

    def run_loop():
        for _ in range(calls):
            table.reset()
            for k in range(steps):
                batch.outcome_update(*table.live, flags[k], NOW)

    def run_settle():
        for _ in range(calls):
            table.reset()
            batch.settle(plan, *table.live, NOW)

    run_loop()
    torch.cuda.synchronize()
    a = table.snapshot()
    run_settle()
    torch.cuda.synchronize()
    ok = same(a, table.snapshot())
    say(f"== (d) uniform slice: {m} markets, {n} signals, {S} sources, longest chain {steps} steps; "
        f"tables identical: {ok}")
    tl, ts = [], []
    for _ in range(max(args.reps, 3)):
        tl.append(timed(run_loop)[0] / calls)
        ts.append(timed(run_settle)[0] / calls)
    fmt = lambda xs: " ".join(f"{t * 1e3:.3f}" for t in xs)  # noqa: E731
    say(f"(d) outcome_update x {steps} steps   ms/call: {fmt(tl)}   (min {min(tl) * 1e3:.3f})")
    say(f"    batch.settle (defaults)       ms/call: {fmt(ts)}   (min {min(ts) * 1e3:.3f}); "
        f"loop / settle by minima {min(tl) / min(ts):.1f}x (compile not included)")
    return ok


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--signals", type=int, default=10_000_000)
    ap.add_argument("--sources", type=int, default=100_000)
    ap.add_argument("--slice", type=int, default=1_000_000, help="signals of the (d) comparison")
    ap.add_argument("--calls", type=int, default=10, help="calls per timing")
    ap.add_argument("--reps", type=int, default=3, help="interleaved repetitions (>= 3)")
    ap.add_argument("--long-min", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--chunk-bits", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--shapes", default="c3,uniform")
    ap.add_argument("--out", default=os.path.join(ROOT, "measurements", "settle.txt"))
    args = ap.parse_args()
    N.require_gpu()  # a measurement without a GPU fails; there is nothing else to time
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    from bench_extra import make_c3_full

    off_h, sid_h, _, _ = make_c3_full(total=args.signals, S=args.sources)
    ok = True
    for shape in args.shapes.split(","):
        if shape == "c3":
            ok = run_shape("c3 (Zipf 1.1 sources)", off_h, sid_h, args.sources, args, say)[0] and ok
        elif shape == "uniform":
            usid = np.random.default_rng(71).integers(0, args.sources, len(sid_h)).astype(np.int32)
            good, _, data = run_shape("uniform sources", off_h, usid, args.sources, args, say)
            ok = run_slice(*data, args.sources, args, say) and good and ok
        else:
            raise SystemExit(f"unknown shape {shape!r}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
