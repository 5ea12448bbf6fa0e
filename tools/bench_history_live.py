#!/usr/bin/env python3
"""Time the live consensus history (batch.LivePlan / live_trace / walk_history_live).

Batches: the walk-forward benchmark's ``c3`` (ragged markets with log-uniform lengths on [1, 4096],
Zipf(1.1) sources) and ``uniform`` (the same markets, sources drawn uniformly), every market
resolved with a random outcome.  Market m opens at hour m; its signals arrive spread evenly over a
life of ``--life-hours`` and it resolves 0 to ``--life-hours`` after its last arrival, so dozens of
other markets resolve inside every market's life.

  (a) LivePlan.build: the compile, once per batch (host clock between synchronises);
  (b) batch.live_trace: every prefix state of every chain (HIP events);
  (c) the live kernels alone (walk_history_live with ``states=`` and the length-bin plan built
      beforehand; HIP events), from this library -- the per-run window -- and, with ``--alt-lib``,
      from a library built with -DBCE_LIVE_WINDOW=0, where every read bisects its source's whole
      chain; the two outputs are compared bit for bit;
  (d) on the first markets whose prefix expansion holds at most ``--slice-expanded`` signals: the
      only other route -- the batch expanded into its prefixes (tests/history_live_ref.py, on the
      host, timed apart) through WalkPlan.build_lagged and walk_forward(commit=False) -- against
      LivePlan.build + live_trace + the kernels on the same slice (host clock between
      synchronises), the plan builds included and excluded.  The outputs are compared bit for bit
      in the same run.

The variants of a part run interleaved, ``--reps`` times each; every repetition is printed, with
the minimum and the spread (max / min - 1).

    python tools/bench_history_live.py [--signals N] [--alt-lib PATH] [--out measurements/history_live.txt]
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bayesian-consensus-engine_amd"), ROOT, os.path.join(ROOT, "tools"),
          os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_engine import _native as N  # noqa: E402
from bayesian_engine import batch  # noqa: E402
from bench_settle import Table, outcomes_and_probs, timed  # noqa: E402
from history_live_ref import expand_prefixes  # noqa: E402

HOUR = 3_600_000_000
T0 = 1_790_000_000_000_000
FIELDS = ("consensus", "confidence", "total_weight", "n_unique")


def event_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def line(label, ts):
    best = min(ts)
    return f"{label:<58} ms: " + " ".join(f"{t:.3f}" for t in ts) + f"   (min {best:.3f}, spread " \
        f"{100 * (max(ts) / best - 1):.1f}%)"


def times_of(off_h, life_hours, seed):
    """Arrival time of every signal and resolve time of every market."""
    rng = np.random.default_rng(seed)
    M = len(off_h) - 1
    lens = np.diff(off_h)
    market = np.repeat(np.arange(M), lens)
    k = np.arange(int(off_h[-1])) - off_h[:-1][market]
    life = life_hours * HOUR
    arrival = T0 + market * HOUR + (k * life) // np.maximum(lens[market], 1)
    last = np.where(lens > 0, arrival[np.maximum(off_h[1:] - 1, 0)], T0 + np.arange(M) * HOUR)
    return arrival.astype(np.int64), (last + rng.integers(0, life_hours + 1, M) * HOUR).astype(np.int64)


@contextlib.contextmanager
def library(lib):
    """Route the package's calls through another build of the library."""
    keep = N._lib
    N._lib = lib
    try:
        yield
    finally:
        N._lib = keep


def same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS)


def run_shape(name, off_h, sid_h, S, args, alt, say):
    dev = torch.device("cuda", 0)
    T = batch.to_device(dev)
    outcome_h, prob_h = outcomes_and_probs(off_h, sid_h, S, seed=17)
    arrival_h, resolve_h = times_of(off_h, args.life_hours, 19)
    off, sid, prob, outcome, arrival, resolve = (T(x) for x in (off_h, sid_h, prob_h, outcome_h, arrival_h, resolve_h))
    M, Nsig = len(off_h) - 1, len(sid_h)
    build = lambda: batch.LivePlan.build(off, sid, prob, outcome, S, arrival, resolve)  # noqa: E731
    build()  # warm-up: code objects, torch sort workspaces
    ta = [timed(build) for _ in range(args.reps)]
    plan = ta[-1][1]
    sp = plan.settle
    say(f"== {name}: {M} markets, {Nsig} signals, {S} sources; {sp.n_bits} chain bits, longest chain "
        f"{int(sp.lens_desc[0])}; states {16 * sp.n_bits / 1e6:.1f} MB; {args.calls} calls per event timing")
    say(line("(a) LivePlan.build", [t * 1e3 for t, _ in ta]))
    table = batch.ReliabilityTable(*Table(S, dev).live, [""] * S)
    bins = batch.Plan.build(off_h, dev)
    states = batch.live_trace(plan, table)
    out = batch.HistoryResult.alloc(Nsig, dev)
    kern = lambda: batch.walk_history_live(plan, table, offsets=off, sid=sid, prob=prob, states=states, bins=bins,  # noqa: E731
                                           out=out)
    variants = {"(b) live_trace": lambda: batch.live_trace(plan, table), "(c) live kernels, per-run window": kern}
    ok = True
    kern()
    N.check_faults(dev, "live kernels")
    if alt is not None:
        def kern_alt():
            with library(alt):
                return batch.walk_history_live(plan, table, offsets=off, sid=sid, prob=prob, states=states, bins=bins,
                                               out=out_alt)
        out_alt = batch.HistoryResult.alloc(Nsig, dev)
        kern_alt()
        with library(alt):
            N.check_faults(dev, "live kernels, no window")
        ok = same(out, out_alt)
        say(f"(c) per-run window == whole-chain bisect, bit for bit: {ok}")
        variants["(c) live kernels, whole-chain bisect per read"] = kern_alt
    ts = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            ts[k].append(event_ms(fn, args.calls))
    for k, t in ts.items():
        say(line(k, t))
    best = {k: min(t) for k, t in ts.items()}
    if alt is not None:
        say(f"(c) whole-chain bisect / per-run window, by minima: "
            f"{best['(c) live kernels, whole-chain bisect per read'] / best['(c) live kernels, per-run window']:.2f}x")
    say(f"(a) + (b) + (c) by minima: {min(t for t, _ in ta) * 1e3 + best['(b) live_trace'] + best['(c) live kernels, per-run window']:.3f} ms")
    return ok and run_slice(name, off_h, sid_h, prob_h, outcome_h, arrival_h, resolve_h, S, args, say)


def run_slice(name, off_h, sid_h, prob_h, outcome_h, arrival_h, resolve_h, S, args, say):
    """(d): the expanded lagged walk against the live route on a slice small enough to expand."""
    dev = torch.device("cuda", 0)
    T = batch.to_device(dev)
    lens = np.diff(off_h)
    m = int(np.searchsorted(np.cumsum(lens * (lens + 1) // 2), args.slice_expanded, side="right"))
    if m == 0:
        say(f"== (d) {name} slice: the first market alone expands past --slice-expanded; nothing compared")
        return True
    n = int(off_h[m])
    off_h, sid_h, prob_h, outcome_h = off_h[:m + 1], sid_h[:n], prob_h[:n], outcome_h[:m]
    arrival_h, resolve_h = arrival_h[:n], resolve_h[:m]
    t0 = time.perf_counter()
    xoff, xsid, xprob, xout, fc, rs, point = expand_prefixes(off_h, sid_h, prob_h, outcome_h, arrival_h, resolve_h)
    t_expand = time.perf_counter() - t0
    say(f"== (d) {name} slice: the first {m} markets, {n} signals expand to {len(xsid)} in {len(xoff) - 1} markets "
        f"({len(xsid) / max(n, 1):.1f}x; {t_expand * 1e3:.0f} ms of numpy on the host, not in the timings below)")
    x = tuple(T(a) for a in (xoff, xsid, xprob, xout, fc, rs))
    live = tuple(T(a) for a in (off_h, sid_h, prob_h, outcome_h, arrival_h, resolve_h))
    table = batch.ReliabilityTable(*Table(S, dev).live, [""] * S)
    xbuild = lambda: batch.WalkPlan.build_lagged(*x[:4], S, x[4], x[5])  # noqa: E731
    lbuild = lambda: batch.LivePlan.build(*live[:4], S, live[4], live[5])  # noqa: E731
    xplan, lplan = xbuild(), lbuild()
    xbins, lbins = batch.Plan.build(xoff, dev), batch.Plan.build(off_h, dev)
    xrun = lambda: batch.walk_forward(xplan, table, offsets=x[0], prob=x[2], bins=xbins, validate=False,  # noqa: E731
                                      commit=False)
    lrun = lambda: batch.walk_history_live(lplan, table, offsets=live[0], sid=live[1], prob=live[2], bins=lbins)  # noqa: E731
    res, h = xrun(), lrun()
    N.check_faults(dev, "slice")
    sel = T(np.flatnonzero(point >= 0))
    at = T(point[point >= 0])
    ok = all(torch.equal(getattr(res, f)[sel], getattr(h, f)[at]) for f in FIELDS)
    say(f"(d) live history == expanded lagged walk_forward at the {at.numel()} points, bit for bit: {ok}")
    variants = {"(d) expanded: WalkPlan.build_lagged": xbuild, "(d) expanded: walk_forward(commit=False)": xrun,
                "(d) live: LivePlan.build": lbuild, "(d) live: live_trace + kernels": lrun}
    ts = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            ts[k].append(timed(fn)[0] * 1e3)
    for k, t in ts.items():
        say(line(k, t))
    b = {k: min(t) for k, t in ts.items()}
    xw, lw = b["(d) expanded: walk_forward(commit=False)"], b["(d) live: live_trace + kernels"]
    xb, lb = b["(d) expanded: WalkPlan.build_lagged"], b["(d) live: LivePlan.build"]
    say(f"(d) ratio of minima, expanded / live: {xw / lw:.2f}x without the plan builds, {(xw + xb) / (lw + lb):.2f}x "
        f"with them ({args.reps} interleaved repetitions)")
    return ok


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--signals", type=int, default=10_000_000)
    ap.add_argument("--sources", type=int, default=100_000)
    ap.add_argument("--life-hours", type=int, default=72)
    ap.add_argument("--slice-expanded", type=int, default=20_000_000, help="signals of the (d) expansion, at most")
    ap.add_argument("--calls", type=int, default=3, help="calls per event timing")
    ap.add_argument("--reps", type=int, default=3, help="interleaved repetitions")
    ap.add_argument("--shapes", default="c3,uniform")
    ap.add_argument("--alt-lib", default=None, help="a libbce_hip.so built with -DBCE_LIVE_WINDOW=0")
    ap.add_argument("--out", default=os.path.join(ROOT, "measurements", "history_live.txt"))
    args = ap.parse_args()
    N.require_gpu()  # a measurement without a GPU fails; there is nothing else to time
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    alt = None
    if args.alt_lib:
        alt = C.CDLL(args.alt_lib)
        for fn, (res, argtypes) in N._SIGS.items():
            getattr(alt, fn).restype, getattr(alt, fn).argtypes = res, argtypes
    say(f"alternative library (no per-run window): {args.alt_lib or 'none given'}")

    from bench_extra import make_c3_full

    off_h, sid_h, _, _ = make_c3_full(total=args.signals, S=args.sources)
    ok = True
    for shape in args.shapes.split(","):
        if shape == "c3":
            ok = run_shape("c3 (Zipf 1.1 sources)", off_h, sid_h, args.sources, args, alt, say) and ok
        elif shape == "uniform":
            usid = np.random.default_rng(71).integers(0, args.sources, len(sid_h)).astype(np.int32)
            ok = run_shape("uniform sources", off_h, usid, args.sources, args, alt, say) and ok
        else:
            raise SystemExit(f"unknown shape {shape!r}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
