#!/usr/bin/env python3
"""Time walk-forward consensus (batch.WalkPlan / batch.walk_forward) on about 10M signals.

Batches: the settlement benchmark's ``c3`` (ragged markets with log-uniform lengths on [1, 4096],
Zipf(1.1) sources) and ``uniform`` (the same markets, sources drawn uniformly), every market
resolved with a random outcome, market times one hour apart.

  (a) WalkPlan.build: the compile, once per batch;
  (b) batch.walk_trace: the trace and read kernels, long path off and over a grid of
      ``long_min`` x ``chunk_bits``;
  (c) the whole batch.walk_forward call (trace + read + consensus + commit), the consensus
      length-bin plan built beforehand;
  (d) batch.settle alone on the same plan: the floor the trace is measured against;
  (e) on the first ``--slice-markets`` markets only: the per-market loop that existed before --
      consensus_table + consensus + SettlePlan.build + settle for every market -- against
      WalkPlan.build + walk_forward on the same slice.  Reported as markets per second and not
      extrapolated to the whole batch.

  (f) ``--lag``, in place of (a)-(e): the walk with a forecast and a resolve time per market
      (WalkPlan.build_lagged), once with a lag drawn per market (0 to 72 hours, so the markets
      settle out of forecast order) and once with ``resolve == forecast``, against the ordinary
      plan and walk on the same batch: the build, the bce_walk_lag_queries launch alone, and the
      whole walk_forward call.  Written to measurements/walk_lag.txt.

  (g) ``--scoped-lag``, in place of (a)-(e): the NAMESPACED walk with resolution lag
      (WalkScopePlan.build_lagged) on the same batches, 3 domains assigned at random, against the
      ordinary namespaced plan and walk: the build (``resolve == forecast`` and a lag of 0 to 72
      hours), the whole walk_forward_scoped call, and a K = 6 walk_sweep_scoped against six
      separate walk_forward_scoped(commit=False) + score calls.  Written to
      measurements/walk_scope_lag.txt.

Every timing is ``--calls`` back-to-back calls between two device synchronises on the host
clock, each call that writes the table preceded by a reset from a pristine copy; the variants run
interleaved, ``--reps`` times each.  All (b) variants must give identical tables.

    python tools/bench_walk_forward.py [--signals N] [--sources S] [--out measurements/walk_forward.txt]
    python tools/bench_walk_forward.py --lag [--out measurements/walk_lag.txt]
    python tools/bench_walk_forward.py --scoped-lag [--out measurements/walk_scope_lag.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "bayesian-consensus-engine_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_engine import _native as N  # noqa: E402
from bayesian_engine import batch  # noqa: E402
from bench_settle import Table, outcomes_and_probs, same, timed  # noqa: E402

HOUR = 3_600_000_000
T0 = 1_790_000_000_000_000
fmt = lambda ts: " ".join(f"{t * 1e3:.3f}" for t in ts)  # noqa: E731


def run_shape(name, off_h, sid_h, S, args, say):
    dev = torch.device("cuda", 0)
    outcome_h, prob_h = outcomes_and_probs(off_h, sid_h, S, seed=17)
    off, sid, prob, outcome = (torch.from_numpy(x).to(dev) for x in (off_h, sid_h, prob_h, outcome_h))
    M, Nsig = len(off_h) - 1, len(sid_h)
    mtime = torch.from_numpy(T0 + HOUR * np.arange(M, dtype=np.int64)).to(dev)
    calls = args.calls
    batch.WalkPlan.build(off, sid, prob, outcome, S)  # warm-up: code objects, torch sort workspaces
    ta = [timed(lambda: batch.WalkPlan.build(off, sid, prob, outcome, S)) for _ in range(3)]
    plan = ta[-1][1]
    ts_ = [timed(lambda: batch.SettlePlan.build(off, sid, prob, outcome, S))[0] for _ in range(3)]
    E = plan.pairs.n_entries
    ld = plan.settle.lens_desc
    say(f"== {name}: {M} markets, {Nsig} signals, {S} sources, {E} entries; longest chain {int(ld[0])}, "
        f"median {int(np.median(ld))}; {calls} calls per timing")
    say("(a) WalkPlan.build ms: " + fmt(t for t, _ in ta) + "   of which SettlePlan.build: " + fmt(ts_))
    bins = batch.Plan.build_device(off)
    table = Table(S, dev)
    names = [""] * S

    def rt():
        return batch.ReliabilityTable(*table.live, names)

    def trace(long_min, chunk_bits):
        def run():
            out = None
            for _ in range(calls):
                out = batch.walk_trace(plan, rt(), mtime, long_min=long_min, chunk_bits=chunk_bits)
            return out
        return run

    def whole():
        for _ in range(calls):
            table.reset()
            batch.walk_forward(plan, rt(), mtime, offsets=off, prob=prob, bins=bins, validate=False)

    def settle_only():
        for _ in range(calls):
            table.reset()
            batch.settle(plan.settle, *table.live, T0)

    def reset_only():
        for _ in range(calls):
            table.reset()

    grid = [(lm, cb) for lm in args.long_min for cb in args.chunk_bits if cb <= lm]
    variants = [("(b) trace+read, long path off", trace(batch.SETTLE_LONG_OFF, 64))]
    variants += [(f"(b) trace+read, long_min {lm:>5} chunk_bits {cb:>5}", trace(lm, cb)) for lm, cb in grid]
    ok, base = True, None
    for label, run in variants:  # warm-up and the result check
        wt, exists = run()
        torch.cuda.synchronize()
        snap = (wt.relconf.clone(), wt.bits.clone(), exists.clone())
        base = base or snap
        ok = ok and all(x.view(torch.int64).equal(y.view(torch.int64)) if x.dtype == torch.float64 else x.equal(y)
                        for x, y in zip(base, snap))
    say(f"all {len(variants)} (b) variants give identical tables: {ok}")
    variants += [("(c) walk_forward, whole call (defaults)", whole), ("(d) settle alone (defaults)", settle_only),
                 ("    table reset alone", reset_only)]
    whole()
    settle_only()
    N.check_faults(dev, "bench walk_forward")
    times = {label: [] for label, _ in variants}
    for _ in range(max(args.reps, 3)):
        for label, run in variants:
            times[label].append(timed(run)[0] / calls)
    for label, _ in variants:
        say(f"{label:<50} ms/call: {fmt(times[label])}   (min {min(times[label]) * 1e3:.3f})")
    td = min(times["(d) settle alone (defaults)"]) - min(times["    table reset alone"])
    tb = min(times[f"(b) trace+read, long_min {batch.WALK_LONG_MIN:>5} chunk_bits {batch.WALK_CHUNK_BITS:>5}"]) \
        if (batch.WALK_LONG_MIN, batch.WALK_CHUNK_BITS) in grid else float("nan")
    nbytes = plan.settle.n_bits // 8 + plan.settle.n_touched * 40 + E * (8 + 4 + 16) + E * (16 + 4 + 4 + 4 + 16 + 1)
    say(f"(b) at the defaults / (d) less the reset, by minima: {tb / td:.2f}x; byte model of (b): "
        f"{nbytes / 1e6:.1f} MB -> {100 * nbytes / tb / 8.0e12:.2f}% of 8 TB/s")
    return ok, (off_h, sid_h, prob_h, outcome_h)


def run_lag(name, off_h, sid_h, S, args, say):
    """(f): build_lagged / bce_walk_lag_queries / walk_forward of a lagged plan against the ordinary ones."""
    dev = torch.device("cuda", 0)
    outcome_h, prob_h = outcomes_and_probs(off_h, sid_h, S, seed=17)
    off, sid, prob, outcome = (torch.from_numpy(x).to(dev) for x in (off_h, sid_h, prob_h, outcome_h))
    M, Nsig = len(off_h) - 1, len(sid_h)
    forecast_h = T0 + HOUR * np.arange(M, dtype=np.int64)
    lag_h = HOUR * np.random.default_rng(23).integers(0, 73, M)
    forecast, drawn = torch.from_numpy(forecast_h).to(dev), torch.from_numpy(forecast_h + lag_h).to(dev)
    calls = args.calls
    builds = [("WalkPlan.build", lambda: batch.WalkPlan.build(off, sid, prob, outcome, S)),
              ("build_lagged, resolve == forecast",
               lambda: batch.WalkPlan.build_lagged(off, sid, prob, outcome, S, forecast, forecast)),
              ("build_lagged, lag 0..72 h",
               lambda: batch.WalkPlan.build_lagged(off, sid, prob, outcome, S, forecast, drawn))]
    plans = [run() for _, run in builds]  # warm-up: code objects, torch sort workspaces
    plain, zero, lagged = plans
    E, nb = plain.pairs.n_entries, plain.settle.n_bits
    moved = int((lagged.qpos != plain.qpos).sum())
    say(f"== {name}: {M} markets, {Nsig} signals, {S} sources, {E} entries, {nb} chain bits; {calls} calls per "
        f"timing; the drawn lag moves qpos of {moved} entries")
    same_plan = torch.equal(zero.settle.bits, plain.settle.bits) and all(
        torch.equal(getattr(zero, k), getattr(plain, k)) for k in ("qstart", "qpos", "qentry", "qlast", "slast"))
    say(f"resolve == forecast gives the ordinary plan's arrays: {same_plan}")
    times = {label: [] for label, _ in builds}
    for _ in range(max(args.reps, 3)):
        for label, run in builds:
            times[label].append(timed(run)[0])
    for label, _ in builds:
        say(f"(f) {label:<46} ms: {fmt(times[label])}   (min {min(times[label]) * 1e3:.3f})")
    # the query launch alone, on the arrays of either lagged plan
    L = N.lib()
    market = torch.repeat_interleave(torch.arange(M, dtype=torch.int32, device=dev), off[1:] - off[:-1])
    launches = []
    for label, p in (("resolve == forecast", zero), ("lag 0..72 h", lagged)):
        # the market of every chain bit, restated: the signals by (source, resolve time, market, position)
        t = p.resolve_time_us[market.long()]
        o = torch.sort(t, stable=True).indices
        o = o[torch.sort(sid[o], stable=True).indices]
        bm = market[o].contiguous()
        qpos, qlast, slast = torch.empty_like(p.qpos), torch.empty_like(p.qlast), torch.empty_like(p.slast)

        def launch(p=p, bm=bm, qpos=qpos, qlast=qlast, slast=slast):
            for _ in range(calls):
                N.check(L.bce_walk_lag_queries(E, N.ptr(p.qentry), N.ptr(p.pairs.usid), N.ptr(p.pairs.emarket), E,
                                               N.ptr(p.settle.start), S, N.ptr(bm), nb, N.ptr(p.forecast_time_us),
                                               N.ptr(p.resolve_time_us), M, N.ptr(qpos), N.ptr(qlast), N.ptr(slast),
                                               N.stream(dev)), "bce_walk_lag_queries")
        launch()
        torch.cuda.synchronize()
        same_q = torch.equal(qpos, p.qpos) and torch.equal(qlast, p.qlast) and torch.equal(slast, p.slast)
        launches.append((f"bce_walk_lag_queries alone, {label}", launch, same_q))
    say(f"the launch alone reproduces the plans' queries: {all(x[2] for x in launches)}")
    bins = batch.Plan.build_device(off)
    table = Table(S, dev)
    names = [""] * S

    def whole(p, *mt):
        def run():
            for _ in range(calls):
                table.reset()
                batch.walk_forward(p, batch.ReliabilityTable(*table.live, names), *mt, offsets=off, prob=prob,
                                   bins=bins, validate=False)
        return run

    variants = [(label, run) for label, run, _ in launches]
    variants += [("walk_forward, ordinary plan", whole(plain, forecast)),
                 ("walk_forward, lagged plan, resolve == forecast", whole(zero)),
                 ("walk_forward, lagged plan, lag 0..72 h", whole(lagged))]
    snaps = []
    for label, run in variants[2:]:  # warm-up and the result check
        run()
        torch.cuda.synchronize()
        snaps.append(table.snapshot())
    same_table = same(snaps[0], snaps[1])
    say(f"the ordinary walk and the lagged one with resolve == forecast leave identical tables: {same_table}")
    N.check_faults(dev, "bench walk lag")
    times = {label: [] for label, _ in variants}
    for _ in range(max(args.reps, 3)):
        for label, run in variants:
            times[label].append(timed(run)[0] / calls)
    for label, _ in variants:
        say(f"(f) {label:<46} ms/call: {fmt(times[label])}   (min {min(times[label]) * 1e3:.3f})")
    steps = 1 + int(np.ceil(np.log2(max(nb / max(plain.settle.n_touched, 1), 1) + 1)))
    nbytes = E * (4 + 4 + 4 + 8 + 8 + 4) + E * steps * (4 + 8) + S * (16 + 4 + 8)
    tq = min(times[launches[1][0]])
    say(f"byte model of the launch: {nbytes / 1e6:.1f} MB at about {steps} bisection steps per query -> "
        f"{100 * nbytes / tq / 8.0e12:.2f}% of 8 TB/s")
    return same_plan and same_table and all(x[2] for x in launches)


def run_scoped_lag(name, off_h, sid_h, S, args, say):
    """(g): WalkScopePlan.build_lagged / walk_forward_scoped / walk_sweep_scoped against the ordinary ones."""
    dev = torch.device("cuda", 0)
    D = 3
    outcome_h, prob_h = outcomes_and_probs(off_h, sid_h, S, seed=17)
    M, Nsig = len(off_h) - 1, len(sid_h)
    rng = np.random.default_rng(29)
    md_h = rng.integers(0, D, M).astype(np.int32)
    off, sid, prob, outcome, md = (torch.from_numpy(x).to(dev) for x in (off_h, sid_h, prob_h, outcome_h, md_h))
    forecast_h = T0 + HOUR * np.arange(M, dtype=np.int64)
    lag_h = HOUR * np.random.default_rng(23).integers(0, 73, M)
    forecast, drawn = torch.from_numpy(forecast_h).to(dev), torch.from_numpy(forecast_h + lag_h).to(dev)
    calls = args.calls
    common = (off, sid, prob, outcome, md, S, D)
    builds = [("WalkScopePlan.build", lambda: batch.WalkScopePlan.build(*common, update_global=True)),
              ("build_lagged, resolve == forecast",
               lambda: batch.WalkScopePlan.build_lagged(*common, forecast, forecast, update_global=True)),
              ("build_lagged, lag 0..72 h",
               lambda: batch.WalkScopePlan.build_lagged(*common, forecast, drawn, update_global=True))]
    plain, zero, lagged = [run() for _, run in builds]  # warm-up: code objects, torch sort workspaces
    E, F = plain.pairs.n_entries, plain.dplan.n_entries
    moved = [int((getattr(lagged, q).qlast != getattr(plain, q).qlast).sum()) for q in ("dq", "gq")]
    say(f"== {name}: {M} markets, {Nsig} signals, {S} sources, {D} domains at random; {E} entries, {F} (domain, "
        f"source) chains; {calls} calls per timing; the drawn lag moves qlast of {moved[0]} domain and {moved[1]} "
        f"global queries")
    same_plan = all(torch.equal(getattr(getattr(zero, q), k), getattr(getattr(plain, q), k))
                    for q in ("dq", "gq") for k in ("qstart", "qpos", "qentry", "qlast", "slast")) and \
        all(torch.equal(getattr(zero, sp).bits, getattr(plain, sp).bits) for sp in ("dsettle", "gsettle"))
    say(f"resolve == forecast gives the ordinary plan's arrays: {same_plan}")
    times = {label: [] for label, _ in builds}
    for _ in range(max(args.reps, 3)):
        for label, run in builds:
            times[label].append(timed(run)[0])
    for label, _ in builds:
        say(f"(g) {label:<52} ms: {fmt(times[label])}   (min {min(times[label]) * 1e3:.3f})")
    bins = batch.Plan.build_device(off)
    table = Table(S, dev)
    names = [""] * S
    d, s = np.nonzero(rng.random((D, S)) < 0.5)  # a row for half of the (domain, source) pairs, a fifth without a stamp
    has = (rng.random(len(d)) < 0.8).astype(np.uint8)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    stamps = np.where(has, 1_700_000_000_000_000, N.NO_TIMESTAMP).astype(np.int64)
    domains = batch.PairTable.from_rows(T(d.astype(np.int64)), T(s.astype(np.int32)), T(rng.random(len(d))),
                                        T(rng.random(len(d))), T(stamps), T(has), D, S)

    def rt():
        return batch.ReliabilityTable(*table.live, names)

    def whole(p, *mt):
        def run():
            out = None
            for _ in range(calls):
                table.reset()
                out = batch.walk_forward_scoped(p, domains, rt(), *mt, offsets=off, prob=prob, bins=bins,
                                                validate=False)
            return out
        return run

    hl, mr = [30.0, 5.0, 90.0], [0.1, 0.4]

    def sweep(p, *mt):
        def run():
            for _ in range(calls):
                batch.walk_sweep_scoped(p, domains, rt(), *mt, offsets=off, prob=prob, half_life_days=hl, min_rel=mr,
                                        bins=bins, validate=False)
        return run

    def six(p, *mt):
        def run():
            for _ in range(calls):
                for _ in range(len(hl) * len(mr)):
                    res = batch.walk_forward_scoped(p, domains, rt(), *mt, offsets=off, prob=prob, bins=bins,
                                                    validate=False, commit=False)
                    batch.score_markets(res, off, outcome)
        return run

    variants = [("walk_forward_scoped, ordinary plan", whole(plain, forecast)),
                ("walk_forward_scoped, lagged plan, resolve == forecast", whole(zero)),
                ("walk_forward_scoped, lagged plan, lag 0..72 h", whole(lagged)),
                ("walk_sweep_scoped K = 6, ordinary plan", sweep(plain, forecast)),
                ("six walk_forward_scoped(commit=False) + score, ordinary", six(plain, forecast)),
                ("walk_sweep_scoped K = 6, lagged plan, lag 0..72 h", sweep(lagged)),
                ("six walk_forward_scoped(commit=False) + score, lagged", six(lagged))]
    snaps = []
    for label, run in variants[:2]:  # warm-up and the result check
        res = run()
        torch.cuda.synchronize()
        snaps.append((table.snapshot(), res))
    same_walk = same(snaps[0][0], snaps[1][0]) and \
        snaps[0][1].consensus.view(torch.int64).equal(snaps[1][1].consensus.view(torch.int64)) and \
        snaps[0][1].scope.equal(snaps[1][1].scope) and \
        all(torch.equal(getattr(snaps[0][1].domains, f), getattr(snaps[1][1].domains, f))
            for f in ("poffsets", "psid", "rel", "conf", "t_us", "has"))
    say(f"the ordinary walk and the lagged one with resolve == forecast agree in every consensus, scope, domain row "
        f"and global row: {same_walk}")
    for label, run in variants[2:]:
        run()
    table.reset()
    N.check_faults(dev, "bench walk scope lag")
    times = {label: [] for label, _ in variants}
    for _ in range(max(args.reps, 3)):
        for label, run in variants:
            times[label].append(timed(run)[0] / calls)
    for label, _ in variants:
        say(f"(g) {label:<56} ms/call: {fmt(times[label])}   (min {min(times[label]) * 1e3:.3f})")
    mn = {label: min(t) for label, t in times.items()}
    say(f"lagged (resolve == forecast) / ordinary whole call by minima: "
        f"{mn[variants[1][0]] / mn[variants[0][0]]:.3f}x; six separate / sweep by minima: ordinary "
        f"{mn[variants[4][0]] / mn[variants[3][0]]:.2f}x, lagged {mn[variants[6][0]] / mn[variants[5][0]]:.2f}x")
    return same_plan and same_walk


def run_slice(off_h, sid_h, prob_h, outcome_h, S, args, say):
    """(e): the first --slice-markets markets, the per-market loop against one walk_forward."""
    dev = torch.device("cuda", 0)
    m = min(args.slice_markets, len(off_h) - 1)
    n = int(off_h[m])
    off_h, sid_h, prob_h, outcome_h = off_h[:m + 1], sid_h[:n], prob_h[:n], outcome_h[:m]
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    off, sid, prob, outcome = T(off_h), T(sid_h), T(prob_h), T(outcome_h)
    mtime_h = T0 + HOUR * np.arange(m, dtype=np.int64)
    mtime = T(mtime_h)
    table = Table(S, dev)
    names = [""] * S
    per = []  # the one-market CSRs, prepared and not timed
    for i in range(m):
        a, b = int(off_h[i]), int(off_h[i + 1])
        per.append((T(np.array([0, b - a], np.int64)), sid[a:b], prob[a:b], outcome[i:i + 1], b - a))

    def loop():
        table.reset()
        rt = batch.ReliabilityTable(*table.live, names)
        out = []
        for i, (o1, s1, p1, oc1, ln) in enumerate(per):
            tab = rt.consensus_table(int(mtime_h[i]))
            out.append(batch.consensus(o1, s1, p1, tab, max_len=max(ln, 1), validate=False))
            sp = batch.SettlePlan.build(o1, s1, p1, oc1, S, check=False)
            rt.settle(sp, int(mtime_h[i]))
        return out

    def walk():
        table.reset()
        plan = batch.WalkPlan.build(off, sid, prob, outcome, S, check=False)
        return batch.walk_forward(plan, batch.ReliabilityTable(*table.live, names), mtime, offsets=off, prob=prob,
                                  validate=False)

    lo = loop()
    torch.cuda.synchronize()
    a = table.snapshot()
    cons_loop = torch.stack([r.consensus[0] for r in lo])
    w = walk()
    torch.cuda.synchronize()
    ok = same(a, table.snapshot()) and cons_loop.view(torch.int64).equal(w.consensus.view(torch.int64))
    N.check_faults(dev, "bench walk_forward slice")
    say(f"== (e) uniform slice: the first {m} markets, {n} signals, {S} sources; final tables and every consensus "
        f"identical: {ok}")
    tl, tw = [], []
    for _ in range(max(args.reps, 3)):
        tl.append(timed(loop)[0])
        tw.append(timed(walk)[0])
    say(f"(e) per-market loop (consensus_table + consensus + SettlePlan.build + settle)  s: "
        + " ".join(f"{t:.3f}" for t in tl) + f"   -> {m / min(tl):.0f} markets/s")
    say(f"    WalkPlan.build + walk_forward on the same slice                            s: "
        + " ".join(f"{t:.4f}" for t in tw) + f"   -> {m / min(tw):.0f} markets/s; loop / walk by minima "
        f"{min(tl) / min(tw):.0f}x (this slice only; not extrapolated)")
    return ok


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--signals", type=int, default=10_000_000)
    ap.add_argument("--sources", type=int, default=100_000)
    ap.add_argument("--slice-markets", type=int, default=2000, help="markets of the (e) comparison")
    ap.add_argument("--calls", type=int, default=5, help="calls per timing")
    ap.add_argument("--reps", type=int, default=3, help="interleaved repetitions (>= 3)")
    ap.add_argument("--long-min", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--chunk-bits", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--shapes", default="c3,uniform")
    ap.add_argument("--lag", action="store_true", help="(f): the walk with resolution lag, in place of (a)-(e)")
    ap.add_argument("--scoped-lag", action="store_true",
                    help="(g): the namespaced walk with resolution lag and its sweep, in place of (a)-(e)")
    ap.add_argument("--out", default=None,
                    help="default: measurements/walk_forward.txt (--lag: walk_lag.txt, --scoped-lag: "
                         "walk_scope_lag.txt)")
    args = ap.parse_args()
    if args.lag and args.scoped_lag:
        ap.error("--lag and --scoped-lag are two runs")
    if args.out is None:
        args.out = os.path.join(ROOT, "measurements", "walk_scope_lag.txt" if args.scoped_lag else
                                "walk_lag.txt" if args.lag else "walk_forward.txt")
    N.require_gpu()  # a measurement without a GPU fails; there is nothing else to time
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    from bench_extra import make_c3_full

    off_h, sid_h, _, _ = make_c3_full(total=args.signals, S=args.sources)
    ok = True
    for shape in args.shapes.split(","):
        if (args.lag or args.scoped_lag) and shape in ("c3", "uniform"):
            src = sid_h
            if shape == "uniform":
                src = np.random.default_rng(71).integers(0, args.sources, len(sid_h)).astype(np.int32)
            run = run_scoped_lag if args.scoped_lag else run_lag
            ok = run("c3 (Zipf 1.1 sources)" if shape == "c3" else "uniform sources", off_h, src, args.sources,
                         args, say) and ok
        elif shape == "c3":
            ok = run_shape("c3 (Zipf 1.1 sources)", off_h, sid_h, args.sources, args, say)[0] and ok
        elif shape == "uniform":
            usid = np.random.default_rng(71).integers(0, args.sources, len(sid_h)).astype(np.int32)
            good, data = run_shape("uniform sources", off_h, usid, args.sources, args, say)
            ok = run_slice(*data, args.sources, args, say) and good and ok
        else:
            raise SystemExit(f"unknown shape {shape!r}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
