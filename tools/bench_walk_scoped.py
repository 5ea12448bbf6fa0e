#!/usr/bin/env python3
"""Time the namespaced walk-forward (batch.WalkScopePlan / batch.walk_forward_scoped) on about 10M
signals.

Batches: the settlement benchmark's ``c3`` (ragged markets with log-uniform lengths on [1, 4096],
Zipf(1.1) sources) and ``uniform`` (the same markets, sources drawn uniformly), every market
resolved with a random outcome, market times one hour apart; 8 domains assigned round-robin, 10% of
the markets without one, ``update_global=True``.  The domain table holds a row for half of the
(domain, source) pairs (a fifth of them with a falsy stamp), the global table for 80% of the
sources; there are no market-scope rows.

  (a) WalkScopePlan.build: the compile, once per batch;
  (b) batch.walk_scope_trace: the raw lookup of the domain start rows, the two traces and the read
      kernel, at the default ``long_min`` / ``chunk_bits``;
  (c) the whole batch.walk_forward_scoped call (trace + read + consensus + commit of both
      families, the domain rows merged into a new table), the consensus length-bin plan built
      beforehand;
  (d) batch.walk_trace / batch.walk_forward on the same batch collapsed to ONE global scope: the
      yardstick for "two families cost about twice one";
  (e) on the first ``--slice-markets`` markets of ``uniform`` only: the per-market loop of the
      batched calls that existed before -- scope_resolve + consensus + settle_domains + settle for
      every market, the one-market CSRs and their PairPlan / DomainPlan prepared beforehand --
      against WalkScopePlan.build + walk_forward_scoped on the same slice, final tables and every
      consensus compared.  Reported as markets per second and not extrapolated.

Every timing is ``--calls`` back-to-back calls between two device synchronises on the host clock,
each call that writes the global table preceded by a reset from a pristine copy; the variants run
interleaved, ``--reps`` times each.

    python tools/bench_walk_scoped.py [--signals N] [--sources S] [--out measurements/walk_scoped.txt]
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
D = 8
fmt = lambda ts: " ".join(f"{t * 1e3:.3f}" for t in ts)  # noqa: E731
PT_FIELDS = ("poffsets", "psid", "rel", "conf", "t_us", "has")


def market_domains(M, seed=23):
    md = (np.arange(M) % D).astype(np.int32)
    md[np.random.default_rng(seed).random(M) < 0.1] = -1
    return md


def domain_table(S, dev, seed=29):
    """A row for half of the (domain, source) pairs, a fifth of them with a falsy stamp."""
    rng = np.random.default_rng(seed)
    d, s = np.nonzero(rng.random((D, S)) < 0.5)
    P = len(d)
    has = (rng.random(P) < 0.8).astype(np.uint8)
    t_us = np.where(has, 1_700_000_000_000_000, N.NO_TIMESTAMP).astype(np.int64)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return batch.PairTable.from_rows(T(d.astype(np.int64)), T(s.astype(np.int32)), T(rng.random(P)), T(rng.random(P)),
                                     T(t_us), T(has), D, S)


def same_pairs(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in PT_FIELDS)


def run_shape(name, off_h, sid_h, S, args, say):
    dev = torch.device("cuda", 0)
    outcome_h, prob_h = outcomes_and_probs(off_h, sid_h, S, seed=17)
    M, Nsig = len(off_h) - 1, len(sid_h)
    md_h = market_domains(M)
    off, sid, prob, outcome, md = (torch.from_numpy(x).to(dev) for x in (off_h, sid_h, prob_h, outcome_h, md_h))
    mtime = torch.from_numpy(T0 + HOUR * np.arange(M, dtype=np.int64)).to(dev)
    calls = args.calls
    build = lambda: batch.WalkScopePlan.build(off, sid, prob, outcome, md, S, D, update_global=True)  # noqa: E731
    build()  # warm-up: code objects, torch sort workspaces
    ta = [timed(build) for _ in range(3)]
    plan = ta[-1][1]
    tw = [timed(lambda: batch.WalkPlan.build(off, sid, prob, outcome, S)) for _ in range(3)]
    wplan = tw[-1][1]
    E, F = plan.pairs.n_entries, plan.dplan.n_entries
    dl, gl = plan.dsettle.lens_desc, plan.gsettle.lens_desc
    say(f"== {name}: {M} markets ({int((md_h < 0).sum())} without a domain), {Nsig} signals, {S} sources, {D} domains; "
        f"{E} entries, {F} (domain, source) chains; longest domain chain {int(dl[0])} (median {int(np.median(dl))}), "
        f"longest global chain {int(gl[0])} (median {int(np.median(gl))}); {calls} calls per timing")
    say("(a) WalkScopePlan.build ms: " + fmt(t for t, _ in ta) + "   WalkPlan.build (one scope) ms: "
        + fmt(t for t, _ in tw))
    bins = batch.Plan.build_device(off)
    table = Table(S, dev)
    domains = domain_table(S, dev)
    names = [""] * S

    def rt():
        return batch.ReliabilityTable(*table.live, names)

    def trace(**kw):
        def run():
            out = None
            for _ in range(calls):
                out = batch.walk_scope_trace(plan, domains, rt(), mtime, **kw)
            return out
        return run

    def whole():
        out = None
        for _ in range(calls):
            table.reset()
            out = batch.walk_forward_scoped(plan, domains, rt(), mtime, offsets=off, prob=prob, bins=bins,
                                            validate=False)
        return out

    def one_trace():
        for _ in range(calls):
            batch.walk_trace(wplan, rt(), mtime)

    def one_whole():
        for _ in range(calls):
            table.reset()
            batch.walk_forward(wplan, rt(), mtime, offsets=off, prob=prob, bins=bins, validate=False)

    def reset_only():
        for _ in range(calls):
            table.reset()

    wt, scope = trace()()
    wt2, scope2 = trace(long_min=1024, chunk_bits=1024)()
    torch.cuda.synchronize()
    ok = wt.relconf.view(torch.int64).equal(wt2.relconf.view(torch.int64)) and scope.equal(scope2) and \
        wt.bits.equal(wt2.bits)
    counts = torch.bincount(scope.to(torch.int64), minlength=4).tolist()
    say(f"defaults and long_min 1024 / chunk_bits 1024 give identical tables: {ok}; entries read at market / domain / "
        f"global / cold: {counts}")
    res = whole()
    one_trace()
    one_whole()
    N.check_faults(dev, "bench walk_scoped")
    say(f"domain table: {domains.n_rows} rows before, {res.domains.n_rows} after the commit")
    variants = [("(b) lookup + two traces + read (defaults)", trace()), ("(c) walk_forward_scoped, whole call", whole),
                ("(d) one scope: walk_trace", one_trace), ("(d) one scope: walk_forward, whole call", one_whole),
                ("    table reset alone", reset_only)]
    times = {label: [] for label, _ in variants}
    for _ in range(max(args.reps, 3)):
        for label, run in variants:
            times[label].append(timed(run)[0] / calls)
    for label, _ in variants:
        say(f"{label:<46} ms/call: {fmt(times[label])}   (min {min(times[label]) * 1e3:.3f})")
    mn = {label: min(t) for label, t in times.items()}
    tb, tc = mn["(b) lookup + two traces + read (defaults)"], mn["(c) walk_forward_scoped, whole call"]
    db, dc = mn["(d) one scope: walk_trace"], mn["(d) one scope: walk_forward, whole call"]
    say(f"(b) / (d) trace+read by minima: {tb / db:.2f}x; (c) / (d) whole call: {tc / dc:.2f}x")
    # every array moved once: the raw lookup of the F start rows, two traces, the read
    Qd = int(plan.dq.qpos.numel())
    lookup = F * (4 + 4 + 8 + 1 + 8 + 8 + 8 + 1) + F * 25
    traces = sum(sp.n_bits // 8 + sp.n_touched * 40 for sp in (plan.dsettle, plan.gsettle)) + (Qd + E) * (8 + 4 + 16)
    read = E * (4 + 4 + 4 + 4 + 4 + 16 + 16 + 16 + 1)
    say(f"byte model of (b): lookup {lookup / 1e6:.1f} MB + traces {traces / 1e6:.1f} MB + read {read / 1e6:.1f} MB "
        f"(coalesced per-entry arrays; the start-row gathers by dentry / usid and the market times come on top) = "
        f"{(lookup + traces + read) / 1e6:.1f} MB -> {100 * (lookup + traces + read) / tb / 8.0e12:.2f}% of 8 TB/s")
    return ok, (off_h, sid_h, prob_h, outcome_h, md_h)


def run_slice(off_h, sid_h, prob_h, outcome_h, md_h, S, args, say):
    """(e): the first --slice-markets markets, the per-market loop against one walk_forward_scoped."""
    dev = torch.device("cuda", 0)
    m = min(args.slice_markets, len(off_h) - 1)
    n = int(off_h[m])
    off_h, sid_h, prob_h, outcome_h, md_h = off_h[:m + 1], sid_h[:n], prob_h[:n], outcome_h[:m], md_h[:m]
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    off, sid, prob, outcome, md = T(off_h), T(sid_h), T(prob_h), T(outcome_h), T(md_h)
    mtime_h = T0 + HOUR * np.arange(m, dtype=np.int64)
    mtime = T(mtime_h)
    table = Table(S, dev)
    domains = domain_table(S, dev)
    names = [""] * S
    per = []  # the one-market CSRs and their integer plans, prepared and not timed
    for i in range(m):
        a, b = int(off_h[i]), int(off_h[i + 1])
        o1, s1, p1 = T(np.array([0, b - a], np.int64)), sid[a:b].contiguous(), prob[a:b].contiguous()
        per.append((o1, s1, p1, outcome[i:i + 1], md[i:i + 1], batch.PairPlan.build(o1, s1, p1, S),
                    batch.DomainPlan.build(o1, s1, md[i:i + 1], S, D) if md_h[i] >= 0 else None, b - a))

    def loop():
        table.reset()
        dom = domains
        rel, conf, t_us, present = table.live
        glob = batch.ScopeTable(rel, conf, t_us, present)
        out = []
        for i, (o1, s1, p1, oc1, md1, pp, dp, ln) in enumerate(per):
            now = int(mtime_h[i])
            *_, tab, _ = batch.scope_resolve(pp.uoffsets, pp.usid, None, dom, md1, now, emarket=pp.emarket,
                                             global_scope=glob, index=False)
            out.append(batch.consensus(o1, pp.esid, p1, tab, max_len=max(ln, 1), validate=False))
            if dp is not None:
                dom, _ = batch.settle_domains(dp, dom, o1, p1, oc1, now)
            sp = batch.SettlePlan.build(o1, s1, p1, oc1, S, check=False)  # update_global: every market
            batch.settle(sp, rel, conf, t_us, present, now)
        return out, dom

    def walk():
        table.reset()
        plan = batch.WalkScopePlan.build(off, sid, prob, outcome, md, S, D, update_global=True, check=False)
        return batch.walk_forward_scoped(plan, domains, batch.ReliabilityTable(*table.live, names), mtime, offsets=off,
                                         prob=prob, validate=False)

    lo, ldom = loop()
    torch.cuda.synchronize()
    a = table.snapshot()
    cons_loop = torch.stack([r.consensus[0] for r in lo])
    w = walk()
    torch.cuda.synchronize()
    ok = same(a, table.snapshot()) and same_pairs(ldom, w.domains) and \
        cons_loop.view(torch.int64).equal(w.consensus.view(torch.int64))
    N.check_faults(dev, "bench walk_scoped slice")
    say(f"== (e) uniform slice: the first {m} markets, {n} signals, {S} sources; final global and domain tables and "
        f"every consensus identical: {ok}")
    tl, tw = [], []
    for _ in range(max(args.reps, 3)):
        tl.append(timed(loop)[0])
        tw.append(timed(walk)[0])
    say("(e) per-market loop (scope_resolve + consensus + settle_domains + settle)  s: "
        + " ".join(f"{t:.3f}" for t in tl) + f"   -> {m / min(tl):.0f} markets/s")
    say("    WalkScopePlan.build + walk_forward_scoped on the same slice           s: "
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
    ap.add_argument("--shapes", default="c3,uniform")
    ap.add_argument("--out", default=os.path.join(ROOT, "measurements", "walk_scoped.txt"))
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
