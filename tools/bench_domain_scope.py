#!/usr/bin/env python3
"""Time the per-market domain scope (batch.scope_resolve / consensus_pairs(domains=) /
settle_domains) against the single-domain routes it stands beside.

Shapes: the ``short`` and ``ragged`` shapes of tools/bench_pair_scope.py, each with ``--domains``
(16 and 1024) domains; markets are assigned to domains uniformly and stay in their input order
(NOT sorted by domain).  Half of the batch's unique (market, source) pairs have a market row, half
of its unique (domain, source) pairs a domain row, 70% of the sources a global row.

  (a) scope_resolve: market table + sparse domain table with a domain per market + global;
  (b) pair_resolve NAMESPACED on the same batch with ONE dense domain for all markets: what the
      per-market domain costs over the single-domain kernel (the results differ, the work is the
      comparison);
  (c) the route that existed before: the batch cut into one CSR per domain (cuts, per-domain pair
      tables, plans, length bins and dense domain tables prepared beforehand and not timed), then
      one consensus_pairs(namespaced=True, domain=dense) per domain;
  (d) consensus_pairs(domains=, market_domain=) on the whole batch, prebuilt plan; its consensus
      outputs must equal (c)'s, market for market; timed once more on its own before the cuts of
      (c) are built (the thousands of small buffers of (c) live in the same caching allocator);
  (e) settle_domains end to end, its compile (SettlePlan.build over the (domain, source) entry
      space) alone, and DomainPlan.build.

Every timing is ``--calls`` back-to-back calls between two device synchronises on the host clock;
(a)/(b) and (c)/(d) run interleaved, ``--reps`` times each.

Byte model of (a), every array moved once: Q * (4 qsid + 4 emarket + 8 lb + 1 matched + 8 dlb +
1 dmatched + 16 relconf + 1 scope + 1/8 bits) + M * (8 qoffsets + 8 poffsets + 4 market_domain) +
D * 8 doffsets + P * 4 psid + R * 4 dsid + (market hits + domain hits) * 1 has + chosen rows * 24
+ Q_global * 1 ghas, where Q_global counts the entries that reach the global scope.  The search
probes are not in the model: they re-read psid / dsid words that it counts once.

    python tools/bench_domain_scope.py [--out measurements/domain_scope.txt]
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
from bench_pair_scope import HBM_PEAK, NOW, dense_scope, fmt, table_for, timed  # noqa: E402


def dense_of(domains, d, S, dev):
    """Domain d's rows of the sparse table as the dense ScopeTable the single-domain route takes."""
    a, b = int(domains.poffsets[d]), int(domains.poffsets[d + 1])
    at = domains.psid[a:b].long()
    rel = torch.full((S,), 0.5, dtype=torch.float64, device=dev)
    conf = torch.full((S,), 0.25, dtype=torch.float64, device=dev)
    t = torch.full((S,), N.NO_TIMESTAMP, dtype=torch.int64, device=dev)
    has = torch.zeros(S, dtype=torch.uint8, device=dev)
    rel[at], conf[at], t[at], has[at] = domains.rel[a:b], domains.conf[a:b], domains.t_us[a:b], domains.has[a:b]
    return batch.ScopeTable(rel, conf, t, has)


def cut_per_domain(off_h, sid_h, prob_h, md_h, pairs, domains, S, D, dev, cons_kw):
    """The batch as one CSR per domain, in domain order (stable): per domain the arguments of
    consensus_pairs(namespaced=True, domain=dense).  Also the market permutation."""
    perm = np.argsort(md_h, kind="stable")
    lens = np.diff(off_h)
    poff = pairs.poffsets.cpu().numpy()
    cuts = []
    bounds = np.searchsorted(md_h[perm], np.arange(D + 1))
    for d in range(D):
        mk = perm[bounds[d]:bounds[d + 1]]
        if len(mk) == 0:
            continue
        o = np.zeros(len(mk) + 1, np.int64)
        o[1:] = np.cumsum(lens[mk])
        po = np.zeros(len(mk) + 1, np.int64)
        po[1:] = np.cumsum(poff[mk + 1] - poff[mk])
        # the signals / rows of the domain's markets, market after market
        idx = np.repeat(off_h[mk] - o[:-1], np.diff(o)) + np.arange(o[-1])
        rows = np.repeat(poff[mk] - po[:-1], np.diff(po)) + np.arange(po[-1])
        r = torch.from_numpy(rows).to(dev)
        sub = batch.PairTable(torch.from_numpy(po).to(dev), pairs.psid[r], pairs.rel[r], pairs.conf[r],
                              pairs.t_us[r], pairs.has[r], len(mk), S)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        off, sid, prob = T(o), T(sid_h[idx]), T(prob_h[idx])
        cuts.append(dict(off=off, sid=sid, prob=prob, pairs=sub, plan=batch.PairPlan.build(off, sid, prob, S),
                         dense=dense_of(domains, d, S, dev), kw=dict(cons_kw(o, dev))))
    return cuts, perm


def run_shape(name, off_h, sid_h, S, D, args, say, cons_kw):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    prob_h = rng.random(len(sid_h))
    M, Nsig = len(off_h) - 1, len(sid_h)
    md_h = rng.integers(0, D, M).astype(np.int32)
    off, sid, prob, md = (torch.from_numpy(x).to(dev) for x in (off_h, sid_h, prob_h, md_h))
    outcome = torch.from_numpy(rng.integers(0, 2, M).astype(np.int8)).to(dev)
    calls, reps = args.calls, max(args.reps, 3)
    plan = batch.PairPlan.build(off, sid, prob, S)
    batch.DomainPlan.build(off, sid, md, S, D)  # warm-up
    tdp = [timed(lambda: batch.DomainPlan.build(off, sid, md, S, D)) for _ in range(3)]
    dplan = tdp[-1][1]
    pairs = table_for(plan, dev)
    domains = table_for(dplan, dev, seed=6)
    glob = dense_scope(S, dev, 8, 0.7)
    one_dense = dense_scope(S, dev, 7, 0.5)
    Q, P, R = plan.n_entries, pairs.n_rows, domains.n_rows
    dseg = domains.poffsets[1:] - domains.poffsets[:-1]
    say(f"== {name}, D = {D}: {M} markets, {Nsig} signals, {S} sources; {Q} unique (market, source) pairs, {P} market "
        f"rows; {dplan.n_entries} unique (domain, source) pairs, {R} domain rows (longest segment {int(dseg.max())}); "
        f"{calls} calls per timing, {reps} interleaved repetitions")
    say("DomainPlan.build (torch unique + integer work, once per CSR) ms: " + fmt([t for t, _ in tdp]))

    def a_scope():
        return batch.scope_resolve(plan.uoffsets, plan.usid, pairs, domains, md, NOW, emarket=plan.emarket,
                                   global_scope=glob)

    def b_pair():
        return batch.pair_resolve(plan.uoffsets, plan.usid, pairs, NOW, mode="namespaced", emarket=plan.emarket,
                                  domain=one_dense, global_scope=glob)

    ra, rb = a_scope(), b_pair()
    N.check_faults(dev, "scope_resolve")
    same_market_rows = torch.equal(ra[0], rb.lb) and torch.equal(ra[1], rb.matched)
    scope = ra[5]
    counts = [int((scope == c).sum()) for c in range(4)]
    hits, dhits = int(ra[1].sum()), int(ra[3].sum())
    q_glob = counts[2] + counts[3]
    say(f"(a) and (b) find the same market rows: {same_market_rows}; (a) resolves {counts[0]} entries at market, "
        f"{counts[1]} at domain, {counts[2]} at global scope, {counts[3]} cold")
    del ra, rb
    variants = [("(a) scope_resolve, domain per market", a_scope), ("(b) pair_resolve namespaced, one dense domain", b_pair)]
    times = {k: [] for k, _ in variants}
    for _ in range(reps):
        for k, fn in variants:
            times[k].append(timed(lambda: [fn() for _ in range(calls)])[0] / calls)
    for k, _ in variants:
        say(f"{k:<48} ms/call: {fmt(times[k])}")
    ta, tb = times[variants[0][0]], times[variants[1][0]]
    say(f"    (a) / (b) by minima {min(ta) / min(tb):.2f}x; the ranges {'overlap' if min(ta) <= max(tb) and min(tb) <= max(ta) else 'do not overlap'}")
    by = (Q * (4 + 4 + 8 + 1 + 8 + 1 + 16 + 1 + 0.125) + M * 20 + D * 8 + P * 4 + R * 4 + hits + dhits
          + (counts[0] + counts[1] + counts[2]) * 24 + q_glob)
    say(f"byte model of (a): {by / 1e6:.1f} MB -> {100 * by / min(ta) / HBM_PEAK:.1f}% of 8 TB/s at the best repetition")
    # (c) / (d): the consensus step, cut per domain against one batch
    kw = dict(cons_kw(off_h, dev))

    def d_whole():
        return batch.consensus_pairs(off, sid, prob, pairs, NOW, plan=plan, namespaced=True, domains=domains,
                                     market_domain=md, global_scope=glob, validate=False, **dict(kw))

    d_whole()
    td0 = [timed(lambda: [d_whole() for _ in range(calls)])[0] / calls for _ in range(reps)]
    say(f"(d) alone, before the cuts of (c) exist                 ms/call: {fmt(td0)}")
    cuts, perm = cut_per_domain(off_h, sid_h, prob_h, md_h, pairs, domains, S, D, dev, cons_kw)

    def c_cut():
        return [batch.consensus_pairs(c["off"], c["sid"], c["prob"], c["pairs"], NOW, plan=c["plan"], namespaced=True,
                                      domain=c["dense"], global_scope=glob, validate=False, **dict(c["kw"]))
                for c in cuts]

    rc, rd = c_cut(), d_whole()
    N.check_faults(dev, "consensus_pairs")
    p = torch.from_numpy(perm).to(dev)
    raw = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t  # noqa: E731  -- bit for bit
    same = all(torch.equal(torch.cat([raw(getattr(x.result, k)) for x in rc]), raw(getattr(rd.result, k))[p])
               for k in ("consensus", "confidence", "total_weight", "n_unique"))
    say(f"(c) and (d) identical consensus / confidence / total_weight / n_unique, market for market: {same}")
    del rc, rd
    tc, td = [], []
    for _ in range(reps):
        tc.append(timed(lambda: [c_cut() for _ in range(calls)])[0] / calls)
        td.append(timed(lambda: [d_whole() for _ in range(calls)])[0] / calls)
    say(f"(c) {len(cuts)} x consensus_pairs(domain=dense), prebuilt cuts  ms/call: {fmt(tc)}")
    say(f"(d) consensus_pairs(domains=), prebuilt plan            ms/call: {fmt(td)}")
    clear = max(td) < 0.96 * min(tc)
    say(f"    (c) / (d) by minima {min(tc) / min(td):.2f}x; (d) is {'clear of' if clear else 'inside'} (c)'s spread + 4% "
        "in every repetition")
    del cuts
    # (e) settlement at domain scope
    masked = torch.where(md >= 0, outcome, torch.full_like(outcome, -1))
    F = dplan.n_entries
    batch.settle_domains(dplan, domains, off, prob, outcome, NOW)
    te, tcomp = [], []
    for _ in range(reps):
        te.append(timed(lambda: batch.settle_domains(dplan, domains, off, prob, outcome, NOW))[0])
        tcomp.append(timed(lambda: batch.SettlePlan.build(off, dplan.esid, prob, masked, n_sources=max(F, 1)))[0])
    new, splan = batch.settle_domains(dplan, domains, off, prob, outcome, NOW)
    N.check_faults(dev, "settle_domains")
    say(f"(e) settle_domains end to end                 ms: {fmt(te)}   ({R} -> {new.n_rows} rows, longest chain "
        f"{int(splan.lens_desc[0]) if len(splan.lens_desc) else 0} bits)")
    say(f"    its compile (SettlePlan.build) alone      ms: {fmt(tcomp)}")
    return same and same_market_rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--markets", type=int, default=1_000_000, help="markets of the short shape")
    ap.add_argument("--signals", type=int, default=10_000_000, help="signals of the ragged shape")
    ap.add_argument("--domains", default="16,1024")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="short,ragged")
    ap.add_argument("--out", default=os.path.join(ROOT, "measurements", "domain_scope.txt"))
    args = ap.parse_args()
    N.require_gpu()  # a measurement without a GPU fails; there is nothing else to time
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    ok = True
    for shape in args.shapes.split(","):
        for D in (int(x) for x in args.domains.split(",")):
            if shape == "short":
                rng = np.random.default_rng(13)
                off_h = np.arange(0, 32 * args.markets + 1, 32, dtype=np.int64)
                sid_h = rng.integers(0, 10_000, 32 * args.markets).astype(np.int32)
                ok = run_shape("short", off_h, sid_h, 10_000, D, args, say, lambda o, d: {"max_len": 32}) and ok
            elif shape == "ragged":
                from bench_extra import make_c3_full
                off_h, sid_h = make_c3_full(total=args.signals, S=100_000)[:2]
                ok = run_shape("ragged (log-uniform 1..4096, Zipf 1.1)", np.ascontiguousarray(off_h, np.int64),
                               np.ascontiguousarray(sid_h, np.int32), 100_000, D, args, say,
                               lambda o, d: {"bins": batch.Plan.build(o, d)}) and ok
            else:
                raise SystemExit(f"unknown shape {shape!r}")
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:  # after every shape: a run cut short keeps what it measured
                f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
