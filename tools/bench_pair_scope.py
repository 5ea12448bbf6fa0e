#!/usr/bin/env python3
"""Time the market-scope pair table (batch.pair_resolve / consensus_pairs / settle_pairs).

Shapes: ``short`` -- ``--markets`` markets of 32 signals over 10k sources (the config-2 shape);
``ragged`` -- the config-3 shape (log-uniform lengths on [1, 4096], Zipf(1.1) sources over 100k
ranks) reduced to ``--signals``.  Half of a batch's unique (market, source) pairs have a stored row.

  (a) pair_resolve in store mode with decay, and in namespaced mode with both dense scopes;
  (b) the same lookup composed from torch (built here only): torch.searchsorted over the global
      keys ``market * S + sid`` (the key arrays are prepared beforehand and not timed), four
      gathers of the row arrays -- eight more of the two dense scopes in namespaced mode, since
      namespace_resolve wants every scope over one index space -- and the existing
      batch.namespace_resolve over the gathered arrays;
  (c) the whole consensus_pairs step with a prebuilt PairPlan (and length-bin Plan);
  (d) settle_pairs end to end, and its compile (SettlePlan.build over the entry space) alone;
  (e) on a slice only (``--slice-markets`` markets of the short shape in a SQLite file): the routes
      that existed before -- market._batched_consensus's table build (fetch_pairs + the host loop)
      and the per-signal update_reliability(market_id=...) loop -- as throughput, beside
      load_pair_table on the same slice.

Every timing is ``--calls`` back-to-back calls between two device synchronises on the host clock;
(a) and (b) run interleaved, ``--reps`` times each, and must give identical tables.

Byte model of (a), every array moved once: Q * (4 qsid + 4 emarket + 8 lb + 1 matched + 16 relconf
+ 1 scope + 1/8 bits) + P * 4 (psid) + matched * (8 rel + 8 conf + 8 t_us) [+ namespaced: matched *
1 has + Q * 1 has per dense scope, and 24 more per entry that falls back to one].

    python tools/bench_pair_scope.py [--out measurements/pair_scope.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
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
DAY = 86_400_000_000


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def fmt(ts):
    return " ".join(f"{t * 1e3:.3f}" for t in ts) + f"   (min {min(ts) * 1e3:.3f})"


def dense_scope(S, dev, seed, p_has):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rel = torch.rand(S, generator=g, dtype=torch.float64)
    conf = torch.rand(S, generator=g, dtype=torch.float64)
    t = NOW - torch.randint(0, 90 * DAY, (S,), generator=g)
    has = (torch.rand(S, generator=g) < p_has).to(torch.uint8)
    return batch.ScopeTable(rel.to(dev), conf.to(dev), t.to(dev), has.to(dev))


def table_for(plan, dev, seed=5, frac=0.5):
    """A PairTable holding a random ``frac`` of the plan's entries (built on the device)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    E = plan.n_entries
    keep = torch.nonzero((torch.rand(E, generator=g) < frac).to(dev)).flatten()
    P = keep.numel()
    rel = torch.rand(P, generator=g, dtype=torch.float64).to(dev)
    conf = torch.rand(P, generator=g, dtype=torch.float64).to(dev)
    t = (NOW - torch.randint(0, 90 * DAY, (P,), generator=g)).to(dev)
    has = (torch.rand(P, generator=g) < 0.9).to(torch.uint8).to(dev)
    t = torch.where(has.bool(), t, torch.full_like(t, N.NO_TIMESTAMP))
    return batch.PairTable.from_rows(plan.emarket[keep], plan.usid[keep], rel, conf, t, has, plan.n_markets,
                                     plan.n_sources)


def torch_lookup(plan, pairs, tkeys, qkeys, now_us, dom=None, glob=None):
    """(b): searchsorted + gathers + namespace_resolve; returns (table, scope, lb, matched)."""
    P = tkeys.numel()
    lb = torch.searchsorted(tkeys, qkeys)
    at = lb.clamp(max=max(P - 1, 0))
    matched = tkeys[at] == qkeys
    if dom is None and glob is None:  # store mode: a row that exists, whatever its has
        sc0 = batch.ScopeTable(pairs.rel[at], pairs.conf[at], pairs.t_us[at], matched.to(torch.uint8))
        table, scope = batch.namespace_resolve([sc0, None, None], now_us)
        return table, scope, lb, matched
    sc0 = batch.ScopeTable(pairs.rel[at], pairs.conf[at], pairs.t_us[at], pairs.has[at] * matched.to(torch.uint8))
    us = plan.usid.long()
    dense = [None if s is None else batch.ScopeTable(s.rel[us], s.conf[us], s.t_us[us], s.has[us]) for s in (dom, glob)]
    table, scope = batch.namespace_resolve([sc0, *dense], now_us)
    return table, scope, lb, matched


def run_shape(name, off_h, sid_h, S, args, say, cons_kw):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    prob_h = rng.random(len(sid_h))
    off, sid, prob = (torch.from_numpy(x).to(dev) for x in (off_h, sid_h, prob_h))
    M, Nsig = len(off_h) - 1, len(sid_h)
    outcome = torch.from_numpy(rng.integers(0, 2, M).astype(np.int8)).to(dev)
    calls, reps = args.calls, max(args.reps, 3)
    batch.PairPlan.build(off, sid, prob, S)  # warm-up
    tp = [timed(lambda: batch.PairPlan.build(off, sid, prob, S)) for _ in range(3)]
    plan = tp[-1][1]
    pairs = table_for(plan, dev)
    E, P = plan.n_entries, pairs.n_rows
    seg = (pairs.poffsets[1:] - pairs.poffsets[:-1])
    say(f"== {name}: {M} markets, {Nsig} signals, {S} sources; {E} unique pairs ({E / max(M, 1):.1f} per market), "
        f"{P} stored rows (longest segment {int(seg.max())}); {calls} calls per timing, {reps} interleaved repetitions")
    say("PairPlan.build (torch sort + integer work, once per CSR) ms: " + fmt([t for t, _ in tp]))
    dom, glob = dense_scope(S, dev, 7, 0.5), dense_scope(S, dev, 8, 0.7)
    tkeys = (torch.repeat_interleave(torch.arange(M, device=dev), seg, output_size=P) * S + pairs.psid.long())
    qkeys = plan.emarket.long() * S + plan.usid.long()

    def a_store():
        return batch.pair_resolve(plan.uoffsets, plan.usid, pairs, NOW, emarket=plan.emarket)

    def a_ns():
        return batch.pair_resolve(plan.uoffsets, plan.usid, pairs, NOW, mode="namespaced", emarket=plan.emarket,
                                  domain=dom, global_scope=glob)

    def b_store():
        return torch_lookup(plan, pairs, tkeys, qkeys, NOW)

    def b_ns():
        return torch_lookup(plan, pairs, tkeys, qkeys, NOW, dom, glob)

    ra, rb, rna, rnb = a_store(), b_store(), a_ns(), b_ns()
    torch.cuda.synchronize()
    ok = (torch.equal(ra.table.relconf[:E], rb[0].relconf[:E]) and torch.equal(ra.scope, rb[1])
          and torch.equal(ra.lb, rb[2]) and torch.equal(ra.matched.bool(), rb[3])
          and torch.equal(ra.table.bits, rb[0].bits))
    okn = (torch.equal(rna.table.relconf[:E], rnb[0].relconf[:E]) and torch.equal(rna.scope, rnb[1])
           and torch.equal(rna.table.bits, rnb[0].bits))
    N.check_faults(dev, "pair_resolve")
    say(f"(a) and (b) identical: store {ok}, namespaced {okn}")
    n_match = int(ra.matched.sum())
    fell = int(((rna.scope == 1) | (rna.scope == 2)).sum())
    del ra, rb, rna, rnb
    variants = [("(a) pair_resolve store+decay", a_store), ("(b) torch composition store", b_store),
                ("(a) pair_resolve namespaced, 2 scopes", a_ns), ("(b) torch composition namespaced", b_ns)]
    times = {k: [] for k, _ in variants}
    for _ in range(reps):
        for k, fn in variants:
            times[k].append(timed(lambda: [fn() for _ in range(calls)])[0] / calls)
    for k, _ in variants:
        say(f"{k:<42} ms/call: {fmt(times[k])}")
    for a, b in ((variants[0][0], variants[1][0]), (variants[2][0], variants[3][0])):
        clear = max(times[a]) < 0.96 * min(times[b])
        say(f"    (b) / (a) by minima {min(times[b]) / min(times[a]):.2f}x; (a) is "
            f"{'clear of' if clear else 'inside'} (b)'s spread + 4% in every repetition")
    by_store = E * (4 + 4 + 8 + 1 + 16 + 1 + 0.125) + P * 4 + n_match * 24
    by_ns = by_store + n_match + 2 * E + fell * 24
    say(f"byte model of (a): store {by_store / 1e6:.1f} MB -> {100 * by_store / min(times[variants[0][0]]) / HBM_PEAK:.1f}% "
        f"of 8 TB/s; namespaced {by_ns / 1e6:.1f} MB -> {100 * by_ns / min(times[variants[2][0]]) / HBM_PEAK:.1f}% "
        f"({n_match} matched, {fell} entries fall back to a dense scope)")
    # (c) the consensus step
    kw = dict(cons_kw(off_h, dev))
    ck = lambda: batch.consensus_pairs(off, sid, prob, pairs, NOW, plan=plan, validate=False, **kw)  # noqa: E731
    table_only = batch.pair_resolve(plan.uoffsets, plan.usid, pairs, NOW, emarket=plan.emarket).table
    c0 = lambda: batch.consensus(off, plan.esid, prob, table_only, validate=False,  # noqa: E731
                                 **{("plan" if k == "bins" else k): v for k, v in kw.items()})
    ck(), c0()
    tc, t0 = [], []
    for _ in range(reps):
        tc.append(timed(lambda: [ck() for _ in range(calls)])[0] / calls)
        t0.append(timed(lambda: [c0() for _ in range(calls)])[0] / calls)
    N.check_faults(dev, "consensus_pairs")
    say(f"(c) consensus_pairs, prebuilt plan         ms/call: {fmt(tc)}")
    say(f"    batch.consensus alone on the same table ms/call: {fmt(t0)}")
    # (d) settlement
    batch.settle_pairs(plan, pairs, off, prob, outcome, NOW)
    td, tcomp = [], []
    for _ in range(reps):
        td.append(timed(lambda: batch.settle_pairs(plan, pairs, off, prob, outcome, NOW))[0])
        tcomp.append(timed(lambda: batch.SettlePlan.build(off, plan.esid, prob, outcome, n_sources=max(E, 1)))[0])
    new, _ = batch.settle_pairs(plan, pairs, off, prob, outcome, NOW)
    N.check_faults(dev, "settle_pairs")
    say(f"(d) settle_pairs end to end                ms: {fmt(td)}   ({pairs.n_rows} -> {new.n_rows} rows)")
    say(f"    its compile (SettlePlan.build) alone   ms: {fmt(tcomp)}")
    return ok and okn


def run_slice(args, say):
    """(e): the routes of the parent commit on a slice small enough to finish."""
    from bayesian_engine.market import MarketId, MarketStore
    from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore
    rng = np.random.default_rng(41)
    M, S = args.slice_markets, 10_000
    names = [f"s{i:05d}" for i in range(S)]
    with tempfile.TemporaryDirectory() as tmp:
        ns = NamespacedReliabilityStore(os.path.join(tmp, "slice.db"))
        store = ns._store
        ms = MarketStore()
        rows, pairs, signals = [], [], []
        for m in range(M):
            mid = f"mk:{m}"
            market = ms.create_market(MarketId(mid))
            for s in rng.integers(0, S, 32):
                market.add_signal({"sourceId": names[s], "probability": float(rng.random())})
            for sid in sorted({x["sourceId"] for x in market.signals}):
                pairs.append((sid, mid))
                if rng.random() < 0.5:
                    rows.append((sid, mid, float(rng.random()), float(rng.random()), "2026-09-01T00:00:00+00:00"))
            signals += [(x["sourceId"], mid, x["probability"] >= 0.5) for x in market.signals]
        with store._conn:
            store._conn.execute("BEGIN")
            store._conn.executemany("INSERT INTO sources VALUES (?,?,?,?,?)", rows)
        say(f"== (e) slice: {M} markets of 32 signals, {len(pairs)} pairs, {len(rows)} stored rows, SQLite file")

        def host_table():
            from bayesian_engine.timeutil import iso_to_us
            got = store.fetch_pairs(pairs)
            rel, conf, t = np.full(len(pairs), 0.5), np.full(len(pairs), 0.25), np.zeros(len(pairs), np.int64)
            for k, key in enumerate(pairs):
                row = got.get(key)
                if row is not None:
                    rel[k], conf[k], t[k] = row[0], row[1], iso_to_us(row[2])
            return rel

        th = [timed(host_table)[0] for _ in range(3)]
        say(f"(e) fetch_pairs + host loop (_batched_consensus's table build): {fmt(th)} ms -> "
            f"{len(pairs) / min(th) / 1e6:.3f} M pairs/s")
        mids = [f"mk:{m}" for m in range(M)]
        tl = [timed(lambda: store.load_pair_table(mids, names))[0] for _ in range(3)]
        say(f"    load_pair_table on the same slice:                          {fmt(tl)} ms -> "
            f"{len(pairs) / min(tl) / 1e6:.3f} M pairs/s")
        n_upd = min(args.slice_updates, len(signals))
        t0 = time.perf_counter()
        for sid, mid, ok in signals[:n_upd]:
            ns.update_reliability(sid, ok, market_id=mid)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        say(f"(e) update_reliability(market_id=...) per signal: {n_upd} signals in {dt * 1e3:.1f} ms -> "
            f"{n_upd / dt / 1e3:.2f} k signals/s (one repetition: the loop writes the database)")
        ns.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--markets", type=int, default=1_000_000, help="markets of the short shape")
    ap.add_argument("--signals", type=int, default=10_000_000, help="signals of the ragged shape")
    ap.add_argument("--slice-markets", type=int, default=2000)
    ap.add_argument("--slice-updates", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="short,ragged,slice")
    ap.add_argument("--out", default=os.path.join(ROOT, "measurements", "pair_scope.txt"))
    args = ap.parse_args()
    N.require_gpu()  # a measurement without a GPU fails; there is nothing else to time
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    ok = True
    for shape in args.shapes.split(","):
        if shape == "short":
            rng = np.random.default_rng(13)
            off_h = np.arange(0, 32 * args.markets + 1, 32, dtype=np.int64)
            sid_h = rng.integers(0, 10_000, 32 * args.markets).astype(np.int32)
            ok = run_shape("short", off_h, sid_h, 10_000, args, say, lambda o, d: {"max_len": 32}) and ok
        elif shape == "ragged":
            from bench_extra import make_c3_full
            off_h, sid_h = make_c3_full(total=args.signals, S=100_000)[:2]
            ok = run_shape("ragged (log-uniform 1..4096, Zipf 1.1)", off_h, np.ascontiguousarray(sid_h, np.int32),
                           100_000, args, say, lambda o, d: {"bins": batch.Plan.build(o, d)}) and ok
        elif shape == "slice":
            run_slice(args, say)
        else:
            raise SystemExit(f"unknown shape {shape!r}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
