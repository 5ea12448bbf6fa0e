#!/usr/bin/env python3
"""Time the glob kernels (batch.glob_match / glob_members) and the device route of aggregate_many.

Full shape: ``--markets`` ids ``cAA:sBB:name-NNNNNN`` (AA, BB constant inside a block of 1000 ids)
and ``--groups`` pattern lists of 1..3 patterns that select about 1000 members each:
  1 pattern   ``cAA:sBB:name-XYZ???``                       a literal prefix, fails within 3 bytes
  2 patterns  ``*-XYZ[0-4]??``, ``*:name-UVW[5-9]??``        a leading star: retried at every byte
  3 patterns  ``*-XYZ[0-3]??``, ``?*:name-UVW[4-6]??``, ``c??:s*-RST[7-9]??``
The bitmap of all patterns is P x ceil(M / 64) x 8 bytes; above ``--budget-mb`` the groups are
processed in chunks (stated in the output).

  (a) glob_match over every (pattern, id) pair, the prefix and the star patterns also apart;
  (b) glob_members (count + cumulative sum + fill) over the group slots;
  (c) CrossMarketAggregator.aggregate_many(device_match=True) end to end on the full shape, once;
  (d) on a slice both routes finish (``--slice-lists`` lists over ``--slice-markets`` markets):
      aggregate_many(device_match=False) -- the fnmatch loop of the parent commit -- and
      device_match=True, interleaved, as throughput in (pattern, id) pairs per second.

Every timing is on the host clock between two device synchronises, ``--reps`` interleaved
repetitions.  Byte model of (a): the names once per pattern stripe + the bitmap once.

    python tools/bench_glob.py [--out measurements/glob_match.txt]
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def fmt(ts):
    return " ".join(f"{t * 1e3:.3f}" for t in ts) + f"   (min {min(ts) * 1e3:.3f})"


def make_ids(M):
    return [f"c{(i // 1000) % 16:02d}:s{(i // 1000) % 7:02d}:name-{i:06d}" for i in range(M)]


def make_lists(G, M, seed=3):
    rng = np.random.default_rng(seed)
    blocks = max(M // 1000, 1)
    lists = []
    for g in range(G):
        b = [int(x) for x in rng.integers(0, blocks, 3)]
        k = g % 3
        if k == 0:
            lists.append([f"c{b[0] % 16:02d}:s{b[0] % 7:02d}:name-{b[0]:03d}???"])
        elif k == 1:
            lists.append([f"*-{b[0]:03d}[0-4]??", f"*:name-{b[1]:03d}[5-9]??"])
        else:
            lists.append([f"*-{b[0]:03d}[0-3]??", f"?*:name-{b[1]:03d}[4-6]??", f"c??:s*-{b[2]:03d}[7-9]??"])
    return lists


def run_full(args, say):
    dev = torch.device("cuda", 0)
    M, G, reps = args.markets, args.groups, max(args.reps, 3)
    ids = make_ids(M)
    t_pack, names = timed(lambda: batch.NameTable.from_strings(ids, dev))
    lists = make_lists(G, M)
    flat = [p for pl in lists for p in pl]
    t_comp, globs = timed(lambda: batch.GlobSet.compile(flat))
    nw = (M + 63) // 64
    say(f"== full: {M} ids ({int(names.off_host[-1])} bytes), {G} groups, {len(flat)} patterns ({globs.n} distinct, "
        f"{len(globs.declined)} declined, {globs.prog.size} ops, {globs.n_cls} classes)")
    say(f"NameTable.from_strings (host encode + upload, once per store): {t_pack * 1e3:.1f} ms; "
        f"GlobSet.compile (host): {t_comp * 1e3:.1f} ms")
    per_chunk = max(int(args.budget_mb * (1 << 20) // (nw * 8)), 1)
    n_chunks = -(-globs.n // per_chunk)
    say(f"bitmap: {globs.n} x {nw} words = {globs.n * nw * 8 / 1e6:.1f} MB; budget {args.budget_mb} MB -> "
        f"{n_chunks} chunk(s) of at most {per_chunk} patterns")
    if n_chunks > 1:
        say("the patterns do not fit the budget in one bitmap: (a) and (b) below time the FIRST chunk only")
        lists = lists[:max(per_chunk // 3, 1)]  # at most 3 patterns per group
        flat = [p for pl in lists for p in pl]
        globs = batch.GlobSet.compile(flat)
        G = len(lists)
    bits = torch.empty((globs.n, nw), dtype=torch.int64, device=dev)
    subsets = {"all": globs,
               "prefix (1-pattern groups)": batch.GlobSet.compile([p for pl in lists if len(pl) == 1 for p in pl]),
               "star (2- and 3-pattern groups)": batch.GlobSet.compile([p for pl in lists if len(pl) > 1 for p in pl])}
    for gs in subsets.values():
        batch.glob_match(names, gs, out=bits[:gs.n])  # warm-up
    N.check_faults(dev, "glob_match")
    times = {k: [] for k in subsets}
    for _ in range(reps):
        for k, gs in subsets.items():
            times[k].append(timed(lambda: batch.glob_match(names, gs, out=bits[:gs.n]))[0])
    for k, gs in subsets.items():
        t = min(times[k])
        by = gs.n * nw * 8 + int(names.off_host[-1]) + 8 * M
        say(f"(a) glob_match {k:<32} P={gs.n:<6} ms: {fmt(times[k])}   {gs.n * M / t / 1e9:.1f} G pairs/s; "
            f"{by / 1e6:.1f} MB -> {100 * by / t / HBM_PEAK:.2f}% of 8 TB/s")
    batch.glob_match(names, globs, out=bits)
    rows = torch.tensor(globs.index, dtype=torch.int64, device=dev)
    sg = np.zeros(G + 1, np.int64)
    sg[1:] = np.cumsum([len(pl) for pl in lists])
    batch.glob_members(bits, M, rows, sg)
    tm = [timed(lambda: batch.glob_members(bits, M, rows, sg))[0] for _ in range(reps)]
    goff, members = batch.glob_members(bits, M, rows, sg)
    N.check_faults(dev, "glob_members")
    sizes = (goff[1:] - goff[:-1]).double()
    by = 2 * rows.numel() * nw * 8 + members.numel() * 8
    say(f"(b) glob_members (count + cumsum + fill), {rows.numel()} slots ms: {fmt(tm)}   {members.numel()} members "
        f"(per group mean {float(sizes.mean()):.0f}, min {int(sizes.min())}, max {int(sizes.max())}); "
        f"{by / 1e6:.1f} MB -> {100 * by / min(tm) / HBM_PEAK:.2f}% of 8 TB/s")
    # spot check against fnmatch: three groups
    import fnmatch
    for gi in (0, 1, 2):
        exp = [m for p in lists[gi] for m in range(M) if fnmatch.fnmatchcase(ids[m], p)]
        assert members[int(goff[gi]):int(goff[gi + 1])].cpu().tolist() == exp, gi
    say("groups 0..2 equal the fnmatch loop's member lists")
    del bits
    return ids


def run_store(ids, lists, say, label, reps, routes):
    from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore
    rng = np.random.default_rng(11)
    t0 = time.perf_counter()
    ms = MarketStore()
    cons, conf = rng.random(len(ids)), rng.random(len(ids))
    for i, s in enumerate(ids):
        m = ms.create_market(MarketId(s))
        if i % 5:
            m.consensus_result = {"consensus": float(cons[i]), "confidence": float(conf[i])}
    say(f"== {label}: {len(ids)} markets, {len(lists)} pattern lists, {sum(map(len, lists))} patterns "
        f"(store built in {time.perf_counter() - t0:.1f} s)")
    agg = CrossMarketAggregator(ms)
    pairs = len(ids) * sum(map(len, lists))
    out, times = {}, {r: [] for r in routes}
    if True in routes:
        agg.aggregate_many(lists[:3], device_match=True)  # warm-up: name table, kernels
    for _ in range(reps):
        for r in routes:
            t, out[r] = timed(lambda: agg.aggregate_many(lists, device_match=r))
            times[r].append(t)
    for r in routes:
        say(f"aggregate_many(device_match={r!s:<5}) s: " + " ".join(f"{t:.3f}" for t in times[r]) +
            f"   -> {pairs / min(times[r]) / 1e6:.2f} M pairs/s")
    if len(routes) == 2:
        say(f"identical results on both routes: {out[True] == out[False]}")
        clear = max(times[True]) < 0.96 * min(times[False])
        say(f"host / device by minima {min(times[False]) / min(times[True]):.1f}x; the device route is "
            f"{'clear of' if clear else 'inside'} the host route's spread + 4% in every repetition")
    N.check_faults(torch.device("cuda", 0), "aggregate_many")
    return times


def run_crossover(args, say):
    """(e): where the device route starts to win: 4 pattern lists (8 patterns) over growing stores."""
    from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore
    say("== (e) crossover: 4 pattern lists (8 patterns), 5 interleaved repetitions, ms per aggregate_many call")
    first_clear = None
    for M in (16, 64, 256, 1024, 4096, 16384):
        ms = MarketStore()
        for i, s in enumerate(make_ids(M)):
            ms.create_market(MarketId(s)).consensus_result = {"consensus": (i % 97) / 97.0, "confidence": 0.5}
        agg = CrossMarketAggregator(ms)
        lists = make_lists(4, M, seed=M) + [["c00:*"]]
        lists = lists[:4]
        n_pat = sum(map(len, lists))
        for r in (False, True):
            agg.aggregate_many(lists, device_match=r)
        t = {False: [], True: []}
        for _ in range(5):
            for r in (False, True):
                t[r].append(timed(lambda: agg.aggregate_many(lists, device_match=r))[0])
        clear = max(t[True]) < 0.96 * min(t[False])
        if clear and first_clear is None:
            first_clear = M * n_pat
        if not clear:
            first_clear = None
        say(f"M={M:<6} pairs={M * n_pat:<7} host ms: {fmt(t[False])}   device ms: {fmt(t[True])}   device clear: {clear}")
    say(f"smallest measured size from which the device route is clear in every repetition: {first_clear} pairs")


def run_ab(args):
    """One JSON line for tools/gpu_ab.sh (AB_BENCH): the full shape's match and members times with
    whichever library BCE_LIB names."""
    import json
    dev = torch.device("cuda", 0)
    M = args.markets
    names = batch.NameTable.from_strings(make_ids(M), dev)
    lists = make_lists(args.groups, M)
    globs = batch.GlobSet.compile([p for pl in lists for p in pl])
    pre = batch.GlobSet.compile([p for pl in lists if len(pl) == 1 for p in pl])
    bits = torch.empty((globs.n, (M + 63) // 64), dtype=torch.int64, device=dev)
    batch.glob_match(names, globs, out=bits)
    batch.glob_match(names, pre, out=bits[:pre.n])
    t_pre = min(timed(lambda: batch.glob_match(names, pre, out=bits[:pre.n]))[0] for _ in range(3))
    t_all = min(timed(lambda: batch.glob_match(names, globs, out=bits))[0] for _ in range(3))
    N.check_faults(dev, "glob_match")
    print(json.dumps({"ms_per_step": t_all * 1e3, "roofline": {"avg_launch_ms": t_pre * 1e3}, "lib": N.LIB_PATH,
                      "note": "ms_per_step = glob_match over all patterns, avg_launch_ms = the prefix patterns"}))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--markets", type=int, default=1_000_000)
    ap.add_argument("--groups", type=int, default=10_000)
    ap.add_argument("--budget-mb", type=int, default=4096, help="bitmap budget per chunk")
    ap.add_argument("--slice-markets", type=int, default=20_000)
    ap.add_argument("--slice-lists", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parts", default="full,e2e,slice")
    ap.add_argument("--out", default=os.path.join(ROOT, "measurements", "glob_match.txt"))
    args = ap.parse_args()
    N.require_gpu()  # a measurement without a GPU fails; there is nothing else to time
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    parts = args.parts.split(",")
    if parts == ["ab"]:
        run_ab(args)
        return 0
    ids = None
    if "full" in parts:
        ids = run_full(args, say)
    if "e2e" in parts:
        ids = ids or make_ids(args.markets)
        run_store(ids, make_lists(args.groups, args.markets), say, "(c) full shape end to end, device route", 1, [True])
    if "slice" in parts:
        run_store(make_ids(args.slice_markets), make_lists(args.slice_lists, args.slice_markets), say,
                  "(d) slice, both routes", max(args.reps, 3), [False, True])
    if "crossover" in parts:
        run_crossover(args, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
