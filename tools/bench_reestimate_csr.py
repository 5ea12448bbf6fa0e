#!/usr/bin/env python3
"""Time one round of CSR re-estimation two ways, on about 10M signals.

Batches: ``c3`` -- the config-3 shape (ragged markets with log-uniform lengths on [1, 4096],
Zipf(1.1) sources), reduced to ``--signals``; ``short`` -- the same sources over markets of
1..96 signals (the shape the 64-market tile of the consensus kernel keeps every lane busy on).

  (a) batch.reestimate_csr on a compiled ReestimateCsrPlan (the compile is timed separately);
  (b) the loop a caller had to write before: per round SourceTable.from_arrays, batch.consensus
      with a prebuilt Plan (exact mode), the consensus vote, batch.agreement_stats and the
      weights in torch.

The two are run interleaved, ``--reps`` times each, ``--iters`` rounds per timing; the host clock
brackets work that ends in a device synchronise.  Both must end on the same weights.  Each stage
is also timed on its own (``--iters`` back-to-back calls between two synchronises).  The byte
model of (a) is what a round has to move if every array is read or written exactly once:

  consensus   E * (4 usid + 8 avg) + S * 8 w + M * (8 uoffsets + 1 bad + 8 cons + 1 null + 1 outcome)
  agreement   E * (4 usid + 4 votes + 4 emarket) + M * 1 outcome + S * 16 counts
  weights     S * (8 correct + 8 total + 8 w)

    python tools/bench_reestimate_csr.py [--signals N] [--sources S] [--out measurements/reestimate_csr.txt]
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


def consensus_bytes(E: int, M: int, S: int) -> int:
    return E * 12 + S * 8 + M * 19


def agreement_bytes(E: int, M: int, S: int) -> int:
    return E * 12 + M + S * 16


def model_bytes(E: int, M: int, S: int) -> int:
    return consensus_bytes(E, M, S) + agreement_bytes(E, M, S) + S * 24


def make_short(total: int, S: int):
    """Markets of 1..96 signals, Zipf(1.1) sources over S ranks (redrawn past S), uniform prob."""
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 97, size=total // 48 + 1).astype(np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    z = rng.zipf(1.1, size=n)
    bad = np.nonzero(z > S)[0]
    while bad.size:
        z[bad] = rng.zipf(1.1, size=bad.size)
        bad = bad[z[bad] > S]
    sid = np.random.default_rng(33).permutation(S).astype(np.int32)[z - 1]
    return off, sid, rng.random(n)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def run_shape(name, off_h, sid_h, prob_h, S, args, say):
    M, Nsig = len(off_h) - 1, len(sid_h)
    dev = torch.device("cuda", 0)
    off, sid, prob = (torch.from_numpy(x).to(dev) for x in (off_h, sid_h, prob_h))
    it = args.iters
    say(f"== {name}: {M} markets, {Nsig} signals, {S} sources, longest market {int(np.diff(off_h).max())} "
        f"signals; {it} rounds per timing, w0 = 0.5")
    batch.ReestimateCsrPlan.build(off, sid, prob, S)  # warm-up: code objects, torch sort workspaces
    t_compile, plan = timed(lambda: batch.ReestimateCsrPlan.build(off, sid, prob, S))
    E = plan.n_entries
    seg = plan.uoffsets[1:] - plan.uoffsets[:-1]
    say(f"compile (once per batch): {t_compile * 1e3:.2f} ms -> {E} entries ({E / Nsig:.3f} per signal), "
        f"longest market {int(seg.max())} entries")

    cplan = batch.Plan.build(off_h, dev)
    conf = torch.full((S,), 0.25, dtype=torch.float64, device=dev)
    res = batch._alloc(M, Nsig, dev, True, True)
    empty = off[1:] == off[:-1]
    correct32 = torch.zeros(S, dtype=torch.int32, device=dev)
    total32 = torch.zeros(S, dtype=torch.int32, device=dev)

    def b_table(w):
        return batch.SourceTable.from_arrays(w, conf, None)

    def b_consensus(table):
        return batch.consensus(off, sid, prob, table, plan=cplan, out=res)

    def b_vote(r):
        skip = empty | (r.total_weight == 0) | (r.err_idx >= 0)
        return torch.where(skip, -1, (r.consensus >= 0.5).to(torch.int8)).to(torch.int8)

    def b_agreement(outcome):
        correct32.zero_()
        total32.zero_()
        batch.agreement_stats(off, sid, prob, outcome, S, correct32, total32)

    def b_weights():
        return torch.where(total32 > 0, correct32.to(torch.float64) / total32.clamp(min=1).to(torch.float64), 0.5)

    def run_a():
        return batch.reestimate_csr(plan, it).w

    def run_b():
        w = torch.full((S,), 0.5, dtype=torch.float64, device=dev)
        for _ in range(it):
            b_agreement(b_vote(b_consensus(b_table(w))))
            w = b_weights()
        return w

    wa, wb = run_a(), run_b()  # warm-up of both, and the result check
    torch.cuda.synchronize()
    same = bool(torch.equal(wa, wb))
    say(f"weights after {it} rounds identical between (a) and (b): {same}")
    ta, tb = [], []
    for _ in range(max(args.reps, 3)):
        ta.append(timed(run_a)[0] / it)
        tb.append(timed(run_b)[0] / it)
    fmt = lambda ts: " ".join(f"{t * 1e3:.3f}" for t in ts)  # noqa: E731
    say(f"(a) reestimate_csr           ms/round: {fmt(ta)}   (min {min(ta) * 1e3:.3f})")
    say(f"(b) consensus+agreement loop ms/round: {fmt(tb)}   (min {min(tb) * 1e3:.3f})")
    apart = max(ta) < min(tb) or max(tb) < min(ta)
    say(f"(b)/(a) by minima: {min(tb) / min(ta):.2f}x; ranges {'do not overlap' if apart else 'overlap'}")
    nbytes = model_bytes(E, M, S)
    say(f"byte model of (a): {nbytes / 1e6:.1f} MB per round -> {nbytes / min(ta) / 1e9:.1f} GB/s = "
        f"{100 * nbytes / min(ta) / HBM_PEAK:.2f}% of 8 TB/s (whole round, launches included)")

    # stages on their own
    L = N.lib()
    st = N.stream(dev)
    w = torch.full((S,), 0.5, dtype=torch.float64, device=dev)
    c64 = torch.zeros(S, dtype=torch.int64, device=dev)
    t64 = torch.zeros(S, dtype=torch.int64, device=dev)
    cons, nul, outc = batch.reestimate_csr_step(plan, w, c64, t64)

    def rep(fn):
        fn()
        return timed(lambda: [fn() for _ in range(it)])[0] / it

    t_cons = rep(lambda: L.bce_reestimate_csr_consensus(
        N.ptr(plan.uoffsets), M, N.ptr(plan.usid), N.ptr(plan.avg), N.ptr(plan.bad), None, N.ptr(w), S,
        N.ptr(cons), N.ptr(nul), N.ptr(outc), st))
    t_agree = rep(lambda: L.bce_reestimate_csr_agreement(
        E, N.ptr(plan.usid), N.ptr(plan.votes), N.ptr(plan.emarket), N.ptr(outc), M, S, N.ptr(c64), N.ptr(t64), st))
    t_w = rep(lambda: batch.reestimate_csr_weights(c64, t64, w.clone()))
    cb, ab = consensus_bytes(E, M, S), agreement_bytes(E, M, S)
    say(f"(a) stages, ms: consensus {t_cons * 1e3:.3f} ({100 * cb / t_cons / HBM_PEAK:.2f}% of 8 TB/s on "
        f"{cb / 1e6:.1f} MB), agreement {t_agree * 1e3:.3f} ({100 * ab / t_agree / HBM_PEAK:.2f}% on {ab / 1e6:.1f} MB), "
        f"weights {t_w * 1e3:.3f}")
    w.fill_(0.5)
    table = b_table(w)
    r = b_consensus(table)
    outcome = b_vote(r)
    say(f"(b) stages, ms: table pack {rep(lambda: b_table(w)) * 1e3:.3f}, consensus "
        f"{rep(lambda: b_consensus(table)) * 1e3:.3f}, vote {rep(lambda: b_vote(r)) * 1e3:.3f}, agreement_stats "
        f"{rep(lambda: b_agreement(outcome)) * 1e3:.3f}, weights {rep(b_weights) * 1e3:.3f}")
    return same


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--signals", type=int, default=10_000_000)
    ap.add_argument("--sources", type=int, default=100_000)
    ap.add_argument("--iters", type=int, default=10, help="rounds per timing")
    ap.add_argument("--reps", type=int, default=3, help="interleaved repetitions (>= 3)")
    ap.add_argument("--shapes", default="c3,short")
    ap.add_argument("--out", default=os.path.join(ROOT, "measurements", "reestimate_csr.txt"))
    args = ap.parse_args()
    N.require_gpu()  # a measurement without a GPU fails; there is nothing else to time
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    ok = True
    for shape in args.shapes.split(","):
        if shape == "c3":
            from bench_extra import make_c3_full

            off_h, sid_h, prob_h, _ = make_c3_full(total=args.signals, S=args.sources)
        elif shape == "short":
            off_h, sid_h, prob_h = make_short(args.signals, args.sources)
        else:
            raise SystemExit(f"unknown shape {shape!r}")
        ok = run_shape(shape, off_h, sid_h, prob_h, args.sources, args, say) and ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
