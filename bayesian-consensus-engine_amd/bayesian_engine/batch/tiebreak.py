"""DeterministicTieBreaker over CSR batches: length buckets and the launches."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _native as N


@dataclass
class TieBreakResult:
    winner: torch.Tensor
    label: torch.Tensor
    n_groups: torch.Tensor
    variance: torch.Tensor
    g_key: torch.Tensor
    g_count: torch.Tensor
    g_density: torch.Tensor
    g_avgconf: torch.Tensor
    g_maxrel: torch.Tensor
    g_of: torch.Tensor      # int32[N]: each signal's group ordinal (first-seen order)


@dataclass
class TiePlan:
    """Markets of <= 32 agents bucketed by length for the lane-per-market tie-break: lists of the
    markets with <= 8, 9..16 and 17..32 agents, each run by a kernel walking 8 / 16 / 32
    positions per lane over rows gathered into LDS (tiebreak_lpm.hip GATHER) -- or None when
    bucketing would not pay (a uniform batch: contiguous tiles, the FULL-tile kernel)."""

    buckets: Optional[list]  # [(device int32 list, max_len)], or None: contiguous tiles


# relative cost of a 64-market tile, measured (kernel traces, 1M markets, profiles/r06gb/):
# contiguous FULL (every market 32 agents: 42 ns per tile) / contiguous ragged (the general
# 32-position body: 45.4 ns) / gathered buckets of 8 / 16 / 32 positions (20.7 / 34.9 / 58.3 ns,
# since round 6's batched row loads: 20 / 40 / 70 before, profiles/archive/r05f/).  The lane
# kernels are latency-bound by their stage -> compute -> flush phases, so fewer positions per
# lane save less than the arithmetic suggests; a uniform 1..32 ragged batch is now bucketed
# (0.674-0.680 vs 0.721 ms contiguous), a uniform 32 batch stays contiguous.
_TILE_COST = {"full": 0.92, "ragged": 1.0, 8: 0.46, 16: 0.77, 32: 1.28}
_BUCKET_GAIN = 0.97  # bucket when the model saves >= 3% (one launch more per call)


def tiebreak_plan(offsets_host: np.ndarray, device=None, force: bool = False) -> TiePlan:
    """Length buckets for batch.tiebreak (markets of <= 32 agents), when they cost less than
    the contiguous tiles by the kernels' relative tile costs (_TILE_COST), or always (force)."""
    lens = np.diff(np.asarray(offsets_host, np.int64))
    if len(lens) == 0 or int(lens.max()) > 32 or int(lens.min()) < 0:
        # a negative length (decreasing offsets) falls in no bucket: the contiguous kernel
        # records it as a device fault (kFaultTooLong) instead of leaving outputs unwritten
        return TiePlan(None)
    M = len(lens)
    pad = (-M) % 64
    t = np.concatenate([lens, np.full(pad, 32)]).reshape(-1, 64)
    full = (t == 32).all(axis=1)
    contig = _TILE_COST["full"] * int(full.sum()) + _TILE_COST["ragged"] * int((~full).sum())
    edges = ((0, 8), (9, 16), (17, 32))
    idx = [np.nonzero((lens >= lo) & (lens <= hi))[0].astype(np.int32) for lo, hi in edges]
    bucket = sum(_TILE_COST[hi] * ((len(i) + 63) // 64) for (lo, hi), i in zip(edges, idx))
    if bucket >= _BUCKET_GAIN * contig and not force:
        return TiePlan(None)
    dev = device or N.device()
    return TiePlan([(torch.from_numpy(i).to(dev), hi) for (lo, hi), i in zip(edges, idx) if len(i)])


def tiebreak(offsets: torch.Tensor, pred: torch.Tensor, conf: torch.Tensor, weight: torch.Tensor,
             rel: torch.Tensor, *, precision: int = 6, offsets_host: Optional[np.ndarray] = None,
             out: Optional[TieBreakResult] = None, max_len: Optional[int] = None,
             plan: Optional[TiePlan] = None) -> TieBreakResult:
    """DeterministicTieBreaker(precision).resolve for every CSR market (tiebreak.py:73-152).

    Any market length (> 4096 agents sort in a global scratch slice).  ``precision`` as
    CPython round() for every int, bit for bit (exact big integers where 10^|precision| is
    not a double); a rounded key too large for a double raises OverflowError, as CPython's
    round() does (precision <= -16 only, checked with one stream synchronisation).

    ``max_len`` (optional, <= 64): the caller's bound on every market's length; the host then
    skips its length scan of the offsets and does not synchronise.  A market longer than the
    bound is left unprocessed and recorded in the device fault word, as the C ABI does --
    ``_native.check_faults`` raises it (the bench and tests call it after their steps).

    ``plan`` (optional, :func:`tiebreak_plan`): length buckets of a ragged batch of <= 32-agent
    markets, reused across calls on the same CSR (no host scan per call).  Without one, a
    ragged batch scanned on the host is bucketed the same way when that pays -- an O(M) host
    pass and up to three host-to-device list copies on EVERY call: a caller that reruns the
    same CSR should build the TiePlan once with :func:`tiebreak_plan` and pass it in."""
    L = N.require_gpu()
    M = offsets.numel() - 1
    Nsig = pred.numel()
    dev = offsets.device
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    r = out or TieBreakResult(torch.empty(M, **f64), torch.empty(M, **i32), torch.empty(M, **i32),
                              torch.empty(M, **f64), torch.empty(max(Nsig, 1), **f64),
                              torch.empty(max(Nsig, 1), **i32), torch.empty(max(Nsig, 1), **f64),
                              torch.empty(max(Nsig, 1), **f64), torch.empty(max(Nsig, 1), **f64),
                              torch.empty(max(Nsig, 1), **i32))
    outs = (N.ptr(r.winner), N.ptr(r.label), N.ptr(r.n_groups), N.ptr(r.variance), N.ptr(r.g_key),
            N.ptr(r.g_count), N.ptr(r.g_density), N.ptr(r.g_avgconf), N.ptr(r.g_maxrel), N.ptr(r.g_of))
    ins = (N.ptr(pred), N.ptr(conf), N.ptr(weight), N.ptr(rel))
    st = N.stream(dev)

    def run_buckets(buckets):
        for lst, hi in buckets:
            N.check(L.bce_tiebreak_csr(N.ptr(offsets), M, N.ptr(lst), lst.numel(), *ins, int(hi), int(precision),
                                       *outs, st), "bce_tiebreak_csr")
        return _round_overflow_check(r, precision, dev)

    if plan is not None and plan.buckets is not None:
        return run_buckets(plan.buckets)
    if max_len is not None and 0 < int(max_len) <= 64:
        N.check(L.bce_tiebreak_csr(N.ptr(offsets), M, N.ptr(None), 0, *ins, int(max_len), int(precision), *outs, st),
                "bce_tiebreak_csr")
        return _round_overflow_check(r, precision, dev)
    offh = offsets_host if offsets_host is not None else offsets.cpu().numpy()
    lens = np.diff(offh)
    if len(lens) and int(lens.max()) <= 32:
        tp = tiebreak_plan(offh, dev)
        if tp.buckets is not None:
            return run_buckets(tp.buckets)
    long_ = np.nonzero(lens > 64)[0]
    if len(long_) == 0:
        N.check(L.bce_tiebreak_csr(N.ptr(offsets), M, N.ptr(None), 0, *ins, int(max(int(lens.max(initial=1)), 1)),
                                   int(precision), *outs, st), "bce_tiebreak_csr")
        return _round_overflow_check(r, precision, dev)
    # n <= 32: the lane-per-market kernel; 33..64: wave per market; longer: workgroup per market
    for lo, hi in ((0, 32), (33, 64)):
        short = np.nonzero((lens >= lo) & (lens <= hi))[0].astype(np.int32)
        if len(short):
            sl = torch.from_numpy(short).to(dev)
            N.check(L.bce_tiebreak_csr(N.ptr(offsets), M, N.ptr(sl), len(short), *ins, hi, int(precision), *outs,
                                       st), "bce_tiebreak_csr")
    ll = torch.from_numpy(long_.astype(np.int32)).to(dev)
    N.check(L.bce_tiebreak_csr_long(N.ptr(offsets), M, N.ptr(ll), len(long_), int(precision), *ins,
                                    int(lens[long_].max()), *outs, st), "bce_tiebreak_csr_long")
    return _round_overflow_check(r, precision, dev)


def _round_overflow_check(r, precision: int, dev):
    """round(x, n) with -308 <= n <= -16 can exceed DBL_MAX (CPython: OverflowError,
    "rounded value too large to represent"); the kernels record that as device fault 6."""
    if -308 <= int(precision) <= -16:
        try:
            N.check_faults(dev, "tiebreak round()")
        except N.BCEError as exc:
            if "too large to represent" in str(exc):
                raise OverflowError("rounded value too large to represent") from None
            raise
    return r
