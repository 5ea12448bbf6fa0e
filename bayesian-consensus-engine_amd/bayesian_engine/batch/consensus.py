"""compute_consensus over CSR batches: the length-bin plan, the launch, the range check."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _native as N
from .tables import SourceTable

_MODES = {"exact": N.MODE_EXACT, "fast": N.MODE_FAST}


@dataclass
class Plan:
    """Markets binned by length (bce_plan_bins), reusable across calls on the same CSR."""

    order: torch.Tensor
    bin_start: np.ndarray
    max_len: int
    scratch: Optional[torch.Tensor]

    @classmethod
    def build(cls, offsets_host: np.ndarray, device=None) -> "Plan":
        L = N.lib()
        off = np.ascontiguousarray(offsets_host, np.int64)
        M = len(off) - 1
        order = np.zeros(max(M, 1), np.int32)
        bins = np.zeros(N.NBINS + 1, np.int64)
        mx = np.zeros(1, np.int32)
        N.check(L.bce_plan_bins(N.ptr(off), M, N.ptr(order), N.ptr(bins), N.ptr(mx)), "plan_bins")
        sb = int(L.bce_consensus_scratch_bytes(N.ptr(off), N.ptr(order), N.ptr(bins)))
        dev = device or N.device()
        scratch = torch.empty(sb, dtype=torch.uint8, device=dev) if sb > 0 else None
        return cls(torch.from_numpy(order).to(dev), bins, int(mx[0]), scratch)

    @classmethod
    def build_device(cls, offsets: torch.Tensor) -> "Plan":
        """The same plan built on the GPU from the device offsets (bce_plan_bins_device: a
        stable radix sort by bin and LPT key, no D2H copy of the CSR).  One stream
        synchronisation returns the bin boundaries to the host."""
        L = N.require_gpu()
        dev = offsets.device
        M = offsets.numel() - 1
        order = torch.empty(max(M, 1), dtype=torch.int32, device=dev)
        sb = int(L.bce_plan_device_scratch_bytes(M))
        work = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
        bins = np.zeros(N.NBINS + 1, np.int64)
        mx = np.zeros(1, np.int32)
        lsb = np.zeros(1, np.int64)
        N.check(L.bce_plan_bins_device(N.ptr(offsets), M, N.ptr(order), N.ptr(bins), N.ptr(mx), N.ptr(lsb),
                                       N.ptr(work), sb, N.stream(dev)), "plan_bins_device")
        scratch = torch.empty(int(lsb[0]), dtype=torch.uint8, device=dev) if lsb[0] > 0 else None
        return cls(order, bins, int(mx[0]), scratch)

    @staticmethod
    def device_bins_async(offsets: torch.Tensor, stream):
        """``(order, bins)``, both on the device: the plan order int32[M] and the bin boundaries
        int64[NBINS + 1] of bce_plan_bins_device_async, enqueued on ``stream`` with no host
        synchronisation -- for the entries that read the boundaries on the device."""
        L = N.require_gpu()
        dev = offsets.device
        M = offsets.numel() - 1
        order = torch.empty(max(M, 1), dtype=torch.int32, device=dev)
        sb = int(L.bce_plan_device_scratch_bytes(M))
        work = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
        bins = torch.empty(N.NBINS + 1, dtype=torch.int64, device=dev)
        N.check(L.bce_plan_bins_device_async(N.ptr(offsets), M, N.ptr(order), N.ptr(bins), N.ptr(work), sb, stream),
                "bce_plan_bins_device_async")
        return order, bins

    @classmethod
    def for_markets(cls, offsets_host: np.ndarray, markets: np.ndarray, device=None) -> "Plan":
        """The plan of a market subset over the FULL CSR (a rank's markets of
        sharding.shard_markets_planned left in place): the subset binned and LPT-ordered as
        bce_plan_bins would, its order holding the full batch's market indices, so outputs land
        at those markets and per-unique outputs at their absolute CSR offsets."""
        from ..sharding import gather_csr, plan_order
        L = N.lib()
        off = np.ascontiguousarray(offsets_host, np.int64)
        mk = np.asarray(markets, np.int64)
        loc = gather_csr(off, mk)[0]
        lorder, bins = plan_order(loc)
        order = np.ascontiguousarray(mk[lorder].astype(np.int32))
        lens = np.diff(loc)
        sb = int(L.bce_consensus_scratch_bytes(N.ptr(off), N.ptr(order), N.ptr(bins)))
        dev = device or N.device()
        scratch = torch.empty(sb, dtype=torch.uint8, device=dev) if sb > 0 else None
        return cls(torch.from_numpy(order).to(dev), bins, int(lens.max(initial=0)), scratch)


@dataclass
class ConsensusResult:
    consensus: torch.Tensor      # fp64[M]  (0.0 where null)
    confidence: torch.Tensor     # fp64[M]
    total_weight: torch.Tensor   # fp64[M]
    n_unique: torch.Tensor       # int32[M]
    err_idx: Optional[torch.Tensor]   # int32[M]: first out-of-range signal, -1 if none
    usid: Optional[torch.Tensor]      # int32[N]: rank | cold<<31 at CSR offsets
    weight: Optional[torch.Tensor]    # fp64[N]
    nweight: Optional[torch.Tensor]   # fp64[N]

    def is_null(self, offsets: torch.Tensor) -> torch.Tensor:
        """consensus is None: empty market (core.py:88) or total weight == 0 (core.py:131)."""
        return (self.total_weight == 0) | (offsets[1:] == offsets[:-1])


def _alloc(M: int, Nsig: int, dev, unique: bool, validate: bool) -> ConsensusResult:
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    return ConsensusResult(
        torch.empty(M, **f64), torch.empty(M, **f64), torch.empty(M, **f64), torch.empty(M, **i32),
        torch.empty(M, **i32) if validate else None,
        torch.empty(max(Nsig, 1), **i32) if unique else None,
        torch.empty(max(Nsig, 1), **f64) if unique else None,
        torch.empty(max(Nsig, 1), **f64) if unique else None)


def consensus(offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, table: SourceTable, *,
              plan: Optional[Plan] = None, max_len: Optional[int] = None, mode: str = "exact",
              unique_outputs: bool = True, validate: bool = True, check: bool = False,
              out: Optional[ConsensusResult] = None) -> ConsensusResult:
    """core.compute_consensus for every CSR market (+ the validation range check).

    Pass ``max_len`` (<= 64: one launch, no planning) or a prebuilt :class:`Plan` for
    ragged batches.  Without a plan, the batch is planned on the GPU: with a ``max_len`` bound
    of 65..4096 entirely on the device, with no host synchronisation
    (bce_plan_bins_device_async + bce_consensus_planned_device; a market longer than the bound
    raises the device fault word), else by :meth:`Plan.build_device` (one stream
    synchronisation returns the bin boundaries).  A caller that reruns the same CSR should
    build the Plan once.

    ``mode="fast"`` (fixed-order trees, <= 1e-9 absolute vs the reference order) is
    deterministic per call shape but not invariant to batch composition: a small call (e.g. a
    market shard) may run a length bin in the wider launch of the bin above it, which sums the
    partial totals in another fixed order, so the same market's float outputs can differ in the
    last bits between a full batch and a shard (within 1e-9; include/bce.h BCE_MODE_FAST).
    ``mode="exact"`` is bit-identical in every launch shape.

    Raw CSR is trusted for speed: a ``sid`` outside ``[0, table.n)`` has its row read
    clamped and a market longer than ``max_len`` is left unprocessed; either raises the
    device fault word.  ``check=True`` synchronises and raises :class:`BCEError` for it
    (otherwise call ``_native.check_faults()`` when convenient).
    """
    L = N.require_gpu()
    M = offsets.numel() - 1
    Nsig = sid.numel()
    dev = offsets.device
    res = out or _alloc(M, Nsig, dev, unique_outputs, validate)
    common = (N.ptr(offsets), M, N.ptr(sid), N.ptr(prob), Nsig, N.ptr(table.relconf), N.ptr(table.bits),
              table.n)
    outs = (N.ptr(res.consensus), N.ptr(res.confidence), N.ptr(res.total_weight), N.ptr(res.n_unique),
            N.ptr(res.err_idx), N.ptr(res.usid), N.ptr(res.weight), N.ptr(res.nweight))
    md = _MODES[mode]
    if plan is None and max_len is not None and 0 < max_len <= 64:
        rc = L.bce_consensus_csr(*common, N.ptr(None), 0, int(max_len), md, *outs, N.stream(dev))
        N.check(rc, "bce_consensus_csr")
        if check:
            N.check_faults(dev, "consensus")
        return res
    if plan is None and max_len is not None and 64 < max_len <= 4096 and table.n <= (1 << 25):
        # a fresh ragged batch under the caller's bound: planned on the device and launched with
        # no host synchronisation (bce_plan_bins_device_async + bce_consensus_planned_device)
        st = N.stream(dev)
        order, bins = Plan.device_bins_async(offsets, st)
        N.check(L.bce_consensus_planned_device(*common, N.ptr(order), N.ptr(bins), md, *outs, st),
                "bce_consensus_planned_device")
        if check:
            N.check_faults(dev, "consensus")
        return res
    if plan is None:
        plan = Plan.build_device(offsets)
    sb = plan.scratch.numel() if plan.scratch is not None else 0
    rc = L.bce_consensus_planned(*common, N.ptr(plan.order), N.ptr(plan.bin_start), md, *outs,
                                 N.ptr(plan.scratch), sb, N.stream(dev))
    N.check(rc, "bce_consensus_planned")
    if check:
        N.check_faults(dev, "consensus")
    return res


def validate(offsets: torch.Tensor, prob: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """validate_input_payload's range check for every market: first bad index or -1."""
    L = N.require_gpu()
    M = offsets.numel() - 1
    err = out if out is not None else torch.empty(max(M, 1), dtype=torch.int32, device=offsets.device)
    N.check(L.bce_validate_csr(N.ptr(offsets), M, N.ptr(prob), N.ptr(err), N.stream(offsets.device)),
            "bce_validate_csr")
    return err[:M]
