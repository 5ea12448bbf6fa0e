"""Batched entry points over millions of markets.

All array arguments are device tensors (torch, ``cuda:N``); results stay in HBM.  Each
function is one or a few launches of the HIP kernels in ``libbce_hip.so`` on the current
stream -- there is no CPU fallback (see :mod:`bayesian_engine._native`).

Layout (include/bce.h):
  markets  CSR  offsets int64[M+1], sid int32[N] (interned source ranks in Python
           ``sorted()`` order), prob fp64[N]
  sources  dense table over ranks: rel fp64[S], conf fp64[S] (cold-start defaults baked
           in), present u8[S]; optional t_us int64[S] for decay
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM, DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY

_MODES = {"exact": N.MODE_EXACT, "fast": N.MODE_FAST}


# ---------------------------------------------------------------------------------------
# host-side interning and table building
# ---------------------------------------------------------------------------------------
def intern(ids: Iterable[str]) -> Dict[str, int]:
    """Rank ids in Python ``sorted()`` (code-point) order: integer order == str order."""
    return {s: i for i, s in enumerate(sorted(set(ids)))}


def to_device(dev):
    """``T = to_device(dev)``: ``T(a)`` is the numpy array ``a`` as a tensor on ``dev``."""
    return lambda a: torch.from_numpy(a).to(dev)


@dataclass
class SourceTable:
    """Dense per-source table resident in HBM, in the consensus kernel's layout.

    relconf [S, 2] fp64: interleaved {reliability, confidence} -> one 16-B gather per
    unique source; bits [ceil(S/32)] int32: present bitmask ("sourceId is a key of the
    reliability dict", core.py:167-170).  Cold-start defaults are baked into relconf.
    """

    relconf: torch.Tensor
    bits: torch.Tensor
    names: List[str]
    t_us: Optional[torch.Tensor] = None

    @property
    def n(self) -> int:
        return len(self.names)

    @property
    def rel(self) -> torch.Tensor:
        return self.relconf[:, 0]

    @property
    def conf(self) -> torch.Tensor:
        return self.relconf[:, 1]

    @classmethod
    def from_arrays(cls, rel: torch.Tensor, conf: torch.Tensor, present: Optional[torch.Tensor],
                    names: Optional[Sequence[str]] = None, t_us: Optional[torch.Tensor] = None) -> "SourceTable":
        """Pack device arrays with bce_table_pack (one launch)."""
        L = N.require_gpu()
        S = rel.numel()
        dev = rel.device
        relconf = torch.empty((max(S, 1), 2), dtype=torch.float64, device=dev)
        bits = torch.zeros(max((S + 31) // 32, 1), dtype=torch.int32, device=dev)
        rel = rel.to(torch.float64).contiguous()
        conf = conf.to(torch.float64).contiguous()
        pres = present.to(torch.uint8).contiguous() if present is not None else None
        N.check(L.bce_table_pack(S, N.ptr(rel), N.ptr(conf), N.ptr(pres), N.ptr(relconf), N.ptr(bits),
                                 N.stream(dev)), "bce_table_pack")
        return cls(relconf, bits, list(names) if names is not None else [""] * S, t_us)

    @classmethod
    def from_dict(cls, names: Sequence[str], source_reliability: Optional[dict], device=None) -> "SourceTable":
        """core.py:110-112 semantics: a key present (even with a partial dict) is not cold."""
        S = len(names)
        rel = np.full(max(S, 1), DEFAULT_RELIABILITY, np.float64)
        conf = np.full(max(S, 1), DEFAULT_CONFIDENCE, np.float64)
        present = np.zeros(max(S, 1), np.uint8)
        sr = source_reliability or {}
        for i, n in enumerate(names):
            if n in sr:
                present[i] = 1
                d = sr.get(n, {})  # a None value raises AttributeError, as core.py:110-111 does
                r = d.get("reliability", DEFAULT_RELIABILITY)
                c = d.get("confidence", DEFAULT_CONFIDENCE)
                acc = 0.0
                acc += r  # same TypeError as core.py:120 for non-numbers
                rel[i] = float(r)
                conf[i] = float(c)
        dev = device or N.device()
        T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        return cls.from_arrays(T(rel[:S]), T(conf[:S]), T(present[:S]), names)


@dataclass
class ReliabilityTable:
    """Store-side table (SoA) for the streaming decay / outcome-update kernels.

    rel, conf fp64[S], t_us int64[S] (updated_at as microseconds, NO_TIMESTAMP if
    falsy/unparseable), present u8[S] (a row exists).  Absent rows hold the baked
    cold-start values (0.5, 0.25, NO_TIMESTAMP), reliability.py:133-140.
    """

    rel: torch.Tensor
    conf: torch.Tensor
    t_us: torch.Tensor
    present: torch.Tensor
    names: List[str]

    @property
    def n(self) -> int:
        return len(self.names)

    def view(self, now_us: int) -> torch.Tensor:
        """get_reliability(apply_decay=True).reliability of every source."""
        return decay_view(self.rel, self.t_us, now_us, present=self.present)

    def consensus_table(self, now_us: Optional[int] = None, all_present: bool = True) -> "SourceTable":
        """Packed consensus table; reliability decayed at ``now_us`` when given.  Callers that
        fetch every source through get_reliability (market.py:209-219, cli.py:37-44) put
        every sourceId in the dict, hence ``all_present``."""
        rel = self.view(now_us) if now_us is not None else self.rel
        return SourceTable.from_arrays(rel, self.conf, None if all_present else self.present, self.names)

    def settle(self, plan: "SettlePlan", now_us: int, **kw) -> None:
        """:func:`settle` in place on this table (a domain or the global scope)."""
        settle(plan, self.rel, self.conf, self.t_us, self.present, now_us, **kw)

    def walk_forward(self, plan: "WalkPlan", market_time_us: torch.Tensor, **kw) -> "WalkResult":
        """:func:`walk_forward` on this table (a domain or the global scope)."""
        return walk_forward(plan, self, market_time_us, **kw)


# ---------------------------------------------------------------------------------------
# consensus
# ---------------------------------------------------------------------------------------
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

    @classmethod
    def for_markets(cls, offsets_host: np.ndarray, markets: np.ndarray, device=None) -> "Plan":
        """The plan of a market subset over the FULL CSR (a rank's markets of
        sharding.shard_markets_planned left in place): the subset binned and LPT-ordered as
        bce_plan_bins would, its order holding the full batch's market indices, so outputs land
        at those markets and per-unique outputs at their absolute CSR offsets."""
        from .sharding import gather_csr, plan_order
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
        order = torch.empty(max(M, 1), dtype=torch.int32, device=dev)
        sb = int(L.bce_plan_device_scratch_bytes(M))
        work = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
        bins = torch.empty(N.NBINS + 1, dtype=torch.int64, device=dev)
        st = N.stream(dev)
        N.check(L.bce_plan_bins_device_async(N.ptr(offsets), M, N.ptr(order), N.ptr(bins), N.ptr(work), sb, st),
                "bce_plan_bins_device_async")
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


# ---------------------------------------------------------------------------------------
# decay / outcome update
# ---------------------------------------------------------------------------------------
def decay_view(rel: torch.Tensor, t_us: torch.Tensor, now_us: int, present: Optional[torch.Tensor] = None,
               half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM,
               default_rel: float = DEFAULT_RELIABILITY, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """get_reliability(apply_decay=True) for a whole table (reliability.py:110-131)."""
    L = N.require_gpu()
    n = rel.numel()
    view = out if out is not None else torch.empty(max(n, 2), dtype=torch.float64, device=rel.device)
    N.check(L.bce_decay_view(n, N.ptr(rel), N.ptr(t_us), N.ptr(present), int(now_us), float(half_life_days),
                             float(min_rel), float(default_rel), N.ptr(view), N.stream(rel.device)),
            "bce_decay_view")
    return view[:n]


def decay_apply(rel: Optional[torch.Tensor], elapsed_days: torch.Tensor,
                half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM,
                want_factor: bool = False):
    """decay.compute_decay_factor / apply_reliability_decay on arrays (decay.py:31-100)."""
    L = N.require_gpu()
    n = elapsed_days.numel()
    dev = elapsed_days.device
    out = torch.empty(n, dtype=torch.float64, device=dev) if rel is not None else None
    fac = torch.empty(n, dtype=torch.float64, device=dev) if want_factor else None
    N.check(L.bce_decay_apply(n, N.ptr(rel), N.ptr(elapsed_days), float(half_life_days), float(min_rel),
                              N.ptr(out), N.ptr(fac), N.stream(dev)), "bce_decay_apply")
    return out, fac


def outcome_update(rel: torch.Tensor, conf: torch.Tensor, t_us: torch.Tensor, present: torch.Tensor,
                   flags: torch.Tensor, now_us: int, default_rel: float = DEFAULT_RELIABILITY,
                   default_conf: float = DEFAULT_CONFIDENCE) -> None:
    """In-place update_reliability math for every participant (reliability.py:142-183).

    flags u8[S]: bit0 participates, bit1 correct (at most one outcome per source per call;
    :func:`settle` applies a whole batch of resolved markets, any number per source).
    """
    L = N.require_gpu()
    N.check(L.bce_outcome_update(rel.numel(), N.ptr(rel), N.ptr(conf), N.ptr(t_us), N.ptr(present),
                                 N.ptr(flags), int(now_us), float(default_rel), float(default_conf),
                                 N.stream(rel.device)), "bce_outcome_update")


def replay_step(rel, conf, t_us, present, flags2, now_us: int, view: torch.Tensor,
                half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM) -> None:
    """Config-4 step: decayed view at ``now_us`` then the outcome update, fused.

    flags2: 2 bits per source (bit0 participates, bit1 correct), 4 sources per byte.
    Absent rows must hold the baked cold-start values (rel 0.5, conf 0.25, t = NO_TIMESTAMP).
    """
    L = N.require_gpu()
    N.check(L.bce_replay_step(rel.numel(), N.ptr(rel), N.ptr(conf), N.ptr(t_us), N.ptr(present),
                              N.ptr(flags2), int(now_us), float(half_life_days), float(min_rel),
                              DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE, N.ptr(view), N.stream(rel.device)),
            "bce_replay_step")


def pack_flags2(participate: np.ndarray, correct: np.ndarray) -> np.ndarray:
    """Host helper: (participate, correct) bool arrays -> the 2-bit packed flags2 layout."""
    S = len(participate)
    f = participate.astype(np.uint8) | (correct.astype(np.uint8) << 1)
    pad = (-S) % 4
    f = np.concatenate([f, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    return (f[:, 0] | (f[:, 1] << 2) | (f[:, 2] << 4) | (f[:, 3] << 6)).astype(np.uint8)


# ---------------------------------------------------------------------------------------
# tie-break, agreement statistics, re-estimation
# ---------------------------------------------------------------------------------------
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
    positions per lane over rows gathered into LDS (tiebreak.hip GATHER) -- or None when
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


def agreement_stats(offsets, sid, prob, outcome, n_sources: int, correct=None, total=None):
    """summarize_sources counts (market.py:279-304): outcome int8[M] (-1 skip, 0, 1)."""
    L = N.require_gpu()
    dev = offsets.device
    if correct is None:
        correct = torch.zeros(max(n_sources, 1), dtype=torch.int32, device=dev)
    if total is None:
        total = torch.zeros(max(n_sources, 1), dtype=torch.int32, device=dev)
    N.check(L.bce_agreement_stats(N.ptr(offsets), offsets.numel() - 1, N.ptr(sid), N.ptr(prob),
                                  N.ptr(outcome), N.ptr(correct), N.ptr(total), N.stream(dev)),
            "bce_agreement_stats")
    return correct, total


# ---------------------------------------------------------------------------------------
# namespaced fallback (reliability_abstraction.py:119-188) and cross-market aggregation
# ---------------------------------------------------------------------------------------
@dataclass
class ScopeTable:
    """One namespace scope of the store (rows of one market_id key) over a rank space:
    rel, conf fp64[S], t_us int64[S] (NO_TIMESTAMP = unparseable), has u8[S] = a row with a
    truthy updated_at exists (the ``if record.updated_at`` test)."""

    rel: torch.Tensor
    conf: torch.Tensor
    t_us: torch.Tensor
    has: torch.Tensor


NS_MARKET, NS_DOMAIN, NS_GLOBAL, NS_COLD = 0, 1, 2, 3


def namespace_resolve(scopes: Sequence[Optional[ScopeTable]], now_us: int, apply_decay: bool = True,
                      mark_cold: bool = False, names: Optional[Sequence[str]] = None,
                      half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM):
    """Fallback chain market -> domain -> global -> cold start for every source in one launch
    (bce_namespace_resolve).  ``scopes`` = [market, domain, global], None = not requested.
    Returns (SourceTable ready for :func:`consensus`, scope u8[S] with NS_* codes)."""
    L = N.require_gpu()
    sc = list(scopes) + [None] * (3 - len(scopes))
    live = [x for x in sc if x is not None]
    if live:
        S = live[0].rel.numel()
        dev = live[0].rel.device
    else:
        S = len(names) if names is not None else 0
        dev = N.device()
    relconf = torch.empty((max(S, 1), 2), dtype=torch.float64, device=dev)
    bits = torch.zeros(max((S + 31) // 32, 1), dtype=torch.int32, device=dev)
    scope = torch.empty(max(S, 1), dtype=torch.uint8, device=dev)
    args, keep = [], []
    for x in sc:
        if x is None:
            args += [None] * 4
        else:
            assert x.rel.numel() == S and x.conf.numel() == S and x.has.numel() == S, "scope sizes differ"
            arrs = (x.rel.to(torch.float64).contiguous(), x.conf.to(torch.float64).contiguous(),
                    x.t_us.to(torch.int64).contiguous(), x.has.to(torch.uint8).contiguous())
            keep.append(arrs)  # alive until the launch is enqueued
            args += [N.ptr(a) for a in arrs]
    N.check(L.bce_namespace_resolve(S, *args, int(bool(apply_decay)), int(now_us), float(half_life_days),
                                    float(min_rel), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE, int(bool(mark_cold)),
                                    N.ptr(relconf), N.ptr(bits), N.ptr(scope), N.stream(dev)),
            "bce_namespace_resolve")
    table = SourceTable(relconf, bits, list(names) if names is not None else [""] * S)
    return table, scope[:S]


@dataclass
class AggregateResult:
    """Per group: weighted_average, median, majority, mean confidence (NaN where no member
    has a consensus) and the number of members with a consensus."""

    wavg: torch.Tensor
    median: torch.Tensor
    majority: torch.Tensor
    mean_conf: torch.Tensor
    n_included: torch.Tensor


def aggregate(group_offsets: torch.Tensor, members: torch.Tensor, consensus: torch.Tensor,
              confidence: torch.Tensor, has_consensus: torch.Tensor, median: bool = True) -> AggregateResult:
    """CrossMarketAggregator.aggregate_consensus (market.py:340-408) for many member groups
    in one launch (bce_aggregate_groups); sums in list order, bit-exact."""
    L = N.require_gpu()
    dev = consensus.device
    G = group_offsets.numel() - 1
    f64 = dict(dtype=torch.float64, device=dev)
    r = AggregateResult(torch.empty(max(G, 1), **f64), torch.empty(max(G, 1), **f64),
                        torch.empty(max(G, 1), **f64), torch.empty(max(G, 1), **f64),
                        torch.empty(max(G, 1), dtype=torch.int64, device=dev))
    N.check(L.bce_aggregate_groups(N.ptr(group_offsets), G, N.ptr(members), consensus.numel(), N.ptr(consensus),
                                   N.ptr(confidence), N.ptr(has_consensus), N.ptr(r.wavg),
                                   N.ptr(r.median) if median else None, N.ptr(r.majority), N.ptr(r.mean_conf),
                                   N.ptr(r.n_included), N.stream(dev)), "bce_aggregate_groups")
    return AggregateResult(*(t[:G] for t in (r.wavg, r.median, r.majority, r.mean_conf, r.n_included)))


def reestimate(P: torch.Tensor, iters: int, w0: float = 0.5, w: Optional[torch.Tensor] = None,
               keep_history: bool = False, mode: str = "exact"):
    """Config 5: ``iters`` rounds of consensus <-> reliability on agent-major P [A, M].

    Each round reads P once: the consensus pass records every cell's vote as one bit and the
    agreement pass counts from those bits (bce_reestimate_consensus_votes /
    bce_reestimate_agreement_votes; A*ceil(M/64)*8 bytes of scratch).  ``mode="exact"`` sums
    in agent order on the vector ALUs (bit-identical to the reference); ``mode="fast"`` runs the
    same kernel -- it streams P at the HBM rate and is the fastest form.  ``mode="mfma"`` runs
    the consensus pass on the matrix cores (bce_reestimate_consensus_votes_mfma,
    v_mfma_f64_4x4x4_4b_f64: consensus within 4*A*2^-53, votes, agreement counts and weights
    identical to exact) -- the config-5 MFMA contraction, 1.3-1.8% behind the vector pass
    (DESIGN.md §4.6).  Its summation order needs every weight finite and >= 0; the library
    checks that on the device and runs the exact kernel for an iteration whose weights break
    it."""
    L = N.require_gpu()
    A, M = P.shape
    dev = P.device
    ld = P.stride(0)
    assert P.stride(1) == 1
    w = torch.full((A,), w0, dtype=torch.float64, device=dev) if w is None else w
    cons = torch.empty(M, dtype=torch.float64, device=dev)
    nul = torch.empty(max(M, 1), dtype=torch.uint8, device=dev)
    agree = torch.zeros(A, dtype=torch.int64, device=dev)
    resolved = torch.zeros(1, dtype=torch.int64, device=dev)
    K = max((M + 63) // 64, 1)
    votes = torch.empty((K, A), dtype=torch.int64, device=dev)
    words = torch.empty((2, K), dtype=torch.int64, device=dev)  # cvote, ok
    hist = []
    st = N.stream(dev)
    if mode not in _MODES and mode != "mfma":
        raise ValueError(f"mode must be one of {sorted([*_MODES, 'mfma'])}")
    scratch = None
    if mode == "mfma":
        nb = int(L.bce_reestimate_mfma_scratch_bytes(M))
        scratch = torch.empty((nb + 7) // 8, dtype=torch.int64, device=dev)
    for _ in range(iters):
        if scratch is None:
            N.check(L.bce_reestimate_consensus_votes(N.ptr(P, row_strided=True), A, M, ld, N.ptr(w), N.ptr(cons),
                                                     N.ptr(nul), N.ptr(votes), N.ptr(words[0]), N.ptr(words[1]),
                                                     st), "bce_reestimate_consensus_votes")
        else:
            N.check(L.bce_reestimate_consensus_votes_mfma(N.ptr(P, row_strided=True), A, M, ld, N.ptr(w),
                                                          N.ptr(cons), N.ptr(nul), N.ptr(votes), N.ptr(words[0]),
                                                          N.ptr(words[1]), N.ptr(scratch), scratch.numel() * 8, st),
                    "bce_reestimate_consensus_votes_mfma")
        agree.zero_()
        resolved.zero_()
        N.check(L.bce_reestimate_agreement_votes(N.ptr(votes), A, M, N.ptr(words[0]), N.ptr(words[1]),
                                                 N.ptr(agree), N.ptr(resolved), st), "bce_reestimate_agreement_votes")
        N.check(L.bce_reestimate_weights(A, N.ptr(agree), N.ptr(resolved), N.ptr(w), st),
                "bce_reestimate_weights")
        if keep_history:
            hist.append((cons.clone(), nul[:M].clone(), agree.clone(), w.clone()))
    return w, cons, nul[:M], agree, hist


# ---------------------------------------------------------------------------------------
# re-estimation over a ragged CSR batch: compile once, iterate on the compact form
# ---------------------------------------------------------------------------------------
_RC_MAX_RUN = 65535  # signals of one source in one market: the votes are two 16-bit counts


def _reestimate_csr_order(offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, n_sources: int,
                          max_run: Optional[int] = _RC_MAX_RUN):
    """The integer half of :meth:`ReestimateCsrPlan.build` and :meth:`PairPlan.build` (any device,
    no kernel): checks the shapes, sorts the signals by (market, sid) keeping input order inside
    a pair, and returns ``(key, perm, group_start, uoffsets)`` as bce_reestimate_csr_compile takes
    them.  ``max_run`` bounds the signals of one source in one market (None: no bound)."""
    M = offsets.numel() - 1
    Nsig = sid.numel()
    S = int(n_sources)
    if M < 0 or offsets.dim() != 1:
        raise ValueError("offsets must be a 1-D tensor of n_markets + 1 entries")
    if M >= (1 << 31):
        raise ValueError(f"reestimate_csr: {M} markets (the compact form indexes markets with int32)")
    if not 0 < S < (1 << 31):
        raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources})")
    if prob.numel() != Nsig:
        raise ValueError("sid and prob differ in length")
    dev = offsets.device
    offsets = offsets.to(torch.int64)
    lens = offsets[1:] - offsets[:-1]
    if M and (int(offsets[0]) != 0 or int(offsets[-1]) != Nsig or int(lens.min()) < 0):
        raise ValueError("offsets must rise from 0 to len(sid)")
    if M == 0 and Nsig:
        raise ValueError("offsets must rise from 0 to len(sid)")
    i64 = dict(dtype=torch.int64, device=dev)
    market = torch.repeat_interleave(torch.arange(M, **i64), lens, output_size=Nsig)
    key = market * S + sid.to(torch.int64).clamp(0, S - 1)
    del market
    key, perm = torch.sort(key, stable=True)
    first = torch.ones(Nsig, dtype=torch.bool, device=dev)
    if Nsig > 1:
        first[1:] = key[1:] != key[:-1]
    start = torch.nonzero(first).flatten()
    E = start.numel()
    group_start = torch.cat([start, torch.tensor([Nsig], **i64)])
    if E and max_run is not None and int((group_start[1:] - group_start[:-1]).max()) > max_run:
        raise ValueError(f"reestimate_csr: a source has more than {_RC_MAX_RUN} signals in one market")
    per_market = torch.bincount(torch.div(key[start], S, rounding_mode="floor"), minlength=M)
    uoffsets = torch.zeros(M + 1, **i64)
    uoffsets[1:] = torch.cumsum(per_market, 0)
    return key, perm, group_start, uoffsets


@dataclass
class ReestimateCsrPlan:
    """Everything of a CSR batch that does not change between re-estimation rounds: one entry
    per unique (market, source) pair in (market, ascending sid) order -- the order
    compute_consensus sums in (core.py:103).  SoA over the E entries: ``usid`` int32, ``avg``
    fp64 (the source's average probability, core.py:116), ``votes`` int32 (``n_ge << 16 |
    n_lt``: its raw signals with p >= 0.5 / below, market.py:298-299), ``emarket`` int32;
    ``uoffsets`` int64[M+1] (the entry range of every market) and ``bad`` u8[M] (a signal
    outside [0, 1], core.py:59-60).  Reusable across :func:`reestimate_csr` calls."""

    uoffsets: torch.Tensor
    usid: torch.Tensor
    avg: torch.Tensor
    votes: torch.Tensor
    emarket: torch.Tensor
    bad: torch.Tensor
    n_markets: int
    n_entries: int
    n_sources: int

    @classmethod
    def build(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor,
              n_sources: int) -> "ReestimateCsrPlan":
        """Compile ``(offsets, sid, prob)``.  The ordering is a stable torch sort of the key
        ``market * n_sources + sid``; the averages, votes and range flags are one launch of
        bce_reestimate_csr_compile.  Synchronises (off the per-round path).  A ``sid`` outside
        ``[0, n_sources)`` is clamped and raises :class:`BCEError` like ``consensus(check=True)``;
        more than 65535 signals of one source in one market, or 2^31 markets, ``ValueError``."""
        key, perm, group_start, uoffsets = _reestimate_csr_order(offsets, sid, prob, n_sources)
        M, Nsig, S, E = offsets.numel() - 1, sid.numel(), int(n_sources), group_start.numel() - 1
        dev = offsets.device
        L = N.require_gpu()
        i32 = dict(dtype=torch.int32, device=dev)
        plan = cls(uoffsets, torch.empty(max(E, 1), **i32), torch.empty(max(E, 1), dtype=torch.float64, device=dev),
                   torch.empty(max(E, 1), **i32), torch.empty(max(E, 1), **i32),
                   torch.zeros(max(M, 1), dtype=torch.uint8, device=dev), M, E, S)
        sid = sid.to(torch.int32).contiguous()
        prob = prob.to(torch.float64).contiguous()
        N.check(L.bce_reestimate_csr_compile(N.ptr(group_start), E, N.ptr(perm), N.ptr(key), Nsig, N.ptr(sid),
                                             N.ptr(prob), S, M, N.ptr(plan.usid), N.ptr(plan.avg),
                                             N.ptr(plan.votes), N.ptr(plan.emarket), N.ptr(plan.bad),
                                             N.stream(dev)), "bce_reestimate_csr_compile")
        N.check_faults(dev, "reestimate_csr compile")
        return plan


@dataclass
class ReestimateCsrResult:
    w: torch.Tensor          # fp64[S]   final weights
    consensus: torch.Tensor  # fp64[M]   last round (0.0 where null)
    null: torch.Tensor       # u8[M]     consensus is None (core.py:88,131)
    outcome: torch.Tensor    # int8[M]   -1 skipped, 0, 1
    correct: torch.Tensor    # int64[S]  last round's counts (after ``reduce``)
    total: torch.Tensor      # int64[S]
    history: list            # per round (consensus, null, outcome, correct, total, w) when kept


def reestimate_csr_step(plan: ReestimateCsrPlan, w: torch.Tensor, correct: torch.Tensor, total: torch.Tensor,
                        known: Optional[torch.Tensor] = None, out=None):
    """One round over the plan's markets: consensus with source weights ``w`` (fp64[S]), the
    outcome of every market (``known`` int8[M]: -1 unknown, 0/1 resolved), and the agreement
    counts ADDED into ``correct`` / ``total`` (int64[S]; the caller zeroes them, so the plans of
    several market shards can share them).  Returns ``(consensus, null, outcome)``; ``out``
    reuses a previous call's tensors.  Two launches, no synchronisation."""
    L = N.require_gpu()
    dev = w.device
    M, S = plan.n_markets, plan.n_sources
    assert w.dtype == torch.float64 and w.numel() == S, "w must be fp64[n_sources]"
    assert correct.dtype == torch.int64 and total.dtype == torch.int64, "counts must be int64"
    assert correct.numel() == S and total.numel() == S, "counts must be int64[n_sources]"
    assert known is None or (known.dtype == torch.int8 and known.numel() == M), "known must be int8[n_markets]"
    if out is None:
        out = (torch.empty(max(M, 1), dtype=torch.float64, device=dev),
               torch.empty(max(M, 1), dtype=torch.uint8, device=dev),
               torch.empty(max(M, 1), dtype=torch.int8, device=dev))
    cons, nul, outcome = out
    st = N.stream(dev)
    N.check(L.bce_reestimate_csr_consensus(N.ptr(plan.uoffsets), M, N.ptr(plan.usid), N.ptr(plan.avg),
                                           N.ptr(plan.bad), N.ptr(known), N.ptr(w), S, N.ptr(cons), N.ptr(nul),
                                           N.ptr(outcome), st), "bce_reestimate_csr_consensus")
    N.check(L.bce_reestimate_csr_agreement(plan.n_entries, N.ptr(plan.usid), N.ptr(plan.votes),
                                           N.ptr(plan.emarket), N.ptr(outcome), M, S, N.ptr(correct),
                                           N.ptr(total), st), "bce_reestimate_csr_agreement")
    return cons[:M], nul[:M], outcome[:M]


def reestimate_csr_weights(correct: torch.Tensor, total: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``w[s] = correct[s] / total[s]``, 0.5 where ``total[s] == 0`` (market.py:309-310), in place."""
    L = N.require_gpu()
    N.check(L.bce_reestimate_csr_weights(w.numel(), N.ptr(correct), N.ptr(total), N.ptr(w), N.stream(w.device)),
            "bce_reestimate_csr_weights")
    return w


def reestimate_csr(plan: ReestimateCsrPlan, iters: int, w0: float = 0.5, w: Optional[torch.Tensor] = None,
                   known: Optional[torch.Tensor] = None, keep_history: bool = False,
                   reduce=None) -> ReestimateCsrResult:
    """``iters`` rounds of consensus <-> source reliability over a compiled CSR batch: the
    composition :func:`reestimate` runs on a dense matrix (compute_consensus with the weights as
    ``source_reliability``, then the summarize_sources counts and ``correct / total``), bit-exact,
    for ragged markets with any number of signals per source.  ``w`` (fp64[S], updated in place)
    or ``w0`` gives the initial weights.  ``reduce(correct, total)`` runs between the counts and
    the weights of every round (``sharding.allreduce_counts`` for market shards).  Nothing in
    the loop synchronises with the host."""
    N.require_gpu()
    dev = plan.usid.device
    S = plan.n_sources
    w = torch.full((S,), float(w0), dtype=torch.float64, device=dev) if w is None else w
    correct = torch.zeros(S, dtype=torch.int64, device=dev)
    total = torch.zeros(S, dtype=torch.int64, device=dev)
    out, res, hist = None, None, []
    for _ in range(int(iters)):
        correct.zero_()
        total.zero_()
        res = out = reestimate_csr_step(plan, w, correct, total, known, out)
        if reduce is not None:
            reduce(correct, total)
        reestimate_csr_weights(correct, total, w)
        if keep_history:
            hist.append(tuple(t.clone() for t in (*res, correct, total, w)))
    if res is None:
        M = plan.n_markets
        res = (torch.zeros(M, dtype=torch.float64, device=dev), torch.zeros(M, dtype=torch.uint8, device=dev),
               torch.full((M,), -1, dtype=torch.int8, device=dev))
    return ReestimateCsrResult(w, res[0], res[1], res[2], correct, total, hist)


# ---------------------------------------------------------------------------------------
# settlement: a batch of resolved markets into one scope of the reliability table
# ---------------------------------------------------------------------------------------
# Chains of at least SETTLE_LONG_MIN bits are cut into chunks of SETTLE_CHUNK_BITS bits that run
# in parallel (settle_long_kernel): the best point of the measured grid (DESIGN.md §4.14,
# measurements/settle.txt).  2**62 disables the long path.
SETTLE_LONG_MIN = 256
SETTLE_CHUNK_BITS = 256
SETTLE_LONG_OFF = 1 << 62


def _settle_order(offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
                  n_sources: int):
    """The integer half of :meth:`SettlePlan.build` (any device, no kernel): checks the shapes,
    lists the signals of markets with ``outcome >= 0`` in CSR order and sorts them by ``sid``
    keeping that order inside a source.  Returns ``(market, perm, key, total, start, order,
    lens_desc)``: the market of every signal (int32[N]), the signal index and clamped sid of every
    sorted position, the chain length and bit offset per source, the touched sources longest
    chain first and their lengths."""
    M = offsets.numel() - 1
    Nsig = sid.numel()
    if M < 0 or offsets.dim() != 1:
        raise ValueError("offsets must be a 1-D tensor of n_markets + 1 entries")
    if M >= (1 << 31):
        raise ValueError(f"settle: {M} markets (the signal-to-market map is int32)")
    try:
        S = int(n_sources)
    except (TypeError, ValueError):
        raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources!r})") from None
    if not 0 < S < (1 << 31):
        raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources})")
    if prob.numel() != Nsig:
        raise ValueError("sid and prob differ in length")
    if outcome.dtype != torch.int8:
        raise ValueError(f"outcome must be int8 (-1 unresolved, 0, 1), got {outcome.dtype}")
    if outcome.dim() != 1 or outcome.numel() != M:
        raise ValueError(f"outcome must have one entry per market ({M}), got {tuple(outcome.shape)}")
    dev = offsets.device
    offsets = offsets.to(torch.int64)
    lens = offsets[1:] - offsets[:-1]
    if M and (int(offsets[0]) != 0 or int(offsets[-1]) != Nsig or int(lens.min()) < 0):
        raise ValueError("offsets must rise from 0 to len(sid)")
    if M == 0 and Nsig:
        raise ValueError("offsets must rise from 0 to len(sid)")
    i64 = dict(dtype=torch.int64, device=dev)
    market = torch.repeat_interleave(torch.arange(M, **i64), lens, output_size=Nsig)
    idx = torch.nonzero(outcome[market] >= 0).flatten()  # ascending: market, then position
    key = sid[idx].to(torch.int32).clamp(0, S - 1)
    key, p = torch.sort(key, stable=True)
    perm = idx[p]
    total = torch.bincount(key, minlength=S).to(torch.int64)
    start = torch.zeros(S + 1, **i64)
    start[1:] = torch.cumsum(total, 0)
    lens_desc, order = torch.sort(total, descending=True, stable=True)
    T = int((total > 0).sum())
    return (market.to(torch.int32), perm, key, total, start, order[:T].to(torch.int32).contiguous(),
            lens_desc[:T].cpu().numpy())


@dataclass
class SettlePlan:
    """A batch of resolved markets compiled for :func:`settle`: one correctness bit per signal
    of a market with ``outcome >= 0`` -- ``(probability >= 0.5) == outcome``, market.py:298-301 --
    the bits of one source contiguous and in the reference's loop order (market ascending, then
    position in the market).  ``bits`` u64[ceil(n_bits / 64)] (as int64), ``start`` int64[S+1]
    (bit offset of every source's chain), ``order`` int32[T] (the touched sources, longest chain
    first), ``total`` / ``correct`` int64[S] (chain length and its popcount: the
    summarize_sources counts, market.py:293-304).  Reusable: the same plan settles the domain and
    the global scope."""

    bits: torch.Tensor
    start: torch.Tensor
    order: torch.Tensor
    total: torch.Tensor
    correct: torch.Tensor
    n_bits: int
    n_sources: int
    lens_desc: np.ndarray   # host: chain lengths in ``order``
    _chunks: Optional[dict] = None  # (long_min, chunk_bits) -> (n_long, chunk_start, n_chunks)

    @property
    def n_touched(self) -> int:
        return int(self.order.numel())

    @classmethod
    def build(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
              n_sources: int, check: bool = True) -> "SettlePlan":
        """Compile ``(offsets, sid, prob)`` with ``outcome`` int8[M] (-1 unresolved, 0, 1).  The
        ordering is a stable torch sort by ``sid``; the bits and ``correct`` are one launch of
        bce_settle_compile.  Synchronises (once per batch).  A ``sid`` outside ``[0, n_sources)``
        is clamped and raises :class:`BCEError` like ``consensus(check=True)`` (``check=False``
        leaves the device fault word for a later ``_native.check_faults``); 2^31 markets or
        sources, an ``outcome`` of the wrong length or dtype, ``ValueError``."""
        market, perm, key, total, start, order, lens_desc = _settle_order(offsets, sid, prob, outcome, n_sources)
        M, Nsig, S, Np = offsets.numel() - 1, sid.numel(), int(n_sources), perm.numel()
        dev = offsets.device
        L = N.require_gpu()
        bits = torch.zeros(max((Np + 63) // 64, 1), dtype=torch.int64, device=dev)
        correct = torch.zeros(S, dtype=torch.int64, device=dev)
        sid = sid.to(torch.int32).contiguous()
        prob = prob.to(torch.float64).contiguous()
        outcome = outcome.contiguous()
        N.check(L.bce_settle_compile(N.ptr(perm), Np, N.ptr(key), N.ptr(sid), N.ptr(prob), N.ptr(market), Nsig,
                                     N.ptr(outcome), M, S, N.ptr(bits), N.ptr(correct), N.stream(dev)),
                "bce_settle_compile")
        if check:
            N.check_faults(dev, "settle compile")
        return cls(bits, start, order, total, correct, Np, S, lens_desc)

    def chunks(self, long_min: int, chunk_bits: int):
        """``(n_long, chunk_start, n_chunks)`` of the long path for these parameters (cached)."""
        long_min, chunk_bits = int(long_min), int(chunk_bits)
        if long_min < 1:
            raise ValueError(f"long_min must be >= 1 (got {long_min})")
        if chunk_bits < 64:
            raise ValueError(f"chunk_bits must be >= 64 (got {chunk_bits})")
        if self._chunks is None:
            self._chunks = {}
        hit = self._chunks.get((long_min, chunk_bits))
        if hit is None:
            ld = self.lens_desc
            n_long = int(np.searchsorted(-ld, -long_min, side="right"))  # descending: the leading >= long_min
            cs = np.zeros(n_long + 1, np.int64)
            cs[1:] = np.cumsum((ld[:n_long] + chunk_bits - 1) // chunk_bits)
            dev = self.order.device
            hit = (n_long, torch.from_numpy(cs).to(dev) if n_long else None, int(cs[-1]))
            self._chunks[(long_min, chunk_bits)] = hit
        return hit


def settle(plan: SettlePlan, rel: torch.Tensor, conf: torch.Tensor, t_us: torch.Tensor,
           present: Optional[torch.Tensor], now_us: int, *, long_min: Optional[int] = None,
           chunk_bits: Optional[int] = None, default_rel: float = DEFAULT_RELIABILITY,
           default_conf: float = DEFAULT_CONFIDENCE) -> None:
    """update_reliability for every signal of the compiled batch, in the reference's order, in
    place on one scope table (reliability.py:142-233 per signal; bit-exact, there is no fast
    mode).  Every touched source starts from its row -- the cold defaults where ``present`` is 0
    -- takes one update per bit of its chain, and gets ``t_us = now_us`` and ``present = 1``;
    rows of other sources are not written.

    The scope is a domain (``__domain__:<d>``) or the global table, where one row per source
    collects the updates of all its markets.  Market-level scope, whose rows are keyed by
    (source, market), is :func:`settle_pairs`: it runs this function over the batch's unique
    pairs, where a chain is a market's duplicate signals of one source.

    ``long_min`` / ``chunk_bits`` (defaults SETTLE_LONG_MIN / SETTLE_CHUNK_BITS): chains of at
    least ``long_min`` bits run one worker per ``chunk_bits`` bits (settle_long_kernel); the
    result does not depend on either.  ``long_min=2**62`` walks every chain by one lane."""
    L = N.require_gpu()
    S = plan.n_sources
    assert rel.dtype == torch.float64 and conf.dtype == torch.float64 and t_us.dtype == torch.int64, \
        "rel / conf must be fp64 and t_us int64"
    assert rel.numel() == S and conf.numel() == S and t_us.numel() == S, "the table must have n_sources rows"
    assert present is None or (present.dtype == torch.uint8 and present.numel() == S), "present must be u8[n_sources]"
    long_min = SETTLE_LONG_MIN if long_min is None else long_min
    chunk_bits = SETTLE_CHUNK_BITS if chunk_bits is None else chunk_bits
    n_long, chunk_start, n_chunks = plan.chunks(long_min, chunk_bits)
    dev = rel.device
    snap = torch.empty((n_long, 2), dtype=torch.float64, device=dev) if n_long else None
    N.check(L.bce_settle_apply(N.ptr(plan.bits), plan.n_bits, N.ptr(plan.start), N.ptr(plan.order), plan.n_touched,
                               n_long, N.ptr(chunk_start), n_chunks, int(chunk_bits), S, N.ptr(rel), N.ptr(conf),
                               N.ptr(t_us), N.ptr(present), int(now_us), float(default_rel), float(default_conf),
                               N.ptr(snap), N.stream(dev)), "bce_settle_apply")


# ---------------------------------------------------------------------------------------
# market scope: the (source, market) rows of the store as a sparse table in HBM
# ---------------------------------------------------------------------------------------
@dataclass
class PairTable:
    """The market-scope rows of a batch of markets, CSR by market over the batch's market index:
    ``poffsets`` int64[M+1] (the row range of every market), ``psid`` int32[P] (source ranks,
    strictly ascending inside a market), ``rel`` / ``conf`` fp64[P], ``t_us`` int64[P]
    (NO_TIMESTAMP where ``updated_at`` is falsy or unparseable), ``has`` u8[P] (``updated_at`` is
    truthy: the ``if record.updated_at`` test).  Only rows that exist are stored."""

    poffsets: torch.Tensor
    psid: torch.Tensor
    rel: torch.Tensor
    conf: torch.Tensor
    t_us: torch.Tensor
    has: torch.Tensor
    n_markets: int
    n_sources: int

    @property
    def n_rows(self) -> int:
        return int(self.psid.numel())

    @classmethod
    def empty(cls, n_markets: int, n_sources: int, device=None) -> "PairTable":
        dev = device if device is not None else N.device()
        z = lambda dt: torch.zeros(0, dtype=dt, device=dev)  # noqa: E731
        return cls(torch.zeros(int(n_markets) + 1, dtype=torch.int64, device=dev), z(torch.int32),
                   z(torch.float64), z(torch.float64), z(torch.int64), z(torch.uint8), int(n_markets),
                   int(n_sources))

    @classmethod
    def from_rows(cls, market: torch.Tensor, sid: torch.Tensor, rel: torch.Tensor, conf: torch.Tensor,
                  t_us: torch.Tensor, has: torch.Tensor, n_markets: int, n_sources: int) -> "PairTable":
        """Rows in any order (tensors of one device, CPU included: torch only, no kernel) sorted
        into the table.  A duplicate (market, sid), or an index outside the batch, ``ValueError``."""
        M, S = int(n_markets), int(n_sources)
        if M < 0 or M >= (1 << 31):
            raise ValueError(f"n_markets must be in [0, 2^31) (got {n_markets})")
        if not 0 < S < (1 << 31):
            raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources})")
        P = market.numel()
        if not all(x.numel() == P for x in (sid, rel, conf, t_us, has)):
            raise ValueError("the row arrays differ in length")
        dev = market.device
        if P == 0:
            return cls.empty(M, S, dev)
        mk = market.to(torch.int64)
        sd = sid.to(torch.int64)
        if int(mk.min()) < 0 or int(mk.max()) >= M:
            raise ValueError("a row's market index is outside [0, n_markets)")
        if int(sd.min()) < 0 or int(sd.max()) >= S:
            raise ValueError("a row's source rank is outside [0, n_sources)")
        key, perm = torch.sort(mk * S + sd)
        if P > 1 and bool((key[1:] == key[:-1]).any()):
            raise ValueError("duplicate (market, sid) row")
        poffsets = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        poffsets[1:] = torch.cumsum(torch.bincount(mk, minlength=M), 0)
        return cls(poffsets, sd[perm].to(torch.int32), rel.to(torch.float64)[perm].contiguous(),
                   conf.to(torch.float64)[perm].contiguous(), t_us.to(torch.int64)[perm].contiguous(),
                   has.to(torch.uint8)[perm].contiguous(), M, S)


@dataclass
class PairPlan:
    """A CSR batch compiled over its unique (market, source) pairs ("entries"), in (market,
    ascending sid) order -- the order compute_consensus sums in (core.py:103): ``uoffsets``
    int64[M+1] (the entry range of every market), ``usid`` int32[E] (the source of every entry),
    ``emarket`` int32[E], and ``esid`` int32[N]: every signal's entry index, which stands in for
    its source rank wherever a per-pair table is gathered."""

    uoffsets: torch.Tensor
    usid: torch.Tensor
    emarket: torch.Tensor
    esid: torch.Tensor
    n_markets: int
    n_entries: int
    n_sources: int

    @classmethod
    def build(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, n_sources: int) -> "PairPlan":
        """Torch only (any device, CPU included), synchronises.  A ``sid`` outside ``[0,
        n_sources)`` or 2^31 entries, ``ValueError``."""
        S = int(n_sources)
        if sid.numel() and (int(sid.min()) < 0 or int(sid.max()) >= S):
            raise ValueError("a sid is outside [0, n_sources)")
        key, perm, group_start, uoffsets = _reestimate_csr_order(offsets, sid, prob, n_sources, max_run=None)
        M, Nsig, E = offsets.numel() - 1, sid.numel(), group_start.numel() - 1
        if E >= (1 << 31):
            raise ValueError(f"{E} unique (market, source) pairs (entries are indexed with int32)")
        dev = offsets.device
        ukey = key[group_start[:E]]
        emarket = torch.div(ukey, S, rounding_mode="floor")
        usid = (ukey - emarket * S).to(torch.int32)
        runs = group_start[1:] - group_start[:-1]
        esid = torch.empty(Nsig, dtype=torch.int32, device=dev)
        esid[perm] = torch.repeat_interleave(torch.arange(E, dtype=torch.int32, device=dev), runs, output_size=Nsig)
        return cls(uoffsets, usid, emarket.to(torch.int32), esid, M, E, S)


@dataclass
class PairResolveResult:
    """Outputs of :func:`pair_resolve` (None where the mode does not produce them)."""

    lb: Optional[torch.Tensor]       # int64[Q] lower-bound row of every entry (global row index)
    matched: Optional[torch.Tensor]  # u8[Q]    that row holds the entry's sid
    table: Optional[SourceTable]     # store / namespaced: the consensus table over the entry index
    scope: Optional[torch.Tensor]    # u8[Q]    NS_* codes (store: NS_MARKET or NS_COLD)
    rel: Optional[torch.Tensor]      # raw: the start state in batch.settle's table layout
    conf: Optional[torch.Tensor]
    t_us: Optional[torch.Tensor]
    present: Optional[torch.Tensor]


_PAIR_MODES = {"store": N.PAIR_STORE, "namespaced": N.PAIR_NAMESPACED, "raw": N.PAIR_RAW}


# What :func:`pair_resolve` and :func:`scope_resolve` share on the host.
def _check_queries(qoffsets: torch.Tensor, qsid: torch.Tensor, emarket: Optional[torch.Tensor], M: int) -> int:
    Q = qsid.numel()
    if qoffsets.numel() != M + 1:
        raise ValueError(f"qoffsets must have n_markets + 1 = {M + 1} entries")
    if emarket is not None and emarket.numel() != Q:
        raise ValueError("emarket and qsid differ in length")
    assert qoffsets.dtype == torch.int64 and qsid.dtype == torch.int32, "qoffsets int64, qsid int32"
    assert emarket is None or emarket.dtype == torch.int32, "emarket must be int32"
    return Q


def _entry_outputs(Q: int, dev, index: bool, table: bool = True):
    """``(lb, matched, relconf, bits, scope)`` over max(Q, 1) entries; None where not asked for."""
    Q1 = max(Q, 1)
    lb = torch.empty(Q1, dtype=torch.int64, device=dev) if index else None
    matched = torch.empty(Q1, dtype=torch.uint8, device=dev) if index else None
    if not table:
        return lb, matched, None, None, None
    return (lb, matched, torch.empty((Q1, 2), dtype=torch.float64, device=dev),
            torch.zeros(max((Q + 31) // 32, 1), dtype=torch.int32, device=dev),
            torch.empty(Q1, dtype=torch.uint8, device=dev))


def _dense_scope(x: Optional[ScopeTable], S: int, what: str):
    """A dense scope as the four tensors the launch reads (the caller keeps them alive until it is
    enqueued) and their pointers; None: NULLs."""
    if x is None:
        return None, [N.ptr(None)] * 4
    assert x.rel.numel() == S and x.conf.numel() == S and x.has.numel() == S and x.t_us.numel() == S, what
    arrs = (x.rel.to(torch.float64).contiguous(), x.conf.to(torch.float64).contiguous(),
            x.t_us.to(torch.int64).contiguous(), x.has.to(torch.uint8).contiguous())
    return arrs, [N.ptr(a) for a in arrs]


def _pair_pointers(t: Optional["PairTable"]):
    """psid / rel / conf / t_us / has of a pair table; no table or no rows: NULLs."""
    if t is None or not t.n_rows:
        return [N.ptr(None)] * 5
    return [N.ptr(a) for a in (t.psid, t.rel, t.conf, t.t_us, t.has)]


def _cut(Q: int, *tensors):
    return [None if t is None else t[:Q] for t in tensors]


def _bins_as_plan(consensus_kwargs: dict) -> dict:
    """``bins=`` of the wrappers that have a ``plan=`` of their own is :func:`consensus`'s ``plan=``."""
    if "bins" in consensus_kwargs:
        consensus_kwargs["plan"] = consensus_kwargs.pop("bins")
    return consensus_kwargs


def pair_resolve(qoffsets: torch.Tensor, qsid: torch.Tensor, pairs: PairTable, now_us: int, *,
                 mode: str = "store", emarket: Optional[torch.Tensor] = None,
                 domain: Optional[ScopeTable] = None, global_scope: Optional[ScopeTable] = None,
                 apply_decay: bool = True, mark_cold: bool = False, index: bool = True,
                 half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM) -> PairResolveResult:
    """The market-scope row of every query entry in one launch (bce_pair_resolve).  The queries
    are CSR by market like the table: ``qoffsets`` int64[M+1], ``qsid`` int32[Q] ascending and
    unique inside a market (a :class:`PairPlan`'s or :class:`ReestimateCsrPlan`'s ``uoffsets`` /
    ``usid``), ``emarket`` the market of every entry (optional: searched in ``qoffsets``).

    ``mode="store"``: SQLiteReliabilityStore.get_reliability(sid, market, apply_decay) per entry;
    ``"namespaced"``: NamespacedReliabilityStore.get_reliability with the fallback pair row ->
    ``domain`` -> ``global_scope`` -> cold start (dense :class:`ScopeTable` over the source ranks,
    None = not requested); ``"raw"``: the undecayed row, or the cold defaults, as the table
    :func:`settle` updates.  ``index=False`` skips the ``lb`` / ``matched`` outputs."""
    L = N.require_gpu()
    md = _PAIR_MODES[mode]
    M, S = pairs.n_markets, pairs.n_sources
    if md != N.PAIR_NAMESPACED and (domain is not None or global_scope is not None):
        raise ValueError("domain / global_scope need mode='namespaced'")
    Q = _check_queries(qoffsets, qsid, emarket, M)
    dev = qoffsets.device
    lb, matched, relconf, bits, scope = _entry_outputs(Q, dev, index, table=md != N.PAIR_RAW)
    rel = conf = t_us = present = None
    if md == N.PAIR_RAW:
        rel, conf, t_us, present = (torch.empty(max(Q, 1), dtype=dt, device=dev)
                                    for dt in (torch.float64, torch.float64, torch.int64, torch.uint8))
    dom, dptr = _dense_scope(domain, S, "a dense scope must have n_sources rows")  # alive until enqueued
    glob, gptr = _dense_scope(global_scope, S, "a dense scope must have n_sources rows")
    N.check(L.bce_pair_resolve(md, N.ptr(qoffsets), M, N.ptr(qsid if Q else None), N.ptr(emarket if Q else None), Q,
                               N.ptr(pairs.poffsets), *_pair_pointers(pairs), pairs.n_rows, S, *dptr, *gptr,
                               int(bool(apply_decay)), int(now_us), float(half_life_days), float(min_rel),
                               DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE, int(bool(mark_cold)), N.ptr(lb),
                               N.ptr(matched), N.ptr(relconf), N.ptr(bits), N.ptr(scope), N.ptr(rel), N.ptr(conf),
                               N.ptr(t_us), N.ptr(present), N.stream(dev)), "bce_pair_resolve")
    table = SourceTable(relconf, bits, range(Q)) if relconf is not None else None  # "names": the entry indices
    lb, matched, scope, rel, conf, t_us, present = _cut(Q, lb, matched, scope, rel, conf, t_us, present)
    return PairResolveResult(lb, matched, table, scope, rel, conf, t_us, present)


@dataclass
class PairConsensusResult:
    """:func:`consensus_pairs`: ``result`` is the :class:`ConsensusResult` of the batch, whose
    per-unique rank field (``usid``) holds the ENTRY index (| cold << 31) -- the source of entry
    ``e`` is ``plan.usid[e]``; inside a market entries ascend with the sid, so slot j of a market
    is its j-th source as in :func:`consensus`.  ``scope`` / ``matched`` / ``lb`` are per entry."""

    result: ConsensusResult
    plan: PairPlan
    scope: torch.Tensor
    matched: torch.Tensor
    lb: torch.Tensor
    dmatched: Optional[torch.Tensor] = None  # with ``domains=``: the domain row of every entry
    dlb: Optional[torch.Tensor] = None


def consensus_pairs(offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, pairs: PairTable, now_us: int, *,
                    plan: Optional[PairPlan] = None, domain: Optional[ScopeTable] = None,
                    global_scope: Optional[ScopeTable] = None, namespaced: bool = False, apply_decay: bool = True,
                    mark_cold: bool = False, domains: Optional[PairTable] = None,
                    market_domain: Optional[torch.Tensor] = None, **consensus_kwargs) -> PairConsensusResult:
    """compute_consensus for every CSR market with the reliability of every signal read at
    MARKET scope: one :func:`pair_resolve` launch builds the consensus table over the batch's
    unique pairs, then :func:`consensus` runs unchanged with ``plan.esid`` as the ranks.
    ``namespaced=False`` is what MarketStore.compute_all_consensus(store) reads
    (get_reliability(sid, str(market.id), apply_decay=True), every source present);
    ``namespaced=True`` adds the fallback to ``domain`` / ``global_scope`` / cold start.  A caller
    that reruns the same CSR builds the :class:`PairPlan` once.  ``consensus_kwargs`` go to
    :func:`consensus` (``plan=`` there is the length-bin :class:`Plan`, passed as ``bins``).

    ``domains=`` / ``market_domain=`` (together, with ``namespaced=True`` and without the dense
    ``domain=``, else ``ValueError``) give every market a domain of its own: the sparse domain
    rows as a :class:`PairTable` over the domain index and the domain index of every market
    (int32[M], -1 = none).  The lookup is then :func:`scope_resolve` and the result carries
    ``dlb`` / ``dmatched`` as well."""
    per_market = domains is not None or market_domain is not None
    if per_market:
        if domains is None or market_domain is None:
            raise ValueError("domains= and market_domain= go together")
        if domain is not None:
            raise ValueError("domains= (a domain per market) and domain= (one dense domain) exclude each other")
        if not namespaced:
            raise ValueError("domains= needs namespaced=True")
    if plan is None:
        plan = PairPlan.build(offsets, sid, prob, pairs.n_sources)
    if plan.n_markets != pairs.n_markets or plan.n_sources != pairs.n_sources:
        raise ValueError("the plan and the pair table describe different batches")
    _bins_as_plan(consensus_kwargs)
    if per_market:
        lb, matched, dlb, dmatched, table, scope = scope_resolve(
            plan.uoffsets, plan.usid, pairs, domains, market_domain, now_us, emarket=plan.emarket,
            global_scope=global_scope, apply_decay=apply_decay, mark_cold=mark_cold)
        res = consensus(offsets, plan.esid, prob.to(torch.float64), table, **consensus_kwargs)
        return PairConsensusResult(res, plan, scope, matched, lb, dmatched, dlb)
    r = pair_resolve(plan.uoffsets, plan.usid, pairs, now_us, mode="namespaced" if namespaced else "store",
                     emarket=plan.emarket, domain=domain, global_scope=global_scope, apply_decay=apply_decay,
                     mark_cold=mark_cold)
    res = consensus(offsets, plan.esid, prob.to(torch.float64), r.table, **consensus_kwargs)
    return PairConsensusResult(res, plan, r.scope, r.matched, r.lb)


def _pair_merge_index(lb: torch.Tensor, matched: torch.Tensor, touched: torch.Tensor, emarket: torch.Tensor,
                      poffsets: torch.Tensor):
    """Where the rows of a settled pair table go (torch only, any device).  ``lb`` / ``matched``
    per entry (:func:`pair_resolve`), ``touched`` bool per entry; entries are in (market, sid)
    order, so ``lb`` does not decrease.  Returns ``(dst_old, ins, dst_ins, upd, dst_upd,
    new_poffsets)``: the new position of every old row, the entries to insert and their
    positions, the entries that overwrite their matched row and those rows' new positions, and
    the new row offsets."""
    P = int(poffsets[-1]) if poffsets.numel() else 0
    M = poffsets.numel() - 1
    hit = matched.to(torch.bool)
    ins = torch.nonzero(touched & ~hit).flatten()
    upd = torch.nonzero(touched & hit).flatten()
    # an old row p moves behind every inserted entry whose lower bound is <= p
    shift = torch.cumsum(torch.bincount(lb[ins], minlength=P + 1), 0)
    dst_old = torch.arange(P, dtype=torch.int64, device=lb.device) + shift[:P]
    # the j-th inserted entry sits behind the lb old rows and the j inserts before it
    dst_ins = lb[ins] + torch.arange(ins.numel(), dtype=torch.int64, device=lb.device)
    dst_upd = dst_old[lb[upd]]
    new_poffsets = poffsets.clone()
    new_poffsets[1:] += torch.cumsum(torch.bincount(emarket[ins].to(torch.int64), minlength=M), 0)
    return dst_old, ins, dst_ins, upd, dst_upd, new_poffsets


def settle_pairs(plan: PairPlan, pairs: PairTable, offsets: torch.Tensor, prob: torch.Tensor,
                 outcome: torch.Tensor, now_us: int, **settle_kwargs):
    """``update_reliability(sid, correct, market_id=m)`` for every signal of every market with
    ``outcome >= 0`` (int8[M]: -1 unresolved, 0, 1), at MARKET scope
    (reliability_abstraction.py:211-229).  The chain of a pair is its signals in that market in
    position order -- the order the reference's loop over ``market.signals`` reaches the row.

    A :class:`SettlePlan` is compiled over the entry space (``plan.esid`` as the ranks), the start
    states come from :func:`pair_resolve` in raw mode, :func:`settle` applies the chains in place
    on that entry table, and the result is merged into a NEW :class:`PairTable`: touched pairs
    with a row overwrite it, touched pairs without one are inserted in sid order, every other row
    is carried over bit for bit; settled rows get ``t_us = now_us`` and ``has = 1``.  The merge's
    destinations are cumulative sums and its row movement torch ``index_copy_`` (once per batch,
    bytes-bound).  Returns ``(table, settle_plan)``; the plan's ``total`` / ``correct`` are the
    counts per entry.  ``settle_kwargs`` go to :func:`settle` (``long_min``, ``chunk_bits``)."""
    if plan.n_markets != pairs.n_markets or plan.n_sources != pairs.n_sources:
        raise ValueError("the plan and the pair table describe different batches")
    E = plan.n_entries
    splan = SettlePlan.build(offsets, plan.esid, prob, outcome, n_sources=max(E, 1))
    if E == 0:
        return pairs, splan
    r = pair_resolve(plan.uoffsets, plan.usid, pairs, now_us, mode="raw", emarket=plan.emarket)
    settle(splan, r.rel, r.conf, r.t_us, r.present, now_us, **settle_kwargs)
    return _pair_merge(plan, pairs, r, splan.total[:E] > 0), splan


def _pair_merge(plan: PairPlan, pairs: PairTable, r: PairResolveResult, touched: torch.Tensor) -> PairTable:
    """The settled entry table ``r`` (raw mode: ``lb`` / ``matched`` and the rows' new state over
    the entries of ``plan``) merged into a NEW :class:`PairTable`: the ``touched`` entries
    overwrite their matched row or are inserted in sid order (``has`` from ``r.present``), every
    other row is carried over bit for bit."""
    dst_old, ins, dst_ins, upd, dst_upd, poffsets = _pair_merge_index(r.lb, r.matched, touched, plan.emarket,
                                                                      pairs.poffsets)
    P2 = pairs.n_rows + ins.numel()
    new = []
    for old, ent in ((pairs.psid, plan.usid), (pairs.rel, r.rel), (pairs.conf, r.conf), (pairs.t_us, r.t_us),
                     (pairs.has, r.present)):
        out = torch.empty(P2, dtype=old.dtype, device=old.device)
        out.index_copy_(0, dst_old, old)
        out.index_copy_(0, dst_ins, ent[ins])
        out.index_copy_(0, dst_upd, ent[upd])
        new.append(out)
    return PairTable(poffsets, *new, pairs.n_markets, pairs.n_sources)


# ---------------------------------------------------------------------------------------
# walk-forward consensus: every market reads the table as of its turn
# ---------------------------------------------------------------------------------------
# Chains of at least WALK_LONG_MIN bits are traced one worker per WALK_CHUNK_BITS bits.
WALK_LONG_MIN = SETTLE_LONG_MIN
WALK_CHUNK_BITS = SETTLE_CHUNK_BITS


def _walk_queries(pairs: PairPlan, offsets: torch.Tensor, outcome: torch.Tensor):
    """The integer half of :meth:`WalkPlan.build` behind the entry list (torch only, any device):
    ``(qstart, qpos, qentry, qlast, slast)``.  An entry of a resolved market contributes as many
    chain bits as it has signals; the queries are the entries in (source, market) order, ``qpos``
    the bits of the source before the entry's market, ``qlast`` (by ENTRY) the market of the last
    of those bits and ``slast`` (by source) the source's last resolved market, -1 where none."""
    E = pairs.n_entries
    emarket = pairs.emarket[:E].to(torch.int64)
    cnt = _entry_signals(pairs) * (outcome[emarket] >= 0)
    return _chain_queries(pairs.usid[:E].to(torch.int64), cnt, emarket, pairs.n_sources)


def _entry_signals(pairs: PairPlan) -> torch.Tensor:
    """int64[E]: the signals of every entry."""
    E = pairs.n_entries
    if not E:
        return torch.zeros(0, dtype=torch.int64, device=pairs.esid.device)
    return torch.bincount(pairs.esid.to(torch.int64), minlength=E)[:E]


def _chain_queries(chain: torch.Tensor, cnt: torch.Tensor, emarket: torch.Tensor, n_chains: int,
                   partial: bool = False):
    """:func:`_walk_queries` for any family of chains over the entries (torch only, any device):
    ``chain`` int64[E] is the chain every entry reads and feeds, ``cnt`` int64[E] the bits it
    leaves behind, ``emarket`` int64[E] its market (entries ascend by market).  Returns ``(qstart
    [n_chains + 1], qpos, qentry, qlast [E, by entry], slast [n_chains])`` as there.  ``partial``:
    entries with ``chain < 0`` are no queries (their ``qlast`` stays -1), so ``qpos`` / ``qentry``
    are shorter than E."""
    E, C = chain.numel(), int(n_chains)
    dev = chain.device
    i64 = dict(dtype=torch.int64, device=dev)
    if partial:
        sel = torch.nonzero(chain >= 0).flatten()
        chain = chain[sel]
    skey, qentry = torch.sort(chain, stable=True)  # entries ascend by market: (chain, market) order
    Q = qentry.numel()
    qstart = torch.zeros(C + 1, **i64)
    qstart[1:] = torch.cumsum(torch.bincount(chain, minlength=C), 0)
    if partial:
        qentry = sel[qentry]
    c = cnt[qentry]
    excl = torch.cumsum(c, 0) - c
    first = qstart[skey]                       # the chain's first query
    qpos = excl - excl[first] if Q else excl
    # the last query before this one, in the same chain, whose market left bits
    at = torch.where(c > 0, torch.arange(Q, **i64), torch.full((Q,), -1, **i64))
    incl = torch.cummax(at, 0).values if Q else at
    prev = torch.cat([torch.full((1,), -1, **i64), incl[:-1]]) if Q else incl
    has = prev >= first
    qm = emarket[qentry]
    qlast = torch.full((E,), -1, dtype=torch.int32, device=dev)
    qlast[qentry] = torch.where(has, qm[prev.clamp(min=0)], torch.full((Q,), -1, **i64)).to(torch.int32)
    slast = torch.full((C,), -1, **i64)
    live = torch.nonzero(qstart[1:] > qstart[:-1]).flatten()
    if live.numel():
        end = incl[qstart[1:][live] - 1]
        ok = end >= qstart[:-1][live]
        slast[live[ok]] = qm[end[ok]]
    return qstart, qpos.contiguous(), qentry.to(torch.int32).contiguous(), qlast, slast


@dataclass
class WalkPlan:
    """A chronological CSR batch compiled for :func:`walk_forward`: the :class:`SettlePlan` of its
    resolved markets, the :class:`PairPlan` entry list over ALL markets, and one query per entry,
    regrouped by source: ``qstart`` int64[S+1], ``qpos`` int64[E] (query order, ascending inside a
    source: the chain position whose before-state the query reads, 0 <= qpos <= chain length),
    ``qentry`` int32[E] (the entry a query answers), ``qlast`` int32[E] (by entry: the market of
    chain bit ``qpos - 1``, -1 when ``qpos == 0``) and ``slast`` int64[S] (the last resolved
    market of every source, -1 where none).  ``n_clamped``: sids outside ``[0, n_sources)``."""

    settle: SettlePlan
    pairs: PairPlan
    qstart: torch.Tensor
    qpos: torch.Tensor
    qentry: torch.Tensor
    qlast: torch.Tensor
    slast: torch.Tensor
    n_clamped: int
    outcome: Optional[torch.Tensor] = None  # int8[M], as given to build (scoring reads it)

    @property
    def total(self) -> torch.Tensor:
        return self.settle.total

    @property
    def correct(self) -> torch.Tensor:
        return self.settle.correct

    @classmethod
    def order(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
              n_sources: int):
        """The integer half of :meth:`build` (torch only, CPU tensors included): ``(pairs, qstart,
        qpos, qentry, qlast, slast, n_clamped)``.  Argument errors as :meth:`SettlePlan.build`."""
        M = offsets.numel() - 1
        try:
            S = int(n_sources)
        except (TypeError, ValueError):
            raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources!r})") from None
        if not 0 < S < (1 << 31):
            raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources})")
        if outcome.dtype != torch.int8:
            raise ValueError(f"outcome must be int8 (-1 unresolved, 0, 1), got {outcome.dtype}")
        if outcome.dim() != 1 or outcome.numel() != M:
            raise ValueError(f"outcome must have one entry per market ({M}), got {tuple(outcome.shape)}")
        clamped = sid.to(torch.int32).clamp(0, S - 1)
        n_clamped = int((clamped != sid).sum())
        pairs = PairPlan.build(offsets, clamped, prob, S)  # checks offsets / prob
        return (pairs, *_walk_queries(pairs, offsets, outcome), n_clamped)

    @classmethod
    def build(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
              n_sources: int, check: bool = True) -> "WalkPlan":
        """Compile ``(offsets, sid, prob)`` in chronological market order with ``outcome``
        int8[M] (-1 unresolved, 0, 1).  Torch sorts and scans plus :meth:`SettlePlan.build`;
        synchronises.  A ``sid`` outside ``[0, n_sources)`` is clamped and raises
        :class:`BCEError` (``check=False``: the fault is left for :func:`walk_forward`)."""
        pairs, qstart, qpos, qentry, qlast, slast, n_clamped = cls.order(offsets, sid, prob, outcome, n_sources)
        splan = SettlePlan.build(offsets, sid, prob, outcome, n_sources, check=check)
        if check and n_clamped:  # in an unresolved market: the settlement compile does not see it
            raise N.BCEError(f"walk plan: {n_clamped} sid outside [0, {int(n_sources)})")
        return cls(splan, pairs, qstart, qpos, qentry, qlast, slast, n_clamped, outcome.contiguous())


@dataclass
class WalkResult:
    """:func:`walk_forward`: ``result`` is the batch's :class:`ConsensusResult`, its ``usid``
    holding the ENTRY index (| cold << 31) as in :class:`PairConsensusResult`; ``scope_present``
    u8[E]: a row existed when the entry was read; ``total`` / ``correct`` int64[S] of the plan."""

    result: ConsensusResult
    plan: WalkPlan
    scope_present: torch.Tensor
    total: torch.Tensor
    correct: torch.Tensor

    def __getattr__(self, name):  # the ConsensusResult fields, directly
        if name in ConsensusResult.__dataclass_fields__:
            res = self.__dict__.get("result")
            if res is not None:
                return getattr(res, name)
        raise AttributeError(name)

    def is_null(self, offsets: torch.Tensor) -> torch.Tensor:
        return self.result.is_null(offsets)


def walk_trace(plan: WalkPlan, table: "ReliabilityTable", market_time_us: torch.Tensor, *,
               all_present: bool = True, long_min: Optional[int] = None, chunk_bits: Optional[int] = None,
               half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM):
    """The read side of :func:`walk_forward` alone (bce_settle_trace + bce_walk_read): the
    consensus table over the entry index -- every entry's ``get_reliability(apply_decay=True)`` at
    its market's time, after the earlier markets were settled -- and ``scope_present`` u8[E].
    The table is not written."""
    E = plan.pairs.n_entries
    dev = table.rel.device
    relconf, bits, exists = _walk_buffers(E, dev)  # relconf: the trace, decayed in place
    _walk_settle_trace(plan, table, market_time_us, relconf, long_min, chunk_bits)
    _walk_read(plan, table, market_time_us, relconf, relconf, bits, exists, all_present, half_life_days, min_rel)
    return SourceTable(relconf, bits, range(E)), exists[:E]  # "names": the entry indices


def _walk_buffers(E: int, dev):
    """``(relconf [E, 2], present bits, exists u8[E])`` of a walk read, at least one row each."""
    E1 = max(E, 1)
    return (torch.empty((E1, 2), dtype=torch.float64, device=dev),
            torch.zeros(max((E + 31) // 32, 1), dtype=torch.int32, device=dev),
            torch.empty(E1, dtype=torch.uint8, device=dev))


def _walk_settle_trace(plan: WalkPlan, table: "ReliabilityTable", market_time_us: torch.Tensor,
                       trace: torch.Tensor, long_min: Optional[int], chunk_bits: Optional[int]) -> None:
    """bce_settle_trace of ``plan`` from ``table`` into ``trace`` [E, 2] (raw states: they do not
    depend on the decay parameters, reliability.py:161); checks the table and the times."""
    L = N.require_gpu()
    sp, pp = plan.settle, plan.pairs
    S, E, M = sp.n_sources, pp.n_entries, pp.n_markets
    assert table.rel.dtype == torch.float64 and table.conf.dtype == torch.float64 and \
        table.t_us.dtype == torch.int64, "rel / conf must be fp64 and t_us int64"
    assert table.rel.numel() == S and table.conf.numel() == S and table.t_us.numel() == S, \
        "the table must have n_sources rows"
    assert table.present is None or (table.present.dtype == torch.uint8 and table.present.numel() == S), \
        "present must be u8[n_sources]"
    if market_time_us.dtype != torch.int64 or market_time_us.dim() != 1 or market_time_us.numel() != M:
        raise ValueError(f"market_time_us must be int64 with one entry per market ({M})")
    long_min = WALK_LONG_MIN if long_min is None else long_min
    chunk_bits = WALK_CHUNK_BITS if chunk_bits is None else chunk_bits
    n_long, chunk_start, n_chunks = sp.chunks(long_min, chunk_bits)
    N.check(L.bce_settle_trace(N.ptr(sp.bits), sp.n_bits, N.ptr(sp.start), N.ptr(sp.order), sp.n_touched, n_long,
                               N.ptr(chunk_start), n_chunks, int(chunk_bits), S, N.ptr(table.rel),
                               N.ptr(table.conf), N.ptr(table.present), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE,
                               N.ptr(plan.qstart), N.ptr(plan.qpos if E else None),
                               N.ptr(plan.qentry if E else None), E, N.ptr(trace), N.stream(table.rel.device)),
            "bce_settle_trace")


def _walk_read(plan: WalkPlan, table: "ReliabilityTable", market_time_us: torch.Tensor, trace: torch.Tensor,
               relconf: torch.Tensor, bits: torch.Tensor, exists: torch.Tensor, all_present: bool,
               half_life_days: float, min_rel: float) -> None:
    """bce_walk_read from ``trace`` into ``relconf`` (may be ``trace`` itself) / ``bits`` / ``exists``."""
    L = N.require_gpu()
    sp, pp = plan.settle, plan.pairs
    S, E, M = sp.n_sources, pp.n_entries, pp.n_markets
    mtime = market_time_us.contiguous()
    ent = lambda t: N.ptr(t if E else None)  # noqa: E731
    N.check(L.bce_walk_read(E, ent(pp.usid), ent(pp.emarket), ent(plan.qlast), N.ptr(trace),
                            N.ptr(mtime if M else None), M, N.ptr(table.rel), N.ptr(table.conf), N.ptr(table.t_us), N.ptr(table.present), S,
                            float(half_life_days), float(min_rel), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE,
                            int(not all_present), int(plan.n_clamped > 0), N.ptr(relconf), N.ptr(bits),
                            N.ptr(exists), N.stream(table.rel.device)), "bce_walk_read")


def walk_forward(plan: WalkPlan, table: "ReliabilityTable", market_time_us: torch.Tensor, *,
                 offsets: torch.Tensor, prob: torch.Tensor, all_present: bool = True, mode: str = "exact",
                 long_min: Optional[int] = None, chunk_bits: Optional[int] = None, commit: bool = True,
                 **consensus_kwargs) -> WalkResult:
    """The reference run online over a chronological batch, bit-exact: for m = 0..M-1, market m
    is scored by compute_consensus with ``get_reliability(s, scope, apply_decay=True)`` of every
    source read with the clock at ``market_time_us[m]`` (reliability.py:104-140), and then, if
    ``outcome[m] >= 0``, ``update_reliability`` runs for every signal of m in position order and
    stamps ``updated_at = market_time_us[m]`` (reliability.py:142-233).  ``table`` is one dense
    scope (a domain or the global table).  Times need not increase: an equal or earlier time reads
    undecayed.  ``all_present=False`` sets the cold bit of ``usid`` where no row existed at read
    time (``present == 0`` in the start table and no earlier update in the batch).

    :func:`walk_trace` builds the consensus table over the entries, :func:`consensus` runs
    unchanged with ``plan.pairs.esid`` as the ranks (``mode`` and ``consensus_kwargs`` go to it;
    ``bins=`` is its length-bin :class:`Plan`).  ``commit=True`` also leaves the table settled:
    :func:`settle`'s ``rel`` / ``conf`` / ``present`` with ``t_us`` the time of each source's last
    resolved market; ``commit=False`` leaves it untouched.  The result does not depend on
    ``long_min`` / ``chunk_bits`` (defaults WALK_LONG_MIN / WALK_CHUNK_BITS)."""
    sp, pp = plan.settle, plan.pairs
    if offsets.numel() - 1 != pp.n_markets or prob.numel() != pp.esid.numel():
        raise ValueError("offsets / prob are not the batch the plan was built from")
    wtable, exists = walk_trace(plan, table, market_time_us, all_present=all_present, long_min=long_min,
                                chunk_bits=chunk_bits)
    res = consensus(offsets, pp.esid, prob.to(torch.float64), wtable, mode=mode, **_bins_as_plan(consensus_kwargs))
    if commit and sp.n_touched:
        kw = {}
        if long_min is not None:
            kw["long_min"] = long_min
        if chunk_bits is not None:
            kw["chunk_bits"] = chunk_bits
        settle(sp, table.rel, table.conf, table.t_us, table.present, 0, **kw)
        touched = sp.order.to(torch.int64)
        table.t_us.index_copy_(0, touched, market_time_us[plan.slast[touched]])
    return WalkResult(res, plan, exists, sp.total, sp.correct)


# ---------------------------------------------------------------------------------------
# domain scope per market: a batch whose markets belong to different domains
# ---------------------------------------------------------------------------------------
# The rows of the domains are a PairTable with the DOMAIN index in the market's place
# (SQLiteReliabilityStore.load_pair_table(["__domain__:<d>", ...], names) builds it);
# ``market_domain`` int32[M] names the domain of every market, -1 = none.
def scope_resolve(qoffsets: torch.Tensor, qsid: torch.Tensor, pairs: Optional[PairTable], domains: PairTable,
                  market_domain: torch.Tensor, now_us: int, *, emarket: Optional[torch.Tensor] = None,
                  global_scope: Optional[ScopeTable] = None, apply_decay: bool = True, mark_cold: bool = False,
                  index: bool = True, half_life_days: float = DECAY_HALF_LIFE_DAYS,
                  min_rel: float = DECAY_MINIMUM):
    """NamespacedReliabilityStore.get_reliability(sid, market_id=m, domain=domain_of(m),
    apply_decay) for every query entry in one launch (bce_scope_resolve): the pair's market row
    -> the source's row in the market's domain -> ``global_scope`` -> cold start.  The queries
    are those of :func:`pair_resolve`; ``pairs=None`` is ``market_id=None``; ``domains`` holds the
    sparse rows of the D domains, ``market_domain`` int32[M] the domain of every market (-1: none).

    Returns ``(lb, matched, dlb, dmatched, table, scope)``: the market row's lower bound and hit
    as :func:`pair_resolve` gives them, the same for the domain row (``dlb`` is a row index of
    ``domains``, 0 for a market without a domain; written whichever scope was chosen), the
    :class:`SourceTable` over the entry index and the NS_* code of every entry.  ``index=False``
    skips the four index outputs.  A ``market_domain`` outside ``[-1, D)`` or offsets that are
    no segments raise the device fault word (``_native.check_faults``)."""
    L = N.require_gpu()
    M, S, D = market_domain.numel(), domains.n_sources, domains.n_markets
    if pairs is not None and (pairs.n_markets != M or pairs.n_sources != S):
        raise ValueError("the pair table, the domain table and market_domain describe different batches")
    Q = _check_queries(qoffsets, qsid, emarket, M)
    dev = qoffsets.device
    assert market_domain.dtype == torch.int32, "market_domain must be int32"
    lb, matched, relconf, bits, scope = _entry_outputs(Q, dev, index)
    dlb, dmatched = _entry_outputs(Q, dev, index, table=False)[:2]
    glob, gptr = _dense_scope(global_scope, S, "the global scope must have n_sources rows")  # alive until enqueued
    mdom = market_domain.contiguous()
    N.check(L.bce_scope_resolve(N.ptr(qoffsets), M, N.ptr(qsid if Q else None), N.ptr(emarket if Q else None), Q,
                                N.ptr(pairs.poffsets if pairs is not None else None), *_pair_pointers(pairs),
                                pairs.n_rows if pairs is not None else 0, N.ptr(mdom if M else None),
                                N.ptr(domains.poffsets), D, *_pair_pointers(domains), domains.n_rows, S, *gptr,
                                int(bool(apply_decay)), int(now_us), float(half_life_days), float(min_rel),
                                DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE, int(bool(mark_cold)), N.ptr(lb),
                                N.ptr(matched), N.ptr(dlb), N.ptr(dmatched), N.ptr(relconf), N.ptr(bits),
                                N.ptr(scope), N.stream(dev)), "bce_scope_resolve")
    table = SourceTable(relconf, bits, range(Q))  # "names": the entry indices
    return (*_cut(Q, lb, matched, dlb, dmatched), table, *_cut(Q, scope))


@dataclass
class DomainPlan(PairPlan):
    """A CSR batch compiled over its unique (domain, source) pairs: a :class:`PairPlan` whose
    "markets" are the D domains.  One entry per pair over the signals of markets with a domain,
    in (domain, ascending sid) order: ``uoffsets`` int64[D+1], ``usid`` int32[F], ``emarket``
    int32[F] (the DOMAIN of every entry), ``esid`` int32[N] (every signal's entry index; 0, a
    valid placeholder, for the signals of markets without a domain), ``n_markets`` = D, and the
    ``market_domain`` int32[M] it was built from.  The functions that take a :class:`PairPlan`
    and a :class:`PairTable` take this plan and the domain table."""

    market_domain: Optional[torch.Tensor] = None

    @classmethod
    def build(cls, offsets: torch.Tensor, sid: torch.Tensor, market_domain: torch.Tensor, n_sources: int,
              n_domains: int) -> "DomainPlan":
        """Torch only (any device, CPU included), synchronises.  A ``sid`` outside ``[0,
        n_sources)``, a ``market_domain`` entry outside ``[-1, n_domains)``, a ``market_domain``
        of another length than the markets, offsets that do not rise from 0 to ``len(sid)`` or
        2^31 entries: ``ValueError``."""
        M, Nsig = offsets.numel() - 1, sid.numel()
        try:
            S, D = int(n_sources), int(n_domains)
        except (TypeError, ValueError):
            raise ValueError(f"n_sources / n_domains must be integers (got {n_sources!r}, {n_domains!r})") from None
        if M < 0 or offsets.dim() != 1:
            raise ValueError("offsets must be a 1-D tensor of n_markets + 1 entries")
        if M >= (1 << 31):
            raise ValueError(f"{M} markets (the signal-to-market map is int32)")
        if not 0 < S < (1 << 31):
            raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources})")
        if not 0 <= D < (1 << 31):
            raise ValueError(f"n_domains must be in [0, 2^31) (got {n_domains})")
        if market_domain.dim() != 1 or market_domain.numel() != M:
            raise ValueError(f"market_domain must have one entry per market ({M}), got {tuple(market_domain.shape)}")
        dev = offsets.device
        offsets = offsets.to(torch.int64)
        lens = offsets[1:] - offsets[:-1]
        if M and (int(offsets[0]) != 0 or int(offsets[-1]) != Nsig or int(lens.min()) < 0):
            raise ValueError("offsets must rise from 0 to len(sid)")
        if M == 0 and Nsig:
            raise ValueError("offsets must rise from 0 to len(sid)")
        if Nsig and (int(sid.min()) < 0 or int(sid.max()) >= S):
            raise ValueError("a sid is outside [0, n_sources)")
        mdom = market_domain.to(torch.int64)
        if M and (int(mdom.min()) < -1 or int(mdom.max()) >= D):
            raise ValueError("a market_domain entry is outside [-1, n_domains)")
        i64 = dict(dtype=torch.int64, device=dev)
        dom = torch.repeat_interleave(mdom, lens, output_size=Nsig)  # the domain of every signal
        idx = torch.nonzero(dom >= 0).flatten()
        ukey, inv = torch.unique(dom[idx] * S + sid[idx].to(torch.int64), return_inverse=True)  # sorted
        F = ukey.numel()
        if F >= (1 << 31):
            raise ValueError(f"{F} unique (domain, source) pairs (entries are indexed with int32)")
        edom = torch.div(ukey, S, rounding_mode="floor")
        uoffsets = torch.zeros(D + 1, **i64)
        uoffsets[1:] = torch.cumsum(torch.bincount(edom, minlength=D), 0)
        esid = torch.zeros(Nsig, dtype=torch.int32, device=dev)
        esid[idx] = inv.to(torch.int32)
        return cls(uoffsets, (ukey - edom * S).to(torch.int32), edom.to(torch.int32), esid, D, F, S,
                   market_domain.to(torch.int32))


def settle_domains(plan: DomainPlan, domains: PairTable, offsets: torch.Tensor, prob: torch.Tensor,
                   outcome: torch.Tensor, now_us: int, **settle_kwargs):
    """``update_reliability(sid, correct, domain=domain_of(market))`` for every signal of every
    market with ``outcome >= 0`` and a domain (reliability_abstraction.py:211-229).  The chain of
    a (domain, source) pair is that source's signals over the domain's markets in (market,
    position) order -- the reference's loop order.

    This is :func:`settle_pairs` over the (domain, source) entry space, and runs through it: the
    :class:`SettlePlan` keeps the CSR order inside an entry whichever markets its signals come
    from, the outcome of a market without a domain is masked to -1 (its signals carry the
    placeholder entry), and the raw lookup, the chains (long ones chunked) and the merge see the
    D domains where they saw M markets.  Returns ``(new domain table, settle_plan)``."""
    if plan.market_domain.numel() != outcome.numel():
        raise ValueError("outcome must have one entry per market of the plan")
    masked = torch.where(plan.market_domain.to(outcome.device) >= 0, outcome, torch.full_like(outcome, -1))
    return settle_pairs(plan, domains, offsets, prob, masked, now_us, **settle_kwargs)


# ---------------------------------------------------------------------------------------
# namespaced walk-forward: a domain per market, the fallback at every read
# ---------------------------------------------------------------------------------------
@dataclass
class WalkQueries:
    """The queries of one chain family of a :class:`WalkScopePlan`, as :class:`WalkPlan` holds
    them for its single family: ``qstart`` int64[C+1], ``qpos`` int64[Q], ``qentry`` int32[Q],
    ``qlast`` int32[E] (by entry, -1: no earlier bit, or the entry is no query of the family),
    ``slast`` int64[C] (the last market that left a bit in the chain, -1: none)."""

    qstart: torch.Tensor
    qpos: torch.Tensor
    qentry: torch.Tensor
    qlast: torch.Tensor
    slast: torch.Tensor


def _global_outcome(outcome: torch.Tensor, market_domain: torch.Tensor, update_global: bool) -> torch.Tensor:
    """The outcome as the global chains see it: every resolved market with ``update_global``,
    else only those without a domain (reliability_abstraction.py:211-229)."""
    if update_global:
        return outcome
    return torch.where(market_domain.to(outcome.device) < 0, outcome, torch.full_like(outcome, -1))


@dataclass
class WalkScopePlan:
    """A chronological CSR batch whose markets belong to different domains, compiled for
    :func:`walk_forward_scoped`.  ``pairs``: the :class:`PairPlan` over ALL markets (entries E);
    ``dplan``: the :class:`DomainPlan` (chains F) and ``dentry`` int32[E], the domain chain of
    every entry (-1: its market has no domain); ``dsettle`` / ``gsettle``: the
    :class:`SettlePlan` of the domain chains (over the F entry space, as :func:`settle_domains`
    compiles it) and of the global chains (over the S sources: the resolved markets without a
    domain, or every resolved market with ``update_global``); ``dq`` / ``gq``: the
    :class:`WalkQueries` of either family -- every entry is a query of its global chain, and of
    its domain chain where ``dentry >= 0``.  ``n_clamped``: sids outside ``[0, n_sources)``."""

    pairs: PairPlan
    dplan: "DomainPlan"
    dentry: torch.Tensor
    dsettle: SettlePlan
    gsettle: SettlePlan
    dq: WalkQueries
    gq: WalkQueries
    update_global: bool
    n_clamped: int

    @classmethod
    def order(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
              market_domain: torch.Tensor, n_sources: int, n_domains: int, update_global: bool = False):
        """The integer half of :meth:`build` (torch only, CPU tensors included): ``(pairs, dplan,
        dentry, dq, gq, n_clamped)``.  Argument errors as :meth:`WalkPlan.order` and
        :meth:`DomainPlan.build`."""
        M = offsets.numel() - 1
        try:
            S = int(n_sources)
        except (TypeError, ValueError):
            raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources!r})") from None
        if not 0 < S < (1 << 31):
            raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources})")
        if outcome.dtype != torch.int8:
            raise ValueError(f"outcome must be int8 (-1 unresolved, 0, 1), got {outcome.dtype}")
        if outcome.dim() != 1 or outcome.numel() != M:
            raise ValueError(f"outcome must have one entry per market ({M}), got {tuple(outcome.shape)}")
        clamped = sid.to(torch.int32).clamp(0, S - 1)
        n_clamped = int((clamped != sid).sum())
        dplan = DomainPlan.build(offsets, clamped, market_domain, S, n_domains)  # checks market_domain / offsets
        pairs = PairPlan.build(offsets, clamped, prob, S)
        E, F = pairs.n_entries, dplan.n_entries
        usid = pairs.usid[:E].to(torch.int64)
        emarket = pairs.emarket[:E].to(torch.int64)
        edom = dplan.market_domain.to(torch.int64)[emarket]
        # the (domain, source) keys of the DomainPlan ascend: the chain of an entry by search
        fkey = dplan.emarket[:F].to(torch.int64) * S + dplan.usid[:F].to(torch.int64)
        at = torch.searchsorted(fkey, edom.clamp(min=0) * S + usid) if F else torch.zeros_like(usid)
        dentry = torch.where(edom >= 0, at, torch.full_like(at, -1))
        signals = _entry_signals(pairs)
        dq = WalkQueries(*_chain_queries(dentry, signals * (outcome[emarket] >= 0), emarket, max(F, 1),
                                         partial=True))
        gout = _global_outcome(outcome, dplan.market_domain, update_global)
        gq = WalkQueries(*_chain_queries(usid, signals * (gout[emarket] >= 0), emarket, S))
        return pairs, dplan, dentry.to(torch.int32), dq, gq, n_clamped

    @classmethod
    def build(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
              market_domain: torch.Tensor, n_sources: int, n_domains: int, update_global: bool = False,
              check: bool = True) -> "WalkScopePlan":
        """Compile ``(offsets, sid, prob)`` in chronological market order with ``outcome``
        int8[M] (-1 unresolved, 0, 1) and ``market_domain`` int32[M] (-1: none).  Torch sorts and
        scans plus two :meth:`SettlePlan.build`; synchronises.  A ``sid`` outside ``[0,
        n_sources)`` is clamped and raises :class:`BCEError` (``check=False``: the fault is left
        for :func:`walk_forward_scoped`)."""
        update_global = bool(update_global)
        pairs, dplan, dentry, dq, gq, n_clamped = cls.order(offsets, sid, prob, outcome, market_domain, n_sources,
                                                            n_domains, update_global)
        masked = torch.where(dplan.market_domain >= 0, outcome, torch.full_like(outcome, -1))
        dsettle = SettlePlan.build(offsets, dplan.esid, prob, masked, max(dplan.n_entries, 1), check=check)
        gsettle = SettlePlan.build(offsets, sid, prob, _global_outcome(outcome, dplan.market_domain, update_global),
                                   n_sources, check=check)
        if check and n_clamped:  # in a market that feeds no global chain: the compile does not see it
            raise N.BCEError(f"walk scope plan: {n_clamped} sid outside [0, {int(n_sources)})")
        return cls(pairs, dplan, dentry, dsettle, gsettle, dq, gq, update_global, n_clamped)


@dataclass
class WalkScopeResult:
    """:func:`walk_forward_scoped`: ``result`` is the batch's :class:`ConsensusResult` (its
    fields are reachable directly; ``usid`` holds the ENTRY index | cold << 31); ``scope`` u8[E]
    the NS_* code every entry was read at; ``domains`` the NEW domain table (the input one where
    nothing was committed); ``domain_total`` / ``domain_correct`` int64[F] and ``global_total`` /
    ``global_correct`` int64[S]: the chain lengths and their set bits per family."""

    result: ConsensusResult
    plan: WalkScopePlan
    scope: torch.Tensor
    domains: PairTable
    domain_total: torch.Tensor
    domain_correct: torch.Tensor
    global_total: torch.Tensor
    global_correct: torch.Tensor

    __getattr__ = WalkResult.__getattr__
    is_null = WalkResult.is_null


def _walk_scope_read(plan: WalkScopePlan, domains: PairTable, global_table: Optional["ReliabilityTable"],
                     market_time_us: torch.Tensor, pairs: Optional[PairTable], global_has: Optional[torch.Tensor],
                     mark_cold: bool, long_min: Optional[int], chunk_bits: Optional[int], half_life_days: float,
                     min_rel: float):
    """The launches of :func:`walk_scope_trace`; also returns the raw start rows of the domain
    chains (:func:`pair_resolve`, None without one) and the ``has`` flags of the global table."""
    L = N.require_gpu()
    pp, dp = plan.pairs, plan.dplan
    S, E, M, F = pp.n_sources, pp.n_entries, pp.n_markets, dp.n_entries
    if domains.n_markets != dp.n_markets or domains.n_sources != S:
        raise ValueError("the plan and the domain table describe different batches")
    if pairs is not None and (pairs.n_markets != M or pairs.n_sources != S):
        raise ValueError("the plan and the pair table describe different batches")
    if market_time_us.dtype != torch.int64 or market_time_us.dim() != 1 or market_time_us.numel() != M:
        raise ValueError(f"market_time_us must be int64 with one entry per market ({M})")
    g = global_table
    if g is None and plan.gsettle.n_touched:
        raise ValueError("the batch updates the global scope: global_table is needed")
    if g is not None:
        assert g.rel.dtype == torch.float64 and g.conf.dtype == torch.float64 and g.t_us.dtype == torch.int64, \
            "rel / conf must be fp64 and t_us int64"
        assert g.rel.numel() == S and g.conf.numel() == S and g.t_us.numel() == S, \
            "the global table must have n_sources rows"
        assert g.present is None or (g.present.dtype == torch.uint8 and g.present.numel() == S), \
            "present must be u8[n_sources]"
        if global_has is None:
            global_has = g.present if g.present is not None else torch.ones(S, dtype=torch.uint8,
                                                                           device=g.rel.device)
        assert global_has.dtype == torch.uint8 and global_has.numel() == S, "global_has must be u8[n_sources]"
    long_min = WALK_LONG_MIN if long_min is None else long_min
    chunk_bits = WALK_CHUNK_BITS if chunk_bits is None else chunk_bits
    dev = pp.esid.device
    st = N.stream(dev)
    E1 = max(E, 1)
    relconf = torch.empty((E1, 2), dtype=torch.float64, device=dev)  # the global trace, overwritten in place
    bits = torch.zeros(max((E + 31) // 32, 1), dtype=torch.int32, device=dev)
    scope = torch.empty(E1, dtype=torch.uint8, device=dev)
    mtime = market_time_us.contiguous()
    ent = lambda t: N.ptr(t if E else None)  # noqa: E731

    def trace(sp, q, rel, conf, present, out):
        n_long, chunk_start, n_chunks = sp.chunks(long_min, chunk_bits)
        N.check(L.bce_settle_trace(N.ptr(sp.bits), sp.n_bits, N.ptr(sp.start), N.ptr(sp.order), sp.n_touched, n_long,
                                   N.ptr(chunk_start), n_chunks, int(chunk_bits), sp.n_sources, N.ptr(rel),
                                   N.ptr(conf), N.ptr(present), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE,
                                   N.ptr(q.qstart), ent(q.qpos), ent(q.qentry), E, N.ptr(out), st),
                "bce_settle_trace")

    raw = dhas = dtrace = None
    if F and E:  # the domain chains: start rows by the raw pair lookup over the (domain, source) entries
        raw = pair_resolve(dp.uoffsets, dp.usid, domains, 0, mode="raw", emarket=dp.emarket)
        R = domains.n_rows
        dhas = (raw.matched & domains.has[raw.lb.clamp(max=R - 1)]) if R else torch.zeros_like(raw.matched)
        dtrace = torch.empty((E1, 2), dtype=torch.float64, device=dev)
        if plan.dsettle.n_touched:
            trace(plan.dsettle, plan.dq, raw.rel, raw.conf, raw.present, dtrace)
    gtraced = g is not None and plan.gsettle.n_touched > 0
    if gtraced:
        trace(plan.gsettle, plan.gq, g.rel, g.conf, g.present, relconf)
    dom = [N.ptr(x) for x in ((plan.dentry, plan.dq.qlast, dtrace, raw.rel, raw.conf, raw.t_us, dhas)
                              if raw is not None else (None,) * 7)]
    glo = [N.ptr(x) for x in ((plan.gq.qlast if gtraced else None, relconf if gtraced else None, g.rel, g.conf,
                               g.t_us, global_has.contiguous()) if g is not None else (None,) * 6)]
    N.check(L.bce_walk_scope_read(E, ent(pp.usid), ent(pp.emarket), N.ptr(mtime if M else None), M, S,
                                  N.ptr(pairs.poffsets if pairs is not None else None), *_pair_pointers(pairs),
                                  pairs.n_rows if pairs is not None else 0, *dom, F if raw is not None else 0, *glo,
                                  float(half_life_days), float(min_rel), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE,
                                  int(bool(mark_cold)), int(plan.n_clamped > 0), N.ptr(relconf), N.ptr(bits),
                                  N.ptr(scope), st), "bce_walk_scope_read")
    return SourceTable(relconf, bits, range(E)), scope[:E], raw, global_has  # "names": the entry indices


def walk_scope_trace(plan: WalkScopePlan, domains: PairTable, global_table: Optional["ReliabilityTable"],
                     market_time_us: torch.Tensor, *, pairs: Optional[PairTable] = None,
                     global_has: Optional[torch.Tensor] = None, mark_cold: bool = False,
                     long_min: Optional[int] = None, chunk_bits: Optional[int] = None,
                     half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM):
    """The read side of :func:`walk_forward_scoped` alone: one bce_settle_trace per chain family
    that has bits (the domain chains from the raw :func:`pair_resolve` rows of ``plan.dplan``, the
    global chains from the dense table), then bce_walk_scope_read.  Returns the consensus table
    over the entry index -- every entry's namespaced ``get_reliability(apply_decay=True)`` at its
    market's time, after the earlier markets were settled -- and ``scope`` u8[E] (NS_* codes).
    No table is written."""
    return _walk_scope_read(plan, domains, global_table, market_time_us, pairs, global_has, mark_cold, long_min,
                            chunk_bits, half_life_days, min_rel)[:2]


def walk_forward_scoped(plan: WalkScopePlan, domains: PairTable, global_table: Optional["ReliabilityTable"],
                        market_time_us: torch.Tensor, *, offsets: torch.Tensor, prob: torch.Tensor,
                        pairs: Optional[PairTable] = None, global_has: Optional[torch.Tensor] = None,
                        mark_cold: bool = False, mode: str = "exact", long_min: Optional[int] = None,
                        chunk_bits: Optional[int] = None, commit: bool = True,
                        **consensus_kwargs) -> WalkScopeResult:
    """:func:`walk_forward` over NamespacedReliabilityStore, bit-exact: for m = 0..M-1, market m
    is scored by compute_consensus with every source fetched by ``get_reliability(s, market_id,
    domain_of(m), apply_decay=True)`` with the clock at ``market_time_us[m]`` -- the first of the
    market row, the domain row, the global row whose ``updated_at`` is truthy AT THAT TURN, else
    the cold start (reliability_abstraction.py:119-188) -- and then, if ``outcome[m] >= 0``,
    ``update_reliability(s, correct, domain=domain_of(m), update_global=plan.update_global)`` runs
    per signal in position order (:190-239) and stamps the rows it writes with that time.

    ``domains``: the sparse rows of the D domains (a :class:`PairTable` over the domain index; a
    row whose ``has`` is 0 is skipped by reads but is the start of its chain); ``global_table``:
    the dense global scope, ``present`` = a row exists, with ``global_has`` u8[S] = its
    ``updated_at`` is truthy (default: ``present``); None = the scope is not requested, which a
    batch that updates it refuses with ``ValueError``.  ``pairs``: the market-scope rows of the
    batch's markets (read only; None = ``market_id=None``).  ``mark_cold`` sets the cold bit of
    ``usid`` where the read ended at the cold start.

    :func:`walk_scope_trace` builds the consensus table over the entries, :func:`consensus` runs
    unchanged with ``plan.pairs.esid`` as the ranks (``mode`` and ``consensus_kwargs`` go to it;
    ``bins=`` is its length-bin :class:`Plan`).  ``commit=True``: the domain chains are settled on
    their raw start rows, stamped with the time of each chain's last market and merged into a NEW
    :class:`PairTable` (``result.domains``; ``domains`` itself is never written); the global table
    is settled in place as :func:`walk_forward` leaves it, ``global_has`` set for the touched
    sources.  ``commit=False`` leaves every input untouched.  The result does not depend on
    ``long_min`` / ``chunk_bits``."""
    pp = plan.pairs
    if offsets.numel() - 1 != pp.n_markets or prob.numel() != pp.esid.numel():
        raise ValueError("offsets / prob are not the batch the plan was built from")
    wtable, scope, raw, ghas = _walk_scope_read(plan, domains, global_table, market_time_us, pairs, global_has,
                                                mark_cold, long_min, chunk_bits, DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM)
    res = consensus(offsets, pp.esid, prob.to(torch.float64), wtable, mode=mode, **_bins_as_plan(consensus_kwargs))
    ds, gs = plan.dsettle, plan.gsettle
    new_domains = domains
    if commit:
        kw = {}
        if long_min is not None:
            kw["long_min"] = long_min
        if chunk_bits is not None:
            kw["chunk_bits"] = chunk_bits
        if ds.n_touched and raw is not None:
            settle(ds, raw.rel, raw.conf, raw.t_us, raw.present, 0, **kw)
            touched = ds.order.to(torch.int64)
            raw.t_us.index_copy_(0, touched, market_time_us[plan.dq.slast[touched]])
            new_domains = _pair_merge(plan.dplan, domains, raw, ds.total[:plan.dplan.n_entries] > 0)
        if gs.n_touched:
            g = global_table
            settle(gs, g.rel, g.conf, g.t_us, g.present, 0, **kw)
            touched = gs.order.to(torch.int64)
            g.t_us.index_copy_(0, touched, market_time_us[plan.gq.slast[touched]])
            if ghas is not g.present:
                ghas.index_fill_(0, touched, 1)
    return WalkScopeResult(res, plan, scope, new_domains, ds.total, ds.correct, gs.total, gs.correct)


# ---------------------------------------------------------------------------------------
# glob patterns over market ids (include/bce.h "market-id glob patterns")
# ---------------------------------------------------------------------------------------
GLOB_MAX_OPS = 256    # include/bce.h BCE_GLOB_MAX_OPS
GLOB_MAX_RANGES = 64  # include/bce.h BCE_GLOB_MAX_RANGES
_GLOB_LIT, _GLOB_ANY, _GLOB_STAR, _GLOB_CLS = 0 << 29, 1 << 29, 2 << 29, 3 << 29
_GLOB_NEGATE = 1 << 28


class _GlobDeclined(Exception):
    """The pattern is left to fnmatch on the host."""


def _glob_bracket(pat: str, i: int, j: int):
    """The bracket expression pat[i:j] (``i`` just behind '[', ``j`` at the closing ']') as
    fnmatch.translate (CPython 3.10, fnmatch.py:110-151) turns it into a regex set, and that set
    as ``re`` reads it: ``("never" | "any" | "set", negate, [(lo, hi), ...])``."""
    stuff = pat[i:j]
    if "-" not in stuff:
        stuff = stuff.replace("\\", "\\\\")
    else:
        chunks = []
        k = i + 2 if pat[i] == "!" else i + 1
        while True:
            k = pat.find("-", k, j)
            if k < 0:
                break
            chunks.append(pat[i:k])
            i = k + 1
            k = k + 3
        chunk = pat[i:j]
        if chunk:
            chunks.append(chunk)
        else:
            chunks[-1] += "-"
        for k in range(len(chunks) - 1, 0, -1):  # "remove empty ranges"
            if chunks[k - 1][-1] > chunks[k][0]:
                chunks[k - 1] = chunks[k - 1][:-1] + chunks[k][1:]
                del chunks[k]
        stuff = "-".join(s.replace("\\", "\\\\").replace("-", "\\-") for s in chunks)
    for c in "&~|":
        stuff = stuff.replace(c, "\\" + c)
    if not stuff:
        return "never", False, []
    if stuff == "!":
        return "any", False, []
    negate = stuff[0] == "!"
    if negate:
        stuff = stuff[1:]
    elif stuff[0] in "^[":
        stuff = "\\" + stuff
    # the set as sre_parse reads it: every escape left is a backslash in front of punctuation (a
    # literal), an unescaped '-' between two members is a range, a trailing one a member
    toks = []
    k = 0
    while k < len(stuff):
        if stuff[k] == "\\":
            toks.append((ord(stuff[k + 1]), False))
            k += 2
        else:
            toks.append((ord(stuff[k]), stuff[k] == "-"))
            k += 1
    ranges = []
    k = 0
    while k < len(toks):
        lo = toks[k][0]
        k += 1
        if k < len(toks) and toks[k][1]:
            if k + 1 == len(toks):
                ranges += [(lo, lo), (0x2D, 0x2D)]
                break
            hi = toks[k + 1][0]
            k += 2
            if hi < lo:
                raise _GlobDeclined("bad character range")  # re.error in the reference
            ranges.append((lo, hi))
        else:
            ranges.append((lo, lo))
    return "set", negate, ranges


def _glob_compile_one(pat: str):
    """One pattern as ``[op]`` with classes still inline: an op is an int, or ``(negate, ranges)``.
    fnmatch.translate's scan (fnmatch.py:89-153); its second half only anchors the pieces between
    stars, which the iterative matcher does by construction."""
    ops: list = []
    i, n = 0, len(pat)
    while i < n:
        c = pat[i]
        i += 1
        if c == "*":
            if not ops or ops[-1] != _GLOB_STAR:
                ops.append(_GLOB_STAR)
        elif c == "?":
            ops.append(_GLOB_ANY)
        elif c == "[":
            j = i
            if j < n and pat[j] == "!":
                j += 1
            if j < n and pat[j] == "]":
                j += 1
            while j < n and pat[j] != "]":
                j += 1
            if j >= n:
                ops.append(_GLOB_LIT | 0x5B)
            else:
                kind, negate, ranges = _glob_bracket(pat, i, j)
                i = j + 1
                if kind == "any":
                    ops.append(_GLOB_ANY)
                elif kind == "never":
                    ops.append((False, ()))
                else:
                    ranges = sorted(set(ranges))
                    if len(ranges) > GLOB_MAX_RANGES:
                        raise _GlobDeclined("too many ranges")
                    ops.append((negate, tuple(ranges)))
        else:
            ops.append(_GLOB_LIT | ord(c))
    if len(ops) > GLOB_MAX_OPS:
        raise _GlobDeclined("too many ops")
    return ops


@dataclass
class NameTable:
    """Names packed for the matcher: UTF-8 bytes ('surrogatepass') and int64 offsets [M+1], on the
    host and -- when built with a device -- in HBM; ``strings`` serves the declined patterns."""

    strings: List[str]
    bytes_host: np.ndarray
    off_host: np.ndarray
    data: Optional[torch.Tensor] = None
    off: Optional[torch.Tensor] = None

    @property
    def n(self) -> int:
        return len(self.strings)

    @classmethod
    def from_strings(cls, names: Sequence[str], device=None) -> "NameTable":
        strings = list(names)
        enc = [s.encode("utf-8", "surrogatepass") for s in strings]
        off = np.zeros(len(enc) + 1, np.int64)
        if enc:
            np.cumsum(np.fromiter(map(len, enc), np.int64, len(enc)), out=off[1:])
        data = np.frombuffer(b"".join(enc), np.uint8)
        if data.size == 0:
            data = np.zeros(1, np.uint8)
        t = cls(strings, data, off)
        if device is not None:
            t.data = torch.from_numpy(data.copy()).to(device)
            t.off = torch.from_numpy(off).to(device)
        return t


@dataclass
class GlobSet:
    """Compiled patterns (host arrays, include/bce.h): ``patterns`` are the distinct patterns in
    first-seen order, ``index[i]`` the row of the i-th pattern given, ``declined`` the rows whose
    pattern is over a cap (or that fnmatch itself rejects) and is evaluated by fnmatch on the host."""

    patterns: List[str]
    index: List[int]
    prog: np.ndarray      # uint32 [n_ops]
    prog_off: np.ndarray  # int64 [P+1]
    cls_rng: np.ndarray   # uint32 [2 * n_rng]
    cls_off: np.ndarray   # int32 [n_cls+1]
    declined: List[int]

    @property
    def n(self) -> int:
        return len(self.patterns)

    @property
    def n_cls(self) -> int:
        return len(self.cls_off) - 1

    @classmethod
    def compile(cls, patterns: Sequence[str]) -> "GlobSet":
        row: Dict[str, int] = {}
        index = []
        for p in patterns:
            if p not in row:
                row[p] = len(row)
            index.append(row[p])
        classes: Dict[tuple, int] = {}
        prog: List[int] = []
        prog_off = [0]
        declined = []
        for p, r in row.items():
            try:
                ops = _glob_compile_one(p)
            except Exception:  # over a cap, or malformed for translate() itself: fnmatch answers (or raises)
                ops = None
                declined.append(r)
            for op in ops or ():
                if isinstance(op, tuple):
                    c = classes.setdefault(op[1], len(classes))
                    op = _GLOB_CLS | (_GLOB_NEGATE if op[0] else 0) | c
                prog.append(op)
            prog_off.append(len(prog))
        rng: List[int] = []
        cls_off = [0]
        for ranges in classes:  # insertion order == class index
            for lo, hi in ranges:
                rng += [lo, hi]
            cls_off.append(len(rng) // 2)
        return cls(list(row), index, np.array(prog, np.uint32), np.array(prog_off, np.int64),
                   np.array(rng, np.uint32), np.array(cls_off, np.int32), declined)


def _glob_host_row(names: NameTable, pattern: str) -> np.ndarray:
    """One bitmap row by fnmatch itself (a declined pattern): uint64 [ceil(M / 64)]."""
    import fnmatch

    M = names.n
    hit = np.zeros(((M + 63) // 64) * 64, np.uint8)
    hit[:M] = np.fromiter((fnmatch.fnmatchcase(s, pattern) for s in names.strings), np.uint8, M)
    return np.packbits(hit, bitorder="little").view(np.uint64)


def _np_or_dummy(a: np.ndarray, dtype) -> np.ndarray:
    return a if a.size else np.zeros(2, dtype)


def glob_match_host(names: NameTable, globs: GlobSet) -> np.ndarray:
    """The bitmap uint64 [P][ceil(M / 64)] by the CPU build of the matcher (bce_glob_match_host):
    no GPU.  Declined patterns are answered by fnmatch."""
    L = N.lib()
    M, P = names.n, globs.n
    bits = np.zeros((P, (M + 63) // 64), np.uint64)
    N.check(L.bce_glob_match_host(N.ptr(names.bytes_host), int(names.off_host[-1]), N.ptr(names.off_host), M,
                                  N.ptr(_np_or_dummy(globs.prog, np.uint32)), globs.prog.size,
                                  N.ptr(globs.prog_off), P, N.ptr(_np_or_dummy(globs.cls_rng, np.uint32)),
                                  globs.cls_rng.size // 2, N.ptr(globs.cls_off), globs.n_cls, N.ptr(bits)),
            "bce_glob_match_host")
    for r in globs.declined:
        bits[r] = _glob_host_row(names, globs.patterns[r])
    return bits


def glob_match(names: NameTable, globs: GlobSet, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Every pattern against every name in one launch (bce_glob_match): int64 [P][ceil(M / 64)]
    holding the 64-bit words, bit ``m % 64`` of word ``m // 64`` of row p set iff
    ``fnmatch.fnmatchcase(names[m], patterns[p])``.  Rows of declined patterns are computed by
    fnmatch on the host and uploaded."""
    L = N.require_gpu()
    if names.data is None:
        raise ValueError("glob_match needs a NameTable built with a device")
    dev = names.data.device
    M, P = names.n, globs.n
    nw = (M + 63) // 64
    bits = out if out is not None else torch.empty((P, nw), dtype=torch.int64, device=dev)
    assert bits.shape == (P, nw) and bits.dtype == torch.int64 and bits.is_contiguous()
    T = lambda a, dt: torch.from_numpy(_np_or_dummy(a, a.dtype).view(dt)).to(dev)  # noqa: E731
    prog, rng = T(globs.prog, np.int32), T(globs.cls_rng, np.int32)
    poff, coff = T(globs.prog_off, np.int64), T(globs.cls_off, np.int32)
    N.check(L.bce_glob_match(N.ptr(names.data), int(names.off_host[-1]), N.ptr(names.off), M, N.ptr(prog),
                             globs.prog.size, N.ptr(poff), P, N.ptr(rng), globs.cls_rng.size // 2, N.ptr(coff),
                             globs.n_cls, N.ptr(bits), N.stream(dev)), "bce_glob_match")
    for r in globs.declined:
        bits[r] = torch.from_numpy(_glob_host_row(names, globs.patterns[r]).view(np.int64)).to(dev)
    return bits


def glob_count(bits: torch.Tensor, n_names: int, rows: torch.Tensor) -> torch.Tensor:
    """Set bits of ``bits[rows[r]]`` per slot r (bce_glob_count): int64 [R]."""
    L = N.require_gpu()
    R = rows.numel()
    cnt = torch.empty(max(R, 1), dtype=torch.int64, device=bits.device)
    N.check(L.bce_glob_count(N.ptr(bits), n_names, bits.shape[0], N.ptr(rows), R, N.ptr(cnt),
                             N.stream(bits.device)), "bce_glob_count")
    return cnt[:R]


def glob_members(bits: torch.Tensor, n_names: int, rows: torch.Tensor, slot_groups) -> tuple:
    """Member lists for bce_aggregate_groups from the bitmap: slot r holds the set bit positions of
    row ``rows[r]`` ascending (store order), group g is the slots ``slot_groups[g] ..
    slot_groups[g+1]`` (int64 [G+1], host or device), so a group lists its patterns' matches in
    pattern order with duplicates kept (market.py:352-357).  Count, cumulative sum (torch; one
    host read sizes ``members``), fill.  Returns ``(group_offsets [G+1], members)``."""
    L = N.require_gpu()
    dev = bits.device
    R = rows.numel()
    cnt = glob_count(bits, n_names, rows)
    slot_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, out=slot_off[1:])
    total = int(slot_off[-1].item())
    members = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    N.check(L.bce_glob_fill(N.ptr(bits), n_names, bits.shape[0], N.ptr(rows), R, N.ptr(slot_off), total,
                            N.ptr(members), N.stream(dev)), "bce_glob_fill")
    sg = torch.as_tensor(slot_groups, dtype=torch.int64).to(dev)
    return slot_off[sg], members[:total]


def glob_any(bits: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """OR of the listed rows: one word row int64 [ceil(M / 64)] ("any of these patterns")."""
    sel = bits.index_select(0, rows)
    if sel.shape[0] == 0:
        return torch.zeros(bits.shape[1], dtype=torch.int64, device=bits.device)
    while sel.shape[0] > 1:
        h = sel.shape[0] // 2
        sel = torch.cat([sel[:h] | sel[h:2 * h], sel[2 * h:]])
    return sel[0]


def glob_mask(words: torch.Tensor, n_names: int) -> torch.Tensor:
    """A word row as bool [M]."""
    sh = torch.arange(64, dtype=torch.int64, device=words.device)
    return (((words.unsqueeze(1) >> sh) & 1) != 0).reshape(-1)[:n_names]


# ---------------------------------------------------------------------------------------
# scoring a back-test: Brier score, log loss, hits and calibration per group
# ---------------------------------------------------------------------------------------
SCORE_SEG = N.SCORE_SEG          # items of a segment (include/bce.h BCE_SCORE_SEG)
SCORE_LANES = N.SCORE_LANES      # lane partials of a segment
SCORE_MAX_BINS = N.SCORE_MAX_BINS
SCORE_COUNTS = ("n_scored", "n_hit", "n_unresolved", "n_null", "n_bad")
SCORE_SUMS = ("brier", "logloss", "brier_base")


def _score_segments(group_offsets: torch.Tensor) -> torch.Tensor:
    """``seg_start`` int64[G+1] of bce_score_groups: ``max(1, ceil(n_g / SCORE_SEG))`` segments per
    group, cumulated (torch only, any device; a decreasing offset counts as an empty group)."""
    lens = (group_offsets[1:] - group_offsets[:-1]).clamp(min=0)
    nseg = ((lens + (SCORE_SEG - 1)) // SCORE_SEG).clamp(min=1)
    seg_start = torch.zeros(group_offsets.numel(), dtype=torch.int64, device=group_offsets.device)
    torch.cumsum(nseg, 0, out=seg_start[1:])
    return seg_start


@dataclass
class ScorePlan:
    """Item lists compiled for :func:`score`: ``group_offsets`` int64[G+1], ``pidx`` int64[n_items]
    (the forecast every item reads), ``oidx`` int64[n_items] or None (= ``pidx``: the market every
    item is scored against) and the segment table ``seg_start`` int64[G+1] / ``seg_group`` int64
    [n_segments] (``n_segments`` = the last entry of ``seg_start``, read once on the host when the
    plan is built).  ``n_clamped``: sids outside
    ``[0, n_sources)`` that :meth:`by_source` clamped."""

    group_offsets: torch.Tensor
    pidx: torch.Tensor
    oidx: Optional[torch.Tensor]
    seg_start: torch.Tensor
    n_segments: int
    n_clamped: int = 0
    seg_group: Optional[torch.Tensor] = None  # int64[n_segments]: the group of every segment

    def __post_init__(self):
        if self.seg_group is None:
            G = self.seg_start.numel() - 1
            self.seg_group = torch.repeat_interleave(
                torch.arange(G, dtype=torch.int64, device=self.seg_start.device),
                self.seg_start[1:] - self.seg_start[:-1], output_size=self.n_segments)

    @property
    def n_groups(self) -> int:
        return int(self.group_offsets.numel()) - 1

    @property
    def n_items(self) -> int:
        return int(self.pidx.numel())

    @classmethod
    def groups(cls, group_offsets: torch.Tensor, members: torch.Tensor, oidx: Optional[torch.Tensor] = None,
               check: bool = True) -> "ScorePlan":
        """Market groups: group g scores the markets ``members[group_offsets[g] : group_offsets
        [g+1]]`` (what :func:`glob_members` returns; overlaps and duplicates kept).  ``check``:
        offsets that decrease or leave the members raise ``ValueError`` here; ``check=False``
        leaves them to the kernel, which raises the device fault word."""
        if group_offsets.dim() != 1 or group_offsets.numel() < 1:
            raise ValueError("group_offsets must be a 1-D tensor of n_groups + 1 entries")
        if members.dim() != 1 or (oidx is not None and oidx.shape != members.shape):
            raise ValueError("members (and oidx) must be 1-D and of one length")
        goff = group_offsets.to(torch.int64).contiguous()
        if check and goff.numel() > 1:
            d = goff[1:] - goff[:-1]
            if int(goff[0]) < 0 or int(goff[-1]) > members.numel() or int(d.min()) < 0:
                raise ValueError("group_offsets must rise inside [0, len(members)]")
        seg_start = _score_segments(goff)
        return cls(goff, members.to(torch.int64).contiguous(),
                   None if oidx is None else oidx.to(torch.int64).contiguous(), seg_start, int(seg_start[-1]))

    @classmethod
    def whole(cls, n_markets: int, device=None) -> "ScorePlan":
        """One group of all markets 0 .. n_markets - 1."""
        M = int(n_markets)
        if M < 0:
            raise ValueError(f"n_markets must be >= 0 (got {n_markets})")
        goff = torch.tensor([0, M], dtype=torch.int64, device=device)
        return cls.groups(goff, torch.arange(M, dtype=torch.int64, device=device), check=False)

    @classmethod
    def by_source(cls, offsets: torch.Tensor, sid: torch.Tensor, n_sources: int) -> "ScorePlan":
        """One group per source over the signals of a CSR batch: ``pidx`` = the signal indices
        stably sorted by ``sid`` (a source's signals in market, then position order, duplicates
        kept: every signal counts, market.py:293-304), ``oidx`` = the market of each.  A ``sid``
        outside ``[0, n_sources)`` is clamped and counted in ``n_clamped``, as
        :meth:`WalkPlan.order` does.  Torch only (CPU tensors included)."""
        M = offsets.numel() - 1
        try:
            S = int(n_sources)
        except (TypeError, ValueError):
            raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources!r})") from None
        if not 0 < S < (1 << 31):
            raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources})")
        if M < 0 or offsets.dim() != 1:
            raise ValueError("offsets must be a 1-D tensor of n_markets + 1 entries")
        Nsig = sid.numel()
        offsets = offsets.to(torch.int64)
        lens = offsets[1:] - offsets[:-1]
        if (M and (int(offsets[0]) != 0 or int(offsets[-1]) != Nsig or int(lens.min()) < 0)) or (M == 0 and Nsig):
            raise ValueError("offsets must rise from 0 to len(sid)")
        dev = offsets.device
        clamped = sid.to(torch.int64).clamp(0, S - 1)
        n_clamped = int((clamped != sid).sum())
        market = torch.repeat_interleave(torch.arange(M, dtype=torch.int64, device=dev), lens, output_size=Nsig)
        _, perm = torch.sort(clamped, stable=True)
        goff = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(clamped, minlength=S), 0, out=goff[1:])
        seg_start = _score_segments(goff)
        return cls(goff, perm.contiguous(), market[perm].contiguous(), seg_start, int(seg_start[-1]), n_clamped)


def _nan_div(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / den in fp64, NaN where den == 0."""
    den = den.to(torch.float64)
    nan = torch.full_like(den, float("nan"))
    return torch.where(den > 0, num.to(torch.float64) / torch.where(den > 0, den, torch.ones_like(den)), nan)


@dataclass
class ScoreResult:
    """:func:`score`: the raw tensors of bce_score_groups -- ``counts`` int64[..., G, 5]
    (SCORE_COUNTS), ``sums`` fp64[..., G, 3] (SCORE_SUMS), ``bin_n`` / ``bin_pos`` int64[..., G, B],
    ``bin_psum`` fp64[..., G, B] -- and the scores derived from them in torch.  Every mean is NaN
    where ``n_scored == 0``.  Leading dimensions (the grid of :func:`walk_sweep`) carry through."""

    counts: torch.Tensor
    sums: torch.Tensor
    bin_n: torch.Tensor
    bin_pos: torch.Tensor
    bin_psum: torch.Tensor
    has_base: bool = False

    @property
    def n_scored(self) -> torch.Tensor:
        return self.counts[..., 0]

    @property
    def n_hit(self) -> torch.Tensor:
        return self.counts[..., 1]

    @property
    def n_unresolved(self) -> torch.Tensor:
        return self.counts[..., 2]

    @property
    def n_null(self) -> torch.Tensor:
        return self.counts[..., 3]

    @property
    def n_bad(self) -> torch.Tensor:
        return self.counts[..., 4]

    @property
    def brier(self) -> torch.Tensor:
        return _nan_div(self.sums[..., 0], self.n_scored)

    @property
    def log_loss(self) -> torch.Tensor:
        return _nan_div(self.sums[..., 1], self.n_scored)

    @property
    def brier_base(self) -> torch.Tensor:
        return _nan_div(self.sums[..., 2], self.n_scored)

    @property
    def accuracy(self) -> torch.Tensor:
        return _nan_div(self.n_hit, self.n_scored)

    @property
    def skill(self) -> torch.Tensor:
        """``brier - brier_base``: negative = better than the base forecast on the same items."""
        if not self.has_base:
            raise ValueError("skill needs score(base=...)")
        return self.brier - self.brier_base

    @property
    def calibration(self):
        """``(mean forecast, observed frequency)`` per bin, fp64[..., G, B], NaN in empty bins."""
        return _nan_div(self.bin_psum, self.bin_n), _nan_div(self.bin_pos, self.bin_n)

    @property
    def ece(self) -> torch.Tensor:
        """Expected calibration error: sum over bins of ``bin_n / n_scored * |mean - observed|``."""
        mean, obs = self.calibration
        gap = torch.where(self.bin_n > 0, (mean - obs).abs(), torch.zeros_like(mean))
        return _nan_div((gap * self.bin_n.to(torch.float64)).sum(-1), self.n_scored)

    @staticmethod
    def merge(parts: Sequence["ScoreResult"]) -> "ScoreResult":
        """The shards of one set of groups added left to right (fp64 sums in list order)."""
        parts = list(parts)
        if not parts:
            raise ValueError("merge needs at least one ScoreResult")
        first = parts[0]
        acc = [t.clone() for t in (first.counts, first.sums, first.bin_n, first.bin_pos, first.bin_psum)]
        for p in parts[1:]:
            if p.bin_n.shape != first.bin_n.shape or p.has_base != first.has_base:
                raise ValueError("merge: the parts differ in groups, bins or base")
            for a, t in zip(acc, (p.counts, p.sums, p.bin_n, p.bin_pos, p.bin_psum)):
                a += t
        return ScoreResult(*acc, has_base=first.has_base)

    @staticmethod
    def stack(parts: Sequence["ScoreResult"]) -> "ScoreResult":
        """The parts along a new leading dimension."""
        parts = list(parts)
        return ScoreResult(*(torch.stack([getattr(p, k) for p in parts])
                             for k in ("counts", "sums", "bin_n", "bin_pos", "bin_psum")),
                           has_base=bool(parts) and parts[0].has_base)


def score(plan: ScorePlan, value: torch.Tensor, outcome: torch.Tensor, *, valid: Optional[torch.Tensor] = None,
          base: Optional[torch.Tensor] = None, n_bins: int = 10, eps: float = 1e-15,
          scratch: Optional[torch.Tensor] = None) -> ScoreResult:
    """Score the forecasts ``value`` fp64 against ``outcome`` int8[M] (-1 unresolved, 0, 1) per
    group of ``plan`` in one call of bce_score_groups (no host synchronisation): item i reads
    ``value[pidx[i]]`` and the market ``oidx[i]``; ``valid`` u8 / bool [M] (0: the market's
    consensus is None) and ``base`` fp64[M] (a second forecast of the market, scored over the same
    items) are optional.  The sums are reproducible to the bit: they depend on the arguments
    alone (include/bce.h: the reduction shape).  Indices outside their array count as ``n_bad``
    and raise the device fault word (``_native.check_faults``)."""
    L = N.require_gpu()
    B = int(n_bins)
    if not 1 <= B <= SCORE_MAX_BINS:
        raise ValueError(f"n_bins must be in [1, {SCORE_MAX_BINS}] (got {n_bins})")
    if not float(eps) >= 0.0:
        raise ValueError(f"eps must be >= 0 (got {eps})")
    if outcome.dtype != torch.int8 or outcome.dim() != 1:
        raise ValueError(f"outcome must be int8[M] (-1 unresolved, 0, 1), got {outcome.dtype}")
    if value.dtype != torch.float64 or value.dim() != 1:
        raise ValueError("value must be a 1-D fp64 tensor")
    M = outcome.numel()
    if valid is not None:
        if valid.dim() != 1 or valid.numel() != M:
            raise ValueError(f"valid must have one entry per market ({M})")
        valid = valid.to(torch.uint8).contiguous()
    if base is not None:
        if base.dtype != torch.float64 or base.dim() != 1 or base.numel() != M:
            raise ValueError(f"base must be fp64 with one entry per market ({M})")
        base = base.contiguous()
    dev = value.device
    G, n_seg = plan.n_groups, plan.n_segments
    G1 = max(G, 1)
    i64 = dict(dtype=torch.int64, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    r = ScoreResult(torch.zeros((G1, 5), **i64), torch.zeros((G1, 3), **f64), torch.zeros((G1, B), **i64),
                    torch.zeros((G1, B), **i64), torch.zeros((G1, B), **f64), has_base=base is not None)
    sb = int(L.bce_score_scratch_bytes(n_seg, B))
    if scratch is None or scratch.numel() * scratch.element_size() < sb:
        scratch = torch.empty(max(sb // 8, 1), **i64)
    value, outcome = value.contiguous(), outcome.contiguous()
    n_items = plan.n_items
    N.check(L.bce_score_groups(N.ptr(plan.group_offsets), G, N.ptr(plan.seg_start), N.ptr(plan.seg_group), n_seg,
                               N.ptr(plan.pidx if n_items else None), N.ptr(plan.oidx if n_items else None), n_items,
                               N.ptr(value if value.numel() else None), value.numel(),
                               N.ptr(outcome if M else None), N.ptr(valid if M else None),
                               N.ptr(base if M else None), M, B, float(eps), N.ptr(scratch), sb, N.ptr(r.counts),
                               N.ptr(r.sums), N.ptr(r.bin_n), N.ptr(r.bin_pos), N.ptr(r.bin_psum), N.stream(dev)),
            "bce_score_groups")
    return ScoreResult(r.counts[:G], r.sums[:G], r.bin_n[:G], r.bin_pos[:G], r.bin_psum[:G], r.has_base)


def score_markets(res, offsets: torch.Tensor, outcome: torch.Tensor, plan: Optional[ScorePlan] = None,
                  **kw) -> ScoreResult:
    """:func:`score` of the consensus of a :class:`ConsensusResult`, :class:`WalkResult` or
    :class:`WalkScopeResult` over the batch's markets: ``valid = ~res.is_null(offsets)``;
    ``plan`` defaults to one group of all markets (:meth:`ScorePlan.whole`)."""
    M = offsets.numel() - 1
    if plan is None:
        plan = ScorePlan.whole(M, device=offsets.device)
    return score(plan, res.consensus, outcome, valid=~res.is_null(offsets), **kw)


def score_sources(plan: ScorePlan, prob: torch.Tensor, outcome: torch.Tensor,
                  consensus: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None,
                  **kw) -> ScoreResult:
    """:func:`score` of every source's own signals (``plan`` from :meth:`ScorePlan.by_source``).
    With ``consensus`` fp64[M] as the base forecast, ``skill`` is a source's Brier score minus the
    consensus's on the markets it forecast (``valid``: leave out markets whose consensus is None)."""
    return score(plan, prob.to(torch.float64), outcome, valid=valid, base=consensus, **kw)


def walk_sweep(plan: WalkPlan, table: "ReliabilityTable", market_time_us: torch.Tensor, *, offsets: torch.Tensor,
               prob: torch.Tensor, half_life_days: Sequence[float], min_rel: Sequence[float],
               score_plan: Optional[ScorePlan] = None, keep_consensus: bool = False, all_present: bool = True,
               mode: str = "exact", long_min: Optional[int] = None, chunk_bits: Optional[int] = None,
               n_bins: int = 10, eps: float = 1e-15, **consensus_kwargs):
    """:func:`walk_forward` (``commit=False``) for every point of a grid of decay parameters,
    scored against the plan's outcomes.  ``update_reliability`` reads without decay
    (reliability.py:161), so the settlement chains -- the trace -- do not depend on
    ``half_life_days`` / ``min_rel``: bce_settle_trace runs ONCE, and every grid point
    ``(half_life_days[i], min_rel[j])`` (row-major, ``min_rel`` fastest) runs bce_walk_read from
    that trace into a second table, :func:`consensus` and :func:`score`.  The table is never
    written; the read table, the consensus outputs and the scoring scratch are allocated once.
    Returns ``(scores, consensus)``: a :class:`ScoreResult` with a leading grid dimension
    ``[len(half_life_days) * len(min_rel), G, ...]`` over ``score_plan`` (default: one group of all
    markets) and, with ``keep_consensus``, the fp64 ``[K, M]`` consensus and bool ``[K, M]``
    null mask of every point (else None)."""
    sp, pp = plan.settle, plan.pairs
    hl, mr = [float(x) for x in half_life_days], [float(x) for x in min_rel]
    if not hl or not mr:
        raise ValueError("walk_sweep needs at least one half_life_days and one min_rel")
    if plan.outcome is None:
        raise ValueError("walk_sweep needs a WalkPlan from WalkPlan.build (it keeps the outcomes)")
    if offsets.numel() - 1 != pp.n_markets or prob.numel() != pp.esid.numel():
        raise ValueError("offsets / prob are not the batch the plan was built from")
    M, E = pp.n_markets, pp.n_entries
    dev = table.rel.device
    if score_plan is None:
        score_plan = ScorePlan.whole(M, device=dev)
    trace, _, _ = _walk_buffers(E, dev)
    relconf, bits, exists = _walk_buffers(E, dev)
    _walk_settle_trace(plan, table, market_time_us, trace, long_min, chunk_bits)
    prob = prob.to(torch.float64)
    kw = _bins_as_plan(consensus_kwargs)
    unique = kw.pop("unique_outputs", False)
    validate = kw.pop("validate", False)
    if kw.get("plan") is None and kw.get("max_len") is None:
        kw["plan"] = Plan.build_device(offsets)  # the length bins once, not once per grid point
    out = _alloc(M, pp.esid.numel(), dev, unique, validate)
    L = N.require_gpu()
    sb = int(L.bce_score_scratch_bytes(score_plan.n_segments, int(n_bins))) if 1 <= int(n_bins) <= SCORE_MAX_BINS else 8
    scratch = torch.empty(max(sb // 8, 1), dtype=torch.int64, device=dev)
    wtable = SourceTable(relconf, bits, range(E))
    empty = offsets[1:] == offsets[:-1]
    parts, cons, nulls = [], [], []
    for h in hl:
        for m in mr:
            _walk_read(plan, table, market_time_us, trace, relconf, bits, exists, all_present, h, m)
            res = consensus(offsets, pp.esid, prob, wtable, mode=mode, unique_outputs=unique, validate=validate,
                            out=out, **kw)
            null = (res.total_weight == 0) | empty
            parts.append(score(score_plan, res.consensus, plan.outcome, valid=~null, n_bins=n_bins, eps=eps,
                               scratch=scratch))
            if keep_consensus:
                cons.append(res.consensus.clone())
                nulls.append(null)
    scores = ScoreResult.stack(parts)
    return scores, ((torch.stack(cons), torch.stack(nulls)) if keep_consensus else None)
