"""Consensus history: every market's consensus after each of its signals arrived."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _native as N
from .tables import SourceTable
from .consensus import ConsensusResult, Plan
from .walk import WalkScopePlan, walk_scope_trace, walk_trace
from .score import ScorePlan, ScoreResult, score

HISTORY_MAX_LEN = 4096  # the longest market the history kernels take (the wide kernels' limit)


def _alloc_per_signal(n_signals: int, device):
    """The four uninitialised per-signal arrays (fp64 x 3, int32) of a per-signal result."""
    f64 = dict(dtype=torch.float64, device=device)
    n = max(int(n_signals), 1)
    return (torch.empty(n, **f64)[:n_signals], torch.empty(n, **f64)[:n_signals],
            torch.empty(n, **f64)[:n_signals], torch.empty(n, dtype=torch.int32, device=device)[:n_signals])


@dataclass
class HistoryResult:
    """:func:`consensus_history`: one point per signal, at the signal's CSR position.  Point k of
    a market is ``compute_consensus`` of its first k + 1 signals."""

    consensus: torch.Tensor      # fp64[N]  (0.0 where null)
    confidence: torch.Tensor     # fp64[N]  (0.0 where null)
    total_weight: torch.Tensor   # fp64[N]
    n_unique: torch.Tensor       # int32[N]

    @classmethod
    def alloc(cls, n_signals: int, device) -> "HistoryResult":
        """Uninitialised outputs for ``n_signals`` points."""
        return cls(*_alloc_per_signal(n_signals, device))

    def is_null(self) -> torch.Tensor:
        """bool[N]: consensus is None at the point (total weight == 0, core.py:131)."""
        return self.total_weight == 0

    def last(self, offsets: torch.Tensor) -> ConsensusResult:
        """The four per-market arrays gathered at every market's last point -- what
        :func:`consensus` returns for the batch; an empty market reads as null (zeros).  The
        per-unique outputs and ``err_idx`` are None."""
        lens = offsets[1:] - offsets[:-1]
        has = lens > 0
        at = (offsets[1:] - 1).clamp(min=0)
        if self.consensus.numel() == 0:
            M = lens.numel()
            z = torch.zeros(M, dtype=torch.float64, device=offsets.device)
            return ConsensusResult(z, z.clone(), z.clone(), torch.zeros(M, dtype=torch.int32, device=offsets.device),
                                   None, None, None, None)
        pick = lambda t: torch.where(has, t[at], torch.zeros((), dtype=t.dtype, device=t.device))  # noqa: E731
        return ConsensusResult(pick(self.consensus), pick(self.confidence), pick(self.total_weight),
                               pick(self.n_unique), None, None, None, None)


def _per_signal(name: str, entry: str, offsets, sid, prob, table, outputs, plan, max_len, offsets_host, check):
    """The routes :func:`consensus_history` and :func:`leave_one_out` share (documented there):
    validates ``max_len``, refuses a market over ``HISTORY_MAX_LEN`` signals where the host knows
    the lengths (a ``ValueError`` that starts with ``name``), picks the route, calls ``entry`` and
    checks its status.  ``outputs(M, Nsig, dev)`` is called once the arguments have passed and
    returns the result, whose four per-signal arrays the entry takes, and the pointers the entry
    takes behind them; the result is returned."""
    def too_long(market: int, n: int) -> ValueError:
        return ValueError(f"{name}: market {market} has {n} signals; the longest market it takes has "
                          f"{HISTORY_MAX_LEN}")

    if max_len is not None and not 0 < int(max_len) <= HISTORY_MAX_LEN:
        raise ValueError(f"max_len must be in [1, {HISTORY_MAX_LEN}] (got {max_len})")
    if offsets_host is not None:
        lens = np.diff(np.asarray(offsets_host, np.int64))
        if lens.size and int(lens.max()) > HISTORY_MAX_LEN:
            m = int(np.argmax(lens > HISTORY_MAX_LEN))
            raise too_long(m, int(lens[m]))
        if plan is None and max_len is None:
            max_len = max(int(lens.max(initial=0)), 1)
            if max_len > 64:
                plan = Plan.build(offsets_host, offsets.device)
    M = offsets.numel() - 1
    Nsig = sid.numel()
    dev = offsets.device
    call = getattr(N.require_gpu(), entry)
    if plan is None and max_len is None:
        plan = Plan.build_device(offsets)
    if plan is not None:
        b = plan.bin_start
        if b[N.NBINS] > b[N.NBINS - 1]:
            m = int(plan.order[int(b[N.NBINS - 1])])
            raise too_long(m, int(offsets[m + 1] - offsets[m]))
    res, more = outputs(M, Nsig, dev)
    common = (N.ptr(offsets), M, N.ptr(sid), N.ptr(prob), Nsig, N.ptr(table.relconf), N.ptr(table.bits), table.n)
    outs = (N.ptr(res.consensus), N.ptr(res.confidence), N.ptr(res.total_weight), N.ptr(res.n_unique), *more)
    st = N.stream(dev)
    null = N.ptr(None)
    if plan is not None:
        rc = call(*common, N.ptr(plan.order), int(plan.bin_start[N.NBINS]),
                  N.ptr(np.ascontiguousarray(plan.bin_start, np.int64)), null, 0, *outs, st)
    elif max_len <= 64:
        rc = call(*common, null, 0, null, null, int(max_len), *outs, st)
    else:  # planned on the device under the caller's bound: no host synchronisation
        order, bins = Plan.device_bins_async(offsets, st)
        rc = call(*common, N.ptr(order), M, null, N.ptr(bins), 0, *outs, st)
    N.check(rc, entry)
    if check:
        N.check_faults(dev, name)
    return res


def consensus_history(offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, table: SourceTable, *,
                      plan: Optional[Plan] = None, max_len: Optional[int] = None,
                      offsets_host: Optional[np.ndarray] = None, out: Optional[HistoryResult] = None,
                      check: bool = False) -> HistoryResult:
    """``compute_consensus(signals[:k + 1], table)`` for every prefix of every CSR market, in one
    pass over the signals (bce_consensus_history): point k of market m lands at position
    ``offsets[m] + k`` of the four fp64 / int32 [N] outputs.  Bit-identical to :func:`consensus` on
    the batch expanded into its prefixes, which reads (n + 1) / 2 times the signals.  Exact order
    only, no per-unique outputs; probabilities outside [0, 1] are computed (:func:`validate` is
    the range check).  The arithmetic is quadratic in a market's length; markets of up to
    ``HISTORY_MAX_LEN`` signals.

    Routes, as :func:`consensus`: ``max_len <= 64`` is one launch with no planning and no host
    synchronisation; a :class:`Plan` (``Plan.for_markets`` restricts the work to a market list;
    the positions of every other market are left untouched, so pass ``out``) launches once per
    length bin; ``64 < max_len <= 4096`` plans on the device without synchronising; with
    ``offsets_host`` the host plans; with nothing, :meth:`Plan.build_device` (one
    synchronisation).  When the host knows the lengths (``offsets_host`` or a plan) a market
    longer than 4096 signals is a ``ValueError`` that names it; otherwise it is left untouched and
    raises the device fault word, as does a market longer than a ``max_len <= 64`` bound and a
    ``sid`` outside ``[0, table.n)`` (its row read clamped).  ``check=True`` synchronises and
    raises :class:`BCEError` for those.  Positions left untouched hold what ``out`` held."""
    return _per_signal("consensus_history", "bce_consensus_history", offsets, sid, prob, table,
                       lambda M, Nsig, dev: (out or HistoryResult.alloc(Nsig, dev), ()),
                       plan, max_len, offsets_host, check)


def _check_arrival_order(offsets: torch.Tensor, arrival_us: torch.Tensor) -> None:
    """``ValueError`` naming the first signal whose arrival time is earlier than that of the signal
    before it in the same market (torch only, any device)."""
    Nsig = arrival_us.numel()
    if Nsig < 2:
        return
    lo0 = offsets[:-1].to(torch.int64)
    hi0 = offsets[1:].to(torch.int64)
    down = arrival_us[1:] < arrival_us[:-1]  # down[i]: signal i + 1 is earlier than signal i
    starts = lo0[(lo0 > 0) & (lo0 < Nsig)]   # a market's first signal has no predecessor
    down[starts - 1] = False
    if bool(down.any()):
        i = int(torch.nonzero(down)[0]) + 1
        m = int(torch.searchsorted(hi0, torch.tensor(i, device=hi0.device), right=True))
        raise ValueError(f"arrival times must not decrease inside a market: signal {i} (market {m}) arrived "
                         f"before signal {i - 1}")


def history_at(offsets: torch.Tensor, arrival_us: torch.Tensor, at_us: torch.Tensor,
               check: bool = True) -> torch.Tensor:
    """The point of every market's history that stood at a given time: ``arrival_us`` int64[N] is
    the arrival time of every signal (not decreasing inside a market), ``at_us`` int64[M] or
    [M, K] the times asked for per market.  Returns int64 of ``at_us``'s shape: the ABSOLUTE index
    (CSR position) of the last point of market m that had arrived by the time (``arrival <=
    at``), -1 where none had (an empty market included).  Torch only: CPU tensors work.
    ``check=True``: an arrival time that decreases inside a market is a ``ValueError``."""
    if arrival_us.dtype != torch.int64 or arrival_us.dim() != 1:
        raise ValueError("arrival_us must be int64[N]")
    M = offsets.numel() - 1
    if at_us.dtype != torch.int64 or at_us.dim() not in (1, 2) or at_us.shape[0] != M:
        raise ValueError(f"at_us must be int64[M] or [M, K] with M = {M}")
    Nsig = arrival_us.numel()
    lo0 = offsets[:-1].to(torch.int64)
    hi0 = offsets[1:].to(torch.int64)
    if check:
        _check_arrival_order(offsets, arrival_us)
    if at_us.dim() == 2:
        lo0, hi0 = lo0[:, None], hi0[:, None]
    lo, hi = lo0.expand_as(at_us).clone(), hi0.expand_as(at_us).clone()
    longest = int((offsets[1:] - offsets[:-1]).max()) if M else 0
    for _ in range(max(longest, 0).bit_length()):  # lo = the first signal of the market that arrived after at_us
        open_ = lo < hi
        mid = (lo + hi) // 2
        arrived = arrival_us[mid.clamp(max=max(Nsig - 1, 0))] <= at_us if Nsig else torch.zeros_like(open_)
        lo = torch.where(open_ & arrived, mid + 1, lo)
        hi = torch.where(open_ & ~arrived, mid, hi)
    return torch.where(lo > lo0, lo - 1, torch.full_like(lo, -1))


def _market_of_point(offsets: torch.Tensor, n_points: int) -> torch.Tensor:
    M = offsets.numel() - 1
    return torch.repeat_interleave(torch.arange(M, dtype=torch.int64, device=offsets.device),
                                   offsets[1:] - offsets[:-1], output_size=n_points)


def _history_items(offsets: torch.Tensor, plan: ScorePlan) -> ScorePlan:
    """The :class:`ScorePlan` over the POINTS of a history for the market groups of ``plan``: every
    member market contributes its points, in member order, then position order (torch only)."""
    mem = plan.pidx
    start = offsets[:-1][mem]
    n = (offsets[1:] - offsets[:-1])[mem]
    end = torch.zeros(mem.numel() + 1, dtype=torch.int64, device=mem.device)
    torch.cumsum(n, 0, out=end[1:])
    total = int(end[-1])
    member = torch.repeat_interleave(torch.arange(mem.numel(), dtype=torch.int64, device=mem.device), n,
                                     output_size=total)
    points = start[member] + (torch.arange(total, dtype=torch.int64, device=mem.device) - end[:-1][member])
    return ScorePlan.groups(end[plan.group_offsets], points, check=False)


def score_history(hist: HistoryResult, offsets: torch.Tensor, outcome: torch.Tensor, *,
                  points: Optional[torch.Tensor] = None, plan: Optional[ScorePlan] = None, **kw) -> ScoreResult:
    """:func:`score` of a history against the markets' outcomes ``outcome`` int8[M], per market
    group of ``plan`` (a :meth:`ScorePlan.groups` over markets; default one group of all).

    ``points=None``: every point is an item, scored against its market's outcome, null points
    (``hist.is_null()``) counted as such; the items of a group run in member order, then position
    order -- the arrival-averaged Brier score (and log loss, calibration, ...) of the group.
    ``points`` int64[M] (what :func:`history_at` returns): every market contributes ONE item, the
    chosen point; -1 counts as a null market.  No kernel of its own: the sums are :func:`score`'s
    and keep its bit-reproducibility."""
    M = offsets.numel() - 1
    dev = offsets.device
    if plan is None:
        plan = ScorePlan.whole(M, device=dev)
    if points is not None:
        if points.dim() != 1 or points.numel() != M:
            raise ValueError(f"points must be int64[M] with M = {M}")
        if hist.consensus.numel() == 0:
            return score(plan, torch.zeros(M, dtype=torch.float64, device=dev), outcome,
                         valid=torch.zeros(M, dtype=torch.bool, device=dev), **kw)
        at = points.to(torch.int64).clamp(min=0)
        valid = (points >= 0) & ~hist.is_null()[at]
        return score(plan, hist.consensus[at].contiguous(), outcome, valid=valid, **kw)
    n_points = hist.consensus.numel()
    per_point = outcome[_market_of_point(offsets, n_points)]
    return score(_history_items(offsets, plan), hist.consensus, per_point, valid=~hist.is_null(), **kw)


def _walk_entry_table(plan, scopes, offsets: torch.Tensor, prob: torch.Tensor, trace_kwargs) -> SourceTable:
    """The entry table of a walk-forward plan -- :func:`walk_trace` or, for a
    :class:`WalkScopePlan`, :func:`walk_scope_trace` ``(plan, *scopes, **trace_kwargs)`` -- after
    checking that ``offsets`` / ``prob`` are the plan's batch (its entry ids: ``plan.pairs.esid``)."""
    pp = plan.pairs
    if offsets.numel() - 1 != pp.n_markets or prob.numel() != pp.esid.numel():
        raise ValueError("offsets / prob are not the batch the plan was built from")
    trace = walk_scope_trace if isinstance(plan, WalkScopePlan) else walk_trace
    return trace(plan, *scopes, **trace_kwargs)[0]


def walk_history(plan, *scopes, offsets: torch.Tensor, prob: torch.Tensor, bins: Optional[Plan] = None,
                 max_len: Optional[int] = None, offsets_host: Optional[np.ndarray] = None,
                 out: Optional[HistoryResult] = None, check: bool = False, **trace_kwargs) -> HistoryResult:
    """The history of every market of a walk-forward back-test: for a :class:`WalkPlan`,
    :func:`walk_trace` ``(plan, *scopes, **trace_kwargs)`` -- ``scopes`` is the table and, for an
    ordinary plan, ``market_time_us`` -- followed by :func:`consensus_history` on the entry table;
    for a :class:`WalkScopePlan` the same over :func:`walk_scope_trace` (``scopes``: ``domains,
    global_table[, market_time_us]``).  ``bins`` / ``max_len`` / ``offsets_host`` / ``out`` /
    ``check`` go to :func:`consensus_history` (``bins`` is its length-bin :class:`Plan`).  Nothing
    is committed.  The last point of every market equals ``walk_forward(commit=False)``.

    One limit: every market's history uses the reliabilities of ONE read per market -- as they
    stood at that market's own turn (its forecast time for a lagged plan).  They are not re-read
    at every arrival, so an outcome that resolved between two signals of the same market does not
    move the later points.  :func:`walk_history_live` (batch/live.py) is the history that does
    re-read them, given every signal's arrival time."""
    wtable = _walk_entry_table(plan, scopes, offsets, prob, trace_kwargs)
    return consensus_history(offsets, plan.pairs.esid, prob.to(torch.float64), wtable, plan=bins, max_len=max_len,
                             offsets_host=offsets_host, out=out, check=check)
