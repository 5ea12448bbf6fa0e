"""Leave-one-source-out consensus: every source's marginal effect on its market."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _native as N
from .tables import SourceTable, _check_csr
from .consensus import ConsensusResult, Plan, _alloc
from .score import ScorePlan, ScoreResult, _score_segments, score
from .history import _alloc_per_signal, _market_of_point, _per_signal, _walk_entry_table


@dataclass
class LeaveOneOutResult:
    """:func:`leave_one_out`: one entry per signal, at the signal's CSR position -- the consensus
    of the signal's market WITHOUT the signal's source (all signals of one source in one market
    hold the same values); ``full`` is the market's own consensus, per market."""

    consensus: torch.Tensor      # fp64[N]  (0.0 where null)
    confidence: torch.Tensor     # fp64[N]  (0.0 where null)
    total_weight: torch.Tensor   # fp64[N]
    n_unique: torch.Tensor       # int32[N]: the market's unique sources less one
    full: Optional[ConsensusResult] = None

    @classmethod
    def alloc(cls, n_signals: int, device, n_markets: Optional[int] = None) -> "LeaveOneOutResult":
        """Uninitialised outputs for ``n_signals`` signals; with ``n_markets``, ``full`` too."""
        full = None if n_markets is None else _alloc(int(n_markets), 0, device, False, False)
        return cls(*_alloc_per_signal(n_signals, device), full)

    def is_null(self) -> torch.Tensor:
        """bool[N]: the consensus without the source is None -- nothing is left, or what is left
        has total weight 0 (core.py:88, 131)."""
        return self.total_weight == 0

    def influence(self, offsets: torch.Tensor, full: Optional[ConsensusResult] = None) -> torch.Tensor:
        """fp64[N]: the market's full consensus minus the consensus without the signal's source
        (positive: the source pulls the consensus up); NaN where either is null.  ``full``
        defaults to the result's own."""
        full = full if full is not None else self.full
        if full is None:
            raise ValueError("influence needs the full consensus: leave_one_out(full=True), or pass full=")
        market = _market_of_point(offsets, self.consensus.numel())
        null = self.is_null() | full.is_null(offsets)[market]
        nan = torch.full_like(self.consensus, float("nan"))
        return torch.where(null, nan, full.consensus[market] - self.consensus)


def leave_one_out(offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, table: SourceTable, *,
                  plan: Optional[Plan] = None, max_len: Optional[int] = None,
                  offsets_host: Optional[np.ndarray] = None, out: Optional[LeaveOneOutResult] = None,
                  full: bool = True, check: bool = False) -> LeaveOneOutResult:
    """``compute_consensus([s for s in signals if s["sourceId"] != x], table)`` for every source x
    of every CSR market, in one pass over the signals (bce_consensus_leave_one_out): the four fp64
    / int32 [N] outputs hold, at the CSR position of every signal, the consensus of its market
    without its source.  Bit-identical to :func:`consensus` on the batch expanded into one reduced
    market per signal, which reads about U - 1 times the signals (U: a market's unique sources).
    Where nothing is left, or what is left weighs 0, ``total_weight`` is 0 and ``consensus`` /
    ``confidence`` are 0.0 (:meth:`LeaveOneOutResult.is_null`).  ``full=True`` also returns the
    market's own consensus per market (``.full``), bit-identical to :func:`consensus`; an empty
    market's row is zeros.  Exact order only, no per-unique outputs; probabilities outside [0, 1]
    are computed.  The work is O(n + U^2) per market; markets of up to ``HISTORY_MAX_LEN`` signals.

    Routes, ``ValueError`` s and faults are those of :func:`consensus_history`: ``max_len <= 64``
    is one launch; a :class:`Plan` launches once per length bin (``Plan.for_markets``: the
    positions and ``full`` rows of every other market are left untouched, so pass ``out``);
    ``64 < max_len <= 4096`` plans on the device without synchronising; ``offsets_host`` plans on
    the host; nothing: :meth:`Plan.build_device`.  A market over 4096 signals is a ``ValueError``
    when the host knows the lengths, else it is left untouched and raises the device fault word,
    as does a market over a ``max_len <= 64`` bound and a ``sid`` outside ``[0, table.n)`` (its
    row read clamped).  ``check=True`` synchronises and raises :class:`BCEError` for those."""
    def outputs(M, Nsig, dev):
        res = out or LeaveOneOutResult.alloc(Nsig, dev)
        if full and res.full is None:
            res.full = _alloc(M, 0, dev, False, False)
        fr = res.full if full else None
        return res, (N.ptr(fr.consensus if fr else None), N.ptr(fr.confidence if fr else None),
                     N.ptr(fr.total_weight if fr else None), N.ptr(fr.n_unique if fr else None))

    return _per_signal("leave_one_out", "bce_consensus_leave_one_out", offsets, sid, prob, table, outputs,
                       plan, max_len, offsets_host, check)


def _loo_items(offsets: torch.Tensor, sid: torch.Tensor, n_sources: int, per: str = "pair") -> ScorePlan:
    """The :class:`ScorePlan` over the signals of a batch, one group per source, every item
    reading and scored at its own CSR position (``oidx`` None).  ``per="signal"``: every signal,
    as :meth:`ScorePlan.by_source` orders them.  ``per="pair"``: one item per (market, source),
    the source's first signal in the market, a source's items in market order.  Torch only."""
    if per not in ("pair", "signal"):
        raise ValueError(f"per must be 'pair' or 'signal' (got {per!r})")
    M, Nsig, S, offsets, lens = _check_csr(offsets, sid, n_sources)
    dev = offsets.device
    clamped = sid.to(torch.int64).clamp(0, S - 1)
    n_clamped = int((clamped != sid).sum())
    points = torch.arange(Nsig, dtype=torch.int64, device=dev)
    if per == "pair":
        market = torch.repeat_interleave(torch.arange(M, dtype=torch.int64, device=dev), lens, output_size=Nsig)
        key, perm = torch.sort(market * S + clamped, stable=True)  # equal keys keep position order
        lead = torch.ones(Nsig, dtype=torch.bool, device=dev)
        lead[1:] = key[1:] != key[:-1]
        points = torch.sort(perm[lead]).values  # the first signals, in CSR order
        clamped = clamped[points]
    _, order = torch.sort(clamped, stable=True)
    goff = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(clamped, minlength=S), 0, out=goff[1:])
    seg_start = _score_segments(goff)
    return ScorePlan(goff, points[order].contiguous(), None, seg_start, int(seg_start[-1]), n_clamped)


def score_leave_one_out(loo: LeaveOneOutResult, offsets: torch.Tensor, sid: torch.Tensor, outcome: torch.Tensor,
                        n_sources: int, *, per: str = "pair", **kw) -> ScoreResult:
    """Was the consensus better or worse for having each source?  :func:`score` with one group
    per source over the signals of the batch: the forecast of an item is the consensus of its
    market WITHOUT the source (``loo.consensus``), the base forecast the market's full consensus
    (``loo.full``), both scored against the market's outcome ``outcome`` int8[M]; an item counts
    as null where either consensus is None.  ``per="pair"``: one item per (market, source);
    ``per="signal"``: every signal, as :meth:`ScorePlan.by_source` counts them.

    The sign: ``ScoreResult.skill`` is ``brier - brier_base``, here the Brier score of the
    consensus without the source minus that of the full consensus over the same markets --
    POSITIVE means the consensus is worse without the source (the source helps), negative that
    the consensus would have been better without it.  No kernel of its own: the sums are
    :func:`score`'s and keep its bit-reproducibility."""
    if loo.full is None:
        raise ValueError("score_leave_one_out needs the full consensus: leave_one_out(full=True)")
    plan = _loo_items(offsets, sid, n_sources, per)
    market = _market_of_point(offsets, loo.consensus.numel())
    valid = ~(loo.is_null() | loo.full.is_null(offsets)[market])
    return score(plan, loo.consensus, outcome[market], valid=valid, base=loo.full.consensus[market], **kw)


def walk_leave_one_out(plan, *scopes, offsets: torch.Tensor, prob: torch.Tensor, bins: Optional[Plan] = None,
                       max_len: Optional[int] = None, offsets_host: Optional[np.ndarray] = None,
                       out: Optional[LeaveOneOutResult] = None, full: bool = True, check: bool = False,
                       **trace_kwargs) -> LeaveOneOutResult:
    """The leave-outs of every market of a walk-forward back-test, as :func:`walk_history` takes
    its arguments: :func:`walk_trace` (a :class:`WalkPlan`) or :func:`walk_scope_trace` (a
    :class:`WalkScopePlan`) ``(plan, *scopes, **trace_kwargs)``, then :func:`leave_one_out` on
    the entry table with the plan's entry ids; ``bins`` is its length-bin :class:`Plan`.  Every
    market is read with the reliabilities as they stood at its own turn.  Nothing is committed;
    ``full`` equals ``walk_forward(commit=False)``."""
    wtable = _walk_entry_table(plan, scopes, offsets, prob, trace_kwargs)
    return leave_one_out(offsets, plan.pairs.esid, prob.to(torch.float64), wtable, plan=bins, max_len=max_len,
                         offsets_host=offsets_host, out=out, full=full, check=check)
