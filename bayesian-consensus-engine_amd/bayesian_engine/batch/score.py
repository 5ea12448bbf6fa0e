"""Scoring a back-test: Brier score, log loss, hits and calibration per group."""
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from .. import _native as N
from .tables import ReliabilityTable, SourceTable, _check_csr, _entry_buffers
from .consensus import Plan, _alloc, consensus
from .pairs import _bins_as_plan
from .walk import (WalkPlan, WalkScopePlan, _check_batch, _walk_read, _walk_scope_launch, _walk_scope_traces,
                   _walk_settle_trace)

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
        M, Nsig, S, offsets, lens = _check_csr(offsets, sid, n_sources)
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


def _sweep_setup(plan, offsets: torch.Tensor, prob: torch.Tensor, half_life_days: Sequence[float],
                 min_rel: Sequence[float], what: str, dev):
    """What :func:`walk_sweep` and :func:`walk_sweep_scoped` open with: ``(grid, trace, read
    buffers)`` -- the grid as two lists of floats (an empty axis is a ``ValueError``), the checks
    that ``plan`` keeps its outcomes and fits the batch, a trace buffer [E, 2] and the
    :func:`_entry_buffers` every grid point is read into."""
    grid = [float(x) for x in half_life_days], [float(x) for x in min_rel]
    if not grid[0] or not grid[1]:
        raise ValueError(f"{what} needs at least one half_life_days and one min_rel")
    if plan.outcome is None:
        kind = type(plan).__name__
        raise ValueError(f"{what} needs a {kind} from {kind}.build (it keeps the outcomes)")
    _check_batch(plan, offsets, prob)
    E = plan.pairs.n_entries
    return grid, _entry_buffers(E, dev)[0], _entry_buffers(E, dev)


def _sweep(plan, read, relconf: torch.Tensor, bits: torch.Tensor, offsets: torch.Tensor, prob: torch.Tensor, grid,
           score_plan: Optional[ScorePlan], keep_consensus: bool, mode: str, n_bins: int, eps: float,
           consensus_kwargs: dict):
    """The grid loop of :func:`walk_sweep` and :func:`walk_sweep_scoped`: for every point,
    ``read(half_life_days, min_rel)`` fills ``relconf`` / ``bits`` (the consensus table over the
    entries of ``plan``), then :func:`consensus` and :func:`score` against the plan's outcomes.
    The length-bin plan, the consensus outputs and the scoring scratch are allocated once."""
    pairs, outcome, (hl, mr) = plan.pairs, plan.outcome, grid
    M, E = pairs.n_markets, pairs.n_entries
    wtable = SourceTable(relconf, bits, range(E))
    dev = relconf.device
    if score_plan is None:
        score_plan = ScorePlan.whole(M, device=dev)
    prob = prob.to(torch.float64)
    kw = _bins_as_plan(consensus_kwargs)
    unique = kw.pop("unique_outputs", False)
    validate = kw.pop("validate", False)
    if kw.get("plan") is None and kw.get("max_len") is None:
        kw["plan"] = Plan.build_device(offsets)  # the length bins once, not once per grid point
    out = _alloc(M, pairs.esid.numel(), dev, unique, validate)
    L = N.require_gpu()
    sb = int(L.bce_score_scratch_bytes(score_plan.n_segments, int(n_bins))) if 1 <= int(n_bins) <= SCORE_MAX_BINS else 8
    scratch = torch.empty(max(sb // 8, 1), dtype=torch.int64, device=dev)
    empty = offsets[1:] == offsets[:-1]
    parts, cons, nulls = [], [], []
    for h in hl:
        for m in mr:
            read(h, m)
            res = consensus(offsets, pairs.esid, prob, wtable, mode=mode, unique_outputs=unique, validate=validate,
                            out=out, **kw)
            null = (res.total_weight == 0) | empty
            parts.append(score(score_plan, res.consensus, outcome, valid=~null, n_bins=n_bins, eps=eps,
                               scratch=scratch))
            if keep_consensus:
                cons.append(res.consensus.clone())
                nulls.append(null)
    scores = ScoreResult.stack(parts)
    return scores, ((torch.stack(cons), torch.stack(nulls)) if keep_consensus else None)


def walk_sweep(plan: WalkPlan, table: "ReliabilityTable", market_time_us: Optional[torch.Tensor] = None, *,
               offsets: torch.Tensor, prob: torch.Tensor, half_life_days: Sequence[float], min_rel: Sequence[float],
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
    ``market_time_us`` as :func:`walk_forward`: None for a lagged plan, which has its own times.
    Returns ``(scores, consensus)``: a :class:`ScoreResult` with a leading grid dimension
    ``[len(half_life_days) * len(min_rel), G, ...]`` over ``score_plan`` (default: one group of all
    markets) and, with ``keep_consensus``, the fp64 ``[K, M]`` consensus and bool ``[K, M]``
    null mask of every point (else None)."""
    grid, trace, (relconf, bits, exists) = _sweep_setup(plan, offsets, prob, half_life_days, min_rel, "walk_sweep",
                                                        table.rel.device)
    _walk_settle_trace(plan, table, market_time_us, trace, long_min, chunk_bits)

    def read(h, m):
        _walk_read(plan, table, market_time_us, trace, relconf, bits, exists, all_present, h, m)

    return _sweep(plan, read, relconf, bits, offsets, prob, grid, score_plan, keep_consensus, mode, n_bins, eps,
                  consensus_kwargs)


def walk_sweep_scoped(plan: WalkScopePlan, domains: "PairTable", global_table: Optional["ReliabilityTable"],
                      market_time_us: Optional[torch.Tensor] = None, *, offsets: torch.Tensor, prob: torch.Tensor,
                      half_life_days: Sequence[float], min_rel: Sequence[float], pairs: Optional["PairTable"] = None,
                      global_has: Optional[torch.Tensor] = None, score_plan: Optional[ScorePlan] = None,
                      keep_consensus: bool = False, mark_cold: bool = False, mode: str = "exact",
                      long_min: Optional[int] = None, chunk_bits: Optional[int] = None, n_bins: int = 10,
                      eps: float = 1e-15, **consensus_kwargs):
    """:func:`walk_sweep` over the namespaced walk: :func:`walk_forward_scoped` (``commit=False``),
    ordinary or lagged, for every point of a grid of decay parameters, scored against the plan's
    outcomes.  ``update_reliability`` starts from the undecayed row in every scope
    (reliability_abstraction.py:211-229), so neither chain family depends on ``half_life_days`` /
    ``min_rel``: each is traced ONCE into a buffer of its own, and every grid point runs
    bce_walk_scope_read from the two traces into a THIRD buffer (the single walk lets the read
    overwrite the global trace in place; here the traces must outlive the read), then
    :func:`consensus` and :func:`score`.  No input is written.  The arguments are those of
    :func:`walk_forward_scoped` and :func:`walk_sweep`; returns what :func:`walk_sweep` returns."""
    grid, gtrace, (relconf, bits, scope) = _sweep_setup(plan, offsets, prob, half_life_days, min_rel,
                                                        "walk_sweep_scoped", plan.pairs.esid.device)
    tr = _walk_scope_traces(plan, domains, global_table, market_time_us, pairs, global_has, long_min, chunk_bits,
                            gtrace)

    def read(h, m):
        _walk_scope_launch(plan, tr, global_table, market_time_us, pairs, mark_cold, h, m, relconf, bits, scope)

    return _sweep(plan, read, relconf, bits, offsets, prob, grid, score_plan, keep_consensus, mode, n_bins, eps,
                  consensus_kwargs)
