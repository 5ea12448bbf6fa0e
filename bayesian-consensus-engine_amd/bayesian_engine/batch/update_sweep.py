"""Sweeping the reliability update rule: learning-rate / step-cap grids in one trace."""
import math
import numbers
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _native as N
from ..config import (DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM, DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY,
                      MAX_UPDATE_STEP)
from .tables import ReliabilityTable, _check_table
from .settle import SETTLE_CHUNK_BITS, SETTLE_LONG_MIN
from .walk import WalkPlan, _walk_read, _walk_times
from .score import ScorePlan, ScoreResult, _sweep, _sweep_setup
from .consensus import Plan

UPDATE_MAX_POINTS = N.UPDATE_MAX_POINTS  # rules of one trace (include/bce.h BCE_UPDATE_MAX_POINTS)
_MIN_SYNC_STEP = 2.0 ** -20              # below it no pin run is claimed: the chain is walked by one worker
_MAX_STEP = 1e300


def _numbers(x, name: str):
    """``x`` as a list of floats (a lone number is one); ``TypeError`` for anything else."""
    if isinstance(x, numbers.Real) and not isinstance(x, bool):
        return [float(x)], True
    if isinstance(x, (str, bytes)):
        raise TypeError(f"{name} must be a number or a sequence of numbers")
    try:
        items = list(x)
    except TypeError:
        raise TypeError(f"{name} must be a number or a sequence of numbers") from None
    for v in items:
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise TypeError(f"{name} must hold numbers (got {type(v).__name__})")
    return [float(v) for v in items], False


def update_steps(learning_rate, max_step=MAX_UPDATE_STEP):
    """The points of an update-rule grid as the trace takes them: ``(delta fp64[K], sync_run
    int64[K])`` (numpy; no GPU).  Point i is the PAIR ``(learning_rate[i], max_step[i])`` --
    ``max_step`` a scalar for all points or a sequence of the same length -- not a product: the
    reference's step ``max(-max_step, min(max_step, learning_rate * +-1.0))``
    (reliability.py:163-169) is exactly ``+-delta`` with ``delta = min(max_step, learning_rate)``,
    so only the minimum matters.  ``sync_run``: the equal outcomes in a row that pin the
    reliability to exactly 1.0 / 0.0 under ``delta`` whatever it was, ``ceil(1 / delta) + 1`` (11
    for 0.1); 0 = none do (``delta == 0``, or ``delta < 2**-20``, which is left unbounded).
    ``ValueError`` for an empty sequence, a length mismatch, a negative, NaN or infinite value or
    ``delta > 1e300``; ``TypeError`` for non-numbers."""
    lr, _ = _numbers(learning_rate, "learning_rate")
    ms, one = _numbers(max_step, "max_step")
    if not lr:
        raise ValueError("update_steps needs at least one learning_rate")
    if one:
        ms = ms * len(lr)
    if len(ms) != len(lr):
        raise ValueError(f"max_step has {len(ms)} entries for {len(lr)} learning rates")
    for name, vals in (("learning_rate", lr), ("max_step", ms)):
        if any(not (math.isfinite(v) and v >= 0.0) for v in vals):
            raise ValueError(f"{name} must be finite and >= 0 (got {vals})")
    delta = [min(m, r) for r, m in zip(lr, ms)]  # min(MAX_UPDATE_STEP, raw), as the reference nests it
    if any(d > _MAX_STEP for d in delta):
        raise ValueError(f"the step min(max_step, learning_rate) must be <= {_MAX_STEP} (got {delta})")
    sync = [int(math.ceil(1.0 / d)) + 1 if d >= _MIN_SYNC_STEP else 0 for d in delta]
    return np.array(delta, np.float64), np.array(sync, np.int64)


def _trace_grid(plan: WalkPlan, table: "ReliabilityTable", delta: np.ndarray, sync: np.ndarray, trace: torch.Tensor,
                final: Optional[torch.Tensor], long_min: Optional[int], chunk_bits: Optional[int]) -> None:
    """bce_settle_trace_grid of ``plan`` from ``table`` for the rules ``delta`` / ``sync`` into
    ``trace`` [>= K, E, 2] and, if given, ``final`` [K, S, 2].  The caller has checked the table."""
    L = N.require_gpu()
    sp, q, E = plan.settle, plan.queries, plan.pairs.n_entries
    K = int(delta.size)
    dev = table.rel.device
    long_min = SETTLE_LONG_MIN if long_min is None else long_min
    chunk_bits = SETTLE_CHUNK_BITS if chunk_bits is None else chunk_bits
    n_long, chunk_start, n_chunks = sp.chunks(long_min, chunk_bits)
    step_d = torch.from_numpy(np.ascontiguousarray(delta, np.float64)).to(dev)
    sync_d = torch.from_numpy(np.ascontiguousarray(sync, np.int64)).to(dev)
    N.check(L.bce_settle_trace_grid(N.ptr(sp.bits), sp.n_bits, N.ptr(sp.start), N.ptr(sp.order), sp.n_touched, n_long,
                                    N.ptr(chunk_start), n_chunks, int(chunk_bits), sp.n_sources, N.ptr(table.rel),
                                    N.ptr(table.conf), N.ptr(table.present), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE,
                                    N.ptr(q.qstart), N.ptr(q.qpos if E else None), N.ptr(q.qentry if E else None), E,
                                    N.ptr(step_d), N.ptr(sync_d), K, N.ptr(trace if E else None), N.ptr(final),
                                    N.stream(dev)), "bce_settle_trace_grid")


def _final_buffer(table: "ReliabilityTable", K: int) -> torch.Tensor:
    """``final`` [K, S, 2] before the trace: every source's start state (the cold defaults where
    no row exists), which the sources the batch does not touch keep."""
    rel, conf = table.rel, table.conf
    if table.present is not None:
        pres = table.present != 0
        rel = torch.where(pres, rel, torch.full_like(rel, DEFAULT_RELIABILITY))
        conf = torch.where(pres, conf, torch.full_like(conf, DEFAULT_CONFIDENCE))
    return torch.stack([rel, conf], 1).unsqueeze(0).repeat(K, 1, 1).contiguous()


def _checked_walk(plan: WalkPlan, table: "ReliabilityTable", market_time_us: Optional[torch.Tensor]) -> None:
    if not isinstance(plan, WalkPlan):
        raise TypeError(f"an update-rule sweep needs a WalkPlan (got {type(plan).__name__}): the namespaced walk "
                        "is not swept yet")
    _walk_times(plan, market_time_us)
    N.require_gpu()
    _check_table(table.rel, table.conf, table.t_us, table.present, plan.settle.n_sources)


def walk_trace_grid(plan: WalkPlan, table: "ReliabilityTable", market_time_us: Optional[torch.Tensor] = None, *,
                    learning_rate, max_step=MAX_UPDATE_STEP, final: bool = False, long_min: Optional[int] = None,
                    chunk_bits: Optional[int] = None):
    """The settlement trace of :func:`walk_forward` under every rule of :func:`update_steps`
    (at most UPDATE_MAX_POINTS) in ONE launch of bce_settle_trace_grid: fp64 ``[K, E, 2]``, slice k
    what bce_settle_trace would write with ``_BASE_LEARNING_RATE`` / ``MAX_UPDATE_STEP`` set to
    point k -- raw states, rows of entries without an earlier bit unwritten, exactly as
    :func:`_walk_read` takes them.  The table is not written.  ``final=True`` also returns fp64
    ``[K, S, 2]``: every source's ``{rel, conf}`` behind its whole chain (an untouched source: its
    start state), what :func:`commit_update_point` writes.  Works for a plan of
    :meth:`WalkPlan.build` and :meth:`WalkPlan.build_lagged` alike (the trace sees only the
    queries); ``market_time_us`` as :func:`walk_forward`.  The result does not depend on
    ``long_min`` / ``chunk_bits``."""
    delta, sync = update_steps(learning_rate, max_step)
    K = int(delta.size)
    if K > UPDATE_MAX_POINTS:
        raise ValueError(f"walk_trace_grid takes at most {UPDATE_MAX_POINTS} points (got {K}): "
                         "walk_sweep_update blocks a longer grid")
    _checked_walk(plan, table, market_time_us)
    dev = table.rel.device
    trace = torch.empty((K, plan.pairs.n_entries, 2), dtype=torch.float64, device=dev)
    fin = _final_buffer(table, K) if final else None
    _trace_grid(plan, table, delta, sync, trace, fin, long_min, chunk_bits)
    return (trace, fin) if final else trace


def walk_sweep_update(plan: WalkPlan, table: "ReliabilityTable", market_time_us: Optional[torch.Tensor] = None, *,
                      offsets: torch.Tensor, prob: torch.Tensor, learning_rate, max_step=MAX_UPDATE_STEP,
                      half_life_days: Sequence[float] = (DECAY_HALF_LIFE_DAYS,),
                      min_rel: Sequence[float] = (DECAY_MINIMUM,), score_plan: Optional[ScorePlan] = None,
                      keep_consensus: bool = False, final: bool = False, max_trace_bytes: int = 2 << 30,
                      all_present: bool = True, mode: str = "exact", long_min: Optional[int] = None,
                      chunk_bits: Optional[int] = None, n_bins: int = 10, eps: float = 1e-15, **consensus_kwargs):
    """:func:`walk_sweep` with the update rule as the slowest grid axis: :func:`walk_forward`
    (``commit=False``) for every ``(update point, half_life_days, min_rel)``, row-major, each
    scored against the plan's outcomes.  The update points are the pairs of :func:`update_steps`;
    they are traced together (:func:`walk_trace_grid`), in blocks of at most ``min(
    UPDATE_MAX_POINTS, max_trace_bytes // (16 * E))`` points (at least one), so a long history
    does not hold K traces at once; then every grid point runs bce_walk_read from its rule's
    slice, :func:`consensus` and :func:`score` as :func:`walk_sweep` does.  No input is written.
    Returns what :func:`walk_sweep` returns with the leading dimension ``K * H * R``; with
    ``final=True``, ``(scores, consensus, final)`` with ``final`` the ``[K, S, 2]`` array of
    :func:`walk_trace_grid`.  The other arguments are :func:`walk_sweep`'s."""
    delta, sync = update_steps(learning_rate, max_step)
    _checked_walk(plan, table, market_time_us)
    dev = table.rel.device
    (hl, mr), _, (relconf, bits, exists) = _sweep_setup(plan, offsets, prob, half_life_days, min_rel,
                                                         "walk_sweep_update", dev)
    K, E = int(delta.size), plan.pairs.n_entries
    block = max(1, min(UPDATE_MAX_POINTS, int(max_trace_bytes) // (16 * max(E, 1))))
    block = min(block, K)
    trace = torch.empty((block, E, 2), dtype=torch.float64, device=dev)
    fin = _final_buffer(table, K) if final else None
    kw = dict(consensus_kwargs)
    if "bins" in kw:
        kw["plan"] = kw.pop("bins")
    if kw.get("plan") is None and kw.get("max_len") is None:
        kw["plan"] = Plan.build_device(offsets)  # the length bins once, not once per block
    if score_plan is None:
        score_plan = ScorePlan.whole(plan.pairs.n_markets, device=dev)

    def read(point, m):  # the rule's slice of the block, then the decay parameters
        k, h = point
        _walk_read(plan, table, market_time_us, trace[k], relconf, bits, exists, all_present, h, m)

    parts, cons, nulls = [], [], []
    for k0 in range(0, K, block):
        nb = min(block, K - k0)
        _trace_grid(plan, table, delta[k0:k0 + nb], sync[k0:k0 + nb], trace,
                    None if fin is None else fin[k0:k0 + nb], long_min, chunk_bits)
        # _sweep's outer axis carries (rule, half-life): the rule slowest, min_rel fastest
        grid = [(k, h) for k in range(nb) for h in hl], mr
        scores, kept = _sweep(plan, read, relconf, bits, offsets, prob, grid, score_plan, keep_consensus, mode,
                              n_bins, eps, dict(kw))
        parts.append(scores)
        if kept is not None:
            cons.append(kept[0])
            nulls.append(kept[1])
    scores = ScoreResult(*(torch.cat([getattr(p, f) for p in parts]) for f in
                           ("counts", "sums", "bin_n", "bin_pos", "bin_psum")), has_base=parts[0].has_base)
    kept = (torch.cat(cons), torch.cat(nulls)) if keep_consensus else None
    return (scores, kept, fin) if final else (scores, kept)


def commit_update_point(plan: WalkPlan, table: "ReliabilityTable", final: torch.Tensor, k: int,
                        market_time_us: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Leave ``table`` as :func:`walk_forward` (``commit=True``) would under update point ``k`` of
    a ``final`` [K, S, 2] from :func:`walk_trace_grid` / :func:`walk_sweep_update`: the touched
    sources get the point's final ``rel`` / ``conf``, ``present = 1`` and ``t_us`` = the time of
    their chain's last market (the resolve time for a lagged plan); other rows are not written.
    Plain torch indexing.  Returns the touched rows (int64)."""
    stamp, _ = _walk_times(plan, market_time_us)
    S = plan.settle.n_sources
    _check_table(table.rel, table.conf, table.t_us, table.present, S)
    if final.dim() != 3 or final.shape[1:] != (S, 2) or final.dtype != torch.float64:
        raise ValueError(f"final must be fp64 [K, {S}, 2]")
    k = int(k)
    if not 0 <= k < final.shape[0]:
        raise ValueError(f"update point {k} outside [0, {final.shape[0]})")
    touched = plan.settle.order.to(torch.int64)
    if touched.numel():
        table.rel.index_copy_(0, touched, final[k, touched, 0])
        table.conf.index_copy_(0, touched, final[k, touched, 1])
        if table.present is not None:
            table.present.index_fill_(0, touched, 1)
        table.t_us.index_copy_(0, touched, stamp[plan.slast[touched]])
    return touched
