"""Live consensus history: every market's consensus after each of its signals arrived, with the
reliabilities re-read at every arrival."""
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .. import _native as N
from ..config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM, DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY
from .tables import ReliabilityTable, _check_csr, _check_table
from .consensus import Plan
from .settle import SETTLE_CHUNK_BITS, SETTLE_LONG_MIN, SettlePlan, _commit_chains
from .walk import _resolve_rank
from .history import HistoryResult, _check_arrival_order, _per_signal


def _check_live_times(offsets: torch.Tensor, lens: torch.Tensor, outcome: torch.Tensor, arrival_us: torch.Tensor,
                      resolve_time_us: torch.Tensor) -> None:
    """The validity of a live batch's times (torch only, any device): ``ValueError`` that names
    the signal or the market."""
    M, Nsig = outcome.numel(), int(offsets[-1]) if offsets.numel() else 0
    for name, t, n, per in (("arrival_us", arrival_us, Nsig, "signal"), ("resolve_time_us", resolve_time_us, M, "market")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or t.numel() != n:
            raise ValueError(f"{name} must be int64 with one entry per {per} ({n})")
        if t.device != outcome.device:
            raise ValueError(f"{name} must be on the batch's device")
    _check_arrival_order(offsets, arrival_us)
    if not (M and Nsig):
        return
    last = arrival_us[(offsets[1:] - 1).clamp(min=0)]
    early = (lens > 0) & (outcome >= 0) & (resolve_time_us < last)
    if bool(early.any()):
        at = int(torch.nonzero(early)[0])
        raise ValueError(f"market {at} resolves before its last signal arrives")


@dataclass
class LivePlan:
    """A CSR batch with an arrival time per signal and a resolve time per market, compiled for
    :func:`walk_history_live`: ``settle`` is the :class:`SettlePlan` of its resolved markets with
    the chains in (resolve time, market, position) order, ``bit_market`` int32[n_bits] the market
    of every chain bit in chain order and ``slast`` int64[S] the market of every chain's last bit
    (-1: none).  ``outcome`` int8[M], ``arrival_us`` int64[N] and ``resolve_time_us`` int64[M] are
    the batch's, contiguous.  ``n_clamped``: sids outside ``[0, n_sources)``.  There is no entry
    list and no query: a point finds what it sees by bisection, in the kernel."""

    settle: SettlePlan
    bit_market: torch.Tensor
    slast: torch.Tensor
    outcome: torch.Tensor
    arrival_us: torch.Tensor
    resolve_time_us: torch.Tensor
    n_markets: int
    n_signals: int
    n_clamped: int

    @classmethod
    def build(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
              n_sources: int, arrival_us: torch.Tensor, resolve_time_us: torch.Tensor,
              check: bool = True) -> "LivePlan":
        """Compile ``(offsets, sid, prob)`` with ``outcome`` int8[M] (-1 unresolved, 0, 1),
        ``arrival_us`` int64[N] and ``resolve_time_us`` int64[M] (read where ``outcome >= 0``).
        The markets may come in any order; the market index only breaks ties.  ``ValueError`` (from
        torch checks on whatever device the tensors are on, before the library is touched) for a
        wrong dtype or size, an arrival time that decreases inside a market (names the signal and
        the market) and a resolved market that resolves before its last arrival (names it).

        One stable sort over M for the rank of the resolved markets by (resolve time, market),
        :meth:`SettlePlan.build` with that rank, one gather for ``slast``.  A ``sid`` outside ``[0,
        n_sources)`` is clamped and raises :class:`BCEError` (``check=False``: the fault is left
        for :func:`walk_history_live`)."""
        M, Nsig, S, off64, lens = _check_csr(offsets, sid, n_sources, prob=prob, outcome=outcome,
                                             too_many="live: {} markets (the bit-to-market map is int32)")
        _check_live_times(off64, lens, outcome, arrival_us, resolve_time_us)
        clamped = sid.to(torch.int32).clamp(0, S - 1)
        n_clamped = int((clamped != sid).sum())
        resolve = resolve_time_us.contiguous()
        splan, market, perm = SettlePlan._compile(offsets, sid, prob, outcome, S, check, _resolve_rank(outcome, resolve))
        bit_market = market[perm].contiguous()
        slast = torch.full((S,), -1, dtype=torch.int64, device=offsets.device)
        touched = splan.total > 0
        slast[touched] = bit_market[splan.start[1:][touched] - 1].to(torch.int64)
        if check and n_clamped:
            raise N.BCEError(f"live plan: {n_clamped} sid outside [0, {S})")
        return cls(splan, bit_market, slast, outcome.contiguous(), arrival_us.contiguous(), resolve, M, Nsig,
                   n_clamped)


def live_trace(plan: LivePlan, table: ReliabilityTable, long_min: Optional[int] = None,
               chunk_bits: Optional[int] = None) -> torch.Tensor:
    """bce_settle_trace_all: ``states`` fp64[n_bits, 2], the raw ``{rel, conf}`` of every source
    after each bit of its chain, walked from the start rows of ``table`` (not written).  16 bytes
    per chain bit.  The states do not depend on the decay parameters (reliability.py:161), nor on
    ``long_min`` / ``chunk_bits`` (as :func:`settle`)."""
    L = N.require_gpu()
    sp = plan.settle
    _check_table(table.rel, table.conf, table.t_us, table.present, sp.n_sources)
    long_min = SETTLE_LONG_MIN if long_min is None else long_min
    chunk_bits = SETTLE_CHUNK_BITS if chunk_bits is None else chunk_bits
    n_long, chunk_start, n_chunks = sp.chunks(long_min, chunk_bits)
    dev = table.rel.device
    states = torch.empty((max(sp.n_bits, 1), 2), dtype=torch.float64, device=dev)
    N.check(L.bce_settle_trace_all(N.ptr(sp.bits), sp.n_bits, N.ptr(sp.start), N.ptr(sp.order), sp.n_touched, n_long,
                                   N.ptr(chunk_start), n_chunks, int(chunk_bits), sp.n_sources, N.ptr(table.rel),
                                   N.ptr(table.conf), N.ptr(table.present), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE,
                                   N.ptr(states), N.stream(dev)), "bce_settle_trace_all")
    return states[:sp.n_bits]


def walk_history_live(plan: LivePlan, table: ReliabilityTable, *, offsets: torch.Tensor, sid: torch.Tensor,
                      prob: torch.Tensor, states: Optional[torch.Tensor] = None,
                      half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM,
                      bins: Optional[Plan] = None, max_len: Optional[int] = None,
                      offsets_host: Optional[np.ndarray] = None, out: Optional[HistoryResult] = None,
                      check: bool = False, commit: bool = False, long_min: Optional[int] = None,
                      chunk_bits: Optional[int] = None) -> HistoryResult:
    """The reference run online at arrival granularity, bit-exact, in one pass over the signals:
    the events ``(arrival_us[i], m, 0, k)`` for signal k of market m and ``(resolve_time_us[m], m,
    1)`` for every resolved market run in ascending order; at an arrival
    ``compute_consensus(signals[:k + 1], table)`` runs with every source of the prefix fetched by
    ``get_reliability(s, scope, apply_decay=True)`` with the clock at that arrival, at a
    resolution ``update_reliability`` runs for every signal in position order and stamps the
    resolve time.  Point k of market m lands at CSR position ``offsets[m] + k`` of a
    :class:`HistoryResult` (null where ``total_weight == 0``); :func:`score_history` scores it
    unchanged.  ``table`` is one dense scope; ``offsets`` / ``sid`` / ``prob`` the plan's batch.

    :func:`live_trace` stores every prefix state of every chain once (``states=`` passes one in:
    the states do not depend on the decay parameters, so a decay grid traces once), then
    bce_consensus_history_live sorts every market once and every point reads its sources' rows
    live.  ``bins`` / ``max_len`` / ``offsets_host`` / ``out`` / ``check`` and the routes are
    :func:`consensus_history`'s; markets of up to ``HISTORY_MAX_LEN`` signals; exact order only.
    A ``sid`` outside ``[0, n_sources)`` is clamped and raises the device fault word.
    ``commit=True`` leaves the table settled as :func:`walk_forward` does: :func:`settle`'s rows,
    stamped with the resolve time of each chain's last market.  The result does not depend on
    ``long_min`` / ``chunk_bits``."""
    sp = plan.settle
    if offsets.numel() - 1 != plan.n_markets or sid.numel() != plan.n_signals or prob.numel() != plan.n_signals:
        raise ValueError("offsets / sid / prob are not the batch the plan was built from")
    N.require_gpu()
    _check_table(table.rel, table.conf, table.t_us, table.present, sp.n_sources)
    if states is None:
        states = live_trace(plan, table, long_min, chunk_bits)
    if states.dtype != torch.float64 or tuple(states.shape) != (sp.n_bits, 2) or not states.is_contiguous():
        raise ValueError(f"states must be contiguous fp64[{sp.n_bits}, 2] (live_trace of this plan)")
    live = (N.ptr(plan.arrival_us), N.ptr(sp.start), N.ptr(plan.bit_market), sp.n_bits, N.ptr(plan.resolve_time_us),
            N.ptr(table.rel), N.ptr(table.conf), N.ptr(table.t_us), N.ptr(table.present), float(half_life_days),
            float(min_rel), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE)
    rows = SimpleNamespace(relconf=states if sp.n_bits else None, bits=None, n=sp.n_sources)  # the table slot
    res = _per_signal("walk_history_live", "bce_consensus_history_live", offsets, sid.to(torch.int32).contiguous(),
                      prob.to(torch.float64).contiguous(), rows,
                      lambda M, Nsig, dev: (out or HistoryResult.alloc(Nsig, dev), live),
                      bins, max_len, offsets_host, check)
    if commit and sp.n_touched:
        _commit_chains(sp, table.rel, table.conf, table.t_us, table.present, plan.slast, plan.resolve_time_us,
                       long_min, chunk_bits)
    return res
