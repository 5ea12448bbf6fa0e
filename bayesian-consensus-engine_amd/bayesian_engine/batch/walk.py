"""Walk-forward consensus over one dense scope, and namespaced with a domain per market."""
from dataclasses import dataclass
from typing import Optional

import torch

from .. import _native as N
from ..config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM, DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY
from .tables import (PairTable, ReliabilityTable, SourceTable, _check_csr, _check_market_time, _check_table,
                     _entry_buffers)
from .consensus import ConsensusResult, consensus
from .settle import SETTLE_CHUNK_BITS, SETTLE_LONG_MIN, SettlePlan, _commit_chains, _settle_trace
from .pairs import DomainPlan, PairPlan, _bins_as_plan, _pair_merge, _pair_pointers, pair_resolve


# ---------------------------------------------------------------------------------------
# walk-forward consensus: every market reads the table as of its turn
# ---------------------------------------------------------------------------------------
# Chains of at least WALK_LONG_MIN bits are traced one worker per WALK_CHUNK_BITS bits.
WALK_LONG_MIN = SETTLE_LONG_MIN
WALK_CHUNK_BITS = SETTLE_CHUNK_BITS
_walk_buffers = _entry_buffers  # the name the walk's callers have used


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


def _query_order(chain: torch.Tensor, n_chains: int, partial: bool = False):
    """The queries of a chain family in (chain, market) order (torch only, any device): ``(qstart
    int64[n_chains + 1], qentry int64[Q], skey int64[Q])``, ``skey`` the chain of every query.
    ``chain`` int64[E] is the chain of every entry (entries ascend by market); ``partial``: the
    entries with ``chain < 0`` are no queries."""
    sel = None
    if partial:
        sel = torch.nonzero(chain >= 0).flatten()
        chain = chain[sel]
    skey, qentry = torch.sort(chain, stable=True)  # entries ascend by market: (chain, market) order
    qstart = torch.zeros(n_chains + 1, dtype=torch.int64, device=chain.device)
    qstart[1:] = torch.cumsum(torch.bincount(chain, minlength=n_chains), 0)
    return qstart, (qentry if sel is None else sel[qentry]), skey


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
    qstart, qentry, skey = _query_order(chain, C, partial)
    Q = qentry.numel()
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
class WalkQueries:
    """The queries of one chain family, as :func:`_chain_queries` returns them: ``qstart``
    int64[C+1], ``qpos`` int64[Q], ``qentry`` int32[Q], ``qlast`` int32[E] (by entry, -1: no
    earlier bit, or the entry is no query of the family), ``slast`` int64[C] (the last market that
    left a bit in the chain, -1: none).  A :class:`WalkPlan` has one family (``plan.queries``), a
    :class:`WalkScopePlan` two (``dq`` / ``gq``)."""

    qstart: torch.Tensor
    qpos: torch.Tensor
    qentry: torch.Tensor
    qlast: torch.Tensor
    slast: torch.Tensor


class _WalkPlanBase:
    """What :class:`WalkPlan` and :class:`WalkScopePlan` share.  Each ends in ``outcome`` (int8[M]
    as given to build: scoring reads it) and, from build_lagged, ``forecast_time_us`` /
    ``resolve_time_us`` int64[M] (the latter read where ``outcome >= 0``)."""

    @property
    def lagged(self) -> bool:
        return self.forecast_time_us is not None

    @staticmethod
    def _checked(offsets, sid, outcome, n_sources, times):
        """The argument checks of a compile, ``times`` its ``(forecast, resolve)`` times or None,
        then ``(S, sid clamped into [0, S), how many were outside)`` (torch only, any device)."""
        M, _, S, _, _ = _check_csr(offsets, sid, n_sources, outcome=outcome, values=False)
        if times is not None:
            _check_lag_times(*times, outcome, M)
        clamped = sid.to(torch.int32).clamp(0, S - 1)
        return S, clamped, int((clamped != sid).sum())

    @staticmethod
    def _compiled(what: str, check: bool, lagged: bool, n_clamped: int, n_sources: int, device) -> None:
        """The tail of a checked compile: the fault word of the lag-query launches, then the
        clamped sids (the settlement compile sees one only in a market that feeds a chain)."""
        if check and lagged:
            N.check_faults(device, f"{what} lag queries")
        if check and n_clamped:
            raise N.BCEError(f"{what} plan: {n_clamped} sid outside [0, {int(n_sources)})")


@dataclass
class WalkPlan(_WalkPlanBase):
    """A chronological CSR batch compiled for :func:`walk_forward`: the :class:`SettlePlan` of its
    resolved markets, the :class:`PairPlan` entry list over ALL markets, and one query per entry,
    regrouped by source (together: ``queries``): ``qstart`` int64[S+1], ``qpos`` int64[E] (query
    order, ascending inside a source: the chain position whose before-state the query reads, 0 <=
    qpos <= chain length), ``qentry`` int32[E] (the entry a query answers), ``qlast`` int32[E] (by
    entry: the market of chain bit ``qpos - 1``, -1 when ``qpos == 0``) and ``slast`` int64[S]
    (the last resolved market of every source, -1 where none).  ``n_clamped``: sids outside ``[0,
    n_sources)``.

    A plan from :meth:`build_lagged` (``lagged``) carries a forecast and a resolve time per market
    (DESIGN §4.21): its chains are in (resolve time, market, position) order, ``qpos`` counts the
    bits resolved before the entry's forecast, ``qlast`` / ``slast`` are the markets of bit
    ``qpos - 1`` and of the chain's last bit, and the walk takes its times from the plan."""

    settle: SettlePlan
    pairs: PairPlan
    qstart: torch.Tensor
    qpos: torch.Tensor
    qentry: torch.Tensor
    qlast: torch.Tensor
    slast: torch.Tensor
    n_clamped: int
    outcome: Optional[torch.Tensor] = None
    forecast_time_us: Optional[torch.Tensor] = None
    resolve_time_us: Optional[torch.Tensor] = None

    @property
    def total(self) -> torch.Tensor:
        return self.settle.total

    @property
    def correct(self) -> torch.Tensor:
        return self.settle.correct

    @property
    def queries(self) -> WalkQueries:
        return WalkQueries(self.qstart, self.qpos, self.qentry, self.qlast, self.slast)

    @classmethod
    def order(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
              n_sources: int):
        """The integer half of :meth:`build` (torch only, CPU tensors included): ``(pairs, qstart,
        qpos, qentry, qlast, slast, n_clamped)``.  Argument errors as :meth:`SettlePlan.build`."""
        S, clamped, n_clamped = cls._checked(offsets, sid, outcome, n_sources, None)
        pairs = PairPlan.build(offsets, clamped, prob, S)  # checks offsets / prob
        return (pairs, *_walk_queries(pairs, offsets, outcome), n_clamped)

    @classmethod
    def _compile(cls, offsets, sid, prob, outcome, n_sources, check, times=None):
        """:meth:`build` and, with the ``(forecast, resolve)`` times, :meth:`build_lagged`."""
        S, clamped, n_clamped = cls._checked(offsets, sid, outcome, n_sources, times)
        pairs = PairPlan.build(offsets, clamped, prob, S)  # checks offsets / prob
        if times is None:
            q = WalkQueries(*_walk_queries(pairs, offsets, outcome))
            splan = SettlePlan.build(offsets, sid, prob, outcome, n_sources, check=check)
        else:
            times = forecast, resolve = times[0].contiguous(), times[1].contiguous()
            N.require_gpu()
            splan, q = _lag_family(offsets, sid, prob, outcome, n_sources, check, _resolve_rank(outcome, resolve),
                                   pairs, pairs.usid, forecast, resolve)
        cls._compiled("walk", check, times is not None, n_clamped, n_sources, offsets.device)
        return cls(splan, pairs, q.qstart, q.qpos, q.qentry, q.qlast, q.slast, n_clamped, outcome.contiguous(),
                   *(times or ()))

    @classmethod
    def build(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
              n_sources: int, check: bool = True) -> "WalkPlan":
        """Compile ``(offsets, sid, prob)`` in chronological market order with ``outcome``
        int8[M] (-1 unresolved, 0, 1).  Torch sorts and scans plus :meth:`SettlePlan.build`;
        synchronises.  A ``sid`` outside ``[0, n_sources)`` is clamped and raises
        :class:`BCEError` (``check=False``: the fault is left for :func:`walk_forward`)."""
        return cls._compile(offsets, sid, prob, outcome, n_sources, check)

    @classmethod
    def build_lagged(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
                     n_sources: int, forecast_time_us: torch.Tensor, resolve_time_us: torch.Tensor,
                     check: bool = True) -> "WalkPlan":
        """:meth:`build` for markets that are forecast at one time and settle at a later one:
        market m is read at ``forecast_time_us[m]`` and, if ``outcome[m] >= 0``, its updates run
        at ``resolve_time_us[m]`` -- the reference as an event loop sorted by (time, market,
        forecast before resolution).  Markets are given in forecast order.  ``ValueError`` (from
        torch checks on whatever device the tensors are on, before the library is touched) unless
        both are int64[M], the forecast times do not decrease and ``resolve >= forecast`` for
        every resolved market; resolve times of unresolved markets are ignored.

        The chains are compiled in (resolve time, market, position) order (one stable sort over M
        for the rank, :meth:`SettlePlan.build` with ``market_rank``); the queries are the entries
        in (source, market) order as in :meth:`build`, and one launch of bce_walk_lag_queries
        bisects every query's visible prefix.  With ``resolve == forecast`` the plan equals
        :meth:`build`'s, array for array."""
        return cls._compile(offsets, sid, prob, outcome, n_sources, check, (forecast_time_us, resolve_time_us))


def _resolve_rank(outcome: torch.Tensor, resolve: torch.Tensor) -> torch.Tensor:
    """int64[M]: the rank of every resolved market by (resolve time, market); the others behind
    them (one stable sort over M, any device)."""
    M = outcome.numel()
    i64 = dict(dtype=torch.int64, device=outcome.device)
    key = torch.where(outcome >= 0, resolve, torch.full_like(resolve, torch.iinfo(torch.int64).max))
    rank = torch.empty(M, **i64)
    rank[torch.sort(key, stable=True).indices] = torch.arange(M, **i64)
    return rank


def _lag_family(offsets: torch.Tensor, chain_sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
                n_chains: int, check: bool, rank: torch.Tensor, pairs: PairPlan, chain: torch.Tensor,
                forecast: torch.Tensor, resolve: torch.Tensor, partial: bool = False):
    """One chain family of a lagged plan: ``(SettlePlan, WalkQueries)``.  The chains are those of
    ``(offsets, chain_sid, prob, outcome)`` over ``n_chains`` chain ids, compiled in (``rank``,
    position) order; ``chain`` int32[>= E] is the chain every entry of ``pairs`` reads.  The
    queries are the entries in (chain, market) order -- with ``partial``, only those with ``chain
    >= 0``; the ``qlast`` of the others stays -1 -- and one launch of bce_walk_lag_queries bisects
    every query's visible prefix and reads every chain's last market.  The fault word is left to
    the caller, who has passed ``_native.require_gpu()``."""
    L = N.lib()
    splan, market, perm = SettlePlan._compile(offsets, chain_sid, prob, outcome, n_chains, check, rank)
    bit_market = market[perm].contiguous()
    E, M, C = pairs.n_entries, pairs.n_markets, splan.n_sources
    dev = offsets.device
    qstart, qentry, _ = _query_order(chain[:E].to(torch.int64), C, partial)
    qentry = qentry.to(torch.int32).contiguous()
    Q = qentry.numel()
    qpos = torch.empty(Q, dtype=torch.int64, device=dev)
    qlast = torch.full((E,), -1, dtype=torch.int32, device=dev)
    slast = torch.empty(C, dtype=torch.int64, device=dev)
    ent = lambda t: N.ptr(t if E else None)  # noqa: E731
    qry = lambda t: N.ptr(t if Q else None)  # noqa: E731
    N.check(L.bce_walk_lag_queries(Q, qry(qentry), ent(chain), ent(pairs.emarket), E, N.ptr(splan.start), C,
                                   N.ptr(bit_market if splan.n_bits else None), splan.n_bits,
                                   N.ptr(forecast if M else None), N.ptr(resolve if M else None), M, qry(qpos),
                                   ent(qlast), N.ptr(slast), N.stream(dev)), "bce_walk_lag_queries")
    return splan, WalkQueries(qstart, qpos, qentry, qlast, slast)


def _check_lag_times(forecast_time_us: torch.Tensor, resolve_time_us: torch.Tensor, outcome: torch.Tensor,
                     M: int) -> None:
    """The validity of a lagged batch's times (torch only, any device)."""
    for name, t in (("forecast_time_us", forecast_time_us), ("resolve_time_us", resolve_time_us)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or t.numel() != M:
            raise ValueError(f"{name} must be int64 with one entry per market ({M})")
    if forecast_time_us.device != outcome.device or resolve_time_us.device != outcome.device:
        raise ValueError("forecast_time_us / resolve_time_us must be on the batch's device")
    if M > 1 and bool((forecast_time_us[1:] < forecast_time_us[:-1]).any()):
        at = int(torch.nonzero(forecast_time_us[1:] < forecast_time_us[:-1])[0]) + 1
        raise ValueError(f"forecast times must not decrease: market {at} is forecast before market {at - 1}")
    early = (outcome >= 0) & (resolve_time_us < forecast_time_us)
    if bool(early.any()):
        at = int(torch.nonzero(early)[0])
        raise ValueError(f"market {at} resolves before it is forecast")


def _walk_times(plan, market_time_us: Optional[torch.Tensor]):
    """``(stamp, now)``, both contiguous: the time a market's updates are stamped with and the
    time it is read at -- the plan's resolve and forecast times, or ``market_time_us`` twice.
    ``plan``: a :class:`WalkPlan` or a :class:`WalkScopePlan`."""
    if plan.lagged:
        if market_time_us is not None:
            raise ValueError("a lagged plan carries its own times: market_time_us must be None")
        return plan.resolve_time_us.contiguous(), plan.forecast_time_us.contiguous()
    if market_time_us is None:
        raise ValueError("market_time_us is needed: the plan has no times of its own (WalkPlan.build_lagged does)")
    _check_market_time(market_time_us, plan.pairs.n_markets)
    now = market_time_us.contiguous()
    return now, now


def _check_batch(plan, offsets: torch.Tensor, prob: torch.Tensor) -> None:
    """``offsets`` / ``prob`` have the sizes of the batch ``plan`` (either kind) was built from."""
    pp = plan.pairs
    if offsets.numel() - 1 != pp.n_markets or prob.numel() != pp.esid.numel():
        raise ValueError("offsets / prob are not the batch the plan was built from")


class _ConsensusFields:
    """For a result that holds a :class:`ConsensusResult` as ``result``: its fields, directly."""

    def __getattr__(self, name):
        if name in ConsensusResult.__dataclass_fields__:
            res = self.__dict__.get("result")
            if res is not None:
                return getattr(res, name)
        raise AttributeError(name)

    def is_null(self, offsets: torch.Tensor) -> torch.Tensor:
        return self.result.is_null(offsets)


@dataclass
class WalkResult(_ConsensusFields):
    """:func:`walk_forward`: ``result`` is the batch's :class:`ConsensusResult`, its ``usid``
    holding the ENTRY index (| cold << 31) as in :class:`PairConsensusResult`; ``scope_present``
    u8[E]: a row existed when the entry was read; ``total`` / ``correct`` int64[S] of the plan."""

    result: ConsensusResult
    plan: WalkPlan
    scope_present: torch.Tensor
    total: torch.Tensor
    correct: torch.Tensor


def walk_trace(plan: WalkPlan, table: "ReliabilityTable", market_time_us: Optional[torch.Tensor] = None, *,
               all_present: bool = True, long_min: Optional[int] = None, chunk_bits: Optional[int] = None,
               half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM):
    """The read side of :func:`walk_forward` alone (bce_settle_trace + bce_walk_read): the
    consensus table over the entry index -- every entry's ``get_reliability(apply_decay=True)`` at
    its market's time, after the earlier markets were settled -- and ``scope_present`` u8[E].
    The table is not written.  ``market_time_us``: as :func:`walk_forward`."""
    E = plan.pairs.n_entries
    dev = table.rel.device
    relconf, bits, exists = _entry_buffers(E, dev)  # relconf: the trace, decayed in place
    _walk_settle_trace(plan, table, market_time_us, relconf, long_min, chunk_bits)
    _walk_read(plan, table, market_time_us, relconf, relconf, bits, exists, all_present, half_life_days, min_rel)
    return SourceTable(relconf, bits, range(E)), exists[:E]  # "names": the entry indices


def _walk_settle_trace(plan: WalkPlan, table: "ReliabilityTable", market_time_us: Optional[torch.Tensor],
                       trace: torch.Tensor, long_min: Optional[int], chunk_bits: Optional[int]) -> None:
    """:func:`_settle_trace` of ``plan`` from ``table`` into ``trace`` [E, 2]; checks the table
    and the times."""
    _walk_times(plan, market_time_us)
    N.require_gpu()
    sp, pp = plan.settle, plan.pairs
    _check_table(table.rel, table.conf, table.t_us, table.present, sp.n_sources)
    _settle_trace(sp, plan.queries, table.rel, table.conf, table.present, pp.n_entries, trace, long_min,
                  chunk_bits, N.stream(table.rel.device))


def _walk_read(plan: WalkPlan, table: "ReliabilityTable", market_time_us: Optional[torch.Tensor],
               trace: torch.Tensor, relconf: torch.Tensor, bits: torch.Tensor, exists: torch.Tensor, all_present: bool,
               half_life_days: float, min_rel: float) -> None:
    """bce_walk_read_lag (an ordinary plan: its one time array twice) from ``trace`` into
    ``relconf`` (may be ``trace`` itself) / ``bits`` / ``exists``."""
    L = N.require_gpu()
    sp, pp = plan.settle, plan.pairs
    S, E, M = sp.n_sources, pp.n_entries, pp.n_markets
    stamp, now = _walk_times(plan, market_time_us)
    ent = lambda t: N.ptr(t if E else None)  # noqa: E731
    N.check(L.bce_walk_read_lag(E, ent(pp.usid), ent(pp.emarket), ent(plan.qlast), N.ptr(trace),
                                N.ptr(stamp if M else None), N.ptr(now if M else None), M, N.ptr(table.rel),
                                N.ptr(table.conf), N.ptr(table.t_us), N.ptr(table.present), S, float(half_life_days),
                                float(min_rel), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE, int(not all_present),
                                int(plan.n_clamped > 0), N.ptr(relconf), N.ptr(bits), N.ptr(exists),
                                N.stream(table.rel.device)), "bce_walk_read_lag")


def walk_forward(plan: WalkPlan, table: "ReliabilityTable", market_time_us: Optional[torch.Tensor] = None, *,
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

    A plan from :meth:`WalkPlan.build_lagged` takes its times from the plan (``market_time_us``
    stays None; passing one as well, or none for an ordinary plan, ``ValueError``): market m is
    read at its forecast time, settled at its resolve time, and every state is stamped with the
    resolve time of the market of its last bit.

    :func:`walk_trace` builds the consensus table over the entries, :func:`consensus` runs
    unchanged with ``plan.pairs.esid`` as the ranks (``mode`` and ``consensus_kwargs`` go to it;
    ``bins=`` is its length-bin :class:`Plan`).  ``commit=True`` also leaves the table settled:
    :func:`settle`'s ``rel`` / ``conf`` / ``present`` with ``t_us`` the time of each source's last
    resolved market; ``commit=False`` leaves it untouched.  The result does not depend on
    ``long_min`` / ``chunk_bits`` (defaults WALK_LONG_MIN / WALK_CHUNK_BITS)."""
    sp, pp = plan.settle, plan.pairs
    _check_batch(plan, offsets, prob)
    stamp, _ = _walk_times(plan, market_time_us)
    wtable, exists = walk_trace(plan, table, market_time_us, all_present=all_present, long_min=long_min,
                                chunk_bits=chunk_bits)
    res = consensus(offsets, pp.esid, prob.to(torch.float64), wtable, mode=mode, **_bins_as_plan(consensus_kwargs))
    if commit and sp.n_touched:
        _commit_chains(sp, table.rel, table.conf, table.t_us, table.present, plan.slast, stamp, long_min, chunk_bits)
    return WalkResult(res, plan, exists, sp.total, sp.correct)


def _table_walk_forward(self, plan: WalkPlan, market_time_us: Optional[torch.Tensor] = None, **kw) -> WalkResult:
    """:func:`walk_forward` on this table (a domain or the global scope)."""
    return walk_forward(plan, self, market_time_us, **kw)


ReliabilityTable.walk_forward = _table_walk_forward


# ---------------------------------------------------------------------------------------
# namespaced walk-forward: a domain per market, the fallback at every read
# ---------------------------------------------------------------------------------------
def _global_outcome(outcome: torch.Tensor, market_domain: torch.Tensor, update_global: bool) -> torch.Tensor:
    """The outcome as the global chains see it: every resolved market with ``update_global``,
    else only those without a domain (reliability_abstraction.py:211-229)."""
    if update_global:
        return outcome
    return torch.where(market_domain.to(outcome.device) < 0, outcome, torch.full_like(outcome, -1))


@dataclass
class WalkScopePlan(_WalkPlanBase):
    """A chronological CSR batch whose markets belong to different domains, compiled for
    :func:`walk_forward_scoped`.  ``pairs``: the :class:`PairPlan` over ALL markets (entries E);
    ``dplan``: the :class:`DomainPlan` (chains F) and ``dentry`` int32[E], the domain chain of
    every entry (-1: its market has no domain); ``dsettle`` / ``gsettle``: the
    :class:`SettlePlan` of the domain chains (over the F entry space, as :func:`settle_domains`
    compiles it) and of the global chains (over the S sources: the resolved markets without a
    domain, or every resolved market with ``update_global``); ``dq`` / ``gq``: the
    :class:`WalkQueries` of either family -- every entry is a query of its global chain, and of
    its domain chain where ``dentry >= 0``.  ``n_clamped``: sids outside ``[0, n_sources)``.

    A plan from :meth:`build_lagged` (``lagged``) carries a forecast and a resolve time per market
    (DESIGN §4.22): the chains of both families are in (resolve time, market, position) order, the
    queries count the bits resolved before the entry's forecast, and the walk takes its times from
    the plan."""

    pairs: PairPlan
    dplan: "DomainPlan"
    dentry: torch.Tensor
    dsettle: SettlePlan
    gsettle: SettlePlan
    dq: WalkQueries
    gq: WalkQueries
    update_global: bool
    n_clamped: int
    outcome: Optional[torch.Tensor] = None
    forecast_time_us: Optional[torch.Tensor] = None
    resolve_time_us: Optional[torch.Tensor] = None

    @classmethod
    def _entries(cls, offsets, sid, prob, outcome, market_domain, n_sources, n_domains, update_global, times=None):
        """``(pairs, dplan, dentry int64[E], domain outcome, global outcome, n_clamped)`` behind the
        argument checks: the entry list, the (domain, source) chains, the chain of every entry and
        the outcome as either chain family sees it (torch only, any device)."""
        S, clamped, n_clamped = cls._checked(offsets, sid, outcome, n_sources, times)
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
        dout = torch.where(dplan.market_domain >= 0, outcome, torch.full_like(outcome, -1))
        return pairs, dplan, dentry, dout, _global_outcome(outcome, dplan.market_domain, update_global), n_clamped

    @staticmethod
    def _queries(pairs: PairPlan, dplan: "DomainPlan", dentry: torch.Tensor, dout: torch.Tensor, gout: torch.Tensor):
        """``(dq, gq)`` of an ordinary plan (torch only, any device)."""
        E = pairs.n_entries
        emarket = pairs.emarket[:E].to(torch.int64)
        signals = _entry_signals(pairs)
        dq = _chain_queries(dentry, signals * (dout[emarket] >= 0), emarket, max(dplan.n_entries, 1), partial=True)
        gq = _chain_queries(pairs.usid[:E].to(torch.int64), signals * (gout[emarket] >= 0), emarket, pairs.n_sources)
        return WalkQueries(*dq), WalkQueries(*gq)

    @classmethod
    def order(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
              market_domain: torch.Tensor, n_sources: int, n_domains: int, update_global: bool = False):
        """The integer half of :meth:`build` (torch only, CPU tensors included): ``(pairs, dplan,
        dentry, dq, gq, n_clamped)``.  Argument errors as :meth:`WalkPlan.order` and
        :meth:`DomainPlan.build`."""
        pairs, dplan, dentry, dout, gout, n_clamped = cls._entries(offsets, sid, prob, outcome, market_domain,
                                                                   n_sources, n_domains, update_global)
        return (pairs, dplan, dentry.to(torch.int32), *cls._queries(pairs, dplan, dentry, dout, gout), n_clamped)

    @classmethod
    def _compile(cls, offsets, sid, prob, outcome, market_domain, n_sources, n_domains, update_global, check,
                 times=None):
        """:meth:`build` and, with the ``(forecast, resolve)`` times, :meth:`build_lagged`."""
        update_global = bool(update_global)
        pairs, dplan, dentry, dout, gout, n_clamped = cls._entries(offsets, sid, prob, outcome, market_domain,
                                                                   n_sources, n_domains, update_global, times)
        dchains = (offsets, dplan.esid, prob, dout, max(dplan.n_entries, 1), check)
        gchains = (offsets, sid, prob, gout, n_sources, check)
        dentry32 = dentry.to(torch.int32).contiguous()
        if times is None:
            dq, gq = cls._queries(pairs, dplan, dentry, dout, gout)
            dsettle, gsettle = SettlePlan.build(*dchains), SettlePlan.build(*gchains)
        else:
            times = forecast, resolve = times[0].contiguous(), times[1].contiguous()
            rank = _resolve_rank(outcome, resolve)
            N.require_gpu()
            dsettle, dq = _lag_family(*dchains, rank, pairs, dentry32, forecast, resolve, partial=True)
            gsettle, gq = _lag_family(*gchains, rank, pairs, pairs.usid, forecast, resolve)
        cls._compiled("walk scope", check, times is not None, n_clamped, n_sources, offsets.device)
        return cls(pairs, dplan, dentry32, dsettle, gsettle, dq, gq, update_global, n_clamped, outcome.contiguous(),
                   *(times or ()))

    @classmethod
    def build(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
              market_domain: torch.Tensor, n_sources: int, n_domains: int, update_global: bool = False,
              check: bool = True) -> "WalkScopePlan":
        """Compile ``(offsets, sid, prob)`` in chronological market order with ``outcome``
        int8[M] (-1 unresolved, 0, 1) and ``market_domain`` int32[M] (-1: none).  Torch sorts and
        scans plus two :meth:`SettlePlan.build`; synchronises.  A ``sid`` outside ``[0,
        n_sources)`` is clamped and raises :class:`BCEError` (``check=False``: the fault is left
        for :func:`walk_forward_scoped`)."""
        return cls._compile(offsets, sid, prob, outcome, market_domain, n_sources, n_domains, update_global, check)

    @classmethod
    def build_lagged(cls, offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
                     market_domain: torch.Tensor, n_sources: int, n_domains: int, forecast_time_us: torch.Tensor,
                     resolve_time_us: torch.Tensor, update_global: bool = False,
                     check: bool = True) -> "WalkScopePlan":
        """:meth:`build` for markets that are forecast at one time and settle at a later one, as
        :meth:`WalkPlan.build_lagged` (the same times, the same ``ValueError`` from torch checks
        before the library is touched): market m is read at ``forecast_time_us[m]`` and, if
        ``outcome[m] >= 0``, its updates run at ``resolve_time_us[m]`` at the scopes of its domain
        -- the reference as an event loop sorted by (time, market, forecast before resolution).

        The rank of the resolved markets by (resolve time, market) is computed once; both chain
        families are compiled in that order (:meth:`SettlePlan.build` with ``market_rank``), and
        one launch of bce_walk_lag_queries per family bisects every query's visible prefix: the
        global family over ``usid`` and the S sources, the domain family over ``dentry`` and the F
        chains, its queries only the entries with ``dentry >= 0``.  With ``resolve == forecast``
        the plan equals :meth:`build`'s, array for array."""
        return cls._compile(offsets, sid, prob, outcome, market_domain, n_sources, n_domains, update_global, check,
                            (forecast_time_us, resolve_time_us))


@dataclass
class WalkScopeResult(_ConsensusFields):
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


@dataclass
class _ScopeTraces:
    """What the read of a namespaced walk starts from: ``raw`` the raw start rows of the domain
    chains (:func:`pair_resolve`, None without one) and ``dhas`` their "updated_at is truthy";
    ``dtrace`` / ``gtrace`` the traced states of either family over the entry index (``gtrace``
    None where no global chain has a bit); ``global_has`` the ``has`` flags of the global table."""

    raw: Optional["PairResolveResult"]  # noqa: F821
    dhas: Optional[torch.Tensor]
    dtrace: Optional[torch.Tensor]
    gtrace: Optional[torch.Tensor]
    global_has: Optional[torch.Tensor]


def _walk_scope_traces(plan: WalkScopePlan, domains: PairTable, global_table: Optional["ReliabilityTable"],
                       market_time_us: Optional[torch.Tensor], pairs: Optional[PairTable],
                       global_has: Optional[torch.Tensor], long_min: Optional[int], chunk_bits: Optional[int],
                       gtrace: torch.Tensor) -> _ScopeTraces:
    """The argument checks of a namespaced walk and one bce_settle_trace per chain family that
    has bits: the domain chains from their raw start rows into a buffer of their own, the global
    chains from the dense table into ``gtrace`` [E, 2].  The states do not depend on the decay
    parameters; no table is written."""
    pp, dp = plan.pairs, plan.dplan
    S, E, M, F = pp.n_sources, pp.n_entries, pp.n_markets, dp.n_entries
    _walk_times(plan, market_time_us)
    N.require_gpu()
    if domains.n_markets != dp.n_markets or domains.n_sources != S:
        raise ValueError("the plan and the domain table describe different batches")
    if pairs is not None and (pairs.n_markets != M or pairs.n_sources != S):
        raise ValueError("the plan and the pair table describe different batches")
    g = global_table
    if g is None and plan.gsettle.n_touched:
        raise ValueError("the batch updates the global scope: global_table is needed")
    if g is not None:
        _check_table(g.rel, g.conf, g.t_us, g.present, S, "the global table must have n_sources rows")
        if global_has is None:
            global_has = g.present if g.present is not None else torch.ones(S, dtype=torch.uint8,
                                                                           device=g.rel.device)
        assert global_has.dtype == torch.uint8 and global_has.numel() == S, "global_has must be u8[n_sources]"
    dev = pp.esid.device
    st = N.stream(dev)
    raw = dhas = dtrace = None
    if F and E:  # the domain chains: start rows by the raw pair lookup over the (domain, source) entries
        raw = pair_resolve(dp.uoffsets, dp.usid, domains, 0, mode="raw", emarket=dp.emarket)
        R = domains.n_rows
        dhas = (raw.matched & domains.has[raw.lb.clamp(max=R - 1)]) if R else torch.zeros_like(raw.matched)
        dtrace = torch.empty((E, 2), dtype=torch.float64, device=dev)
        if plan.dsettle.n_touched:
            _settle_trace(plan.dsettle, plan.dq, raw.rel, raw.conf, raw.present, E, dtrace, long_min, chunk_bits, st)
    gtraced = g is not None and plan.gsettle.n_touched > 0
    if gtraced:
        _settle_trace(plan.gsettle, plan.gq, g.rel, g.conf, g.present, E, gtrace, long_min, chunk_bits, st)
    return _ScopeTraces(raw, dhas, dtrace, gtrace if gtraced else None, global_has)


def _walk_scope_launch(plan: WalkScopePlan, tr: _ScopeTraces, global_table: Optional["ReliabilityTable"],
                       market_time_us: Optional[torch.Tensor], pairs: Optional[PairTable], mark_cold: bool,
                       half_life_days: float, min_rel: float, relconf: torch.Tensor, bits: torch.Tensor,
                       scope: torch.Tensor) -> None:
    """bce_walk_scope_read_lag (an ordinary plan: its one time array twice) from the traces of
    ``tr`` into ``relconf`` (may be ``tr.gtrace`` itself) / ``bits`` / ``scope``."""
    L = N.lib()
    pp, g, raw = plan.pairs, global_table, tr.raw
    S, E, M, F = pp.n_sources, pp.n_entries, pp.n_markets, plan.dplan.n_entries
    stamp, now = _walk_times(plan, market_time_us)
    ent = lambda t: N.ptr(t if E else None)  # noqa: E731
    dom = [N.ptr(x) for x in ((plan.dentry, plan.dq.qlast, tr.dtrace, raw.rel, raw.conf, raw.t_us, tr.dhas)
                              if raw is not None else (None,) * 7)]
    gtraced = tr.gtrace is not None
    glo = [N.ptr(x) for x in ((plan.gq.qlast if gtraced else None, tr.gtrace, g.rel, g.conf, g.t_us,
                               tr.global_has.contiguous()) if g is not None else (None,) * 6)]
    N.check(L.bce_walk_scope_read_lag(
        E, ent(pp.usid), ent(pp.emarket), N.ptr(stamp if M else None), N.ptr(now if M else None), M, S,
        N.ptr(pairs.poffsets if pairs is not None else None), *_pair_pointers(pairs),
        pairs.n_rows if pairs is not None else 0, *dom, F if raw is not None else 0, *glo, float(half_life_days),
        float(min_rel), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE, int(bool(mark_cold)), int(plan.n_clamped > 0),
        N.ptr(relconf), N.ptr(bits), N.ptr(scope), N.stream(pp.esid.device)), "bce_walk_scope_read_lag")


def _walk_scope_read(plan: WalkScopePlan, domains: PairTable, global_table: Optional["ReliabilityTable"],
                     market_time_us: Optional[torch.Tensor], pairs: Optional[PairTable],
                     global_has: Optional[torch.Tensor], mark_cold: bool, long_min: Optional[int],
                     chunk_bits: Optional[int], half_life_days: float, min_rel: float):
    """The launches of :func:`walk_scope_trace`; also returns the raw start rows of the domain
    chains (:func:`pair_resolve`, None without one) and the ``has`` flags of the global table."""
    E = plan.pairs.n_entries
    relconf, bits, scope = _entry_buffers(E, plan.pairs.esid.device)  # relconf: the global trace, overwritten in place
    tr = _walk_scope_traces(plan, domains, global_table, market_time_us, pairs, global_has, long_min, chunk_bits,
                            relconf)
    _walk_scope_launch(plan, tr, global_table, market_time_us, pairs, mark_cold, half_life_days, min_rel, relconf,
                       bits, scope)
    return SourceTable(relconf, bits, range(E)), scope[:E], tr.raw, tr.global_has  # "names": the entry indices


def walk_scope_trace(plan: WalkScopePlan, domains: PairTable, global_table: Optional["ReliabilityTable"],
                     market_time_us: Optional[torch.Tensor] = None, *, pairs: Optional[PairTable] = None,
                     global_has: Optional[torch.Tensor] = None, mark_cold: bool = False,
                     long_min: Optional[int] = None, chunk_bits: Optional[int] = None,
                     half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM):
    """The read side of :func:`walk_forward_scoped` alone: one bce_settle_trace per chain family
    that has bits (the domain chains from the raw :func:`pair_resolve` rows of ``plan.dplan``, the
    global chains from the dense table), then bce_walk_scope_read.  Returns the consensus table
    over the entry index -- every entry's namespaced ``get_reliability(apply_decay=True)`` at its
    market's time, after the earlier markets were settled -- and ``scope`` u8[E] (NS_* codes).
    No table is written.  ``market_time_us``: as :func:`walk_forward_scoped`."""
    return _walk_scope_read(plan, domains, global_table, market_time_us, pairs, global_has, mark_cold, long_min,
                            chunk_bits, half_life_days, min_rel)[:2]


def walk_forward_scoped(plan: WalkScopePlan, domains: PairTable, global_table: Optional["ReliabilityTable"],
                        market_time_us: Optional[torch.Tensor] = None, *, offsets: torch.Tensor, prob: torch.Tensor,
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
    ``long_min`` / ``chunk_bits``.

    A plan from :meth:`WalkScopePlan.build_lagged` takes its times from the plan
    (``market_time_us`` stays None; passing one as well, or none for an ordinary plan,
    ``ValueError``): market m is read at its forecast time and settled at its resolve time, a
    scope exists for an entry when a bit of its chain resolved before the entry's forecast or its
    start row has ``has``, and every state and every committed row is stamped with the resolve
    time of the market of its chain's last bit."""
    pp = plan.pairs
    _check_batch(plan, offsets, prob)
    stamp, _ = _walk_times(plan, market_time_us)
    wtable, scope, raw, ghas = _walk_scope_read(plan, domains, global_table, market_time_us, pairs, global_has,
                                                mark_cold, long_min, chunk_bits, DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM)
    res = consensus(offsets, pp.esid, prob.to(torch.float64), wtable, mode=mode, **_bins_as_plan(consensus_kwargs))
    ds, gs = plan.dsettle, plan.gsettle
    new_domains = domains
    if commit:
        if ds.n_touched and raw is not None:
            _commit_chains(ds, raw.rel, raw.conf, raw.t_us, raw.present, plan.dq.slast, stamp, long_min,
                           chunk_bits)
            new_domains = _pair_merge(plan.dplan, domains, raw, ds.total[:plan.dplan.n_entries] > 0)
        if gs.n_touched:
            g = global_table
            touched = _commit_chains(gs, g.rel, g.conf, g.t_us, g.present, plan.gq.slast, stamp, long_min,
                                     chunk_bits)
            if ghas is not g.present:
                ghas.index_fill_(0, touched, 1)
    return WalkScopeResult(res, plan, scope, new_domains, ds.total, ds.correct, gs.total, gs.correct)
