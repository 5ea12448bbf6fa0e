"""Market scope and domain scope per market: lookup, consensus and settlement over sparse rows."""
from dataclasses import dataclass
from typing import Optional

import torch

from .. import _native as N
from ..config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM, DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY
from .tables import PairTable, ScopeTable, SourceTable, _check_csr, _entry_buffers
from .consensus import ConsensusResult, consensus
from .reestimate_csr import _reestimate_csr_order
from .settle import SettlePlan, settle


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
    return (lb, matched, *_entry_buffers(Q, dev))


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
        try:
            int(n_sources)
            D = int(n_domains)
        except (TypeError, ValueError):
            raise ValueError(f"n_sources / n_domains must be integers (got {n_sources!r}, {n_domains!r})") from None
        M, Nsig, S, offsets, lens = _check_csr(offsets, sid, n_sources, market_domain=market_domain,
                                               n_domains=n_domains,
                                               too_many="{} markets (the signal-to-market map is int32)")
        dev = offsets.device
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
