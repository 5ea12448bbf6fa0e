"""Settlement: a batch of resolved markets into one scope of the reliability table."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _native as N
from ..config import DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY
from .tables import ReliabilityTable, _check_csr, _check_table

# Chains of at least SETTLE_LONG_MIN bits are cut into chunks of SETTLE_CHUNK_BITS bits that run
# in parallel (settle_long_kernel): the best point of the measured grid (DESIGN.md §4.14,
# measurements/settle.txt).  2**62 disables the long path.
SETTLE_LONG_MIN = 256
SETTLE_CHUNK_BITS = 256
SETTLE_LONG_OFF = 1 << 62


def _settle_order(offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, outcome: torch.Tensor,
                  n_sources: int, market_rank: Optional[torch.Tensor] = None):
    """The integer half of :meth:`SettlePlan.build` (any device, no kernel): checks the shapes,
    lists the signals of markets with ``outcome >= 0`` in CSR order -- with ``market_rank``
    int64[M], in ``(market_rank[market], position)`` order -- and sorts them by ``sid`` keeping
    that order inside a source.  Returns ``(market, perm, key, total, start, order,
    lens_desc)``: the market of every signal (int32[N]), the signal index and clamped sid of every
    sorted position, the chain length and bit offset per source, the touched sources longest
    chain first and their lengths."""
    M, Nsig, S, offsets, lens = _check_csr(offsets, sid, n_sources, prob=prob, outcome=outcome,
                                           too_many="settle: {} markets (the signal-to-market map is int32)")
    dev = offsets.device
    i64 = dict(dtype=torch.int64, device=dev)
    market = torch.repeat_interleave(torch.arange(M, **i64), lens, output_size=Nsig)
    idx = torch.nonzero(outcome[market] >= 0).flatten()  # ascending: market, then position
    if market_rank is not None:
        if market_rank.dtype != torch.int64 or market_rank.dim() != 1 or market_rank.numel() != M:
            raise ValueError(f"market_rank must be int64 with one entry per market ({M})")
        idx = idx[torch.sort(market_rank[market[idx]], stable=True).indices]
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
    position in the market; with ``market_rank``, the rank of the market ascending).  ``bits``
    u64[ceil(n_bits / 64)] (as int64), ``start`` int64[S+1]
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
              n_sources: int, check: bool = True, market_rank: Optional[torch.Tensor] = None) -> "SettlePlan":
        """Compile ``(offsets, sid, prob)`` with ``outcome`` int8[M] (-1 unresolved, 0, 1).  The
        ordering is a stable torch sort by ``sid``; the bits and ``correct`` are one launch of
        bce_settle_compile.  Synchronises (once per batch).  A ``sid`` outside ``[0, n_sources)``
        is clamped and raises :class:`BCEError` like ``consensus(check=True)`` (``check=False``
        leaves the device fault word for a later ``_native.check_faults``); 2^31 markets or
        sources, an ``outcome`` of the wrong length or dtype, ``ValueError``.

        ``market_rank`` int64[M]: the bits of a source are ordered by ``(market_rank[market],
        position)`` instead of ``(market, position)`` -- the order the markets settle in when
        that is not their index order (:meth:`WalkPlan.build_lagged`)."""
        return cls._compile(offsets, sid, prob, outcome, n_sources, check, market_rank)[0]

    @classmethod
    def _compile(cls, offsets, sid, prob, outcome, n_sources, check, market_rank):
        """:meth:`build`: ``(plan, market, perm)`` with the market of every signal (int32[N]) and
        the signal of every chain bit in chain order (int64[n_bits])."""
        market, perm, key, total, start, order, lens_desc = _settle_order(offsets, sid, prob, outcome, n_sources,
                                                                          market_rank)
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
        return cls(bits, start, order, total, correct, Np, S, lens_desc), market, perm

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
    _check_table(rel, conf, t_us, present, S)
    long_min = SETTLE_LONG_MIN if long_min is None else long_min
    chunk_bits = SETTLE_CHUNK_BITS if chunk_bits is None else chunk_bits
    n_long, chunk_start, n_chunks = plan.chunks(long_min, chunk_bits)
    dev = rel.device
    snap = torch.empty((n_long, 2), dtype=torch.float64, device=dev) if n_long else None
    N.check(L.bce_settle_apply(N.ptr(plan.bits), plan.n_bits, N.ptr(plan.start), N.ptr(plan.order), plan.n_touched,
                               n_long, N.ptr(chunk_start), n_chunks, int(chunk_bits), S, N.ptr(rel), N.ptr(conf),
                               N.ptr(t_us), N.ptr(present), int(now_us), float(default_rel), float(default_conf),
                               N.ptr(snap), N.stream(dev)), "bce_settle_apply")


def _table_settle(self, plan: SettlePlan, now_us: int, **kw) -> None:
    """:func:`settle` in place on this table (a domain or the global scope)."""
    settle(plan, self.rel, self.conf, self.t_us, self.present, now_us, **kw)


ReliabilityTable.settle = _table_settle


def _settle_trace(plan: SettlePlan, queries, rel: torch.Tensor, conf: torch.Tensor, present: Optional[torch.Tensor],
                  n_entries: int, out: torch.Tensor, long_min: Optional[int], chunk_bits: Optional[int],
                  stream) -> None:
    """bce_settle_trace: the chains of ``plan`` walked from the start rows ``rel`` / ``conf`` /
    ``present`` (not written), the raw state in front of chain bit ``qpos`` of every query of
    ``queries`` (``qstart`` / ``qpos`` / ``qentry``, a walk's WalkQueries) written to row ``qentry``
    of ``out`` [n_entries, 2].  The states do not depend on the decay parameters
    (reliability.py:161).  ``long_min`` / ``chunk_bits`` as :func:`settle`.  The caller has passed
    ``_native.require_gpu()``."""
    L = N.lib()
    long_min = SETTLE_LONG_MIN if long_min is None else long_min
    chunk_bits = SETTLE_CHUNK_BITS if chunk_bits is None else chunk_bits
    n_long, chunk_start, n_chunks = plan.chunks(long_min, chunk_bits)
    E = n_entries
    N.check(L.bce_settle_trace(N.ptr(plan.bits), plan.n_bits, N.ptr(plan.start), N.ptr(plan.order), plan.n_touched,
                               n_long, N.ptr(chunk_start), n_chunks, int(chunk_bits), plan.n_sources, N.ptr(rel),
                               N.ptr(conf), N.ptr(present), DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE,
                               N.ptr(queries.qstart), N.ptr(queries.qpos if E else None),
                               N.ptr(queries.qentry if E else None), E, N.ptr(out), stream), "bce_settle_trace")


def _commit_chains(plan: SettlePlan, rel: torch.Tensor, conf: torch.Tensor, t_us: torch.Tensor,
                   present: Optional[torch.Tensor], slast: torch.Tensor, market_time_us: torch.Tensor,
                   long_min: Optional[int], chunk_bits: Optional[int]) -> torch.Tensor:
    """What a walk leaves behind in one scope: :func:`settle` at ``now_us = 0``, then every
    touched row stamped with the time of its chain's last market (``slast``).  Returns the touched
    rows (int64)."""
    settle(plan, rel, conf, t_us, present, 0, long_min=long_min, chunk_bits=chunk_bits)
    touched = plan.order.to(torch.int64)
    t_us.index_copy_(0, touched, market_time_us[slast[touched]])
    return touched
