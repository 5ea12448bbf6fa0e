"""Re-estimation over a ragged CSR batch: compile once, iterate on the compact form."""
from dataclasses import dataclass
from typing import Optional

import torch

from .. import _native as N
from .tables import _check_csr

_RC_MAX_RUN = 65535  # signals of one source in one market: the votes are two 16-bit counts


def _reestimate_csr_order(offsets: torch.Tensor, sid: torch.Tensor, prob: torch.Tensor, n_sources: int,
                          max_run: Optional[int] = _RC_MAX_RUN):
    """The integer half of :meth:`ReestimateCsrPlan.build` and :meth:`PairPlan.build` (any device,
    no kernel): checks the shapes, sorts the signals by (market, sid) keeping input order inside
    a pair, and returns ``(key, perm, group_start, uoffsets)`` as bce_reestimate_csr_compile takes
    them.  ``max_run`` bounds the signals of one source in one market (None: no bound)."""
    int(n_sources)  # not a number: int()'s own TypeError / ValueError, as before the shared check
    M, Nsig, S, offsets, lens = _check_csr(
        offsets, sid, n_sources, prob=prob,
        too_many="reestimate_csr: {} markets (the compact form indexes markets with int32)")
    dev = offsets.device
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
