"""Agreement counts, the namespaced fallback, cross-market aggregation, dense re-estimation."""
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from .. import _native as N
from ..config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM, DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY
from .tables import ScopeTable, SourceTable
from .consensus import _MODES


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
