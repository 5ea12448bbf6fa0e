"""Expected values of the CSR re-estimation: the CPU oracle's consensus_csr and
agreement_stats composed in Python, one round after the other (test infrastructure only).

A round is compute_consensus with ``source_reliability = w`` for every market (core.py:103-144),
the outcome of every market (a known outcome; else skipped when the consensus is None or a
probability is out of range; else ``consensus >= 0.5``), the summarize_sources counts over the
raw signals (market.py:293-304) and ``w = correct / total`` (0.5 where total == 0,
market.py:309-310)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import oracle as orc


class Round(NamedTuple):
    cons: np.ndarray     # float64[M], 0.0 where null
    null: np.ndarray     # uint8[M]
    outcome: np.ndarray  # int8[M]: -1 skipped, 0, 1
    correct: np.ndarray  # int64[S]
    total: np.ndarray    # int64[S]
    w: np.ndarray        # float64[S], the weights AFTER the round


def reference_rounds(offsets, sid, prob, n_sources, iters, w0=0.5, w=None, known=None):
    """Every round's (cons, null, outcome, correct, total, w) as a list of :class:`Round`."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    sid = np.ascontiguousarray(sid, np.int32)
    prob = np.ascontiguousarray(prob, np.float64)
    S = int(n_sources)
    w = np.full(S, float(w0), np.float64) if w is None else np.array(w, np.float64)
    conf = np.full(S, 0.25)            # any confidence: it never reaches the consensus
    present = np.ones(S, np.uint8)     # every source is a key of the reliability dict
    empty = np.diff(offsets) == 0
    rounds = []
    for _ in range(iters):
        r = orc.consensus_csr(offsets, sid, prob, w, conf, present)
        null = empty | (r["total_weight"] == 0)
        cons = r["consensus"].copy()
        outcome = np.where(null | (r["err_idx"] >= 0), -1, cons >= 0.5).astype(np.int8)
        if known is not None:
            kn = np.asarray(known, np.int8)
            outcome = np.where(kn >= 0, kn, outcome).astype(np.int8)
        correct, total = orc.agreement_stats(offsets, sid, prob, outcome, S)
        correct, total = correct.astype(np.int64), total.astype(np.int64)
        w = np.where(total > 0, correct / np.maximum(total, 1), 0.5)
        rounds.append(Round(cons, null.astype(np.uint8), outcome, correct, total, w.copy()))
    return rounds
