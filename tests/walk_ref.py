"""Expected values of walk-forward consensus: the reference run online, composed from the CPU
oracle one market at a time (test infrastructure only).

For m = 0..M-1: the table is read through ``orc.decay_view`` with the clock at the market's time
(get_reliability(apply_decay=True) of every source), ``orc.consensus_csr`` scores the one-market
CSR against it, and a resolved market is then settled by ``settle_ref.apply_chains`` on its own
slice with ``now = market_time_us[m]`` (update_reliability per signal, in position order)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc
from settle_ref import apply_chains, chains

COLD = np.int32(-2**31)


def walk_ref(offsets, sid, prob, outcome, n_sources, rel, conf, t_us, present, market_time_us,
             all_present=True):
    """Returns ``(out, state)``: ``out`` the consensus_csr fields over the whole batch (per market
    and per signal slot; ``usid`` holds the SOURCE rank | cold << 31) plus ``exists`` per slot (a
    row existed when the slot's source was read) and ``rel_read`` / ``conf_read`` per slot;
    ``state`` the final ``(rel, conf, t_us, present)``."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    S = int(n_sources)
    sid = np.clip(np.ascontiguousarray(sid, np.int64), 0, S - 1).astype(np.int32)  # as the builder clamps
    prob = np.ascontiguousarray(prob, np.float64)
    outcome = np.ascontiguousarray(outcome, np.int8)
    rel, conf = np.array(rel, np.float64), np.array(conf, np.float64)
    t_us, present = np.array(t_us, np.int64), np.array(present, np.uint8)
    M, Nsig = len(offsets) - 1, len(sid)
    out = dict(consensus=np.zeros(M), confidence=np.zeros(M), total_weight=np.zeros(M),
               n_unique=np.zeros(M, np.int32), err_idx=np.zeros(M, np.int32), usid=np.full(Nsig, -1, np.int32),
               weight=np.zeros(Nsig), nweight=np.zeros(Nsig), exists=np.zeros(Nsig, np.uint8),
               rel_read=np.zeros(Nsig), conf_read=np.zeros(Nsig))
    for m in range(M):
        a, b = int(offsets[m]), int(offsets[m + 1])
        now = int(market_time_us[m])
        view = orc.decay_view(rel, t_us, present, now)            # absent rows read 0.5
        cview = np.where(present != 0, conf, 0.25)
        seen = np.ones(S, np.uint8) if all_present else present
        one = orc.consensus_csr(np.array([0, b - a], np.int64), sid[a:b], prob[a:b], view, cview, seen)
        for k in ("consensus", "confidence", "total_weight", "n_unique", "err_idx"):
            out[k][m] = one[k][0]
        for k in ("usid", "weight", "nweight"):
            out[k][a:b] = one[k]
        nu = int(one["n_unique"][0])
        src = one["usid"][:nu] & ~COLD
        out["exists"][a:a + nu] = present[src]
        out["rel_read"][a:a + nu] = view[src]
        out["conf_read"][a:a + nu] = cview[src]
        if outcome[m] >= 0:
            ch = chains(np.array([0, b - a], np.int64), sid[a:b], prob[a:b], outcome[m:m + 1], S)
            rel, conf, t_us, present = apply_chains(ch, rel, conf, t_us, present, now)
    return out, (rel, conf, t_us, present)
