"""Expected values of batch settlement: the CPU oracle's ``outcome_update`` (one outcome per
source per call) composed one chain step at a time (test infrastructure only).

A source's chain is its signals in markets with ``outcome >= 0``, in CSR order (market
ascending, then position): the order the reference's per-signal loop calls
``update_reliability`` in.  Step ``k`` flags every source whose chain has a ``k``-th bit, the bit
being ``(probability >= 0.5) == outcome`` (market.py:298-301)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import oracle as orc


class Chains(NamedTuple):
    bits: np.ndarray     # uint8[n_part], the correctness bits grouped by source, chain order inside
    start: np.ndarray    # int64[S + 1]
    total: np.ndarray    # int64[S] chain length
    correct: np.ndarray  # int64[S] set bits


def chains(offsets, sid, prob, outcome, n_sources) -> Chains:
    offsets = np.ascontiguousarray(offsets, np.int64)
    sid = np.clip(np.ascontiguousarray(sid, np.int64), 0, int(n_sources) - 1)  # as the builder clamps
    prob = np.ascontiguousarray(prob, np.float64)
    outcome = np.ascontiguousarray(outcome, np.int8)
    market = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    idx = np.flatnonzero(outcome[market] >= 0)
    with np.errstate(invalid="ignore"):
        bit = ((prob[idx] >= 0.5) == (outcome[market[idx]] != 0)).astype(np.uint8)  # NaN >= 0.5 is False
    order = np.argsort(sid[idx], kind="stable")
    total = np.bincount(sid[idx], minlength=n_sources).astype(np.int64)
    start = np.zeros(n_sources + 1, np.int64)
    start[1:] = np.cumsum(total)
    bits = bit[order]
    correct = np.bincount(sid[idx][order], weights=bits, minlength=n_sources).astype(np.int64)
    return Chains(bits, start, total, correct)


def apply_chains(ch: Chains, rel, conf, t_us, present, now_us):
    """(rel, conf, t_us, present) after every chain, by orc.outcome_update step after step."""
    rel, conf = np.array(rel, np.float64), np.array(conf, np.float64)
    t_us, present = np.array(t_us, np.int64), np.array(present, np.uint8)
    S = len(ch.total)
    for k in range(int(ch.total.max(initial=0))):
        live = np.flatnonzero(ch.total > k)
        flags = np.zeros(S, np.uint8)
        flags[live] = 1 | (ch.bits[ch.start[live] + k] << 1)
        rel, conf, t_us, present = orc.outcome_update(rel, conf, t_us, present, flags, now_us)
    return rel, conf, t_us, present


def fixture_scope(g, scope):
    """The golden fixture's start table of one scope ("domain" / "global") over its rank space,
    (rel, conf, present), and the expected (rel, conf, present) from the reference's final rows."""
    S = g["n_sources"]
    rel, conf, present = np.full(S, 0.5), np.full(S, 0.25), np.zeros(S, np.uint8)
    for seed in g["seeds"]:
        if seed["scope"] == scope:
            s = seed["source"]
            rel[s], conf[s], present[s] = float(seed["reliability"]), float(seed["confidence"]), 1
    erel, econf, epresent = np.full(S, 0.5), np.full(S, 0.25), np.zeros(S, np.uint8)
    for name, (r, c) in g["final"][scope].items():
        s = g["names"].index(name)
        erel[s], econf[s], epresent[s] = float(r), float(c), 1
    return (rel, conf, present), (erel, econf, epresent)


def settle_ref(offsets, sid, prob, outcome, n_sources, rel, conf, t_us, present, now_us):
    """Returns (rel, conf, t_us, present, total, correct)."""
    ch = chains(offsets, sid, prob, outcome, n_sources)
    return (*apply_chains(ch, rel, conf, t_us, present, now_us), ch.total, ch.correct)
