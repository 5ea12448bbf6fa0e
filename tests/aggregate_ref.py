"""Reference for bce_aggregate_groups (include/bce.h): CrossMarketAggregator.aggregate_consensus
(market.py:340-408) restated literally for one member group, Python floats and builtins only.

Members are taken in list order, duplicates kept; a member outside [0, n_markets) or without a
consensus is skipped.  ``sum`` is the builtin (left to right from 0), ``sorted`` is stable and
compares -0.0 == 0.0, so the median is the element itself, sign of a zero included.  With a NaN
among the values ``sorted`` depends on the input order: the median is returned as None there
(unspecified).
"""
from __future__ import annotations

import math

import numpy as np


def aggregate_ref(members, cons, conf, has):
    """One group -> dict(wavg, median, majority, mean_conf, n_included)."""
    n_markets = len(cons)
    cs, fs = [], []
    for m in members:
        m = int(m)
        if not (0 <= m < n_markets) or not has[m]:
            continue
        cs.append(float(cons[m]))
        fs.append(float(conf[m]))
    k = len(cs)
    if k == 0:
        return dict(wavg=math.nan, median=math.nan, majority=math.nan, mean_conf=math.nan, n_included=0)
    tconf = sum(fs)
    tcons = sum(cs)
    tprod = sum(c * f for c, f in zip(cs, fs))
    wavg = tcons / k if tconf == 0 else tprod / tconf
    median = None if any(c != c for c in cs) else sorted(cs)[k // 2]
    majority = sum(1 for c in cs if c >= 0.5) / k
    return dict(wavg=wavg, median=median, majority=majority, mean_conf=tconf / k, n_included=k)


def aggregate_ref_groups(goff, members, cons, conf, has):
    """Every group of a CSR batch: arrays like oracle.aggregate_groups, plus ``median_known``
    (False where the group holds a NaN consensus; its median entry is NaN and not to be compared)."""
    G = len(goff) - 1
    out = dict(wavg=np.zeros(G), median=np.zeros(G), majority=np.zeros(G), mean_conf=np.zeros(G),
               n_included=np.zeros(G, np.int64), median_known=np.ones(G, bool))
    cons_l, conf_l, has_l = np.asarray(cons).tolist(), np.asarray(conf).tolist(), np.asarray(has).tolist()
    mem_l = np.asarray(members).tolist()
    for g in range(G):
        r = aggregate_ref(mem_l[int(goff[g]):int(goff[g + 1])], cons_l, conf_l, has_l)
        for key in ("wavg", "majority", "mean_conf", "n_included"):
            out[key][g] = r[key]
        if r["median"] is None:
            out["median"][g], out["median_known"][g] = math.nan, False
        else:
            out["median"][g] = r["median"]
    return out


def kept_conf(members, conf, has):
    """The conf values of the kept members, in list order."""
    n = len(conf)
    return [float(conf[int(m)]) for m in members if 0 <= int(m) < n and has[int(m)]]


def order_sensitive(members, conf, has):
    """sum(conf) over the kept members differs between the list and its reverse."""
    fs = kept_conf(members, conf, has)
    return sum(fs) != sum(reversed(fs))


def same_bits(a, b):
    """Bit-for-bit equality of two float64 arrays, every NaN counted as one value."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    an, bn = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(an, bn) and np.array_equal(a[~an].view(np.uint64), b[~bn].view(np.uint64)))
