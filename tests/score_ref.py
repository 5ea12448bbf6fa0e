"""Reference for bce_score_groups (include/bce.h): numpy and ``math`` only.

``score_ref`` applies the item rule as the header states it and sums every fp64 column twice:
in the documented reduction shape (``shaped_sum``: lane-strided partials, halving tree, segments
left to right -- what the kernel must reproduce to the bit) and with ``math.fsum`` (the exactly
rounded sum, independent of any order).  The fixtures of the GPU tests are built here, so the
host test can check the shaped reference against ``math.fsum`` on every one of them.
"""
from __future__ import annotations

import math

import numpy as np

SEG = 2048    # BCE_SCORE_SEG
LANES = 256   # BCE_SCORE_LANES
COUNTS = ("n_scored", "n_hit", "n_unresolved", "n_null", "n_bad")


def segment_sum(x) -> float:
    """One segment (<= SEG terms): lane l adds terms l, l + LANES, ... from 0.0, then the tree."""
    x = np.asarray(x, np.float64)
    assert x.size <= SEG
    pad = np.zeros(SEG, np.float64)
    pad[:x.size] = x  # a missing item is the term 0.0: x + 0.0 == x for non-negative x
    rows = pad.reshape(SEG // LANES, LANES)
    p = np.zeros(LANES, np.float64)
    for k in range(rows.shape[0]):
        p = p + rows[k]
    o = LANES // 2
    while o >= 1:
        p[:o] = p[:o] + p[o:2 * o]
        o //= 2
    return float(p[0])


def shaped_sum(terms) -> float:
    """The documented shape over a group's terms (0.0 for an item that is not scored)."""
    terms = np.asarray(terms, np.float64)
    total = 0.0
    for s in range(0, max(terms.size, 1), SEG):
        total = total + segment_sum(terms[s:s + SEG])
    return total


def sum_bound(terms) -> float:
    """|any summation order - exact sum| <= (n - 1) * 2^-53 * sum|terms| (to first order; the
    standard bound, Higham 4.4 with gamma_(n-1) ~ (n - 1) u)."""
    terms = np.asarray(terms, np.float64)
    n = terms.size
    return max(n - 1, 0) * 2.0 ** -53 * math.fsum(abs(float(t)) for t in terms) * (1 + 1e-9)


def item_terms(v, o, base, B, eps, log=math.log):
    """A scored item: (brier, hit, logloss, brier_base, bin)."""
    d = v - o
    q = v if o else 1.0 - v
    ll = -log(max(q, eps)) if max(q, eps) > 0.0 else math.inf
    db = (base - o) if base is not None else 0.0
    return d * d, (v >= 0.5) == (o == 1), ll, db * db, min(int(v * B), B - 1)


def classify(v, o, valid, base, has_base):
    """0 scored, 2 unresolved, 3 null, 4 bad: the header's order."""
    if o < 0:
        return 2
    if not valid:
        return 3
    if not (0.0 <= v <= 1.0) or (has_base and not (0.0 <= base <= 1.0)):
        return 4
    return 0


def score_ref(fx, log=math.log):
    """Per group: counts [G, 5], bin_n / bin_pos [G, B], and for the fp64 columns both the shaped
    sums (``sums`` [G, 3], ``bin_psum`` [G, B]) and ``terms`` (the per-item term arrays, 0.0 where
    not scored: [G] lists of arrays [3 + B, n_g])."""
    goff, pidx = fx["goff"], fx["pidx"]
    oidx = fx["oidx"] if fx.get("oidx") is not None else pidx
    value, outcome, valid, base = fx["value"], fx["outcome"], fx.get("valid"), fx.get("base")
    B, eps = fx["B"], fx["eps"]
    G = len(goff) - 1
    counts = np.zeros((G, 5), np.int64)
    bin_n = np.zeros((G, B), np.int64)
    bin_pos = np.zeros((G, B), np.int64)
    sums = np.zeros((G, 3), np.float64)
    bin_psum = np.zeros((G, B), np.float64)
    terms = []
    for g in range(G):
        a, b = int(goff[g]), int(goff[g + 1])
        t = np.zeros((3 + B, max(b - a, 0)), np.float64)
        for k, i in enumerate(range(a, b)):
            p, m = int(pidx[i]), int(oidx[i])
            if not (0 <= p < len(value) and 0 <= m < len(outcome)):
                counts[g, 4] += 1
                continue
            v, o = float(value[p]), int(outcome[m])
            bs = float(base[m]) if base is not None else None
            c = classify(v, o, True if valid is None else bool(valid[m]), bs, base is not None)
            counts[g, c] += 1
            if c:
                continue
            br, hit, ll, bb, bn = item_terms(v, o, bs, B, eps, log)
            counts[g, 1] += int(hit)
            bin_n[g, bn] += 1
            bin_pos[g, bn] += int(o == 1)
            t[0, k], t[1, k], t[2, k], t[3 + bn, k] = br, ll, bb, v
        terms.append(t)
        for c in range(3):
            sums[g, c] = shaped_sum(t[c])
        for bn in range(B):
            bin_psum[g, bn] = shaped_sum(t[3 + bn])
    return dict(counts=counts, sums=sums, bin_n=bin_n, bin_pos=bin_pos, bin_psum=bin_psum, terms=terms)


def derived(counts, sums, bin_n, bin_pos, bin_psum):
    """brier, log_loss, accuracy, brier_base, ece per group with plain Python floats."""
    out = []
    for g in range(counts.shape[0]):
        n = int(counts[g, 0])
        if n == 0:
            out.append(dict(n=0, brier=math.nan, log_loss=math.nan, accuracy=math.nan, brier_base=math.nan,
                            ece=math.nan))
            continue
        ece = 0.0
        for b in range(bin_n.shape[1]):
            k = int(bin_n[g, b])
            if k:
                ece += abs(float(bin_psum[g, b]) / k - int(bin_pos[g, b]) / k) * k
        out.append(dict(n=n, brier=float(sums[g, 0]) / n, log_loss=float(sums[g, 1]) / n,
                        accuracy=int(counts[g, 1]) / n, brier_base=float(sums[g, 2]) / n, ece=ece / n))
    return out


# ---- fixtures shared by tests/test_score_host.py and tests/test_gpu_score.py ----------------------
LENGTHS = (0, 1, 63, 64, 65, SEG - 1, SEG, SEG + 1, 2 * SEG + 3)


def _markets(rng, M, p_unresolved=0.15, p_null=0.1):
    outcome = rng.choice(np.array([-1, 0, 1], np.int8), M, p=[p_unresolved, (1 - p_unresolved) / 2,
                                                              (1 - p_unresolved) / 2])
    valid = (rng.random(M) >= p_null).astype(np.uint8)
    return outcome, valid


def fx_lengths(reverse=False):
    """Every group length around the lane stride and the segment size, in one call."""
    rng = np.random.default_rng(11)
    M = 500
    outcome, valid = _markets(rng, M)
    value = rng.random(M)
    lists = [rng.integers(0, M, n).astype(np.int64) for n in LENGTHS]
    if reverse:
        lists = lists[::-1]
    goff = np.zeros(len(lists) + 1, np.int64)
    goff[1:] = np.cumsum([len(x) for x in lists])
    return dict(goff=goff, pidx=np.concatenate(lists), oidx=None, value=value, outcome=outcome, valid=valid,
                base=None, B=10, eps=1e-15)


def fx_overlap():
    """A duplicated member, and two groups that overlap."""
    value = np.array([0.1, 0.7, 0.35, 0.9, 0.5, 0.2])
    outcome = np.array([0, 1, 1, 1, 0, -1], np.int8)
    pidx = np.array([0, 1, 1, 2, 3, 2, 3, 4, 5, 0], np.int64)
    return dict(goff=np.array([0, 5, 10], np.int64), pidx=pidx, oidx=None, value=value, outcome=outcome,
                valid=None, base=None, B=10, eps=1e-15)


def fx_classes():
    """One item of every class: unresolved, null, NaN, below 0, above 1, a bad base, scored."""
    value = np.array([0.3, 0.4, math.nan, -0.1, 1.0000000000000002, 0.6, 0.8, 0.25])
    outcome = np.array([-1, 1, 1, 0, 1, 0, 1, 0], np.int8)
    valid = np.array([1, 0, 1, 1, 1, 1, 1, 1], np.uint8)
    base = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 1.5, 0.5, math.nan])
    goff = np.array([0, 8], np.int64)
    with_base = dict(goff=goff, pidx=np.arange(8, dtype=np.int64), oidx=None, value=value, outcome=outcome,
                     valid=valid, base=base, B=10, eps=1e-15)
    return with_base, dict(with_base, base=None)


def fx_edges(B=8, eps=1e-15):
    """0, 0.5, 1 and every k / 8 with both outcomes: the hit rule at 0.5, the last bin, the clip."""
    vals = sorted({0.0, 0.5, 1.0} | {k / 8 for k in range(9)})
    value = np.array(vals + vals)
    outcome = np.array([0] * len(vals) + [1] * len(vals), np.int8)
    n = len(value)
    return dict(goff=np.array([0, n], np.int64), pidx=np.arange(n, dtype=np.int64), oidx=None, value=value,
                outcome=outcome, valid=None, base=None, B=B, eps=eps)


def fx_random(B, n=700, seed=5):
    """Random forecasts in two groups of more than one lane stride."""
    rng = np.random.default_rng(seed + B)
    M = 300
    outcome, valid = _markets(rng, M)
    value = rng.random(M)
    value[:3] = (0.0, 1.0, 0.5)
    pidx = rng.integers(0, M, n).astype(np.int64)
    return dict(goff=np.array([0, n // 3, n], np.int64), pidx=pidx, oidx=None, value=value, outcome=outcome,
                valid=valid, base=rng.random(M), B=B, eps=1e-15)


def per_item(fx):
    """The same items, one group each: the group sums are the per-item terms."""
    n = len(fx["pidx"])
    return dict(fx, goff=np.arange(n + 1, dtype=np.int64))


def fx_sources():
    """A ragged CSR batch: 300 markets, 40 sources, duplicate signals per source and market, a
    Zipf head longer than a segment.  Returns (offsets, sid, prob, outcome, consensus, valid)."""
    rng = np.random.default_rng(23)
    M, S = 300, 40
    w = 1.0 / np.arange(1, S + 1) ** 1.3
    lens = rng.integers(0, 60, M)
    lens[7] = 0
    offsets = np.zeros(M + 1, np.int64)
    offsets[1:] = np.cumsum(lens)
    n = int(offsets[-1])
    sid = rng.choice(S, n, p=w / w.sum()).astype(np.int32)
    sid[sid == 31] = 30  # source 31 has no signal
    prob = rng.random(n)
    prob[::97] = 0.5
    outcome, valid = _markets(rng, M)
    consensus = rng.random(M)
    assert np.bincount(sid, minlength=S).max() > SEG
    return offsets, sid, prob, outcome, consensus, valid


def by_source_ref(offsets, sid, n_sources):
    """dict-of-lists grouping: (goff, pidx, oidx, n_clamped), sids clamped into [0, n_sources)."""
    lists = {s: [] for s in range(n_sources)}
    clamped = 0
    for m in range(len(offsets) - 1):
        for i in range(int(offsets[m]), int(offsets[m + 1])):
            s = min(max(int(sid[i]), 0), n_sources - 1)
            clamped += s != int(sid[i])
            lists[s].append((i, m))
    goff = np.zeros(n_sources + 1, np.int64)
    goff[1:] = np.cumsum([len(lists[s]) for s in range(n_sources)])
    flat = [x for s in range(n_sources) for x in lists[s]]
    return (goff, np.array([x[0] for x in flat], np.int64), np.array([x[1] for x in flat], np.int64), clamped)


def fx_sources_items():
    offsets, sid, prob, outcome, consensus, valid = fx_sources()
    goff, pidx, oidx, _ = by_source_ref(offsets, sid, 40)
    return dict(goff=goff, pidx=pidx, oidx=oidx, value=prob, outcome=outcome, valid=valid, base=consensus, B=10,
                eps=1e-15)


def all_fixtures():
    """Every item fixture the GPU tests score, by name."""
    cb, cn = fx_classes()
    return {"lengths": fx_lengths(), "lengths_reversed": fx_lengths(True), "overlap": fx_overlap(),
            "classes_base": cb, "classes": cn, "edges8": fx_edges(8), "edges8_eps0": fx_edges(8, 0.0),
            "random1": fx_random(1), "random10": fx_random(10), "random32": fx_random(32),
            "sources": fx_sources_items()}
