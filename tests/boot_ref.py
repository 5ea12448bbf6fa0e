"""Reference for bce_boot_weights_host / bce_score_bootstrap (include/bce.h): numpy,
``math`` and ``decimal`` only.

The weight function is restated in uint64 numpy with the threshold table derived by ``decimal``;
the item rule is the one of tests/score_ref.py (``classify``, ``item_terms``); every fp64 sum is
formed in the documented shape (items left to right inside a segment, then the segments left to
right) and, for checking the shape against an order-free sum, with ``math.fsum`` of the same
products.
"""
from __future__ import annotations

import math
from decimal import Decimal, getcontext

import numpy as np

import score_ref as R

SEG = R.SEG
TILE = 256        # BCE_BOOT_TILE
MAX_SETS = 8      # BCE_BOOT_MAX_SETS
GOLD = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def thresholds():
    """T[k] = min(floor(2^64 * sum_{j <= k} e^-1 / j!), 2^64 - 1), k = 0 .. 20, at 80 digits."""
    getcontext().prec = 80
    e1 = Decimal(-1).exp()
    out, s, f = [], Decimal(0), Decimal(1)
    for k in range(21):
        if k:
            f *= k
        s += e1 / f
        out.append(min(int(s * (1 << 64)), MASK))
    return out


def mix_int(z: int) -> int:
    """The mixer on Python ints (the plainest statement; ``mix`` is checked against it)."""
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def mix(z):
    z = np.asarray(z, np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def hashes(seed: int, reps, units):
    """h(r, u) as uint64 [R, U]; ``units`` are int64 values hashed as their bit patterns."""
    reps = np.asarray(reps, np.int64).astype(np.uint64)
    units = np.asarray(units, np.int64).view(np.uint64)
    with np.errstate(over="ignore"):
        key = mix(np.uint64(seed & MASK) + reps * np.uint64(GOLD))
        hu = mix(units + np.uint64(GOLD))
    return mix(key[:, None] ^ hu[None, :])


def count(h):
    """#{k : h >= T[k]}."""
    h = np.asarray(h, np.uint64)
    w = np.zeros(h.shape, np.int64)
    for t in thresholds():
        w += h >= np.uint64(t)
    return w


def weights(seed: int, reps, units):
    """w(r, u) int64 [R, U]: 1 in replicate 0, the Poisson(1) quantile of h / 2^64 otherwise."""
    reps = np.asarray(reps, np.int64)
    w = count(hashes(seed, reps, units))
    w[reps == 0] = 1
    return w


def poisson_mass(k: int) -> float:
    return math.exp(-1.0) / math.factorial(k)


def _sets(fx, values, valids):
    values = [fx["value"]] if values is None else list(values)
    if valids is None:
        valids = [fx.get("valid")] * len(values)
    elif isinstance(valids, np.ndarray) and valids.ndim == 1:
        valids = [valids] * len(values)
    assert len(valids) == len(values)
    return values, list(valids)


def boot_ref(fx, seed, reps, values=None, valids=None, unit=None, log_terms=None):
    """The reference of bce_score_bootstrap over the items of ``fx`` (a fixture of score_ref).
    ``values`` / ``valids``: one array per forecast set (default: the fixture's own, one set);
    ``unit`` int64[M] or None; ``log_terms[k][i]``: the log-loss term of item i in set k to use
    instead of ``-math.log`` (the device's own terms).  Returns counts int64[R, G, K, 2], sums
    fp64[R, G, K, 3] in the documented shape, and per group the products ``terms`` [R, K, 3, n_g]
    with the integer weights ``w`` [R, n_g] and the masks ``scored`` / ``hit`` [K, n_g]."""
    values, valids = _sets(fx, values, valids)
    K = len(values)
    goff, pidx = fx["goff"], fx["pidx"]
    oidx = fx["oidx"] if fx.get("oidx") is not None else pidx
    outcome, base, eps = fx["outcome"], fx.get("base"), fx["eps"]
    reps = np.asarray(reps, np.int64)
    G, Rn, M = len(goff) - 1, len(reps), len(outcome)
    counts = np.zeros((Rn, G, K, 2), np.int64)
    sums = np.zeros((Rn, G, K, 3), np.float64)
    groups = []
    for g in range(G):
        a, b = int(goff[g]), int(goff[g + 1])
        n = max(b - a, 0)
        term = np.zeros((K, 3, n), np.float64)
        scored = np.zeros((K, n), bool)
        hit = np.zeros((K, n), bool)
        units = np.zeros(n, np.int64)
        for j, i in enumerate(range(a, b)):
            p, m = int(pidx[i]), int(oidx[i])
            if not (0 <= m < M):
                continue
            units[j] = int(unit[m]) if unit is not None else m
            o = int(outcome[m])
            bs = float(base[m]) if base is not None else None
            for k in range(K):
                if not 0 <= p < len(values[k]):
                    continue
                v = float(values[k][p])
                ok = True if valids[k] is None else bool(valids[k][m])
                if R.classify(v, o, ok, bs, base is not None):
                    continue
                br, h, ll, bb, _ = R.item_terms(v, o, bs, 1, eps)
                if log_terms is not None:
                    ll = float(log_terms[k][i])
                scored[k, j], hit[k, j] = True, bool(h)
                term[k, :, j] = (br, ll, bb)
        w = weights(seed, reps, units)  # [R, n]
        with np.errstate(invalid="ignore"):
            prod = w[:, None, None, :].astype(np.float64) * term[None]  # [R, K, 3, n]: the product first
        # an item that is not scored has the terms 0.0: w * 0.0 == 0.0 adds nothing
        total = np.zeros((Rn, K, 3), np.float64)
        for s in range(0, max(n, 1), SEG):
            acc = np.zeros((Rn, K, 3), np.float64)
            for j in range(s, min(s + SEG, n)):
                acc = acc + prod[:, :, :, j]
            total = total + acc
        sums[:, g] = total
        counts[:, g, :, 0] = (w[:, None, :] * scored[None]).sum(-1)
        counts[:, g, :, 1] = (w[:, None, :] * hit[None]).sum(-1)
        groups.append(dict(terms=prod, w=w, scored=scored, hit=hit))
    return dict(counts=counts, sums=sums, groups=groups)


def fsum_sums(ref, rows):
    """``math.fsum`` of the same products for the replicate rows ``rows``: fp64 [len(rows), G, K, 3]."""
    G = len(ref["groups"])
    K = ref["sums"].shape[2]
    out = np.zeros((len(rows), G, K, 3), np.float64)
    for x, r in enumerate(rows):
        for g in range(G):
            t = ref["groups"][g]["terms"][r]
            for k in range(K):
                for c in range(3):
                    col = t[k, c]
                    out[x, g, k, c] = math.fsum(col.tolist()) if np.isfinite(col).all() else col.sum()
    return out


def fx_tile():
    """Groups whose lengths straddle the kernel's tile: TILE - 1, TILE, TILE + 1, 3 * TILE + 1."""
    rng = np.random.default_rng(77)
    M = 400
    outcome, valid = R._markets(rng, M)
    value = rng.random(M)
    lens = (TILE - 1, TILE, TILE + 1, 3 * TILE + 1)
    lists = [rng.integers(0, M, n).astype(np.int64) for n in lens]
    goff = np.zeros(len(lists) + 1, np.int64)
    goff[1:] = np.cumsum(lens)
    return dict(goff=goff, pidx=np.concatenate(lists), oidx=None, value=value, outcome=outcome, valid=valid,
                base=rng.random(M), B=10, eps=1e-15)


def all_fixtures():
    """The fixtures of score_ref plus the tile straddle."""
    return dict(R.all_fixtures(), tile=fx_tile())
