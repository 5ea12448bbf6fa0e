"""The decay arithmetic in plain Python (reference decay.py:52-58, 90-100, 140-145), and the
decay_edges.json fixture as numpy arrays.  Test infrastructure only.

Days come from exact integers (CPython's int / int is rounded once), the factor is
``2.0 ** x`` (CPython float_pow: libm pow) and the clamps are the builtin min / max.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from golden_util import load_json

NO_TIMESTAMP = -(2**63)


def days(t_us: int, now_us: int) -> float:
    if t_us == NO_TIMESTAMP:
        return 0.0
    return max(0.0, (int(now_us) - int(t_us)) / 10**6 / 86400.0)


def factor(e: float, h: float) -> float:
    return 1.0 if e <= 0 else 2.0 ** (-e / h)


def apply(r: float, e: float, h: float, m: float) -> float:
    if e <= 0:
        return r
    return max(m, min(1.0, m + (r - m) * factor(e, h)))


def view(r: float, t_us: int, now_us: int, h: float, m: float) -> float:
    return apply(r, days(t_us, now_us), h, m)


# ---------------------------------------------------------------------------------------
# fixture access: doubles travel as 64-bit patterns, comparisons are on the patterns
# ---------------------------------------------------------------------------------------
def unpack(col) -> list:
    """A column of decay_edges.json (gen_decay_edges.py pack()) as a list of hex strings / ints."""
    if isinstance(col, dict):
        w, ix = col["width"], col["index"]
        return [col["values"][int(ix[i:i + w], 36)] for i in range(0, len(ix), w)]
    if isinstance(col, str):
        return [col[i:i + 16] for i in range(0, len(col), 16)]
    return col


def unhex(col) -> np.ndarray:
    return np.array([int(x, 16) for x in unpack(col)], np.uint64).view(np.float64)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_bits(got, exp, what="") -> None:
    g, e = bits(got), bits(exp)
    bad = np.flatnonzero(g != e)
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} differ; first at {bad[0]}: "
                           f"got {g[bad[0]]:016x} expected {e[bad[0]]:016x}")


@functools.lru_cache(maxsize=None)
def edges() -> SimpleNamespace:
    """days: r, e, h, m, factor, out (float64 arrays); stamps: r, h, m, days, out (float64) and
    t_us, now_us (int64); ratios (float64).  Read-only."""
    d = load_json("decay_edges.json")
    dd = SimpleNamespace(**{k: np.concatenate([unhex(b[k]) for b in d["days"]]) for k in d["days"][0]})
    ss = SimpleNamespace(**{k: np.array(unpack(c), np.int64) if k in ("t_us", "now_us") else unhex(c)
                            for k, c in d["stamps"].items()})
    for ns in (dd, ss):
        for a in vars(ns).values():
            a.setflags(write=False)
    return SimpleNamespace(days=dd, stamps=ss, ratios=unhex(d["ratios"]),
                           single_rounding_rows=int(d["stamps_single_rounding_rows"]))


def groups(*keys) -> list:
    """Row indices grouped by equal key bits (each key a float64 or int64 column), in first-seen
    order: [(tuple of python scalars, index array), ...]."""
    cols = [np.ascontiguousarray(k).view(np.uint64) for k in keys]
    seen = {}
    for i, kb in enumerate(zip(*cols)):
        seen.setdefault(kb, []).append(i)
    out = []
    for idx in seen.values():
        out.append((tuple(k[idx[0]].item() for k in keys), np.array(idx, np.int64)))
    return out


def poisoned_scopes(r: np.ndarray, t_us: np.ndarray, win=None, seed: int = 7) -> list:
    """Three scopes (market, domain, global) as (rel, conf, t_us, has): row i is stored in scope
    win[i] (default i % 3).  The scopes before it have has = 0 over poison (NaN reliability, an
    arbitrary stamp); the scopes after it hold a live decoy row that a correct lookup never
    reaches."""
    rng = np.random.default_rng(seed)
    n = len(r)
    win = np.arange(n) % 3 if win is None else np.asarray(win)
    out = []
    for q in range(3):
        rel = np.where(win == q, r, np.where(win > q, np.nan, 0.77))
        t = np.where(win == q, t_us, np.where(win > q, rng.integers(-2**62, 2**62, n), t_us - 86400 * 10**6))
        conf = np.where(win == q, 0.25 + 0.5 * rng.random(n), np.where(win > q, np.nan, 0.11))
        has = (win <= q).astype(np.uint8)
        out.append((rel.astype(np.float64), conf.astype(np.float64), t.astype(np.int64), has))
    return out
