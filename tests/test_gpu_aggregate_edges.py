"""bce_aggregate_groups at its edges: one small group per branch of aggregate_kernel
(csrc/aggregate.hip), bit for bit against the CPU oracle and against tests/aggregate_ref.py (the
reference's aggregate_consensus restated with Python floats, ``sum`` and ``sorted``).

``build_batch`` makes every group of the file in one CSR batch over M = 4000 markets; the host
test (tests/test_aggregate_host.py) imports it and pins the oracle to aggregate_ref on the same
groups.  The market space is split so that the ``has`` byte can be chosen per group:

  [0, 1000)      has = 1            random values
  [1000, 2000)   has = 0 / 1 / 2 / 255, about half zero
  [2000, 2400)   has = 1            the valid members of the hand-set groups
  [2400, 2800)   has = 0            their skipped members
  [2800, 4000)   has = 1            values set one market at a time (bit patterns, zeros, ...)

Values: cons = normal * 10 ** integers(-12, 13) with pinned 0.5, nextafter(0.5, 0), +-0.0 and
+-5e-324; conf = normal * 10 ** integers(-8, 9) with 30 % exact zeros, so that the sums depend on
the order of the members (asserted on the reference alone in tests/test_aggregate_host.py).
Chunk = 1024 members; groups of up to one chunk take the median from LDS, longer ones re-read
their members.
"""
import functools
import math

import numpy as np
import pytest

from aggregate_ref import aggregate_ref_groups, same_bits
from oracle import oracle as orc

M = 4000
CHUNK = 1024  # kAggCh
LENGTHS = (0, 1, 2, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 5000)
ONES, HALF, C1, C0, CUSTOM = (0, 1000), (1000, 2000), (2000, 2400), (2400, 2800), (2800, 4000)
OUTS = ("wavg", "median", "majority", "mean_conf")
SIGNED_ZERO_LISTS = ([0.0, -0.0], [-0.0, 0.0], [-0.0], [-1.0, -0.0, 0.0], [-1.0, 0.0, -0.0],
                     [0.0, -0.0, -0.0, 0.0, 1.0])
BYTE_BASE = 0x3FE5555555555555  # 0.666..., bit 8 b + 3 flipped: two finite patterns per byte b


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        rng = self.rng
        self.cons = rng.standard_normal(M) * 10.0 ** rng.integers(-12, 13, M)
        pins = (0.5, np.nextafter(0.5, 0.0), 0.0, -0.0, 5e-324, -5e-324)
        edges = np.cumsum((0.0, 0.04, 0.04, 0.02, 0.02, 0.01, 0.01))  # the pinned fractions
        u = rng.random(M)
        for i, p in enumerate(pins):
            self.cons[(u >= edges[i]) & (u < edges[i + 1])] = p
        self.conf = rng.standard_normal(M) * 10.0 ** rng.integers(-8, 9, M)
        self.conf[rng.random(M) < 0.3] = 0.0
        self.has = np.ones(M, np.uint8)
        self.has[HALF[0]:HALF[1]] = rng.choice(np.array([0, 0, 0, 1, 2, 255], np.uint8), HALF[1] - HALF[0])
        self.has[C0[0]:C0[1]] = 0
        self.next_custom = CUSTOM[0]
        self.groups, self.names, self.median_only = [], [], []

    def market(self, value, conf=None):
        """A market of its own holding ``value`` (has = 1, a random confidence unless given)."""
        m = self.next_custom
        assert m < CUSTOM[1], "custom market space used up"
        self.next_custom += 1
        self.cons[m] = value
        if conf is not None:
            self.conf[m] = conf
        return m

    def markets(self, value, n, conf=None):
        return [self.market(value, conf) for _ in range(n)]

    def add(self, name, members, median_only=False):
        self.names.append(name)
        self.groups.append(np.asarray(members, np.int64).reshape(-1))
        self.median_only.append(median_only)

    def draw(self, region, n):
        return self.rng.integers(region[0], region[1], n)

    def pick(self, pool, n):
        return self.rng.choice(np.asarray(pool, np.int64), n)

    def padded(self, members, n):
        """``members`` kept in order inside a list of n, the rest skipped markets."""
        out = self.draw(C0, n)
        at = np.sort(self.rng.choice(n, len(members), replace=False))
        out[at] = members
        return out

    def finish(self):
        goff = np.zeros(len(self.groups) + 1, np.int64)
        goff[1:] = np.cumsum([len(g) for g in self.groups])
        members = np.concatenate(self.groups + [np.zeros(1, np.int64)])  # never empty
        return dict(goff=goff, members=members, cons=self.cons, conf=self.conf, has=self.has,
                    names=list(self.names), median_only=np.array(self.median_only, bool))


def _lengths(B):
    """Every length with has all ones (cnt == length: the chain sees exactly 1024 terms and the
    16-term loop reads its pad), about half, and hand-set: the last chunk without a valid member
    while k > 0, the first chunk without one, only the two ends valid."""
    for n in LENGTHS:
        B.add(f"len{n}-ones", B.draw(ONES, n))
        B.add(f"len{n}-half", B.draw(HALF, n))
        if n > CHUNK:
            last = (n - 1) // CHUNK * CHUNK
            mem = np.where(B.rng.random(n) < 0.7, B.draw(C1, n), B.draw(C0, n))
            mem[last:] = B.draw(C0, n - last)
            B.add(f"len{n}-last-chunk-empty", mem)
            mem = np.where(B.rng.random(n) < 0.7, B.draw(C1, n), B.draw(C0, n))
            mem[:CHUNK] = B.draw(C0, CHUNK)
            mem[CHUNK:] = B.draw(C1, n - CHUNK)  # cnt == length of every later chunk
            B.add(f"len{n}-first-chunk-empty", mem)
        else:
            mem = B.draw(C0, n)
            if n:
                mem[0], mem[-1] = B.draw(C1, 1)[0], B.draw(C1, 1)[0]
            B.add(f"len{n}-ends-only", mem)


def _radix(B):
    """The radix select through both median paths: all values equal; per key byte two bit
    patterns that differ in that byte only, the rank on either side of the split, k even and odd
    and k in {1, 2, 3}; all-negative and sign-mixed groups."""
    same = B.markets(0.3, 4)
    for n in (700, 1500):
        B.add(f"equal-{n}", B.pick(same, n))
    for b in range(8):
        base = BYTE_BASE | (0x8000000000000000 if b & 1 and b != 7 else 0)  # odd bytes on negatives
        pats = np.array([base, base ^ (1 << (8 * b + 3))], np.uint64).view(np.float64)
        lo, hi = (0, 1) if pats[0] < pats[1] else (1, 0)
        pool_lo, pool_hi = B.markets(pats[lo], 4), B.markets(pats[hi], 4)

        def mix(n_lo, n_hi):
            mem = np.concatenate([B.pick(pool_lo, n_lo), B.pick(pool_hi, n_hi)])
            B.rng.shuffle(mem)
            return mem

        for k in (1, 2, 3):
            for n_lo in range(k + 1):
                mem = mix(n_lo, k - n_lo)
                B.add(f"byte{b}-k{k}-lo{n_lo}-lds", mem)
                B.add(f"byte{b}-k{k}-lo{n_lo}-reread", B.padded(mem, CHUNK + 6))
        for k in (700, 701, 1500, 1501):
            for n_lo in (k // 2, k // 2 + 1):  # sorted()[k // 2] is the first high / the last low value
                B.add(f"byte{b}-k{k}-lo{n_lo}", mix(n_lo, k - n_lo))
    neg = [B.market(-abs(v)) for v in B.rng.standard_normal(60) * 10.0 ** B.rng.integers(-12, 13, 60)]
    neg += [B.market(-5e-324), B.market(-0.5), B.market(-2.2250738585072014e-308)]
    for n in (3, 700, 701, 1500):
        B.add(f"negative-{n}", B.pick(neg, n))
    for n in (700, 1501):
        B.add(f"sign-mixed-{n}", np.concatenate([B.pick(neg, n // 2), B.draw(ONES, n - n // 2)]))


def _zeros(B):
    """sorted() is stable and 0.0 == -0.0: the median is the zero at its list position."""
    key = lambda v: (v, math.copysign(1.0, v))  # noqa: E731  (0.0 and -0.0 are one dict key)
    val = {key(v): B.markets(v, 3) for v in (0.0, -0.0, -1.0, 1.0)}
    for i, lst in enumerate(SIGNED_ZERO_LISTS):
        mem = [val[key(v)][j % 3] for j, v in enumerate(lst)]
        B.add(f"zero-list{i}", mem)
        B.add(f"zero-list{i}-reread", B.padded(mem, CHUNK + 1))
    zeros = val[key(0.0)] + val[key(-0.0)]
    for n, n_neg in ((900, 4), (1500, 5), (5000, 7), (1501, 700), (1500, 751)):
        mem = B.pick(zeros, n)
        mem[B.rng.choice(n, n_neg, replace=False)] = B.pick(val[key(-1.0)], n_neg)
        B.add(f"zero-random-sign-{n}-neg{n_neg}", mem)
    # the zeros start after the first 256-member stripe and the wanted one lies in a later wave
    mem = np.concatenate([B.pick(val[key(-1.0)], 300), B.pick(zeros, 500), B.pick(val[key(1.0)], 100)])
    B.add("zero-after-stripe-lds", mem)
    B.add("zero-after-stripe-reread", B.padded(mem, 2 * CHUNK + 5))


def _duplicates_and_range(B):
    B.add("one-market-1025-times", np.full(1025, 17))
    B.add("every-market-twice", np.concatenate([np.arange(M), np.arange(M)]))
    for name, n in (("one-chunk", 600), ("three-chunk", 2500)):
        mem = np.concatenate([B.draw(ONES, n // 2), B.draw(HALF, n - n // 2)])
        B.rng.shuffle(mem)
        at = B.rng.choice(n, n // 5, replace=False)
        mem[at] = B.rng.choice(np.array([-1, M, 2 ** 40], np.int64), len(at))
        mem[0], mem[-1], mem[n // 2] = M, -1, 2 ** 40
        B.add(f"out-of-range-{name}", mem)


def _nonfinite(B):
    """+-inf and +-5e-324 (median and n_included only: the sums are not finite), and groups
    holding a NaN consensus (the median is unspecified there, everything else is compared)."""
    sp = {v: B.market(v, conf=1.0) for v in (math.inf, -math.inf, 5e-324, -5e-324, 1.0, -1.0)}
    z = [B.market(0.0, conf=1.0), B.market(-0.0, conf=1.0)]
    pool = list(sp.values()) + z
    for i, lst in enumerate(([math.inf], [-math.inf], [-math.inf, math.inf], [math.inf, -math.inf, -math.inf],
                             [5e-324, -5e-324], [-5e-324, 5e-324, -5e-324], [-math.inf, 5e-324, math.inf],
                             [math.inf] * 5 + [1.0] * 4, [-math.inf] * 5 + [-1.0] * 4)):
        B.add(f"inf-list{i}", [sp[v] for v in lst], median_only=True)
        B.add(f"inf-list{i}-reread", B.padded([sp[v] for v in lst], CHUNK + 3), median_only=True)
    for n in (9, 700, 1500):
        B.add(f"inf-random-{n}", B.pick(pool, n), median_only=True)
    den = [sp[5e-324], sp[-5e-324]] + z
    for n in (4, 701, 1500):
        B.add(f"denormal-random-{n}", B.pick(den, n))
    nan = [B.market(math.nan), B.market(-math.nan), B.market(math.nan, conf=0.0)]
    for n in (1, 2, 600, 2500):
        mem = B.draw(ONES, n)
        mem[B.rng.choice(n, max(n // 100, 1), replace=False)] = B.pick(nan, max(n // 100, 1))
        B.add(f"nan-{n}", mem)


@functools.lru_cache(maxsize=None)
def build_batch(nonfinite=False):
    """The file's groups as one CSR batch: dict(goff, members, cons, conf, has, names,
    median_only).  ``nonfinite`` = the batch of the +-inf / denormal / NaN groups instead (its
    cons holds inf and NaN, which the every-market group of the main batch must not see)."""
    B = _Builder(2024 + nonfinite)
    if nonfinite:
        _nonfinite(B)
    else:
        _lengths(B)
        _radix(B)
        _zeros(B)
        _duplicates_and_range(B)
    return B.finish()


@functools.lru_cache(maxsize=None)
def reference(nonfinite=False):
    """(aggregate_ref, oracle) over build_batch(nonfinite); computed once, not to be modified."""
    fx = build_batch(nonfinite)
    args = (fx["goff"], fx["members"], fx["cons"], fx["conf"], fx["has"])
    return aggregate_ref_groups(*args), orc.aggregate_groups(*args)


def check_against(got, exp, fx, sel, what, median_known=None):
    """got / exp: dicts of arrays over the batch's groups; sel: group indices to compare."""
    sel = np.asarray(sel, np.int64)
    assert len(sel)
    assert np.array_equal(np.asarray(got["n_included"])[sel], exp["n_included"][sel]), (what, "n_included")
    full = sel[~fx["median_only"][sel]]
    for key in OUTS:
        idx = sel if key == "median" else full
        if key == "median" and median_known is not None:
            idx = idx[median_known[idx]]
        g, e = np.asarray(got[key])[idx], exp[key][idx]
        if not same_bits(g, e):
            bad = [i for i, (x, y) in zip(idx, zip(g, e)) if not same_bits([x], [y])]
            raise AssertionError(f"{what}: {key} differs in {[(fx['names'][i], float(got[key][i]), float(exp[key][i])) for i in bad[:8]]}")


def _groups(fx, *prefixes):
    return [i for i, n in enumerate(fx["names"]) if n.startswith(prefixes)]


def _dev():
    import torch

    return torch.device("cuda", 0)


def _T(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@functools.lru_cache(maxsize=None)
def _gpu(nonfinite=False):
    """batch.aggregate over build_batch(nonfinite), once."""
    import torch

    from bayesian_engine import batch

    fx = build_batch(nonfinite)
    r = batch.aggregate(_T(fx["goff"]), _T(fx["members"]), _T(fx["cons"]), _T(fx["conf"]), _T(fx["has"]))
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in OUTS + ("n_included",)}


def _check(prefixes, nonfinite=False):
    fx = build_batch(nonfinite)
    ref, oracle = reference(nonfinite)
    sel = _groups(fx, *prefixes)
    got = _gpu(nonfinite)
    check_against(got, ref, fx, sel, "kernel vs aggregate_ref", ref["median_known"])
    check_against(got, oracle, fx, sel, "kernel vs oracle", ref["median_known"])
    return fx, ref, sel


pytestmark = pytest.mark.gpu


def test_lengths_and_has_settings():
    fx, ref, sel = _check(("len",))
    k = {fx["names"][g]: int(ref["n_included"][g]) for g in sel}
    assert all(k[f"len{n}-ones"] == n for n in LENGTHS)  # cnt == length: full chunks of 1024 terms
    assert all(0 < k[f"len{n}-half"] < n for n in LENGTHS if n > 16)
    assert all(k[f"len{n}-last-chunk-empty"] > 0 and k[f"len{n}-first-chunk-empty"] == n - CHUNK
               for n in LENGTHS if n > CHUNK)
    assert all(k[f"len{n}-ends-only"] == min(n, 2) for n in LENGTHS if n <= CHUNK)


def test_radix_select_every_key_byte_both_median_paths():
    fx, ref, sel = _check(("equal-", "byte", "negative-", "sign-mixed-"))
    # the fixture does what it says: per byte, medians on both sides of the split
    for b in range(8):
        med = {ref["median"][g] for g in sel if fx["names"][g].startswith(f"byte{b}-")}
        assert len(med) == 2, (b, med)


def test_signed_zero_median_is_the_element_sorted_returns():
    fx, ref, sel = _check(("zero-",))
    for i, lst in enumerate(SIGNED_ZERO_LISTS):
        exp = sorted(lst)[len(lst) // 2]
        for g in _groups(fx, f"zero-list{i}"):
            assert same_bits([ref["median"][g]], [exp]), (lst, ref["median"][g])
    signs = {bool(np.signbit(ref["median"][g])) for g in sel if ref["median"][g] == 0}
    assert signs == {False, True}


def test_duplicates_and_members_out_of_range():
    fx, ref, sel = _check(("one-market-", "every-market-", "out-of-range-"))
    k = {fx["names"][g]: int(ref["n_included"][g]) for g in sel}
    assert k["one-market-1025-times"] == 1025 and k["every-market-twice"] == 2 * int((fx["has"] != 0).sum())
    assert 0 < k["out-of-range-one-chunk"] < 480 and 0 < k["out-of-range-three-chunk"] < 2000


def test_infinities_and_denormals():
    fx, ref, sel = _check(("inf-", "denormal-"), nonfinite=True)
    med = {float(ref["median"][g]) for g in sel}
    assert {math.inf, -math.inf, 5e-324, -5e-324} <= med


def test_nan_consensus_leaves_the_other_outputs_defined():
    fx, ref, sel = _check(("nan-",), nonfinite=True)
    assert not ref["median_known"][sel].any()
    assert np.isnan(ref["wavg"][sel]).all() and not np.isnan(ref["majority"][sel]).any()


def _call_direct(fx, outs):
    """L.bce_aggregate_groups with only ``outs`` non-NULL -> (status, dict of arrays)."""
    import torch

    from bayesian_engine import _native as N

    L = N.require_gpu()
    G = len(fx["goff"]) - 1
    dev = _dev()
    # sentinels: an output that is not written shows
    buf = {k: torch.full((G,), -7.0, dtype=torch.float64, device=dev) for k in OUTS}
    buf["n_included"] = torch.full((G,), -7, dtype=torch.int64, device=dev)
    t = [_T(fx[k]) for k in ("goff", "members", "cons", "conf", "has")]
    rc = L.bce_aggregate_groups(N.ptr(t[0]), G, N.ptr(t[1]), M, N.ptr(t[2]), N.ptr(t[3]), N.ptr(t[4]),
                                *[N.ptr(buf[k]) if k in outs else None for k in OUTS + ("n_included",)],
                                N.stream(dev))
    torch.cuda.synchronize()
    return rc, {k: buf[k].cpu().numpy() for k in outs}


def test_nullable_outputs():
    from bayesian_engine import _native as N

    fx = build_batch()
    every = OUTS + ("n_included",)
    rc, full = _call_direct(fx, every)
    assert rc == N.BCE_OK
    for k in every:
        assert same_bits(full[k], _gpu()[k]) if k != "n_included" else np.array_equal(full[k], _gpu()[k])
    for outs in [(k,) for k in every] + [tuple(k for k in every if k != "median")]:
        rc, got = _call_direct(fx, outs)
        assert rc == N.BCE_OK, outs
        for k in outs:
            same = np.array_equal(got[k], full[k]) if k == "n_included" else same_bits(got[k], full[k])
            assert same, (outs, k)
    rc, _ = _call_direct(fx, ())
    assert rc == -1  # BCE_EINVAL (include/bce.h)
    assert b"no output" in N.lib().bce_last_error()


def test_many_small_groups():
    """G = 70 000 groups of 0..2 members: one workgroup each, the grid far wider than the chip."""
    import torch

    from bayesian_engine import batch

    fx = build_batch()
    rng = np.random.default_rng(70_000)
    G = 70_000
    goff = np.zeros(G + 1, np.int64)
    goff[1:] = np.cumsum(rng.integers(0, 3, G))
    members = rng.integers(0, M, int(goff[-1])).astype(np.int64)
    args = (goff, members, fx["cons"], fx["conf"], fx["has"])
    ref, oracle = aggregate_ref_groups(*args), orc.aggregate_groups(*args)
    r = batch.aggregate(*[_T(a) for a in args])
    torch.cuda.synchronize()
    got = {k: getattr(r, k).cpu().numpy() for k in OUTS + ("n_included",)}
    small = dict(names=[f"group {g}" for g in range(G)], median_only=np.zeros(G, bool))
    assert set(np.unique(ref["n_included"])) == {0, 1, 2}
    check_against(got, ref, small, np.arange(G), "kernel vs aggregate_ref")
    check_against(got, oracle, small, np.arange(G), "kernel vs oracle")
