"""The later trips of the consensus kernels' tile loops (csrc/consensus_tab.hip, consensus_lane.hip,
consensus.hip, consensus_wide.hip).

Every hot kernel is persistent: the launcher caps the grid at CUs x resident workgroups and a wave
or workgroup strides over its tiles, carrying prefetched metadata, registers loaded for the next
market, LDS ring slots, scratch slices and flags from one trip to the next.  At the sizes of the
per-branch suites every wave makes one trip.  Here bce_debug_set_grid_cap shrinks the grid to D
workgroups (D = 1, and a second D so that strides of more than one workgroup are covered), so a
few thousand markets make three and more trips, and consecutive tiles of one wave are of
different kinds.  The cap changes the grid and nothing else: results must not depend on it.

Every case first asserts on the host, from the shape constants restated below, how many trips each
wave or workgroup makes -- trips = ceil(units / (D x units per workgroup trip)) -- and that the
planted tile kinds occur in the order its docstring claims (a restatement of the kernel's own
predicate).  Outputs are pre-filled with a sentinel and compared with the oracle exactly as the
path suites compare (test_gpu_consensus_paths.py, test_gpu_wide_paths.py): == with NaN equal; FAST
wide launches within that suite's TOL.  Inputs carry the usual salt: duplicate sids, out-of-range
probabilities at first and last slots, NaN, cold sources, empty and single-signal markets.  The
fault word is clean after each case.

Each case prints one `grid_cap:` line (units, D, grid, trips, host wall time of the capped calls in
microseconds: uploads, launches and the synchronise)."""
import contextlib
import functools
import time

import numpy as np
import pytest

from test_gpu_consensus_paths import PER_MARKET, PER_UNIQUE, _all_single_positions, _salt, _salted, _table

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = -12345.0, -7

# shape constants of the kernels, restated
TAB_WAVES = 8            # consensus_tab.hip kTabWaves: tile = w * grid + block, stride 8 * grid
TAB_MAX_S = 10112        # consensus_common.hpp kTabMaxSources: plain table up to here, hybrid beyond
TAB_LDS = 160 * 1024     # kTabLdsBytes: the hybrid kernel stages the rows that fit beside the bitmask
PIPE_R = {8: 9, 16: 9, 32: 6}  # consensus_lane.hip PipeCfg<G>::R = C + 3 = 9; kPipeR32 = 6
FLAT_WPB = 2             # kFlatWPB: tile = block * 2 + w, stride 2 * grid
SEG_TM = 8               # consensus_seg_kernel<64, 8>: 8 markets per workgroup trip
WIDE_META = 64           # consensus_wide_kernel: market metadata read 64 markets of the workgroup at a time
PIPE_BOUNDS = 64         # consensus_pipe_kernel: the loader reads the bounds of its next 64 tiles at a time


# ---------------------------------------------------------------------------------------- the cap
@contextlib.contextmanager
def _cap(D, case=None, units=None, per_trip=1):
    """Persistent grids of at most D workgroups inside the block; the default again after it."""
    from bayesian_engine import _native as N
    L = N.lib()
    N.check(L.bce_debug_set_grid_cap(int(D)), "bce_debug_set_grid_cap")
    t0 = time.perf_counter()
    try:
        yield
    finally:
        L.bce_debug_set_grid_cap(0)
        if case is not None:
            grid, trips = _trips(units, D, per_trip)
            print(f"grid_cap: {case}: units={units} D={D} grid={grid} trips={min(trips)}..{max(trips)} "
                  f"wall_us={(time.perf_counter() - t0) * 1e6:.0f}")


@pytest.fixture(autouse=True)
def _uncapped():
    yield
    from bayesian_engine import _native as N
    N.lib().bce_debug_set_grid_cap(0)


def _trips(units, D, per_trip=1):
    """(grid, trips of each of the grid's grid * per_trip striding waves / workgroups) of a launch
    over `units` units whose grid is capped at D workgroups of `per_trip` units per trip."""
    grid = min(D, -(-units // per_trip))
    stride = grid * per_trip
    return grid, [-(-(units - g) // stride) for g in range(stride) if g < units]


def _csr(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # a copy: cached arrays are read-only


def _freeze(*ds):
    for d in ds:
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


def _sentinel_out(M, n, unique=True, validate=True):
    import torch
    from bayesian_engine import batch
    res = batch._alloc(M, n, torch.device("cuda", 0), unique, validate)
    for k in PER_MARKET + PER_UNIQUE:
        t = getattr(res, k)
        if t is not None:
            t.fill_(SENT_F if t.dtype.is_floating_point else SENT_I)
    return res


def _call_csr(g, table, L, *, mode="exact", unique=True, lst=None, base=0, out=None):
    """One bce_consensus_csr call (max_len = L picks the kernel; `lst`: a market list) into
    sentinel-filled outputs.  `base`: the arrays start with `base` signals no market owns and the
    offsets with `base` (an offset view)."""
    import torch
    from bayesian_engine import _native as N
    off, sid, prob = g["offsets"], g["sid"], g["prob"]
    M, n = len(off) - 1, len(sid) + base
    if base:
        off = off + base
        sid = np.r_[np.zeros(base, np.int32), sid]
        prob = np.r_[np.full(base, 0.5), prob]
    d_off, d_sid, d_prob = _dev(off), _dev(sid), _dev(prob)
    res = out or _sentinel_out(M, n, unique)
    d_lst = None if lst is None else _dev(np.asarray(lst, np.int32))
    lib = N.lib()
    rc = lib.bce_consensus_csr(N.ptr(d_off), M, N.ptr(d_sid), N.ptr(d_prob), n, N.ptr(table.relconf),
                               N.ptr(table.bits), table.n, N.ptr(d_lst), 0 if lst is None else len(lst), int(L),
                               N.MODE_FAST if mode == "fast" else N.MODE_EXACT, N.ptr(res.consensus),
                               N.ptr(res.confidence), N.ptr(res.total_weight), N.ptr(res.n_unique), N.ptr(res.err_idx),
                               N.ptr(res.usid), N.ptr(res.weight), N.ptr(res.nweight), N.stream(d_off.device))
    assert rc == 0, lib.bce_last_error()
    torch.cuda.synchronize()
    N.check_faults(torch.device("cuda", 0), "persistent trips")
    return res


def _host(res):
    return {k: (None if getattr(res, k) is None else getattr(res, k).cpu().numpy()) for k in PER_MARKET + PER_UNIQUE}


def _check(out, exp, off, *, unique=True, markets=None, base=0, mode="exact", tol=0.0):
    """The outputs of `markets` (default: all) against the oracle: integers equal, floats == with NaN
    equal (FAST: consensus, confidence, total weight and nweight within `tol`); per-unique outputs
    over the slots below n_unique.  The other markets, and the `base` signals ahead of the first
    market, keep the sentinel."""
    M = len(off) - 1
    mk = np.arange(M) if markets is None else np.asarray(markets, np.int64)
    rest = np.setdiff1d(np.arange(M), mk)

    def same(k, got, want):
        assert got.dtype == want.dtype, k
        if mode == "fast" and k in ("consensus", "confidence", "total_weight", "nweight"):
            np.testing.assert_allclose(got, want, rtol=0, atol=tol, equal_nan=True, err_msg=k)
        else:
            bad = ~((got == want) | ((got != got) & (want != want))) if got.dtype.kind == "f" else got != want
            assert not bad.any(), (k, np.flatnonzero(bad)[:8])

    for k in PER_MARKET:
        same(k, out[k][mk], exp[k][mk])
        assert (out[k][rest] == (SENT_F if out[k].dtype.kind == "f" else SENT_I)).all(), k
    if not unique:
        assert all(out[k] is None for k in PER_UNIQUE)
        return
    u = exp["n_unique"].astype(np.int64)[mk]
    pos = np.repeat(off[:-1][mk], u) + (np.arange(int(u.sum())) - np.repeat(np.cumsum(u) - u, u))
    owned = np.zeros(int(off[-1]) + base, bool)
    for m in mk:
        owned[base + off[m]:base + off[m + 1]] = True
    for k in PER_UNIQUE:
        same(k, out[k][base + pos], exp[k][pos])
        assert (out[k][:len(owned)][~owned] == (SENT_F if out[k].dtype.kind == "f" else SENT_I)).all(), k


# ------------------------------------------------------------------ consensus_tab32_kernel
# What chain g % 8 (the wave that starts at tile g; its tiles are g, g + 8 D, g + 16 D, g + 24 D)
# holds on trips 0..3.  R: regular (64 markets of 32 signals, the base a multiple of 4 signals);
# I: irregular (short markets inside); X: 64 markets of 32 signals at a base that is no multiple of
# 4 (a 31-signal market in the I tile before the run shifted it; the short markets of the I tile
# after the run bring the total shift back to a multiple of 4); E: 64 empty markets.  The last
# tile of the batch (37 markets; chain 3, trip 3) is partial whatever its letter says.
TAB_CHAINS = ("RIRR", "RRII", "IRXR", "XIIR", "XXER", "IIRI", "RERR", "ERIR")


def _tab_tile_kinds(off, base=0):
    """The kernel's predicate restated: a tile is regular iff all its 64 markets have 32 signals and
    its base is a multiple of 4 signals (16 B of sid; the arrays are 16-B aligned)."""
    lens = np.diff(off)
    M = len(lens)
    kinds = []
    for m0 in range(0, M, 64):
        t = lens[m0:m0 + 64]
        if len(t) < 64:
            kinds.append("P")
        elif (t == 0).all():
            kinds.append("E")
        elif (t == 32).all():
            kinds.append("R" if (off[m0] + base) % 4 == 0 else "X")
        else:
            kinds.append("I")
    return kinds


@functools.lru_cache(maxsize=None)
def _tab_batch(D, S):
    """28 D tiles (the last of 37 markets) laid out by TAB_CHAINS for a grid of D workgroups, over S
    sources, and the oracle's outputs."""
    from oracle import oracle as orc
    rng = np.random.default_rng(1000 * D + S)
    T, stride = 28 * D, TAB_WAVES * D
    want = [TAB_CHAINS[(t % stride) % 8][t // stride] for t in range(T)]
    lens = np.full(64 * T, 32, np.int64)
    shift = 0  # signals before the tile, mod 4
    for t, kind in enumerate(want):
        tile = lens[64 * t:64 * t + 64]
        if kind == "E":
            tile[:] = 0
        elif kind == "I":
            nxt = next((k for k in want[t + 1:] if k in "RX"), "R")
            target = 0 if nxt == "R" else 3
            if shift == 0 and target == 3:
                tile[rng.integers(0, 64)] = 31  # one 31-signal market shifts every later base
            else:
                at = rng.choice(64, 4, replace=False)
                tile[at[:3]] = [0, 1, rng.integers(2, 31)]
                d = next(d for d in (1, 2, 3, 4) if (shift + tile.sum() - tile[at[3]] + 32 - d) % 4 == target)
                tile[at[3]] = 32 - d
        else:
            assert (shift == 0) == (kind == "R"), (t, kind, shift)
        shift = (shift + int(tile.sum())) % 4
    lens = lens[:64 * (T - 1) + 37]
    off = _csr(lens)
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    _salt(off, sid, prob, rng)
    rel, conf, present = _table(S, rng)
    g = dict(offsets=off, sid=sid, prob=prob, rel=rel, conf=conf, present=present)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _freeze(g, exp)
    return g, exp, tuple(want[:-1] + ["P"])


def _assert_tab_chains(g, want, D, base=0):
    off = g["offsets"]
    kinds = _tab_tile_kinds(off, base)
    assert kinds == list(want), (kinds, want)
    T, stride = len(kinds), TAB_WAVES * D
    grid, trips = _trips(T, D, TAB_WAVES)
    assert grid == D and T == 28 * D and sorted(set(trips)) == [3, 4] and trips.count(4) == 4 * D
    chains = ["".join(kinds[g0::stride]) for g0 in range(stride)]
    reg = [c.replace("X", "I").replace("E", "I").replace("P", "I") for c in chains]  # regular or not
    for pair in ("RI", "IR", "RR", "II"):
        assert any(pair in c for c in reg), pair
    assert any("XX" in c for c in chains) and "XX" in "".join(kinds)  # a misaligned run, in a chain and in tile order
    assert any("RER" in c for c in chains)                            # 64 empty markets between two regular tiles
    last = chains[(T - 1) % stride]
    assert last.endswith("P") and len(last) == 4                      # the partial tile ends a chain of four trips
    return T


TAB_VARIANTS = {  # S, unique outputs, signals ahead of the first market
    "plain": (9000, True, 0),
    "hybrid": (12000, True, 0),
    "plain_no_unique": (9000, False, 0),
    "hybrid_no_unique": (12000, False, 0),
    "offset_view": (9000, True, 8),
}


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("variant", list(TAB_VARIANTS))
def test_tab32_chains_of_regular_and_irregular_tiles(variant, D):
    """consensus_tab32_kernel: 64 x (28 D - 1) + 37 markets on D workgroups of 8 waves: 28 D tiles,
    so the waves that start at the first 4 D tiles make four trips and the rest three, each tile's
    Meta read at the top of the tile before it in the chain.  The chains (TAB_CHAINS) hold
    regular -> irregular, irregular -> regular, regular -> regular and irregular -> irregular, a run
    of tiles of 64 x 32 signals at a misaligned base, 64 empty markets between two regular tiles,
    and the partial last tile at the end of a four-trip chain.  Plain table (S = 9000), hybrid
    table (S = 12000: sids on both sides of the staged rows), with and without the per-unique
    outputs, and an offset view (offsets[0] = 8: the same tile kinds at an aligned base)."""
    import torch
    from bayesian_engine import batch
    S, unique, base = TAB_VARIANTS[variant]
    g, exp, want = _tab_batch(D, S)
    T = _assert_tab_chains(g, want, D, base)
    assert _salted(g) and base % 4 == 0
    staged = min((TAB_LDS - 4 * ((S + 31) // 32)) // 16, S)  # launch_tab32_t: rows in LDS
    assert (S <= TAB_MAX_S and staged == S) or ((g["sid"] < staged).any() and (g["sid"] >= staged).any())
    table = batch.SourceTable.from_arrays(_dev(g["rel"]), _dev(g["conf"]), _dev(g["present"]))
    torch.cuda.synchronize()
    with _cap(D, f"tab32[{variant}]", T, TAB_WAVES):
        res = _call_csr(g, table, 32, unique=unique, base=base)
    _check(_host(res), exp, g["offsets"], unique=unique, base=base)


# ------------------------------------------------------------------ consensus_pipe_kernel<G>
PIPE_TILES = 67  # on one workgroup the ring of R slots wraps 7 (G = 32: 11) times and the
#                  loader reads its second batch of 64 tile bounds; D = 2: 34 and 33 tiles


@functools.lru_cache(maxsize=None)
def _pipe_batch(G, S):
    """PIPE_TILES tiles whose kinds cycle F, E, O, E, Rg: F 64 full rows of distinct sids (the
    all-single walk arm), E even lengths, O even lengths and one odd market (every later row starts
    at the other parity), Rg ragged 0..G with an even total.  The last tile holds 29 markets."""
    from oracle import oracle as orc
    rng = np.random.default_rng(G * 7 + S)
    T = PIPE_TILES
    lens = np.zeros(64 * T, np.int64)
    for t in range(T):
        kind = "FEOER"[t % 5]
        tile = lens[64 * t:64 * t + 64]
        if kind == "F":
            tile[:] = G
        elif kind in "EO":
            tile[:] = 2 * rng.integers(0, G // 2 + 1, 64)
            tile[:3] = [2, G, 0]
            if kind == "O":
                tile[rng.integers(3, 64)] = 3
        else:
            tile[:] = rng.integers(0, G + 1, 64)
            tile[:4] = [1, G, 0, 3]
            if tile.sum() % 2:
                tile[63] += 1 if tile[63] < G else -1
    lens = lens[:64 * (T - 1) + 29]
    off = _csr(lens)
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    full = [t for t in range(T - 1) if t % 5 == 0]
    for t in full:  # 64 full rows of distinct sids, no duplicate salt
        for m in range(64 * t, 64 * t + 64):
            sid[off[m]:off[m + 1]] = rng.permutation(rng.integers(0, S - 7 * G) + 7 * np.arange(G))
    keep = sid.copy(), prob.copy()
    _salt(off, sid, prob, rng)
    for t in full:
        a, b = off[64 * t], off[64 * t + 64]
        sid[a:b], prob[a:b] = keep[0][a:b], keep[1][a:b]
    rel, conf, present = _table(S, rng)
    g = dict(offsets=off, sid=sid, prob=prob, rel=rel, conf=conf, present=present)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _freeze(g, exp)
    return g, exp


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("G,S", [(8, 500), (16, 16384), (16, 16385), (32, 262145)])
def test_pipe_ring_wraps(G, S, D):
    """consensus_pipe_kernel<8 / 16 / 32>: a workgroup's loader streams its tiles (block, block + D,
    ...) into a ring of R LDS slots; slot reuse (wait_free, sequence >= R) needs more than R tiles
    per workgroup.  67 tiles on one workgroup (two: 34 and 33) wrap the ring at least three times,
    and the loader refills its batch of 64 tile bounds.  Neighbouring tiles of a workgroup differ:
    pair copy-out (every row start of the tile even) and single-slot copy-out, the all-single walk
    arm (full rows of distinct sids) and the general arm, ragged rows.  Present bits from LDS
    (S = 16384) and from global memory (S = 16385); <32> runs past 2^18 sources."""
    import torch
    from bayesian_engine import batch
    g, exp = _pipe_batch(G, S)
    off = g["offsets"]
    T = -(-(len(off) - 1) // 64)
    R = PIPE_R[G]
    grid, trips = _trips(T, D)
    assert grid == D and T == PIPE_TILES and min(trips) >= 2 * R + 1 and (D > 1 or max(trips) > PIPE_BOUNDS)
    assert _salted(g) and (len(off) - 1) % 64 == 29
    pairs = [bool((off[64 * t:min(64 * t + 64, len(off) - 1)] % 2 == 0).all()) for t in range(T)]
    arm = _all_single_positions(g, G)
    for b in range(D):  # every workgroup's chain: both copy-outs and both walk arms, in both orders
        p, s = pairs[b::D], [x == G for x in arm[b::D]]
        for seq in (p, s):
            steps = set(zip(seq[:-1], seq[1:]))
            assert {(True, False), (False, True)} <= steps, (b, seq)
    table = batch.SourceTable.from_arrays(_dev(g["rel"]), _dev(g["conf"]), _dev(g["present"]))
    torch.cuda.synchronize()
    with _cap(D, f"pipe<{G}>[S={S}]", T):
        res = _call_csr(g, table, G)
    _check(_host(res), exp, off)


# ------------------------------------------------------------------ consensus_flat_kernel<G>
@functools.lru_cache(maxsize=None)
def _profiled_batch(G, D, per_trip, S, tiny_signals=None):
    """3 x D x per_trip + 1 tiles of 64 markets; tile t is `full` (every market G signals) on a
    wave's even trips and `tiny` (0..2 signals) on its odd ones, so a wave's chain reads full,
    tiny, full (tiny again on the fourth trip of wave 0: the partial last tile, 21 markets)."""
    from oracle import oracle as orc
    rng = np.random.default_rng(G * 11 + D * 3 + per_trip + S)
    stride = D * per_trip
    T = 3 * stride + 1
    lens = np.zeros(64 * T, np.int64)
    for t in range(T):
        tile = lens[64 * t:64 * t + 64]
        tile[:] = G if (t // stride) % 2 == 0 else rng.integers(0, 3, 64)
    lens = lens[:64 * (T - 1) + 21]
    if tiny_signals is not None:  # fewer than 4 signals in all: one in the first tile, two in a second-trip tile
        lens[:] = 0
        lens[5], lens[64 * stride + 9] = tiny_signals
    off = _csr(lens)
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    if tiny_signals is None:
        _salt(off, sid, prob, rng)
    else:
        sid[-1] = sid[-2]  # the market of two signals is one run of 2
        prob[0] = 1.5
    rel, conf, present = _table(S, rng)
    if tiny_signals is not None:
        present[sid[0]] = 0
        rel[sid[0]], conf[sid[0]] = 0.5, 0.25
    g = dict(offsets=off, sid=sid, prob=prob, rel=rel, conf=conf, present=present)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _freeze(g, exp)
    return g, exp, T


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("G,S", [(8, 500), (16, 16385), (32, 262145)])
def test_flat_kernel_full_then_tiny_then_full(G, S, D):
    """consensus_flat_kernel<G> (unique_outputs=False): wave w of workgroup b starts at tile 2 b + w
    and steps by 2 D; 6 D + 1 tiles give every wave three trips (wave 0 four): a tile of full rows,
    a tile of markets of 0..2 signals, full rows again."""
    import torch
    from bayesian_engine import batch
    g, exp, T = _profiled_batch(G, D, FLAT_WPB, S)
    grid, trips = _trips(T, D, FLAT_WPB)
    lens = np.diff(g["offsets"])
    assert grid == D and sorted(set(trips)) == [3, 4] and _salted(g)
    for w in range(FLAT_WPB * D):
        prof = [int(lens[64 * t:64 * t + 64].max()) for t in range(w, T, FLAT_WPB * D)]
        assert prof[0] == G and prof[1] <= 2 and prof[2] == G, (w, prof)
    table = batch.SourceTable.from_arrays(_dev(g["rel"]), _dev(g["conf"]), _dev(g["present"]))
    torch.cuda.synchronize()
    with _cap(D, f"flat<{G}>", T, FLAT_WPB):
        res = _call_csr(g, table, G, unique=False)
    _check(_host(res), exp, g["offsets"], unique=False)


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("G,S", [(8, 500), (32, 262145)])
def test_flat_kernel_below_four_signals_over_many_tiles(G, S, D):
    """Fewer than 4 signals with every output go to the flat kernel with its per-unique copy-out:
    6 D + 1 tiles of empty markets, one signal (out of range, a cold source) in a first-trip tile
    and a run of 2 in a second-trip tile of another wave."""
    import torch
    from bayesian_engine import batch
    g, exp, T = _profiled_batch(G, D, FLAT_WPB, S, tiny_signals=(1, 2))
    grid, trips = _trips(T, D, FLAT_WPB)
    assert grid == D and min(trips) == 3 and len(g["sid"]) == 3
    assert list(exp["n_unique"][[5, 64 * FLAT_WPB * D + 9]]) == [1, 1] and exp["err_idx"][5] == 0
    table = batch.SourceTable.from_arrays(_dev(g["rel"]), _dev(g["conf"]), _dev(g["present"]))
    torch.cuda.synchronize()
    with _cap(D, f"flat<{G}>[3 signals]", T, FLAT_WPB):
        res = _call_csr(g, table, G)
    _check(_host(res), exp, g["offsets"])


# ------------------------------------------------------------------ consensus_lpm_kernel<G>, consensus_seg_kernel<64, 8>
@functools.lru_cache(maxsize=None)
def _listed_batch():
    """2600 markets of 0..64 signals in shuffled order (rows at odd and even offsets), about a
    quarter each full-length for a bound of 8 / 16 / 32 / 64 or tiny."""
    from oracle import oracle as orc
    rng = np.random.default_rng(5151)
    lens = rng.choice([8, 16, 32, 64, 0, 1, 2, 3], 2600, p=[.15, .15, .15, .07, .12, .12, .12, .12]).astype(np.int64)
    off = _csr(lens)
    n, S = int(off[-1]), 3000
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    _salt(off, sid, prob, rng)
    rel, conf, present = _table(S, rng)
    g = dict(offsets=off, sid=sid, prob=prob, rel=rel, conf=conf, present=present)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _freeze(g, exp)
    return g, exp


def _profiled_list(lens, G, per_tile, D, rng):
    """A market list of 3 D tiles and a partial one (`per_tile` entries each) for a grid of D
    workgroups: tile t holds markets of exactly G signals on a workgroup's even trips and of 0..3
    signals on its odd ones."""
    full, tiny = rng.permutation(np.flatnonzero(lens == G)), rng.permutation(np.flatnonzero(lens <= 3))
    lst, T = [], 3 * D + 1
    for t in range(T):
        k = per_tile if t < T - 1 else per_tile // 2 + 1
        src = full if (t // D) % 2 == 0 else tiny
        take, rest = src[:k], src[k:]
        assert len(take) == k, (G, t)
        lst.append(take)
        if (t // D) % 2 == 0:
            full = rest
        else:
            tiny = rest
    return np.concatenate(lst).astype(np.int32), T


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_market_list_kernels_full_then_tiny_then_full(G, D):
    """consensus_lpm_kernel<8 / 16 / 32> (a tile = 64 list entries per one-wave workgroup) and
    consensus_seg_kernel<64, 8> (8 list entries) over a market list, the launch a plan's bin makes:
    3 D + 1 tiles, every workgroup three trips (workgroup 0 four): markets of exactly G signals,
    then of 0..3 signals, then of G again; the listed rows lie scattered over a shuffled batch
    and every other market keeps the sentinel."""
    import torch
    from bayesian_engine import batch
    g, exp = _listed_batch()
    lens = np.diff(g["offsets"])
    per_tile = SEG_TM if G == 64 else 64
    lst, T = _profiled_list(lens, G, per_tile, D, np.random.default_rng(G + D))
    grid, trips = _trips(T, D)
    assert grid == D and trips == [4, 3][:D] and _salted(g) and len(set(lst.tolist())) == len(lst)
    assert -(-len(lst) // per_tile) == T and len(lst) % per_tile != 0
    for b in range(D):
        prof = [int(lens[lst[per_tile * t:per_tile * (t + 1)]].max()) for t in range(b, T, D)]
        assert prof[0] == G and prof[1] <= 3 and prof[2] == G, (b, prof)
    assert (g["offsets"][lst] % 2 == 1).any() and (g["offsets"][lst] % 2 == 0).any()
    table = batch.SourceTable.from_arrays(_dev(g["rel"]), _dev(g["conf"]), _dev(g["present"]))
    torch.cuda.synchronize()
    with _cap(D, f"{'seg<64, 8>' if G == 64 else f'lpm<{G}>'}", T):
        res = _call_csr(g, table, G, lst=lst)
    _check(_host(res), exp, g["offsets"], markets=lst)


# ------------------------------------------------------------------ consensus_wide_kernel
WIDE_SHORTEST = {128: 65, 512: 257, 1024: 513, 1536: 1025, 4096: 3073}
WIDE_MARKETS = 131  # D = 1: refills at the 65th and the 129th market, a last batch of 3; D = 2: 66 and 65
WIDE_SALTED = (0, 63, 64, 128)  # positions in a workgroup's chain that carry the duplicates and the bad probabilities
WIDE_BIG = (1024, (1 << 22) + 1)  # the 64-bit-key case: the smallest table past the bin's packed key


def _wide_salted(D):
    """(chain position, market) of the salted markets: workgroup b's p-th market is market p D + b."""
    return [(p, p * D + b) for p in WIDE_SALTED for b in range(D) if p * D + b < WIDE_MARKETS]


@functools.lru_cache(maxsize=None)
def _wide_batch(L, S, D):
    """131 markets of bin L for a grid of D workgroups: the p-th market of every workgroup's chain
    (market p D + b) is of the bin's longest length for even p and of its shortest for odd p (every
    16th short one empty), so the registers loaded ahead for a long market are followed by a short
    one and the reverse."""
    from oracle import oracle as orc
    from test_gpu_wide_paths import _table as wide_table
    rel, conf, present, pool = wide_table(S)
    rng = np.random.default_rng(L * 31 + S + D)
    pos = np.arange(WIDE_MARKETS) // D
    lens = np.where(pos % 2 == 0, L, WIDE_SHORTEST[L]).astype(np.int64)
    lens[pos % 16 == 1] = 0
    off = _csr(lens)
    n = int(off[-1])
    sid = pool[rng.integers(0, len(pool), n)].astype(np.int32)
    prob = rng.random(n)
    for p, m in _wide_salted(D):
        a, k, i = int(off[m]), int(lens[m]), WIDE_SALTED.index(p)
        assert k >= 65
        sid[a + rng.choice(k, 40, replace=False)] = sid[a]   # a run of 40 or more over scattered slots
        sid[a + k - 1] = sid[a + 1]                          # and a run of 2
        prob[a if i % 2 == 0 else a + k - 1] = -0.5 if i < 2 else 1.5  # bad first / last slot
        prob[a + k // 2] = np.nan
    sid[off[2 * D]], sid[off[2 * D] + 1] = pool[0], pool[-1]  # sid 0 and the top sid
    g = dict(offsets=off, sid=sid, prob=prob)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _freeze(g, exp)
    for p, m in _wide_salted(D):
        assert exp["err_idx"][m] == (0 if WIDE_SALTED.index(p) % 2 == 0 else lens[m] - 1), (p, m)
    assert (exp["usid"] < -1).any() and (lens == 0).any() and pool[-1] == S - 1
    return g, exp


def _assert_wide_chains(g, L, D):
    """Every workgroup's chain b::D goes long -> short and short -> long, holds empty markets, and
    its markets at chain positions 0, 63 and 64 (one workgroup: 128 too) are the salted ones."""
    lens = np.diff(g["offsets"])
    salted = _wide_salted(D)
    assert len(salted) == (4 if D == 1 else 3 * D)
    for b in range(D):
        chain = lens[b::D]
        steps = set(zip(chain[:-1].tolist(), chain[1:].tolist()))
        assert {(L, WIDE_SHORTEST[L]), (WIDE_SHORTEST[L], L), (L, 0), (0, L)} <= steps, (b, steps)
        mine = [p for p, m in salted if m % D == b]
        assert mine[:3] == [0, 63, 64] and all(chain[p] >= 65 for p in mine), (b, mine)
        assert len(chain) > WIDE_META  # the refill past the chain's 64th market
    prob, off = g["prob"], g["offsets"]
    for p, m in salted:
        assert np.isnan(prob[off[m]:off[m + 1]]).any() and ((prob[off[m]:off[m + 1]] < 0) | (prob[off[m]:off[m + 1]] > 1)).any()
        assert np.unique(g["sid"][off[m]:off[m + 1]], return_counts=True)[1].max() >= 40


WIDE_CASES = [(L, 5000, "exact") for L in (128, 512, 1024, 1536, 4096)] + \
             [(L, 5000, "fast") for L in (128, 1024, 4096)] + [WIDE_BIG + ("exact",)]


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("L,S,mode", WIDE_CASES)
def test_wide_kernel_metadata_refill_and_prefetch(L, S, mode, D):
    """consensus_wide_kernel: a workgroup reads the metadata of its next 64 markets at once (refill(),
    k == 0 in meta()) and issues the loads of market li + G while market li finishes.  131 markets
    in one launch: on one workgroup the refills at its 65th and 129th market and a last batch of 3;
    on two, 66 and 65 markets.  Within every workgroup's chain the lengths alternate between the
    bin's longest and shortest (asserted on the host per chain), and the chain's markets at
    positions 0, 63 and 64 (one workgroup: 128 too) carry the duplicate runs and the bad
    probabilities.  EXACT by ==, FAST within the wide suite's TOL; one bin with 64-bit keys."""
    from test_gpu_wide_paths import BIG, BINS, TOL, _device_table
    g, exp = _wide_batch(L, S, D)
    M = len(g["offsets"]) - 1
    grid, trips = _trips(M, D)
    assert L in BINS and (S == 5000 or S == BIG[L]) and M == WIDE_MARKETS and grid == D
    assert trips == ([131] if D == 1 else [66, 65]) and min(trips) > WIDE_META
    _assert_wide_chains(g, L, D)
    table = _device_table(S)
    with _cap(D, f"wide[{L}, S={S}, {mode}]", M):
        res = _call_csr(g, table, L, mode=mode)
    _check(_host(res), exp, g["offsets"], mode=mode, tol=TOL)


PLANNED_LENS = (100, 65, 128, 200, 400, 1300, 1536, 1800, 2048, 1537, 4096, 3500, 3073, 5, 0, 40, 64, 33, 1)


@functools.lru_cache(maxsize=None)
def _planned_mixed_batch():
    """Few markets per bin, so that a schedule made with one resident workgroup per kernel still
    merges (fewer than 6 markets = kMergeRounds rounds of that grid): 65..512 as one launch and
    1025..2048 as one launch in both modes."""
    from oracle import oracle as orc
    from test_gpu_wide_paths import _table as wide_table
    rel, conf, present, pool = wide_table(5000)
    rng = np.random.default_rng(99)
    off = _csr(np.array(PLANNED_LENS, np.int64))
    n = int(off[-1])
    sid = pool[(rng.zipf(1.1, n) - 1) % len(pool)].astype(np.int32)
    prob = rng.random(n)
    prob[off[3]], prob[off[7] - 1], prob[off[8] + 5] = -0.5, 1.5, np.nan
    g = dict(offsets=off, sid=sid, prob=prob)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _freeze(g, exp)
    return g, exp


@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_wide_planned_call_on_one_workgroup(mode):
    """One planned call (batch.consensus with a plan) over a mixed batch with the cap at 1: the
    schedule is made with wide_resident = 1 (restated through bce_plan_schedule and asserted: in
    both modes the 65..512 bins run as one launch and the 1025..1536 bin in the 2048 launch, so
    list_hi / n_hi are in use with markets on both sides), and each launch's one workgroup walks
    all its markets, five in either merged launch.  The plan is host data and the schedule is made
    at call time, so a plan built inside the cap equals one built outside; both are run."""
    import torch
    from bayesian_engine import _native as N, batch, sharding
    from test_gpu_wide_paths import TOL, _device_table
    g, exp = _planned_mixed_batch()
    off = g["offsets"]
    M, n = len(off) - 1, len(g["sid"])
    plan_out = batch.Plan.build(off)
    cnt = np.diff(plan_out.bin_start)
    launches, fork = sharding.plan_schedule(plan_out.bin_start, mode, {b: 1 for b in range(N.NBINS)})
    assert (4, 6, 0) in launches and (8, 9, 0) in launches and fork, launches
    assert cnt[4] == 3 and cnt[5] == 1 and cnt[6] == 1 and cnt[8] == 2 and cnt[9] == 3 and cnt[11] == 3
    outs = []
    with _cap(1, f"wide planned[{mode}]", 5):
        plan_in = batch.Plan.build(off)
        for plan in (plan_in, plan_out):
            res = _sentinel_out(M, n)
            batch.consensus(_dev(off), _dev(g["sid"]), _dev(g["prob"]), _device_table(5000), mode=mode, plan=plan,
                            out=res)
            torch.cuda.synchronize()
            N.check_faults(torch.device("cuda", 0), "wide planned")
            outs.append(_host(res))
    assert np.array_equal(plan_in.bin_start, plan_out.bin_start) and torch.equal(plan_in.order, plan_out.order)
    u = exp["n_unique"].astype(np.int64)
    pos = np.repeat(off[:-1], u) + (np.arange(int(u.sum())) - np.repeat(np.cumsum(u) - u, u))
    for k in PER_MARKET + PER_UNIQUE:
        a, b = (outs[0][k][pos], outs[1][k][pos]) if k in PER_UNIQUE else (outs[0][k], outs[1][k])
        assert a.tobytes() == b.tobytes(), k
    _check(outs[0], exp, off, mode=mode, tol=TOL)


# ------------------------------------------------------------------ consensus_long_kernel
LONG_S = (1 << 25) + 1  # past the short-market kernels' packed key: a plan's bins of n <= 64 run the LDS form


@functools.lru_cache(maxsize=None)
def _long_batch(lens, S):
    from oracle import oracle as orc
    from test_gpu_wide_paths import _table as wide_table
    rel, conf, present, pool = wide_table(S)
    rng = np.random.default_rng(sum(lens) + S)
    off = _csr(np.array(lens, np.int64))
    n = int(off[-1])
    sid = pool[(rng.zipf(1.1, n) - 1) % len(pool)].astype(np.int32)  # duplicate runs in every market
    prob = rng.random(n)
    sid[off[1]], sid[off[1] + 1] = pool[-1], pool[0]
    prob[off[1]], prob[off[2] - 1], prob[off[2] + 1] = 1.5, -0.25, np.nan
    g = dict(offsets=off, sid=sid, prob=prob)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _freeze(g, exp)
    assert (exp["usid"] < -1).any() and exp["err_idx"][1] == 0 and (exp["n_unique"] < np.diff(off)).all()
    return g, exp


def _planned(g, S, plan):
    import torch
    from bayesian_engine import _native as N, batch
    from test_gpu_wide_paths import _device_table
    res = _sentinel_out(len(g["offsets"]) - 1, len(g["sid"]))
    batch.consensus(_dev(g["offsets"]), _dev(g["sid"]), _dev(g["prob"]), _device_table(S), plan=plan, out=res)
    torch.cuda.synchronize()
    N.check_faults(torch.device("cuda", 0), "long kernel")
    return res


@pytest.mark.parametrize("D", [1, 2])
def test_long_kernel_lds_reused_by_shorter_and_longer_markets(D):
    """consensus_long_kernel<true> sorts a market of up to 4096 signals in the workgroup's LDS arrays,
    padded to the next power of two; the planned call past 2^25 sources sends it the bins of
    n <= 64.  The kernel itself takes any market that fits its arrays, so a hand-made plan that
    lists markets of 4096, 65, 3000, 70, 4096, 66 and 2000 signals (in this order) in the 33..64
    bin makes one workgroup (two: 4 and 3 markets, the plan's order dealing them so that either
    chain alternates) sort a short market in the arrays a long one just left, and the reverse.

    This files markets in a bin they do not belong to and depends on consensus_long_kernel<true>
    not checking a market against its bin's bound (the tab and wide kernels do, and raise the fault
    word): a bound check added to that kernel later makes this case fail without being a
    regression; the case then has to go, or reach the kernel another way."""
    import torch
    from bayesian_engine import _native as N, batch
    lens = (4096, 65, 3000, 70, 4096, 66, 2000)
    g, exp = _long_batch(lens, LONG_S)
    grid, trips = _trips(len(lens), D)
    assert grid == D and trips == ([7] if D == 1 else [4, 3])
    order = np.arange(7) if D == 1 else np.array([0, 4, 1, 5, 2, 6, 3])  # D = 2: chains 0 1 2 3 and 4 5 6
    for b in range(D):
        chain = np.array(lens)[order[b::D]]
        assert ((chain[:-1] > 1000) != (chain[1:] > 1000)).all(), (b, chain)  # long, short, long, ...
    bin_start = np.zeros(N.NBINS + 1, np.int64)
    bin_start[4:] = len(lens)  # all seven in bin 3
    plan = batch.Plan(torch.from_numpy(order.astype(np.int32)).cuda(), bin_start, max(lens), None)
    with _cap(D, "long<lds>[4096, 65, 3000, ...]", len(lens)):
        res = _planned(g, LONG_S, plan)
    _check(_host(res), exp, g["offsets"])


def test_long_kernel_lds_short_markets_on_one_workgroup():
    """The form the planned call does reach: five markets of 33..64 signals past 2^25 sources, one
    launch of consensus_long_kernel<true>, one workgroup, five trips."""
    from bayesian_engine import batch
    lens = (64, 33, 50, 64, 40)
    g, exp = _long_batch(lens, LONG_S)
    plan = batch.Plan.build(g["offsets"])
    assert np.diff(plan.bin_start)[3] == 5 and _trips(5, 1) == (1, [5])
    with _cap(1, "long<lds>[33..64]", 5):
        res = _planned(g, LONG_S, plan)
    _check(_host(res), exp, g["offsets"])


def test_long_kernel_scratch_slice_reused():
    """consensus_long_kernel<false>: markets of 9000, 4100 and 6000 signals through a plan, whose
    scratch holds one slice per workgroup of the default grid (three).  On one workgroup slice 0 is
    reused by a shorter and then a longer market and the other two slices keep the bytes they were
    filled with -- which also shows that the cap reaches the launch: without it every slice is
    written."""
    from bayesian_engine import batch
    lens = (9000, 4100, 6000)
    g, exp = _long_batch(lens, 5000)
    plan = batch.Plan.build(g["offsets"])
    slice_bytes = 4 * 16384 * 8  # four arrays of next_pow2(9000) 8-byte keys (plan_host.hpp long_scratch_bytes)
    assert _trips(3, 1) == (1, [3]) and plan.scratch.numel() == 3 * slice_bytes
    touched = {}
    for D in (1, 0):  # 0: the default grid
        plan.scratch.fill_(0xAB)
        with _cap(D, "long<global>[9000, 4100, 6000]" if D else None, 3):
            res = _planned(g, 5000, plan)
        _check(_host(res), exp, g["offsets"])
        touched[D] = [bool((plan.scratch[k * slice_bytes:(k + 1) * slice_bytes] != 0xAB).any()) for k in range(3)]
    assert touched == {1: [True, False, False], 0: [True, True, True]}, touched
