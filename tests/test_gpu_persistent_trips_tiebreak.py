"""The later trips of the tie-break kernels' tile loops (csrc/tiebreak_lpm.hip, csrc/tiebreak.hip),
run as test_gpu_persistent_trips.py runs the consensus kernels': bce_debug_set_grid_cap shrinks
the grid to D workgroups, the host asserts the trips of every wave from the restated shape
constants and the order of the planted tile kinds from the kernel's own predicate, and every
output is compared with the oracle as test_gpu_tiebreak_paths.py compares (its _launch and
_check: sentinel-filled outputs, bytes equal, unlisted markets untouched, the fault word clean).

tiebreak_lpm_kernel, the FULL / rest pair: PART 1 runs the FULL tiles and carries `left` ("this
wave left a tile to PART 2") across its trips into the wave's split word; PART 2 runs only the
waves whose word was raised.  A tile is FULL iff all its 64 markets have 32 agents and its first
row starts at an even agent.  FULL tiles need an even start, so a tile with one 31-agent market
(the next tile starts odd) and a tile of FULL lengths at an odd start can only stand next to
other non-FULL tiles in tile order; a lone non-FULL tile between FULL ones is a `mixed` tile of
0..32 agents with an even total."""
import functools

import numpy as np
import pytest

from test_gpu_persistent_trips import _cap, _trips
from test_gpu_tiebreak_paths import _check, _csr, _launch

pytestmark = pytest.mark.gpu

TB_LPM_WAVES = 4  # tiebreak_lpm.hip kTbLpmWaves: wave g = 4 block + w takes tiles g, g + 4 D, ...
TB_WAVE_WAVES = 4  # tiebreak_wave_kernel: 256 threads, one market per wave and trip


@pytest.fixture(autouse=True)
def _uncapped():
    yield
    from bayesian_engine import _native as N
    N.lib().bce_debug_set_grid_cap(0)


@functools.lru_cache(maxsize=None)
def _tb_case(lens, precision, seed):
    """(off, pred, conf, weight, rel, keys, expected) of a CSR of the given lengths, salted as
    test_gpu_tiebreak_paths._case salts: forced ties, exact halves at the precision, +-0.0, NaN,
    +-inf, zero and infinite weights.  Computed once, never modified."""
    from oracle import oracle as orc
    rng = np.random.default_rng(seed * 100 + precision)
    off = _csr(np.array(lens, np.int64))
    n = int(off[-1])
    kindv = rng.integers(0, 5, n)
    pred = rng.random(n)
    pred = np.where(kindv == 1, rng.integers(0, 9, n) / 8.0, pred)
    pred = np.where(kindv == 2, (rng.integers(-500, 500, n) + 0.5) * 10.0 ** -precision, pred)
    pred = np.where(kindv == 3, rng.integers(-30, 30, n) * 50.0, pred)
    pred[rng.random(n) < 0.02] = -0.0
    pred[rng.random(n) < 0.02] = 0.0
    pred[rng.random(n) < 0.005] = np.nan
    pred[rng.random(n) < 0.004] = np.inf
    pred[rng.random(n) < 0.004] = -np.inf
    conf, rel = rng.random(n), rng.choice([0.5, 0.9], n)
    weight = rng.choice([0.5, 1.0, 2.0], n)
    weight[rng.random(n) < 0.01] = 0.0
    weight[rng.random(n) < 0.003] = np.inf
    keys = np.array([round(float(x), precision) for x in pred], np.float64)
    exp = orc.tiebreak_csr(off, pred, conf, weight, rel, keys=keys)
    for a in (off, pred, conf, weight, rel, keys, *exp.values()):
        a.setflags(write=False)
    return off, pred, conf, weight, rel, keys, exp


# ------------------------------------------------------------------ the FULL / rest pair
# Tile kinds in tile order, one row per trip.  F: FULL; M: mixed 0..32 with empties, even total;
# 1: 64 x 32 but for one 31-agent market; O: FULL lengths at an odd start; P: the final partial
# tile (37 markets of 32 agents, at an odd start).
SPLIT_TILES = {
    1: ("FMFM", "FFFM", "FFF1", "P"),
    2: ("F1OMFFFM", "FFMFFFFM", "FFMFFMF1", "P"),
}
# D = 1, outside the pattern of roles: 17 tiles, a 1, O, M run of whole tiles on the first and third
# trips of waves 1..3 with FULL tiles on their second and fourth, wave 0 all FULL and then the
# partial tile (here at an even start)
SPLIT_RUN_TILES = ("F1OM", "FFFF", "F1OM", "FFFF", "P")


@functools.lru_cache(maxsize=None)
def _split_lens(D, rows=None):
    rng = np.random.default_rng(40 + D)
    lens, odd = [], False
    for kind in "".join(rows or SPLIT_TILES[D]):
        tile = np.full(37 if kind == "P" else 64, 32, np.int64)
        if kind == "F":
            assert not odd
        elif kind == "O":
            assert odd
        elif kind == "1":
            tile[rng.integers(0, 64)] = 31
        elif kind == "M":
            tile[:] = rng.integers(0, 33, 64)
            tile[rng.choice(64, 6, replace=False)] = 0
            if (int(tile.sum()) % 2 == 1) != odd:  # the next tile starts at an even agent
                k = int(np.argmax(tile > 0))
                tile[k] -= 1
        odd ^= bool(int(tile.sum()) % 2)
        lens.append(tile)
    return tuple(int(x) for x in np.concatenate(lens))


def _split_kinds(off):
    """The kernel's predicate restated: FULL iff 64 markets of 32 agents from an even agent."""
    lens = np.diff(off)
    out = []
    for m0 in range(0, len(lens), 64):
        t = lens[m0:m0 + 64]
        all32 = bool((t == 32).all())
        out.append("P" if len(t) < 64 else
                   ("F" if off[m0] % 2 == 0 else "O") if all32 else
                   "1" if sorted(t)[0] == 31 and sorted(t)[1] == 32 else "M")
    return out


def _assert_split_chains(off, D):
    kinds = _split_kinds(off)
    assert "".join(kinds) == "".join(SPLIT_TILES[D]), kinds
    T, nw = len(kinds), TB_LPM_WAVES * D
    grid, trips = _trips(T, D, TB_LPM_WAVES)
    assert grid == D and trips == [4] + [3] * (nw - 1)
    left = [[k != "F" for k in kinds[g::nw]] for g in range(nw)]  # per wave and trip: the tile is left to PART 2
    assert [True, False, False] in left        # a wave that leaves a tile only on its first trip
    assert [False, False, True] in left or [False, False, False, True] in left  # only on its last
    assert [True, True, True] in left          # on every trip
    assert [False, False, False] in left       # never: its split word is not raised, PART 2 counts it out
    assert left[(T - 1) % nw] == [False, False, False, True] and kinds[-1] == "P" and off[64 * (T - 1)] % 2 == 1
    assert {"F", "M", "1", "P"} <= set(kinds) and (D == 1 or "O" in kinds)
    lens = np.diff(off)
    assert (lens == 0).sum() >= 6 and (lens == 31).any()
    return T


@pytest.mark.parametrize("D", [1, 2])
def test_lpm_split_left_flag_across_trips(D):
    """Contiguous, 16-B aligned, precision 6: the PART 1 / PART 2 pair on D workgroups of four waves;
    12 D + 1 tiles, every wave three trips and wave 0 a fourth.  One wave leaves a tile to PART 2
    only on its first trip, one only on its last, one on every trip, one never, and wave 0 owns the
    final partial tile after three FULL ones (SPLIT_TILES).  With D = 1 the four waves are exactly
    these four roles, whatever the number of trips: a whole tile of FULL lengths at an odd start
    needs a non-FULL tile before and after it in tile order, and the only neighbours that are not
    FULL are the first tiles of two waves or the partial tile, so there it can only be the
    partial tile; test_lpm_split_run_of_odd_start_tiles has the whole-tile run on one workgroup."""
    case = _tb_case(_split_lens(D), 6, 1)
    T = _assert_split_chains(case[0], D)
    with _cap(D, "tiebreak lpm split", T, TB_LPM_WAVES):
        got = _launch(case, 6, 32)
    _check(got, case)


def test_lpm_split_run_of_odd_start_tiles():
    """The PART 1 / PART 2 pair on one workgroup, 17 tiles (SPLIT_RUN_TILES): waves 1, 2 and 3 leave a
    tile with one 31-agent market, a whole tile of FULL lengths at an odd start and a mixed tile on
    their first and third trips and run FULL tiles on their second and fourth (`left` stays set
    across FULL tiles); wave 0 runs four FULL tiles and leaves the partial one."""
    case = _tb_case(_split_lens(1, SPLIT_RUN_TILES), 6, 5)
    kinds = _split_kinds(case[0])
    assert "".join(kinds) == "".join(SPLIT_RUN_TILES) and _trips(17, 1, TB_LPM_WAVES) == (1, [5, 4, 4, 4])
    assert ["".join(kinds[g::4]) for g in range(4)] == ["FFFFP", "1F1F", "OFOF", "MFMF"]
    with _cap(1, "tiebreak lpm split[1, O, M run]", 17, TB_LPM_WAVES):
        got = _launch(case, 6, 32)
    _check(got, case)


@pytest.mark.parametrize("precision,aligned", [(6, False), (30, True)])
def test_lpm_one_general_launch_across_trips(precision, aligned):
    """The same 13 tiles where the split does not apply -- arrays that are not 16-B aligned at
    precision 6, and precision 30 -- on one workgroup: FULL-length, mixed and partial tiles follow
    each other in one general body."""
    case = _tb_case(_split_lens(1), precision, 1)
    T = _assert_split_chains(case[0], 1)
    with _cap(1, f"tiebreak lpm general[p{precision}]", T, TB_LPM_WAVES):
        got = _launch(case, precision, 32, aligned=aligned)
    _check(got, case)


@functools.lru_cache(maxsize=None)
def _ragged_lens():
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 33, 4000)
    lens[:8] = [1, 32, 2, 16, 2, 8, 0, 1]
    return tuple(int(x) for x in lens)


def _list_for(lens, bound, rng):
    """13 tiles (the last partial) of markets of at most `bound` agents, in shuffled order; the
    planted odd-start rows, the empty and the single-agent market among them."""
    lo = {8: 0, 16: 9, 32: 17}[bound]
    own = np.flatnonzero((lens >= lo) & (lens <= bound))
    own = own[own >= 8]
    planted = np.array([m for m in range(8) if lens[m] <= bound])
    few = np.flatnonzero(lens <= 1)[:40]  # empty and single-agent markets in every bound's list
    lst = np.unique(np.concatenate([planted, few, own]))[:64 * 12 + 23]
    return rng.permutation(lst).astype(np.int32)


@pytest.mark.parametrize("bound,aligned", [(8, True), (16, True), (32, True), (32, False)])
def test_lpm_market_lists_across_trips(bound, aligned):
    """A market list on one workgroup, 13 tiles of 64 entries (four trips for wave 0, three for the
    others): rows gathered into the wave's LDS buffer with 8 / 16 / 32 positions per lane, and --
    arrays not 16-B aligned -- every lane reading and writing its own row."""
    case = _tb_case(_ragged_lens(), 6, 2)
    off = case[0]
    lens = np.diff(off)
    lst = _list_for(lens, bound, np.random.default_rng(bound))
    T = -(-len(lst) // 64)
    assert _trips(T, 1, TB_LPM_WAVES) == (1, [4, 3, 3, 3]) and len(lst) % 64 != 0 and lens[lst].max() == bound
    assert (off[lst] & 1).any() and not (off[lst] & 1).all() and (lens[lst] == 0).any() and (lens[lst] == 1).any()
    with _cap(1, f"tiebreak lpm list[{bound}{'' if aligned else ', per lane'}]", T, TB_LPM_WAVES):
        got = _launch(case, 6, bound, lst=lst, aligned=aligned)
    _check(got, case, lst)


@pytest.mark.parametrize("precision", [6, 30])
def test_wave_kernel_across_trips(precision):
    """tiebreak_wave_kernel: 13 markets of 33..64 agents on one workgroup of four waves: wave 0 four
    markets, the others three."""
    rng = np.random.default_rng(9)
    lens = rng.integers(33, 65, 13)
    lens[:4] = [64, 33, 63, 34]
    case = _tb_case(tuple(int(x) for x in lens), precision, 3)
    assert _trips(13, 1, TB_WAVE_WAVES) == (1, [4, 3, 3, 3])
    with _cap(1, f"tiebreak wave[p{precision}]", 13, TB_WAVE_WAVES):
        got = _launch(case, precision, 64)
    _check(got, case)


@pytest.mark.parametrize("lens", [(4096, 65, 2000, 100), (5000, 4097, 4500)], ids=["lds", "scratch"])
def test_block_kernel_across_trips(lens):
    """tiebreak_block_kernel on one workgroup: its LDS arrays (markets of 4096, 65, 2000 and 100 agents,
    in this order) and its global scratch slice (5000, 4097, 4500) are reused by a shorter and then a
    longer market."""
    case = _tb_case(lens, 6, 4)
    assert _trips(len(lens), 1) == (1, [len(lens)])
    with _cap(1, f"tiebreak block[{lens[0]}, ...]", len(lens)):
        got = _launch(case, 6, max(lens), lst=list(range(len(lens))), long_=True)
    _check(got, case)
