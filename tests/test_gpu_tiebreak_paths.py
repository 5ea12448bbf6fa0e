"""One small case per branch of the tie-break launchers (csrc/tiebreak_lpm.hip launch_tb_lpm for
the lane kernel; csrc/tiebreak.hip launch_tb_short for the wave kernel, launch_tb_long for the
block kernel), each compared with the oracle on every output: winner, label, n_groups and
variance by bytes, the per-group outputs over the slots below n_groups, and g_of against
first-seen ordinals.

  contiguous, 16-B aligned arrays, precision 6   PART 1 (FULL tiles) + PART 2 (the rest)
  contiguous, otherwise                          one general launch (8-B aligned staging too)
  market list, aligned arrays                    gathered rows, 8 / 16 / 32 positions per lane
  market list, arrays not 16-B aligned           each lane reads and writes its own row
  33..64 agents                                  wave per market, with and without a list
  longer                                         workgroup per market: LDS (<= 4096) or scratch

Precision 6 is the double path, 30 the exact big-integer one (EXOTIC kernels)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OUTS = ("winner", "label", "n_groups", "variance", "g_key", "g_count", "g_density", "g_avgconf", "g_maxrel", "g_of")


def _csr(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


@functools.lru_cache(maxsize=None)
def _case(kind, precision):
    """(off, pred, conf, weight, rel, keys, expected) of a CSR, salted: exact halves at the
    precision, +-0.0, NaN, +-inf, zero and infinite weights.  Computed once, never modified."""
    from oracle import oracle as orc
    rng = np.random.default_rng({"tiles": 11, "ragged": 12, "wave": 13, "block": 14}[kind] * 100 + precision)
    if kind == "tiles":  # three tiles of 64 x 32 (one market of 31: its tile is not FULL), then 5 markets
        lens = np.full(197, 32, np.int64)
        lens[64 + 9] = 31
        lens[192:] = [32, 3, 0, 1, 17]
    elif kind == "ragged":
        lens = rng.integers(0, 33, 640).astype(np.int64)
        # rows of exactly 32 / 16 / 8 agents starting at odd agents, an empty and a single-agent market
        lens[:8] = [1, 32, 2, 16, 2, 8, 0, 1]
    elif kind == "wave":
        lens = rng.integers(33, 65, 20).astype(np.int64)
        lens[:3] = [33, 64, 63]
        lens = np.concatenate([lens, [5, 0, 32]])  # shorter markets beside them (lists skip them)
    else:
        lens = np.array([65, 100, 4096, 4097], np.int64)
    off = _csr(lens)
    n = int(off[-1])
    kindv = rng.integers(0, 5, n)
    pred = rng.random(n)
    pred = np.where(kindv == 1, rng.integers(0, 9, n) / 8.0, pred)  # forced ties
    pred = np.where(kindv == 2, (rng.integers(-500, 500, n) + 0.5) * 10.0 ** -precision, pred)  # halves
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


def _dev(a, aligned=True):
    import torch
    if aligned:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = torch.from_numpy(np.concatenate([a[:1], a])).cuda()[1:]  # 8-B, not 16-B aligned
    assert t.data_ptr() % 16 == 8
    return t


def _launch(case, precision, max_len, lst=None, aligned=True, long_=False):
    """One bce_tiebreak_csr / bce_tiebreak_csr_long call into sentinel-filled outputs."""
    import torch
    from bayesian_engine import _native as N
    off, pred, conf, weight, rel = case[:5]
    M, n = len(off) - 1, len(pred)
    d_off = _dev(off)
    ins = [_dev(x, aligned) for x in (pred, conf, weight, rel)]
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    out = {"winner": torch.full((M,), -7.0, **f64), "label": torch.full((M,), -7, **i32),
           "n_groups": torch.full((M,), -7, **i32), "variance": torch.full((M,), -7.0, **f64),
           "g_key": torch.full((n,), -7.0, **f64), "g_count": torch.full((n,), -7, **i32),
           "g_density": torch.full((n,), -7.0, **f64), "g_avgconf": torch.full((n,), -7.0, **f64),
           "g_maxrel": torch.full((n,), -7.0, **f64), "g_of": torch.full((n,), -7, **i32)}
    d_lst = None if lst is None else _dev(np.asarray(lst, np.int32))
    L = N.lib()
    lp, ln = (N.ptr(d_lst), len(lst)) if lst is not None else (N.ptr(None), 0)
    ip, op = [N.ptr(x) for x in ins], [N.ptr(out[k]) for k in OUTS]
    st = N.stream(d_off.device)
    if long_:
        rc = L.bce_tiebreak_csr_long(N.ptr(d_off), M, lp, ln, precision, *ip, max_len, *op, st)
    else:
        rc = L.bce_tiebreak_csr(N.ptr(d_off), M, lp, ln, *ip, max_len, precision, *op, st)
    assert rc == 0, L.bce_last_error()
    torch.cuda.synchronize()
    N.check_faults(torch.device("cuda", 0), "tie-break path")
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, case, markets=None):
    """Every output of the given markets (default: all) against the oracle; the other
    markets keep the sentinel."""
    off, keys, exp = case[0], case[5], case[6]
    M = len(off) - 1
    markets = np.arange(M) if markets is None else np.asarray(markets)
    for k in ("winner", "label", "n_groups", "variance"):
        assert got[k][markets].tobytes() == exp[k].astype(got[k].dtype)[markets].tobytes(), k
    rest = np.setdiff1d(np.arange(M), markets)
    assert (got["winner"][rest] == -7.0).all() and (got["n_groups"][rest] == -7).all()
    # nor are their rows touched: a gathered row shares its first and last 16-B pair with the
    # neighbouring markets, and the flush stores only the row's own agents
    listed = np.zeros(int(off[-1]), bool)
    for m in map(int, markets):
        listed[off[m]:off[m + 1]] = True
    for k in ("g_key", "g_count", "g_density", "g_avgconf", "g_maxrel", "g_of"):
        assert (got[k][~listed] == -7).all(), k
    with np.errstate(invalid="ignore", divide="ignore"):
        dens = exp["g_total"] / np.maximum(exp["g_count"], 1)
    want = {"g_key": exp["g_key"], "g_count": exp["g_count"], "g_density": dens, "g_avgconf": exp["g_avgconf"],
            "g_maxrel": exp["g_maxrel"]}
    for m in map(int, markets):
        a, b, g = int(off[m]), int(off[m + 1]), int(exp["n_groups"][m])
        if b == a:
            continue
        for k, w in want.items():
            assert got[k][a:a + g].tobytes() == w[a:a + g].astype(got[k].dtype).tobytes(), (k, m)
        # first-seen ordinal under ==: -0.0 joins 0.0 (one dict slot), a NaN key is its own group
        seen, ords = {}, []
        for x in map(float, keys[a:b]):
            ords.append(seen.setdefault(x, len(seen)))
        assert list(got["g_of"][a:b]) == ords, m


def test_contiguous_aligned_splits_full_and_rest():
    """197 markets, arrays 16-B aligned, precision 6: tile 0 is FULL and goes to PART 1.  PART 2
    takes the other three: tile 1 with the 31-agent market, tile 2 of 64 x 32 that the short
    market moved to an odd agent (no 16-B rows, so not FULL either) and the trailing partial tile."""
    case = _case("tiles", 6)
    _check(_launch(case, 6, 32), case)


@pytest.mark.parametrize("precision,aligned", [(6, False), (30, False), (30, True)])
def test_contiguous_one_general_launch(precision, aligned):
    """The same CSR where the split does not apply: inputs offset by one element (8-B aligned
    staging), and the exotic precision at either alignment."""
    case = _case("tiles", precision)
    _check(_launch(case, precision, 32, aligned=aligned), case)


def _bucket_list(lens, bound):
    """About 130 markets of at most `bound` agents: the ones only this bound takes first, the
    planted odd-start rows, the empty and the single-agent market among them."""
    lo = {8: 0, 16: 9, 32: 17}[bound]
    own = np.nonzero((lens >= lo) & (lens <= bound))[0]
    planted = np.array([m for m in range(8) if lens[m] <= bound])
    return np.unique(np.concatenate([planted, own[:130 - len(planted)]])).astype(np.int32)


@pytest.mark.parametrize("precision", [6, 30])
@pytest.mark.parametrize("bound", [8, 16, 32])
def test_market_list_gathered_rows(bound, precision):
    """A list with max_len 8 / 16 / 32 over aligned arrays: rows gathered into LDS, 8 / 16 / 32
    positions per lane.  Rows start at odd and even agents; a row of exactly `bound` agents at
    an odd start takes the one-lane tail copy."""
    case = _case("ragged", precision)
    off = case[0]
    lens = np.diff(off)
    lst = _bucket_list(lens, bound)
    assert 100 <= len(lst) <= 140 and (off[lst] & 1).any() and not (off[lst] & 1).all()
    assert ((lens[lst] == bound) & (off[lst] & 1 == 1)).any()
    assert (lens[lst] == 1).any() and (lens[lst] == 0).any()
    _check(_launch(case, precision, bound, lst=lst), case, lst)


@pytest.mark.parametrize("precision", [6, 30])
def test_market_list_unaligned_arrays_per_lane_rows(precision):
    """A list over arrays that are not 16-B aligned: no staging, each lane reads its row from
    global memory and writes its outputs there."""
    case = _case("ragged", precision)
    lst = np.arange(3, 3 + 131, dtype=np.int32)
    _check(_launch(case, precision, 32, lst=lst, aligned=False), case, lst)


@pytest.mark.parametrize("precision", [6, 30])
@pytest.mark.parametrize("listed", [False, True])
def test_wave_kernel(listed, precision):
    """Markets of 33..64 agents (max_len 64): one wave per market, over the whole batch or a list."""
    case = _case("wave", precision)
    lens = np.diff(case[0])
    lst = np.nonzero(lens >= 33)[0].astype(np.int32) if listed else None
    _check(_launch(case, precision, 64, lst=lst), case, lst)


@pytest.mark.parametrize("precision", [6, 30])
@pytest.mark.parametrize("market", [0, 1, 2, 3])
def test_block_kernel(market, precision):
    """One market of 65 / 100 / 4096 agents sorted in LDS, one of 4097 in a global scratch slice."""
    case = _case("block", precision)
    n = int(np.diff(case[0])[market])
    _check(_launch(case, precision, n, lst=[market], long_=True), case, [market])
