"""One small case per branch of launch_seg_for_len (csrc/consensus.hip) and per branch inside the
three lane-per-market kernels (csrc/consensus_lane.hip), each compared with the oracle bit for
bit on every output: every float by ==, NaN equal.

  contiguous, all outputs, max_len 8 / 16 / 32       consensus_pipe_kernel<8 / 16 / 32>
  contiguous, unique_outputs=False                   consensus_flat_kernel<8 / 16 / 32>
  contiguous, all outputs, fewer than 4 signals      consensus_flat_kernel with per-unique outputs
  planned ragged batch (market lists)                consensus_lpm_kernel<8 / 16 / 32>, seg<64, 8>

max_len 32 reaches pipe / flat only past 2^18 sources (below, the LDS-table kernel takes it), so
those cases use S = 262145.  Inside the kernels: 16-B and scalar key reads (every row start a
multiple of 4 sids, or not), the array tail that fills no 16-B chunk (an odd n_signals), the
pair and the single-slot copy-out (all lengths and offsets even; one odd market from its tile
on; output views that are not 8-B / 16-B aligned), the pipe kernel's all-single and general walk
arms, present bits from LDS (S = 16384) and from global memory (S = 16385), err_idx NULL.

Every batch carries duplicate sids (runs of 2 and of 5 or more, scattered over the input
slots), probabilities outside [0, 1] at the first and at the last input slot of a market, a NaN,
cold sources and an empty market, the ragged ones a 1-signal market too (the even-length batches
cannot hold one); every launch ends in a partial tile.

n_sources = 0 has no case: the kernels then read the cold row for every sid, but every sid of a
batch must be below n_sources (a larger one raises the fault word), so a batch over an empty
table holds no signal the oracle could be asked about."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PER_MARKET = ("consensus", "confidence", "total_weight", "n_unique", "err_idx")
PER_UNIQUE = ("usid", "weight", "nweight")


def _lens(kind, G, rng):
    if kind == "ragged":      # 0..G, odd offsets: scalar key reads, single-slot copy-out
        lens = rng.integers(0, G + 1, 197)
        lens[:6] = [1, G, 0, 1, G, 3]  # rows of exactly G at odd offsets, an empty, a single
    elif kind == "even":      # all lengths even: the pair copy-out in every tile
        lens = 2 * rng.integers(0, G // 2 + 1, 197)
        lens[:4] = [2, G, 0, G]
    elif kind == "odd_early":  # one odd market in tile 1: pairs in tile 0, single slots after
        lens = 2 * rng.integers(0, G // 2 + 1, 197)
        lens[:4] = [2, G, 0, G]
        lens[70] = 3
    elif kind == "quads":     # tile 0 full rows (of distinct sids: the all-single walk arm), then
        lens = 4 * rng.integers(0, G // 4 + 1, 197)  # multiples of 4: 16-B key reads, no array tail
        lens[:64] = G
    else:
        raise KeyError(kind)
    lens = lens.astype(np.int64)
    if kind == "ragged" and int(lens.sum()) % 2 == 0:  # an odd n_signals: the last tile copies
        lens[-1] += 1 if lens[-1] < G else -1           # the array tail
    return lens


def _salt(off, sid, prob, rng, dup_from=0):
    """Duplicates (markets from `dup_from` on), out-of-range probabilities and NaN, spread over
    the markets (in place)."""
    lens = np.diff(off)
    M = len(lens)
    for m in range(M):
        a, n = int(off[m]), int(lens[m])
        r = m % 13 if m >= dup_from or m % 13 not in (1, 4) else -1
        if r == 1 and n >= 2:    # a run of 2, apart in input order
            sid[a + n - 1] = sid[a]
        elif r == 4 and n >= 5:  # a run of 5 or more over scattered slots
            k = min(n, 5 + m % 3)
            sid[a + rng.choice(n, k, replace=False)] = sid[a + n // 2]
        elif r == 6 and n >= 1:  # first input slot
            prob[a] = -0.5
        elif r == 8 and n >= 1:  # last input slot
            prob[a + n - 1] = 1.5
        elif r == 10 and n >= 2:
            prob[a + n // 2] = np.nan
        elif r == 11 and n >= 3:  # two bad slots: the first one is reported
            prob[a + n - 1] = 2.0
            prob[a + 1] = -1.0


def _table(S, rng):
    rel = rng.uniform(0.1, 1.0, S)
    conf = rng.random(S)
    present = (rng.random(S) < 0.7).astype(np.uint8)
    rel[present == 0] = 0.5
    conf[present == 0] = 0.25
    return rel, conf, present


def _freeze(g, exp):
    for a in (*g.values(), *exp.values()):
        a.setflags(write=False)
    return g, exp


@functools.lru_cache(maxsize=None)
def _contig(kind, G, S):
    """A contiguous batch of 197 markets of at most G signals over S sources and the oracle's
    outputs.  Computed once, never modified."""
    from oracle import oracle as orc
    rng = np.random.default_rng(G * 1000003 + S + {"ragged": 1, "even": 2, "odd_early": 3, "quads": 4}[kind])
    lens = _lens(kind, G, rng)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    if kind == "quads":  # the first tile: 64 full rows of distinct sids, no duplicate salt
        for m in range(64):
            sid[off[m]:off[m + 1]] = rng.choice(S, G, replace=False)
    _salt(off, sid, prob, rng, dup_from=64 if kind == "quads" else 0)
    rel, conf, present = _table(S, rng)
    g = dict(offsets=off, sid=sid, prob=prob, rel=rel, conf=conf, present=present)
    return _freeze(g, orc.consensus_csr(off, sid, prob, rel, conf, present))


def _all_single_positions(g, G):
    """Per tile of 64 markets: at how many sorted positions t < G every one of the 64 lanes holds
    a valid source seen once in its market (the pipe kernel's all-single walk arm); the other
    positions of the tile take the general arm."""
    off, sid = g["offsets"], g["sid"]
    M = len(off) - 1
    counts = []
    for m0 in range(0, M, 64):
        single = np.zeros((64, G), bool)  # lanes past the last market hold nothing
        for q, m in enumerate(range(m0, min(m0 + 64, M))):
            srt = np.sort(sid[off[m]:off[m + 1]], kind="stable")
            n = len(srt)
            first = np.r_[True, srt[1:] != srt[:-1]] if n else np.zeros(0, bool)
            last = np.r_[srt[1:] != srt[:-1], True] if n else np.zeros(0, bool)
            single[q, :n] = first & last
        counts.append(int(single.all(axis=0).sum()))
    return counts


@functools.lru_cache(maxsize=None)
def _ragged_plan_batch():
    """640 markets of 0..64 signals: about 160 in each of the <= 8, <= 16, <= 32 and 33..64 bins,
    rows of exactly 8 / 16 / 32 signals at odd offsets."""
    from oracle import oracle as orc
    rng = np.random.default_rng(4242)
    hi = np.array([8, 16, 32, 64])[rng.integers(0, 4, 640)]
    lo = np.where(hi == 8, 0, hi // 2 + 1)
    lens = rng.integers(lo, hi + 1).astype(np.int64)
    lens[:9] = [1, 8, 2, 16, 2, 32, 0, 1, 64]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    assert all(off[m] % 2 == 1 for m in (1, 3, 5))
    n, S = int(off[-1]), 3000
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    _salt(off, sid, prob, rng)
    rel, conf, present = _table(S, rng)
    g = dict(offsets=off, sid=sid, prob=prob, rel=rel, conf=conf, present=present)
    return _freeze(g, orc.consensus_csr(off, sid, prob, rel, conf, present))


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached arrays are read-only


def _misaligned_out(M, n, validate=True):
    """Per-unique outputs as views one element into their buffers: usid 4-B but not 8-B aligned,
    weight / nweight 8-B but not 16-B aligned."""
    import torch
    from bayesian_engine import batch
    res = batch._alloc(M, n, torch.device("cuda", 0), True, validate)
    res.usid = torch.empty(n + 2, dtype=torch.int32, device="cuda")[1:n + 1]
    res.weight = torch.empty(n + 2, dtype=torch.float64, device="cuda")[1:n + 1]
    res.nweight = torch.empty(n + 2, dtype=torch.float64, device="cuda")[1:n + 1]
    assert res.usid.data_ptr() % 8 == 4 and res.weight.data_ptr() % 16 == 8 and res.nweight.data_ptr() % 16 == 8
    return res


def _run(g, *, max_len=None, plan=None, unique=True, validate=True, misaligned=False):
    import torch
    from bayesian_engine import _native as N, batch
    table = batch.SourceTable.from_arrays(_dev(g["rel"]), _dev(g["conf"]), _dev(g["present"]))
    M, n = len(g["offsets"]) - 1, len(g["sid"])
    out = _misaligned_out(M, n, validate) if misaligned else None
    r = batch.consensus(_dev(g["offsets"]), _dev(g["sid"]), _dev(g["prob"]), table, max_len=max_len, plan=plan,
                        unique_outputs=unique, validate=validate, out=out)
    torch.cuda.synchronize()
    N.check_faults(torch.device("cuda", 0), "consensus path")
    return {k: (None if getattr(r, k) is None else getattr(r, k).cpu().numpy()) for k in PER_MARKET + PER_UNIQUE}


def _check(out, exp, off, unique=True, validate=True):
    """Every output against the oracle: integers equal, floats == with NaN equal; per-unique
    outputs over the slots below n_unique of every market."""
    for k in PER_MARKET:
        if k == "err_idx" and not validate:
            assert out[k] is None
            continue
        assert out[k].dtype == exp[k].dtype and np.array_equal(out[k], exp[k], equal_nan=k != "n_unique"), k
    if not unique:
        assert all(out[k] is None for k in PER_UNIQUE)
        return
    u = exp["n_unique"].astype(np.int64)
    pos = np.repeat(off[:-1], u) + (np.arange(int(u.sum())) - np.repeat(np.cumsum(u) - u, u))
    for k in PER_UNIQUE:
        assert out[k].dtype == exp[k].dtype and np.array_equal(out[k][pos], exp[k][pos], equal_nan=k != "usid"), k


def _salted(g):
    """The batch holds what every case is meant to carry."""
    off, sid, prob = g["offsets"], g["sid"], g["prob"]
    lens = np.diff(off)
    runs = [np.unique(sid[off[m]:off[m + 1]], return_counts=True)[1].max(initial=0) for m in range(len(lens))]
    bad = (prob < 0) | (prob > 1)
    return ((np.array(runs) == 2).any() and (np.array(runs) >= 5).any() and bad[off[:-1][lens > 0]].any()
            and bad[(off[1:] - 1)[lens > 0]].any() and np.isnan(prob).any() and (g["present"] == 0).any()
            and (lens == 0).any() and (lens == 1).any())


# G, S: <32> past the LDS-table kernel's 2^18 sources; <16> at both sides of the present-bit
# staging limit (16384 sources: bits in LDS, 16385: read from global memory)
WIDTHS = [(8, 500), (16, 16384), (16, 16385), (32, 262145)]


@pytest.mark.parametrize("unique", [True, False], ids=["pipe", "flat"])
@pytest.mark.parametrize("G,S", WIDTHS)
def test_contiguous_ragged_rows(G, S, unique):
    """Lengths 0..G: row starts that are no multiple of 4 sids (scalar key reads), odd offsets
    (single-slot copy-out), an odd n_signals (the array tail copy on the last tile)."""
    g, exp = _contig("ragged", G, S)
    n = len(g["sid"])
    assert _salted(g) and n % 2 == 1 and (g["offsets"][:-1] % 4 != 0).any() and (len(g["offsets"]) - 1) % 64 != 0
    assert G < 32 or 2000 <= n <= 5000
    _check(_run(g, max_len=G, unique=unique), exp, g["offsets"], unique=unique)


@pytest.mark.parametrize("unique", [True, False], ids=["pipe", "flat"])
@pytest.mark.parametrize("G,S", [(8, 500), (16, 16384), (32, 262145)])
def test_contiguous_rows_of_whole_16_byte_chunks(G, S, unique):
    """Every length a multiple of 4 and the first tile 64 full rows of distinct sids: 16-B key
    reads, no array tail, the pair copy-out, and a tile in which every lane of the wave holds a
    source seen once at every position (the pipe kernel's all-single walk arm; asserted on the
    host) beside tiles whose duplicates and short markets take the general arm."""
    g, exp = _contig("quads", G, S)
    assert (g["offsets"] % 4 == 0).all() and (np.diff(g["offsets"])[:64] == G).all()
    arm = _all_single_positions(g, G)
    assert arm[0] == G and min(arm[1:]) < G, arm  # tile 0: every position all-single; general elsewhere
    _check(_run(g, max_len=G, unique=unique), exp, g["offsets"], unique=unique)


@pytest.mark.parametrize("kind,misaligned", [("even", False), ("odd_early", False), ("even", True)])
@pytest.mark.parametrize("G,S", [(8, 500), (16, 16385), (32, 262145)])
def test_pipe_copy_out_variants(G, S, kind, misaligned):
    """All lengths and offsets even: slot pairs (8-B usid, 16-B weight stores).  One odd market in
    the second tile: pairs in the first tile, single slots from that tile on.  Output views that
    are not 8-B / 16-B aligned: single slots everywhere."""
    g, exp = _contig(kind, G, S)
    off = g["offsets"]
    assert (off[:71] % 2 == 0).all() and ((off[71:] % 2 == 1).all() if kind == "odd_early" else (off % 2 == 0).all())
    _check(_run(g, max_len=G, misaligned=misaligned), exp, off)


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("lens", [(1, 2), (2, 1)], ids=["odd_offset", "even_offsets"])
@pytest.mark.parametrize("G,S", [(8, 500), (16, 16384), (16, 16385), (32, 262145)])
def test_flat_per_unique_outputs_below_four_signals(G, S, lens, misaligned):
    """Fewer than 4 signals with all outputs go to the flat kernel (the pipe loader's fixed DMA
    shape needs 4), the one route to its per-unique copy-out short of 2^25 sources: markets of 1
    and 2 signals take the single-slot loop, of 2 and 1 the pair loop (a full pair and a half
    one), misaligned output views the single-slot loop again."""
    from oracle import oracle as orc
    rng = np.random.default_rng(G + S + lens[0])
    off = np.array([0, lens[0], 3], np.int64)
    sid = rng.integers(0, S, 3).astype(np.int32)
    sid[2] = sid[1] if lens[0] == 1 else sid[2]  # (1, 2): the second market is one run of 2
    prob = np.array([0.25, 1.5, 0.75])
    rel, conf, present = _table(S, rng)
    present[sid[0]] = 0
    rel[sid[0]], conf[sid[0]] = 0.5, 0.25
    g = dict(offsets=off, sid=sid, prob=prob, rel=rel, conf=conf, present=present)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _check(_run(g, max_len=G, misaligned=misaligned), exp, off)


@pytest.mark.parametrize("unique", [True, False], ids=["pipe", "flat"])
def test_contiguous_without_err_idx(unique):
    """validate=False: err_idx is NULL in the per-market store of pipe and flat."""
    g, exp = _contig("ragged", 16, 16385)
    _check(_run(g, max_len=16, unique=unique, validate=False), exp, g["offsets"], unique=unique, validate=False)


@pytest.mark.parametrize("unique,validate", [(True, True), (False, True), (True, False)])
def test_planned_ragged_batch_market_lists(unique, validate):
    """A host plan over 640 markets of 0..64 signals: its <= 8, <= 16 and <= 32 bins run
    consensus_lpm_kernel<8 / 16 / 32> over market lists, the 33..64 bin consensus_seg_kernel<64, 8>;
    rows of exactly 8 / 16 / 32 signals start at odd offsets.  Also without per-unique outputs
    and without err_idx."""
    from bayesian_engine import batch
    g, exp = _ragged_plan_batch()
    plan = batch.Plan.build(g["offsets"])
    cnt = np.diff(plan.bin_start)
    assert _salted(g) and (cnt[:4] >= 130).all() and (cnt[:4] <= 400).all() and cnt[4:].sum() == 0
    assert (cnt[:4] % 64 != 0).all()  # every launch ends in a partial tile
    _check(_run(g, plan=plan, unique=unique, validate=validate), exp, g["offsets"], unique=unique, validate=validate)
