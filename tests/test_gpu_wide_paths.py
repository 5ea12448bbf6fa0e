"""One small case per instantiation and per branch of consensus_wide_kernel (csrc/consensus_wide.hip,
64 < n <= 4096), each a direct bce_consensus_csr call whose max_len picks the kernel, compared
with the oracle: BCE_MODE_EXACT by == on every output (NaN equal); BCE_MODE_FAST within 1e-9
absolute on consensus, confidence, total weight and nweight and by == on the rest.

  max_len   (NW, R, NN)   P     32-bit keys up to   64-bit-key case
      128   (1, 2, 1)     128   2^25 sources        2^25 + 1
      256   (1, 4, 1)     256   2^24                2^24 + 1
      512   (1, 8, 1)     512   2^23                2^23 + 1
     1024   (2, 8, 2)    1024   2^22                2^22 + 1
     1536   (3, 8, 4)    1536   2^21                2^21 + 1
     2048   (4, 8, 4)    2048   2^21                2^21 + 1
     3072   (6, 8, 8)    3072   2^20                2^20 + 1
     4096   (8, 8, 8)    4096   2^20                2^20 + 1

(A direct call with max_len 128 takes the wide kernel whatever the table size -- only max_len <= 64
looks at the segment kernel's 2^25-source limit -- so the R = 2 64-bit instantiation is reached
with 2^25 + 1 sources, the smallest table past its packed key.)

Branches inside the kernel and the outputs that select them:
  all outputs, NW = 1                  w[j] parked in region A for nweight (a single wave never reads
                                       the weight output back), plain rounds, no barriers
  all outputs, NW > 1, EXACT           the piped path: wave 0 carries the chains in 16-term steps,
                                       waves 1.. fill the two-slot ring of NP = 64 NW - 64 uniques
  all outputs, NW > 1, FAST            w[j] parked past the leaders when u <= P/2, else read back
                                       from the weight output; 64-bit keys never park
  nweight without weight, NW > 1       the barrier arm: w[j] parked in region A; EXACT runs the plain
                                       rounds with 8-term chain steps
  usid, weight, nweight NULL           no per-unique stores, no normalizedWeight phase
  err_idx NULL                         the per-market store without it

Every batch (_batch) carries an empty market, a 65-signal market, markets of exactly max_len
signals, a NaN, probabilities outside [0, 1] in the first and in the last input slot of a market,
a market with two bad slots (the first is reported), cold sources, an ordered and a reversed
market, one market of duplicate runs of 1, 2, 4, 5, 12, 13, 20, 48, 49, 64, 65 and 200 members
scattered over the input slots (run_sum's four-term head, its 8-term loop with 0, 1 and 2 full
steps and a tail, FAST's wave-wide sum on both sides of kWaveRun = 48; a bin too short for the
longest runs leaves them out), an all-distinct full-length market (u = P) and one with u <= P/2,
markets of 5 and of 8 distinct sources (a chain round without and with exactly one full 8-term
step), and for NW > 1 eight markets of u = 2 NP + ce distinct sources, ce in 1, 5, 16, 19, 24,
29, 32, 41: more rounds than ring slots (slot reuse, the sDone wait), the last round 0, 1 and 2
sixteen-term steps long with tails of 0, 1..7, 8 and 9..15 terms.  The 64-bit-key batches hold
the top sid and two sids that agree in their low 32 - IB bits (0 and 2^(32 - IB)).

Large tables are np.full of the cold default row with only a fixed pool of rows overwritten;
tables, batches and the oracle's outputs are built once per (max_len, table size) and frozen.

No case provokes a fault word (a market longer than max_len, a sid >= n_sources).

The last case shares the 2^25 + 1 table: a planned call over it sorts its markets of up to 64
signals in consensus_long_kernel<true> (csrc/consensus.hip), which no other test reaches."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PER_MARKET = ("consensus", "confidence", "total_weight", "n_unique", "err_idx")
PER_UNIQUE = ("usid", "weight", "nweight")
TOL = 1e-9  # the project's FAST tolerance (absolute), as test_gpu_consensus._compare_vec

# max_len -> NW, the workgroup's waves (R and NN in the docstring's table); P = max_len in every bin
BINS = {128: 1, 256: 1, 512: 1, 1024: 2, 1536: 3, 2048: 4, 3072: 6, 4096: 8}
# the smallest table past each bin's packed 32-bit key
BIG = {128: (1 << 25) + 1, 256: (1 << 24) + 1, 512: (1 << 23) + 1, 1024: (1 << 22) + 1, 1536: (1 << 21) + 1,
       2048: (1 << 21) + 1, 3072: (1 << 20) + 1, 4096: (1 << 20) + 1}
SMALL = 5000
RUNS = (1, 2, 4, 5, 12, 13, 20, 48, 49, 64, 65, 200)
RING_CE = (1, 5, 16, 19, 24, 29, 32, 41)  # last-round counts of the piped ring's markets
MODES = ["exact", "fast"]


def _freeze(*ds):
    for d in ds:
        for a in d.values():
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _table(S):
    """(rel, conf, present, pool): the cold default row everywhere but at the `pool` rows (every row
    of the small table), which the batches draw their sids from; about 30 % of the pool is cold too."""
    rng = np.random.default_rng(S)
    if S <= SMALL:
        pool = np.arange(S)
    else:
        pool = np.unique(np.r_[0, S - 1, rng.integers(1, S - 1, 6000)])
    rel = np.full(S, 0.5)
    conf = np.full(S, 0.25)
    present = np.zeros(S, np.uint8)
    hot = pool[rng.random(len(pool)) < 0.7]
    rel[hot] = rng.uniform(0.1, 1.0, len(hot))
    conf[hot] = rng.random(len(hot))
    present[hot] = 1
    for a in (rel, conf, present, pool):
        a.setflags(write=False)
    return rel, conf, present, pool


@functools.lru_cache(maxsize=None)
def _device_table(S):
    import torch
    from bayesian_engine import batch
    rel, conf, present, _ = _table(S)
    T = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731  (a copy: the cached arrays are read-only)
    t = batch.SourceTable.from_arrays(T(rel), T(conf), T(present))
    torch.cuda.synchronize()
    return t


def _runs_market(L, pool, rng):
    """Exactly L signals: the duplicate runs of RUNS that fit (ascending), the rest distinct, the
    members of every run scattered over the input slots."""
    runs = []
    for r in RUNS:
        if sum(runs) + r <= L:
            runs.append(r)
    src = rng.choice(pool, len(runs) + L - sum(runs), replace=False)
    sid = np.r_[np.repeat(src[:len(runs)], runs), src[len(runs):]]
    assert len(sid) == L
    return rng.permutation(sid), tuple(runs)


@functools.lru_cache(maxsize=None)
def _batch(L, S):
    """The batch of bin `L` over a table of S sources, its oracle outputs and what it holds."""
    from oracle import oracle as orc
    rel, conf, present, pool = _table(S)
    rng = np.random.default_rng(L * 7919 + S)
    NW = BINS[L]
    NP = 64 * NW - 64
    distinct = lambda k: rng.choice(pool, k, replace=False)  # noqa: E731
    runs_sid, runs = _runs_market(L, pool, rng)
    half = distinct(L // 2 - 3)
    mk = [
        np.zeros(0, np.int64),                                   # 0 empty
        np.r_[pool[0], pool[-1], distinct(63)],                  # 1 65 signals: sid 0 and the top sid
        runs_sid,                                                # 2 the run lengths, exactly L signals
        distinct(5),                                             # 3 bad first slot; u = 5
        distinct(8),                                             # 4 bad last slot; u = 8
        distinct(70),                                            # 5 two bad slots
        distinct(67),                                            # 6 a NaN
        distinct(L),                                             # 7 all distinct, u = P = L
        rng.permutation(np.r_[half, half[:L // 4]]),             # 8 u = L/2 - 3 <= P/2
        np.unique(np.r_[pool[0], pool[-1], distinct(L - 3)]),    # 9 ordered, sid 0 .. the top sid
        np.unique(np.r_[pool[0], pool[-1], distinct(L // 2)])[::-1],  # 10 reversed
    ]
    ring = []
    if NW > 1:
        for ce in RING_CE:
            d = distinct(2 * NP + ce)
            ring.append(len(mk))
            mk.append(rng.permutation(np.r_[d, d[:7]]))          # a few runs of 2 beside them
    lens = np.array([len(x) for x in mk], np.int64)
    off = np.zeros(len(mk) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    sid = np.concatenate(mk).astype(np.int32)
    prob = rng.random(len(sid))
    prob[off[3]] = -0.5
    prob[off[5] - 1] = 1.5
    prob[off[5] + 1] = -1.0
    prob[off[6] - 1] = 2.0
    prob[off[6] + 33] = np.nan
    g = dict(offsets=off, sid=sid, prob=prob)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _freeze(g, exp)
    u = exp["n_unique"]
    # the batch holds what the cases are meant to carry
    assert len(mk) <= 24 and lens.max() == L and (lens == L).sum() >= 2 and lens[0] == 0 and lens[1] == 65
    assert exp["err_idx"][3] == 0 and exp["err_idx"][4] == 7 and exp["err_idx"][5] == 1 and exp["err_idx"][6] == -1
    assert np.isnan(exp["consensus"][6]) and (exp["err_idx"][[0, 1, 2, 7, 8, 9, 10]] == -1).all()
    assert u[7] == L and u[8] <= L // 2 and u[3] == 5 and u[4] == 8
    assert (exp["usid"] < -1).any()  # cold sources (bit 31 of usid; -1 fills the unused slots)
    assert (np.diff(mk[9]) > 0).all() and (np.diff(mk[10]) < 0).all()
    assert {int(pool[0]), int(pool[-1])} <= set(mk[1].tolist()) and pool[-1] == S - 1
    assert runs == RUNS[:len(runs)] and (L < 512 or runs == RUNS) and 48 in runs and (L == 128 or 49 in runs)
    cnt = np.unique(mk[2], return_counts=True)[1]
    assert sorted(cnt[cnt > 1].tolist()) == [r for r in runs if r > 1]
    if NW > 1:
        assert [int(u[m]) for m in ring] == [2 * NP + ce for ce in RING_CE]
    return g, exp, tuple(ring)


def _run(L, S, mode, *, usid=True, weight=True, nweight=True, err=True):
    """bce_consensus_csr over the batch with max_len = L; an output switched off is passed as NULL."""
    import torch
    from bayesian_engine import _native as N, batch
    g, _, _ = _batch(L, S)
    table = _device_table(S)
    T = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    off, sid, prob = T(g["offsets"]), T(g["sid"]), T(g["prob"])
    M, n = len(g["offsets"]) - 1, len(g["sid"])
    res = batch._alloc(M, n, off.device, True, True)
    on = dict(usid=usid, weight=weight, nweight=nweight, err_idx=err)
    arg = lambda k: N.ptr(getattr(res, k) if on.get(k, True) else None)  # noqa: E731
    lib = N.lib()
    rc = lib.bce_consensus_csr(N.ptr(off), M, N.ptr(sid), N.ptr(prob), n, N.ptr(table.relconf), N.ptr(table.bits),
                               S, N.ptr(None), 0, L, N.MODE_FAST if mode == "fast" else N.MODE_EXACT,
                               arg("consensus"), arg("confidence"), arg("total_weight"), arg("n_unique"),
                               arg("err_idx"), arg("usid"), arg("weight"), arg("nweight"), N.stream(off.device))
    assert rc == 0, lib.bce_last_error()
    torch.cuda.synchronize()
    N.check_faults(off.device, "wide path")
    return {k: getattr(res, k).cpu().numpy() for k in PER_MARKET + PER_UNIQUE if on.get(k, True)}


def _check(out, L, S, mode):
    """The outputs the launch wrote against the oracle: EXACT by ==, NaN equal; FAST within TOL on
    consensus, confidence, total_weight and nweight, == on the rest.  Per-unique outputs over the
    slots below n_unique of every market."""
    g, exp, _ = _batch(L, S)
    off = g["offsets"]
    u = exp["n_unique"].astype(np.int64)
    pos = np.repeat(off[:-1], u) + (np.arange(int(u.sum())) - np.repeat(np.cumsum(u) - u, u))
    for k, got in out.items():
        want = exp[k]
        if k in PER_UNIQUE:
            got, want = got[pos], want[pos]
        assert got.dtype == want.dtype, k
        if mode == "fast" and k in ("consensus", "confidence", "total_weight", "nweight"):
            np.testing.assert_allclose(got, want, rtol=0, atol=TOL, equal_nan=True, err_msg=k)
        else:
            assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), k


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", list(BINS))
def test_every_bin_all_outputs(L, mode):
    """The eight (NW, R, NN) shapes with 32-bit keys and every output: NN > NW at 1536 / 3072, the
    weight read-back (wback) at NW > 1 -- in EXACT the piped ring with more rounds than slots and
    every last-round shape, in FAST the parked (u <= P/2) and the read-back markets -- and the
    run lengths of RUNS in both modes."""
    _, exp, ring = _batch(L, SMALL)
    assert len(exp["n_unique"]) <= 24 and (len(ring) == 8) == (BINS[L] > 1)
    _check(_run(L, SMALL, mode), L, SMALL, mode)


def test_piped_ring_round_shapes():
    """Host-side: the 1024 and 4096 batches hold markets of u > 2 NP distinct sources (129 and up
    at 1024, 897 and up at 4096), and their last rounds cover 0, 1 and 2 sixteen-term steps with
    tails of 0, 1..7, 8 and 9..15 terms (from the oracle's n_unique)."""
    for L, NP in ((1024, 64), (4096, 448)):
        _, exp, ring = _batch(L, SMALL)
        us = [int(exp["n_unique"][m]) for m in ring]
        assert min(us) == 2 * NP + 1 == (129 if L == 1024 else 897) and all(u > 2 * NP for u in us)
        ce = [(u - 1) % NP + 1 for u in us]
        shapes = {(c // 16, "0" if c % 16 == 0 else "1-7" if c % 16 < 8 else "8" if c % 16 == 8 else "9-15")
                  for c in ce}
        assert {(0, "1-7"), (1, "0"), (1, "1-7"), (1, "8"), (1, "9-15"), (2, "0"), (2, "9-15")} <= shapes, shapes


@pytest.mark.parametrize("L", [1024, 4096])
def test_exact_plain_rounds_on_several_waves(L):
    """EXACT at NW > 1 with nweight but without the weight output: the plain rounds behind barriers
    (not the piped ring), w[j] parked in region A, three or more rounds in a market, chain_add
    without a full 8-term step (u = 5), with exactly one (u = 8) and with steps and a tail."""
    _, exp, _ = _batch(L, SMALL)
    NT = 64 * BINS[L]
    u = exp["n_unique"].astype(np.int64)
    last = (u[u > 0] - 1) % NT + 1
    assert ((u + NT - 1) // NT >= 3).any()
    assert (last < 8).any() and (last == 8).any() and ((last > 8) & (last % 8 != 0)).any()
    out = _run(L, SMALL, "exact", weight=False)
    assert "weight" not in out
    _check(out, L, SMALL, "exact")


@pytest.mark.parametrize("weight", [True, False], ids=["wback", "no_weight"])
@pytest.mark.parametrize("L", [1024, 4096])
def test_fast_parked_and_not_parked(L, weight):
    """FAST at NW > 1: one market with u <= P/2 (w[j] parked past the leaders) and one all-distinct
    full-length market (u = P > P/2: read back from the weight output).  Without the weight output
    (!wback) both take the barrier arm that parks w[j] in region A."""
    _, exp, _ = _batch(L, SMALL)
    assert exp["n_unique"][8] <= L // 2 < exp["n_unique"][7] == L
    out = _run(L, SMALL, "fast", weight=weight)
    assert ("weight" in out) == weight
    _check(out, L, SMALL, "fast")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [512, 2048])
@pytest.mark.parametrize("off_", ["per_unique", "err_idx"])
def test_outputs_switched_off(L, mode, off_):
    """usid, weight and nweight NULL (no per-unique stores, no normalizedWeight phase; EXACT at
    NW > 1 then runs the plain rounds) and err_idx NULL."""
    if off_ == "per_unique":
        out = _run(L, SMALL, mode, usid=False, weight=False, nweight=False)
        assert set(out) == set(PER_MARKET)
    else:
        out = _run(L, SMALL, mode, err=False)
        assert "err_idx" not in out
    _check(out, L, SMALL, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", list(BINS))
def test_64bit_keys_every_bin(L, mode):
    """The smallest table past each bin's packed key: the 64-bit-key instantiation of every shape
    (one exchange buffer, two barriers per wave-crossing stage; FAST never parks: WFREE = 0), with
    the top sid, sids 0 and 2^(32 - IB) that agree in their low 32 - IB bits, an ordered and a
    reversed market."""
    S = BIG[L]
    IB = L.bit_length() - 1 if L & (L - 1) == 0 else L.bit_length()  # log2 of the padded network size
    assert S == (1 << (32 - IB)) + 1
    g, _, _ = _batch(L, S)
    sid = g["sid"]
    assert (sid == S - 1).any() and (sid == 0).any() and ((S - 1) & ((1 << (32 - IB)) - 1)) == 0
    _check(_run(L, S, mode), L, S, mode)


@functools.lru_cache(maxsize=None)
def _planned_batch():
    from oracle import oracle as orc
    rng = np.random.default_rng(77)
    lens = np.concatenate([rng.integers(65, 129, 9), rng.integers(129, 257, 4), rng.integers(513, 1025, 4),
                           rng.integers(1025, 1537, 3), rng.integers(1537, 2049, 3), rng.integers(3073, 4097, 2),
                           rng.integers(0, 65, 10), [4096, 65, 512, 1024, 2048]]).astype(np.int64)
    rng.shuffle(lens)
    rel, conf, present, pool = _table(SMALL)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    sid = pool[(rng.zipf(1.1, n) - 1) % SMALL].astype(np.int32)
    prob = rng.random(n)
    g = dict(offsets=off, sid=sid, prob=prob)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _freeze(g, exp)
    return g, exp


@pytest.mark.parametrize("mode", MODES)
def test_planned_call_merged_bins(mode):
    """One small planned call through batch.consensus: 40 markets over the wide bins.  EXACT runs
    the 1025..1536 bin inside the 2048 launch, and a call this small merges 65..512 into one launch
    in both modes: launches with n_hi > 0 (the longer bin's list first, then the shorter bins')."""
    import torch
    from bayesian_engine import _native as N, batch
    g, exp = _planned_batch()
    plan = batch.Plan.build(g["offsets"])
    cnt = np.diff(plan.bin_start)
    assert len(g["offsets"]) - 1 == 40 and cnt[8] > 0 and cnt[9] > 0 and cnt[4] > 0 and cnt[5] > 0 and cnt[6] > 0
    T = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    r = batch.consensus(T(g["offsets"]), T(g["sid"]), T(g["prob"]), _device_table(SMALL), mode=mode, plan=plan)
    torch.cuda.synchronize()
    N.check_faults(torch.device("cuda", 0), "wide planned")
    out = {k: getattr(r, k).cpu().numpy() for k in PER_MARKET + PER_UNIQUE}
    off = g["offsets"]
    u = exp["n_unique"].astype(np.int64)
    pos = np.repeat(off[:-1], u) + (np.arange(int(u.sum())) - np.repeat(np.cumsum(u) - u, u))
    for k in PER_MARKET + PER_UNIQUE:
        got, want = (out[k][pos], exp[k][pos]) if k in PER_UNIQUE else (out[k], exp[k])
        if mode == "fast" and k in ("consensus", "confidence", "total_weight", "nweight"):
            np.testing.assert_allclose(got, want, rtol=0, atol=TOL, equal_nan=True, err_msg=k)
        else:
            assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), k


@functools.lru_cache(maxsize=None)
def _long_lds_batch():
    from oracle import oracle as orc
    S = BIG[128]
    rng = np.random.default_rng(78)
    lens = np.array([0, 1, 2, 8, 9, 16, 17, 33, 63, 64, 64, 65, 4096, 5, 40], np.int64)
    rel, conf, present, pool = _table(S)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    sid = pool[(rng.zipf(1.1, n) - 1) % len(pool)].astype(np.int32)  # duplicate runs in every longer market
    sid[off[9]:off[10]] = rng.choice(pool, 64, replace=False)        # ... and one of 64 distinct sources
    sid[off[8]], sid[off[8] + 1] = S - 1, 0
    prob = rng.random(n)
    prob[off[7] + 3], prob[off[10] - 1] = 1.5, -0.25
    g = dict(offsets=off, sid=sid, prob=prob)
    exp = orc.consensus_csr(off, sid, prob, rel, conf, present)
    _freeze(g, exp)
    return g, exp


def test_planned_call_past_the_seg_key_sorts_short_markets_in_lds():
    """consensus_long_kernel<true> (csrc/consensus.hip; launch_long_lds): a planned call over
    2^25 + 1 sources, one more than the 32-bit (sid, index) key of the short-market kernels packs,
    sorts its markets of up to 64 signals with the u64 bitonic sort in LDS -- the only way to that
    kernel.  Lengths 0, 1, 2, 8, 9, 16, 17, 33, 63 and 64 (padded sizes 1..64), the top sid and sid
    0, duplicate runs, out-of-range probabilities; the markets of 65 and of 4096 signals of the same
    call run in the wide kernel.  EXACT: every output by == with the oracle."""
    import torch
    from bayesian_engine import _native as N, batch
    S = BIG[128]
    g, exp = _long_lds_batch()
    assert S > (1 << 25) and (g["sid"] == S - 1).any() and (g["sid"] == 0).any()
    plan = batch.Plan.build(g["offsets"])
    assert np.diff(plan.bin_start)[:4].min() > 0  # every bin of n <= 64 has markets
    T = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    r = batch.consensus(T(g["offsets"]), T(g["sid"]), T(g["prob"]), _device_table(S), plan=plan)
    torch.cuda.synchronize()
    N.check_faults(torch.device("cuda", 0), "long lds")
    out = {k: getattr(r, k).cpu().numpy() for k in PER_MARKET + PER_UNIQUE}
    u = exp["n_unique"].astype(np.int64)
    pos = np.repeat(g["offsets"][:-1], u) + (np.arange(int(u.sum())) - np.repeat(np.cumsum(u) - u, u))
    for k in PER_MARKET + PER_UNIQUE:
        got, want = (out[k][pos], exp[k][pos]) if k in PER_UNIQUE else (out[k], exp[k])
        assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), k
