"""The later trips of the per-signal kernels' round loops (consensus history, leave-one-out, live
history: csrc/consensus_history.hip, consensus_leave_one_out.hip, consensus_history_live.hip,
consensus_sorted.hpp) and of the stats kernels' stride loops (csrc/stats.hip, reestimate_csr.hip,
consensus_api.hip), run as test_gpu_persistent_trips.py runs the consensus kernels':
bce_debug_set_grid_cap shrinks the grid to D workgroups, the host asserts the trips from the
restated shape constants, and every output is compared with the reference its own suite uses
(tests/history_ref.py, leave_one_out_ref.py, history_live_ref.py, reestimate_csr_ref.py, the oracle,
numpy in agent order), ==, into sentinel-filled outputs, the fault word clean afterwards.

*_short_kernel<G>: a workgroup is one wave and a round is its 64 / G markets (G lanes each); the
workgroup takes rounds block, block + D, ...  Seven rounds: one workgroup seven trips, two
workgroups four and three.  A workgroup's rounds alternate: full-length markets, then empty and
single-signal markets, then full-length markets of two sources (heavy duplicates).  The sorted
(long) kernels take one market per workgroup and trip."""
import functools

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from test_gpu_persistent_trips import _cap, _trips

pytestmark = pytest.mark.gpu

ROUNDS = 7
SENTINEL = -12345.0


@pytest.fixture(autouse=True)
def _uncapped():
    yield
    N.lib().bce_debug_set_grid_cap(0)


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _round_lens(G, D):
    """Market lengths of ROUNDS rounds of 64 / G markets for a grid of D workgroups, the last round
    one market short where a round holds several; and the kind of every round: a workgroup's
    trips read full, small (empty and single-signal markets), dups, full, ..."""
    per = 64 // G
    kinds = [("full", "small", "dups")[(r // D) % 3] for r in range(ROUNDS)]
    rng = np.random.default_rng(G + D)
    lens = np.concatenate([np.full(per, G) if k != "small" else rng.integers(0, 2, per) for k in kinds])
    small = [r for r, k in enumerate(kinds) if k == "small"]
    lens[small[0] * per] = 0
    if per > 1:
        lens[small[0] * per + 1] = 1
        lens = lens[:-1]
    else:
        lens[small[-1] * per] = 1
    return lens.astype(np.int64), kinds, per


def _heavy_duplicates(sid, off, kinds, per, rng):
    """The markets of the `dups` rounds draw their sids from two sources."""
    M = len(off) - 1
    for r, k in enumerate(kinds):
        if k == "dups":
            for m in range(r * per, min((r + 1) * per, M)):
                sid[off[m]:off[m + 1]] = rng.choice(sid[off[m]:off[m] + 2], off[m + 1] - off[m])


def _assert_rounds(lens, kinds, per, G, D):
    M = len(lens)
    rounds = -(-M // per)
    grid, trips = _trips(rounds, D)
    assert rounds == ROUNDS and grid == D and trips == ([7] if D == 1 else [4, 3]) and min(trips) >= 3
    for b in range(D):
        mine = kinds[b::D]
        assert mine[:3] == ["full", "small", "dups"], (b, mine)
    assert (lens == 0).any() and (lens == 1).any() and (lens == G).any() and (per == 1 or M % per != 0)
    return rounds


def _sentinel_history(n):
    return batch.HistoryResult(*(torch.full((n,), SENTINEL, dtype=torch.float64, device=_dev()) for _ in range(3)),
                               torch.full((n,), -7, dtype=torch.int32, device=_dev()))


# ------------------------------------------------------------------ history, leave-one-out: short kernels
@functools.lru_cache(maxsize=None)
def _persignal_batch(G, D):
    import test_gpu_history as H
    lens, kinds, per = _round_lens(G, D)
    b = H._batch(lens, 40, 100 * G + D)
    rng = np.random.default_rng(G * D)
    _heavy_duplicates(b["sid"], b["off"], kinds, per, rng)
    full = np.flatnonzero(lens == G)
    b["prob"][b["off"][full[0]]] = 1.25            # out of range at a first slot: computed, not rejected
    b["prob"][b["off"][full[-1] + 1] - 1] = -0.5   # and at a last slot
    for a in b.values():
        a.setflags(write=False)
    return b, tuple(kinds), per


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_history_short_kernel_rounds(G, D):
    """history_short_kernel<8 / 16 / 32 / 64> (max_len = G: one launch), seven rounds."""
    import test_gpu_history as H
    b, kinds, per = _persignal_batch(G, D)
    rounds = _assert_rounds(np.diff(b["off"]), list(kinds), per, G, D)
    exp = H._expected(b)
    with _cap(D, f"history_short<{G}>", rounds):
        got = H._run(b, max_len=G, out=_sentinel_history(len(b["sid"])), check=True)
    H._same(got, exp, f"history short {G}")


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_leave_one_out_short_kernel_rounds(G, D):
    """loo_short_kernel<8 / 16 / 32 / 64> (max_len = G: one launch), seven rounds; the per-market
    `full` rows against the oracle's consensus of the batch."""
    import test_gpu_leave_one_out as LO
    from oracle import oracle as orc
    b, kinds, per = _persignal_batch(G, D)
    rounds = _assert_rounds(np.diff(b["off"]), list(kinds), per, G, D)
    exp = LO._expected(b)
    full = orc.consensus_csr(b["off"], b["sid"], b["prob"], b["rel"], b["conf"], b["present"])
    with _cap(D, f"loo_short<{G}>", rounds):
        res = LO._run(b, max_len=G, out=LO._sentinels(len(b["sid"]), len(b["off"]) - 1), check=True)
        got = LO._host(res)
    LO._same(got, exp, f"loo short {G}")
    for k in LO.FIELDS:
        g = getattr(res.full, k).cpu().numpy()
        assert g.dtype == full[k].dtype and np.array_equal(g, full[k]), ("full", k)


# ------------------------------------------------------------------ history, leave-one-out: sorted kernels
SORTED_LENS = (256, 129, 200, 130, 256, 131, 180)  # one length bin: one launch of the sorted kernel


@functools.lru_cache(maxsize=None)
def _sorted_batch():
    import test_gpu_history as H
    b = H._batch(SORTED_LENS, 60, 77, zipf=1.1)
    b["sid"][b["off"][2]:b["off"][3]] = np.random.default_rng(5).choice(b["sid"][:2], SORTED_LENS[2])  # two sources
    b["prob"][b["off"][1]], b["prob"][b["off"][2] - 1] = 1.25, -0.5
    for a in b.values():
        a.setflags(write=False)
    return b


def _one_bin_plan(b):
    plan = batch.Plan.build(b["off"], _dev())
    cnt = np.diff(plan.bin_start)
    assert cnt.max() == len(SORTED_LENS) == cnt.sum()  # every market in the 129..256 bin: one launch
    return plan


@pytest.mark.parametrize("D", [1, 2])
def test_history_sorted_kernel_markets(D):
    """history_long_kernel through a plan whose seven markets share one length bin: one workgroup
    sorts them one after the other in its LDS arrays (two workgroups: 4 and 3)."""
    import test_gpu_history as H
    b = _sorted_batch()
    assert _trips(7, D) == (D, [7] if D == 1 else [4, 3])
    exp = H._expected(b)
    plan = _one_bin_plan(b)
    with _cap(D, "history_long[129..256]", 7):
        got = H._run(b, plan=plan, out=_sentinel_history(len(b["sid"])), check=True)
    H._same(got, exp, "history sorted")


@pytest.mark.parametrize("D", [1, 2])
def test_leave_one_out_sorted_kernel_markets(D):
    """loo_long_kernel, as the history case."""
    import test_gpu_leave_one_out as LO
    b = _sorted_batch()
    assert _trips(7, D) == (D, [7] if D == 1 else [4, 3])
    exp = LO._expected(b)
    plan = _one_bin_plan(b)
    with _cap(D, "loo_long[129..256]", 7):
        res = LO._run(b, plan=plan, out=LO._sentinels(len(b["sid"]), 7), check=True)
        got = LO._host(res)
    LO._same(got, exp, "loo sorted")
    LO._full_is_the_consensus(b, res, "loo sorted")


# ------------------------------------------------------------------ live history
@functools.lru_cache(maxsize=None)
def _live_batch(G, D):
    import test_gpu_history_live as HL
    lens, kinds, per = _round_lens(G, D)
    rng = np.random.default_rng(300 + G + D)
    b = HL._batch(rng, lens, 40, used=24)
    _heavy_duplicates(b["sid"], b["off"], kinds, per, rng)
    return b, tuple(kinds), per


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_live_short_kernel_rounds(G, D):
    """live_short_kernel<8 / 16 / 32 / 64> (max_len = G: one launch), seven rounds, against the
    event loop of tests/history_live_ref.py."""
    import test_gpu_history_live as HL
    b, kinds, per = _live_batch(G, D)
    rounds = _assert_rounds(np.diff(b["off"]), list(kinds), per, G, D)
    exp = HL._expected(b)[0]
    with _cap(D, f"live_short<{G}>", rounds):
        got = HL._live(b, max_len=G, out=_sentinel_history(len(b["sid"])), check=True)
    HL._same(got, exp, f"live short {G}")


@pytest.mark.parametrize("D", [1, 2])
def test_live_sorted_kernel_markets(D):
    """live_long_kernel through a plan whose seven markets share one length bin."""
    import test_gpu_history_live as HL
    b = HL._batch(np.random.default_rng(311), SORTED_LENS, 60, used=40, span=90)
    assert _trips(7, D) == (D, [7] if D == 1 else [4, 3])
    exp = HL._expected(b)[0]
    plan = _one_bin_plan(b)
    with _cap(D, "live_long[129..256]", 7):
        got = HL._live(b, bins=plan, out=_sentinel_history(len(b["sid"])), check=True)
    HL._same(got, exp, "live sorted")


# ------------------------------------------------------------------ the stats kernels' stride loops
def test_reestimate_fixup_flag_list_on_one_workgroup():
    """reestimate_fixup_kernel: an MFMA pass over 2500 columns of which 30 % hold a finite cell
    outside [0, 1]: more than 600 flagged columns, redone in agent order by one workgroup of four
    waves, 256 flags per trip, three trips or four.  Against the exact pass: consensus bit-exact on the
    flagged columns, nulls, votes, words and counts identical."""
    from test_gpu_dropin import _votes_both_modes
    rng = np.random.default_rng(12)
    A, M = 100, 2500
    P = rng.beta(2, 2, size=(A, M))
    odd = rng.random(M) < 0.3
    P[rng.integers(0, A, odd.sum()), np.nonzero(odd)[0]] = rng.choice([-1, 1], odd.sum()) * rng.uniform(1.5, 5, odd.sum())
    w = rng.random(A)
    hit = ((P < 0) | (P > 1)).any(axis=0)
    assert hit.sum() > 600 and _trips(int(hit.sum()), 1, 256)[1][0] >= 3
    with _cap(1, "reestimate_fixup", int(hit.sum()), 256):
        (ce, ne, ve, we, ge), (cf, nf, vf, wf, gf) = _votes_both_modes(P, w)
    assert np.array_equal(ne, nf) and np.array_equal(ve, vf) and np.array_equal(we, wf) and np.array_equal(ge, gf)
    assert np.array_equal(cf[hit], ce[hit])
    assert np.abs(cf - ce).max() <= 4 * (A + 2) * 2.0 ** -53
    N.check_faults(_dev(), "fixup")


def test_reestimate_agreement_votes_one_slice_walks_every_word():
    """reestimate_agreement_votes_kernel: A = 17, M = 64 x 21 + 5: 22 vote words.  With the cap at 1
    the words are one blockIdx.y slice (two unrolled steps of 8 words and a tail of 6).  Against the
    same call uncapped and against numpy."""
    rng = np.random.default_rng(17)
    A, M = 17, 64 * 21 + 5
    K = (M + 63) // 64
    P = rng.beta(2, 2, size=(A, M))
    w = rng.uniform(0.01, 0.99, A)
    ws, total = np.zeros(M), 0.0
    for a in range(A):
        ws = ws + (0.0 + P[a]) * w[a]
        total = total + w[a]
    cons = ws / total
    agree_exp = ((P >= 0.5) == (cons >= 0.5)[None, :]).sum(axis=1)
    Pt, wt = _T(P), _T(w)
    L = N.lib()
    st = N.stream(_dev())
    c = torch.empty(M, dtype=torch.float64, device=_dev())
    nu = torch.empty(M, dtype=torch.uint8, device=_dev())
    votes = torch.empty((K, A), dtype=torch.int64, device=_dev())
    words = torch.empty((2, K), dtype=torch.int64, device=_dev())
    N.check(L.bce_reestimate_consensus_votes(N.ptr(Pt), A, M, M, N.ptr(wt), N.ptr(c), N.ptr(nu), N.ptr(votes),
                                             N.ptr(words[0]), N.ptr(words[1]), st), "consensus_votes")
    got = []
    for D in (1, 0):  # 0: the default grid
        g = torch.zeros(A + 1, dtype=torch.int64, device=_dev())
        with _cap(D, "reestimate_agreement_votes" if D else None, K):
            N.check(L.bce_reestimate_agreement_votes(N.ptr(votes), A, M, N.ptr(words[0]), N.ptr(words[1]),
                                                     N.ptr(g[:A]), N.ptr(g[A:]), st), "agreement_votes")
            torch.cuda.synchronize()
        got.append(g.cpu().numpy())
    assert K == 22 and np.array_equal(c.cpu().numpy(), cons)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], np.append(agree_exp, M))
    N.check_faults(_dev(), "agreement votes")


def test_reestimate_csr_agreement_entries_on_one_workgroup():
    """reestimate_csr_agreement_kernel: a plan of more than 3 x 256 entries on one workgroup of 256
    threads (four trips and more), every round against tests/reestimate_csr_ref.py."""
    import test_gpu_reestimate_csr as RC
    from reestimate_csr_ref import reference_rounds
    rng = np.random.default_rng(23)
    M, S = 100, 90
    off = RC._offsets(rng.integers(0, 40, M))
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    dup = np.setdiff1d(np.flatnonzero(rng.random(n) < 0.1), off[:-1])
    sid[dup] = sid[dup - 1]
    prob = rng.random(n)
    prob[rng.integers(0, n, 3)] = [np.nan, 0.5, 1.5]
    rounds = reference_rounds(off, sid, prob, S, 3)
    plan = batch.ReestimateCsrPlan.build(_T(off), _T(sid), _T(prob), S)
    assert plan.n_entries > 3 * 256 and min(_trips(plan.n_entries, 1, 256)[1]) >= 3
    with _cap(1, "reestimate_csr_agreement", plan.n_entries, 256):
        r = batch.reestimate_csr(plan, 3, keep_history=True)
        torch.cuda.synchronize()
    RC._check(r.history, rounds, "capped")
    N.check_faults(_dev(), "reestimate csr")


def _small_markets(M, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 70, M)
    lens[:3] = [0, 1, 65]
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    return off, rng.integers(0, 97, n).astype(np.int32), rng.random(n), rng


def test_agreement_kernel_on_one_workgroup():
    """agreement_kernel: 37 markets on one workgroup of four waves: ten trips for wave 0, nine for
    the others."""
    import test_gpu_stats_edges as SE
    off, sid, prob, rng = _small_markets(37, 31)
    prob[::7] = 0.5
    outcome = rng.choice(np.array([-1, 0, 1], np.int8), 37)
    exp_c, exp_t = SE._reference(off, sid, prob, outcome, SE.S)
    assert _trips(37, 1, 4) == (1, [10, 9, 9, 9])
    with _cap(1, "agreement", 37, 4):
        c, t = SE._run(off, sid, prob, outcome, SE.S)
    assert np.array_equal(t, exp_t) and np.array_equal(c, exp_c)


def test_validate_kernel_on_one_workgroup():
    """bce_validate_csr: 37 markets on one workgroup of four waves; the first out-of-range index of
    every market (NaN passes), -1 where none."""
    off, _, prob, rng = _small_markets(37, 32)
    lens = np.diff(off)
    for m in np.flatnonzero(lens > 0)[::3]:
        prob[off[m] + rng.integers(0, lens[m])] = rng.choice([-0.5, 1.5, np.nan])
    prob[off[3] - 1] = 2.0  # the last slot of the 65-signal market: past the first 64 lanes
    exp = np.full(37, -1, np.int32)
    for m in range(37):
        bad = np.flatnonzero((prob[off[m]:off[m + 1]] < 0) | (prob[off[m]:off[m + 1]] > 1))
        exp[m] = bad[0] if len(bad) else -1
    assert _trips(37, 1, 4) == (1, [10, 9, 9, 9]) and (exp >= 0).sum() > 5 and exp[2] >= 0
    out = torch.full((37,), -7, dtype=torch.int32, device=_dev())
    with _cap(1, "validate", 37, 4):
        got = batch.validate(_T(off), _T(prob), out=out)
        torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), exp)


def test_table_pack_on_one_workgroup():
    """bce_table_pack: S = 3 x 256 + 33 rows on one workgroup of 256 threads, a fourth trip for the first waves, the last
    present word partial (one bit)."""
    S = 3 * 256 + 33
    rng = np.random.default_rng(33)
    rel, conf = rng.random(S), rng.random(S)
    present = (rng.random(S) < 0.6).astype(np.uint8)
    present[-1] = 1
    assert _trips(S, 1, 256) == (1, [4] * 33 + [3] * 223) and S % 32 == 1
    with _cap(1, "table_pack", S, 256):
        t = batch.SourceTable.from_arrays(_T(rel), _T(conf), _T(present))
        torch.cuda.synchronize()
    rc = t.relconf.cpu().numpy()
    assert np.array_equal(rc[:, 0], rel) and np.array_equal(rc[:, 1], conf)
    pad = np.zeros(32 * ((S + 31) // 32), np.uint8)
    pad[:S] = present
    assert np.array_equal(t.bits.cpu().numpy().view(np.uint32), np.packbits(pad, bitorder="little").view(np.uint32))
