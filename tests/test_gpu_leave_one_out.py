"""GPU checks of the leave-one-source-out consensus (bce_consensus_leave_one_out,
batch.leave_one_out and the layers above it).  Every expectation is the oracle's
consensus of the host-expanded batch (tests/leave_one_out_ref.expand: one reduced market per
signal), compared with ``np.array_equal`` on every signal -- null leave-outs compare as their 0.0
values, none is left out; the full_* outputs are compared with ``batch.consensus``."""
import json
import os
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from golden_util import load_json
from leave_one_out_ref import FIELDS, expand, fixture_table, load_fixture
from oracle import oracle as orc
from score_ref import score_ref

pytestmark = pytest.mark.gpu

EDGE_LENS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 4096)
SENTINEL = -12345.0


def _dev():
    return torch.device("cuda", 0)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


def _table(b):
    return batch.SourceTable.from_arrays(_T(b["rel"]), _T(b["conf"]), _T(b["present"]))


def _expected(b):
    exp = orc.consensus_csr(*expand(b["off"], b["sid"], b["prob"]), b["rel"], b["conf"], b["present"])
    return {k: exp[k] for k in FIELDS}


def _host(r):
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in FIELDS}


def _same(got, exp, what="", at=slice(None)):
    for k in FIELDS:
        g, e = got[k][at], exp[k][at]
        assert g.dtype == e.dtype and np.array_equal(g, e), (what, k, np.flatnonzero(g != e)[:8])


def _full_is_the_consensus(b, res, what=""):
    """``res.full`` against batch.consensus on the same batch, every market, bit for bit."""
    ref = batch.consensus(_T(b["off"]), _T(b["sid"]), _T(b["prob"]), _table(b), check=True)
    for k in FIELDS:
        g, e = getattr(res.full, k), getattr(ref, k)
        assert g.dtype == e.dtype and torch.equal(g, e), (what, k)


def _run(b, **kw):
    return batch.leave_one_out(_T(b["off"]), _T(b["sid"]), _T(b["prob"]), _table(b), **kw)


def _batch(lens, S, seed, zipf=None, p_cold=0.2, p_zero=0.1):
    rng = np.random.default_rng(seed)
    off = _offsets(lens)
    n = int(off[-1])
    if zipf:
        w = 1.0 / np.arange(1, S + 1) ** zipf
        sid = rng.choice(S, n, p=w / w.sum()).astype(np.int32)
    else:
        sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    rel, conf = rng.uniform(0.05, 1.0, S), rng.random(S)
    rel[rng.random(S) < p_zero] = 0.0
    present = (rng.random(S) >= p_cold).astype(np.uint8)
    rel[present == 0], conf[present == 0] = 0.5, 0.25
    return dict(off=off, sid=sid, prob=prob, rel=rel, conf=conf, present=present)


def _raw(off, n_markets, sid, prob, table, lst, max_len, out, full):
    """The C entry, unplanned: one launch sized by max_len over a plain market list (or all)."""
    f = [N.ptr(getattr(full, k) if full is not None else None) for k in FIELDS]
    N.check(N.lib().bce_consensus_leave_one_out(
        N.ptr(off), n_markets, N.ptr(sid), N.ptr(prob), sid.numel(), N.ptr(table.relconf), N.ptr(table.bits), table.n,
        N.ptr(lst), 0 if lst is None else lst.numel(), N.ptr(None), N.ptr(None), max_len, N.ptr(out.consensus),
        N.ptr(out.confidence), N.ptr(out.total_weight), N.ptr(out.n_unique), *f, N.stream(_dev())),
        "bce_consensus_leave_one_out")


def _sentinels(n, M=None):
    out = batch.LeaveOneOutResult(*(torch.full((n,), SENTINEL, dtype=torch.float64, device=_dev()) for _ in range(3)),
                                  torch.full((n,), -7, dtype=torch.int32, device=_dev()))
    if M is not None:
        out.full = batch.ConsensusResult(*(torch.full((M,), SENTINEL, dtype=torch.float64, device=_dev())
                                           for _ in range(3)),
                                         torch.full((M,), -7, dtype=torch.int32, device=_dev()), None, None, None, None)
    return out


def _untouched(got, where, what):
    for k in FIELDS:
        assert (got[k][where] == (-7 if k == "n_unique" else SENTINEL)).all(), (what, k)


# ----------------------------------------------------------------------------- lengths at the edges
@pytest.fixture(scope="module")
def edges():
    b = _batch(EDGE_LENS, 3000, 1, zipf=1.1)
    return b, _expected(b)


def test_edge_lengths_on_every_route(edges):
    b, exp = edges
    assert len(b["sid"]) == sum(EDGE_LENS) and (exp["total_weight"] == 0).any()
    routes = {"build_device": {}, "offsets_host": dict(offsets_host=b["off"]), "device plan": dict(max_len=4096),
              "Plan": dict(plan=batch.Plan.build(b["off"], _dev()))}
    for what, kw in routes.items():
        res = _run(b, check=True, **kw)
        _same(_host(res), exp, what)
        _full_is_the_consensus(b, res, what)
        bare = _run(b, check=True, full=False, **kw)
        assert bare.full is None
        _same(_host(bare), exp, what + ", no full")
    assert bool(res.full.is_null(_T(b["off"]))[0]) and float(res.full.total_weight[0]) == 0.0  # the empty market
    N.check_faults(_dev(), "edge lengths")


def test_each_edge_length_alone_in_one_launch(edges):
    """One market per call through the unplanned entry: the short kernel of every width and the
    long kernel of every LDS size, with max_len exactly the market's length and one more; the
    full_* outputs requested and not."""
    b, exp = edges
    table = _table(b)
    for m, n in enumerate(EDGE_LENS):
        if n == 0:
            continue
        a = int(b["off"][m])
        one = dict(b, off=np.array([0, n], np.int64), sid=b["sid"][a:a + n], prob=b["prob"][a:a + n])
        off, sid, prob = _T(one["off"]), _T(one["sid"]), _T(one["prob"])
        own = batch.consensus(off, sid, prob, table, check=True)
        for max_len in {n, min(4096, n + 1)}:
            for want_full in (True, False):
                out = batch.LeaveOneOutResult.alloc(n, _dev(), n_markets=1 if want_full else None)
                _raw(off, 1, sid, prob, table, None, max_len, out, out.full)
                got = _host(out)
                for k in FIELDS:
                    assert np.array_equal(got[k], exp[k][a:a + n]), (n, max_len, want_full, k)
                    assert not want_full or torch.equal(getattr(out.full, k), getattr(own, k)), (n, max_len, k)
    N.check_faults(_dev(), "single markets")


# ----------------------------------------------------------------------------- orderings
def test_orderings_that_stress_the_sort_the_runs_and_the_skip():
    S = 5000
    rng = np.random.default_rng(3)
    rel, conf = rng.uniform(0.05, 1.0, S), rng.random(S)
    markets = {
        "4096 distinct, descending": 4500 - np.arange(4096),
        "4096 of one source": np.full(4096, 17),
        "two sources alternating, 65": np.where(np.arange(65) % 2 == 0, 900, 30),
        "two sources alternating, 4096": np.where(np.arange(4096) % 2 == 0, 31, 2000),
        # sorted order: 60 singles, a run of 9 across sorted positions 60..68, 61 singles; arrival shuffled
        "a run across the 64 boundary": rng.permutation(np.concatenate([np.arange(60), np.full(9, 100),
                                                                          200 + np.arange(61)])),
        "duplicates in 64": rng.integers(0, 12, 64),
        "duplicates in 65": rng.integers(0, 12, 65),
        "first and last, 40": rng.integers(100, 130, 40),
        "first and last, 300": rng.integers(100, 400, 300),
    }
    lens = [len(v) for v in markets.values()]
    sid = np.concatenate(list(markets.values())).astype(np.int32)
    b = dict(off=_offsets(lens), sid=sid, prob=rng.random(len(sid)), rel=rel, conf=conf, present=np.ones(S, np.uint8))
    exp = _expected(b)
    at = dict(zip(markets, zip(b["off"][:-1], b["off"][1:])))
    a0, a1 = at["4096 distinct, descending"]
    assert (exp["n_unique"][a0:a1] == 4095).all() and len(set(exp["consensus"][a0:a1])) > 4000
    a0, a1 = at["4096 of one source"]
    assert (exp["total_weight"][a0:a1] == 0).all() and (exp["n_unique"][a0:a1] == 0).all()
    for what, kw in (("host plan", dict(offsets_host=b["off"])), ("device plan", dict(max_len=4096))):
        res = _run(b, check=True, **kw)
        got = _host(res)
        _same(got, exp, what)
        _full_is_the_consensus(b, res, what)
        for name in ("first and last, 40", "first and last, 300"):  # the left-out source sorts first / last
            a0, a1 = at[name]
            s = sid[a0:a1]
            for p in (a0 + int(np.argmin(s)), a0 + int(np.argmax(s))):
                assert all(got[k][p] == exp[k][p] for k in FIELDS) and got["total_weight"][p] > 0, (name, p)
    # the only weighted source among zero-weight ones: without it the consensus is None; without a
    # zero-weight source it is the full consensus, bit for bit
    for n in (9, 64, 65, 700):
        z = dict(b, off=_offsets([n]), sid=rng.integers(0, 40, n).astype(np.int32), prob=rng.random(n),
                 rel=np.where(np.arange(S) == 23, 0.7, 0.0))
        z["sid"][[1, n // 2, n - 1]] = 23
        res = _run(z, offsets_host=z["off"], check=True)
        got = _host(res)
        _same(got, _expected(z), f"one weighted source, {n}")
        full = {k: getattr(res.full, k).cpu().numpy()[0] for k in FIELDS}
        mine = z["sid"] == 23
        assert (got["total_weight"][mine] == 0).all() and (got["consensus"][mine] == 0).all()
        for k in ("consensus", "confidence", "total_weight"):
            assert (got[k][~mine] == full[k]).all() and full[k] != 0, (n, k)
        assert (got["n_unique"] == full["n_unique"] - 1).all()
    N.check_faults(_dev(), "orderings")


# ----------------------------------------------------------------------------- short markets in bulk
def test_short_markets_in_bulk():
    rng = np.random.default_rng(2)
    for top, count in ((8, 3000), (16, 1500), (32, 1500), (64, 1000)):  # every G; several markets per wave
        b = _batch(rng.integers(0, top + 1, count), 7, 20 + top, p_cold=0.0, p_zero=0.2)
        exp = _expected(b)
        res = _run(b, max_len=top, check=True)
        _same(_host(res), exp, f"0..{top} in one launch")
        _full_is_the_consensus(b, res, f"0..{top}")
        _same(_host(_run(b, offsets_host=b["off"], check=True, full=False)), exp, f"0..{top} host lengths")
    both = _batch(np.concatenate([rng.integers(0, 9, 2000), rng.integers(0, 65, 1000)]), 40, 5, p_cold=0.0)
    exp = _expected(both)
    for what, kw in (("planned", {}), ("one launch", dict(max_len=64)), ("device plan", dict(max_len=100))):
        res = _run(both, check=True, **kw)
        _same(_host(res), exp, what)
        _full_is_the_consensus(both, res, what)
    N.check_faults(_dev(), "bulk")


# ----------------------------------------------------------------------------- market list
def test_market_list_leaves_every_other_market_untouched():
    rng = np.random.default_rng(8)
    lens = np.concatenate([rng.integers(0, 70, 200), [65, 300, 1000, 0, 64]])
    M = len(lens)
    b = _batch(lens, 50, 9)
    exp = _expected(b)
    own = batch.consensus(_T(b["off"]), _T(b["sid"]), _T(b["prob"]), _table(b), check=True)
    own = {k: getattr(own, k).cpu().numpy() for k in FIELDS}
    listed = np.union1d(np.sort(rng.choice(M, 60, replace=False)), [200, 202, 203])
    n = len(b["sid"])

    def check(out, members, what):
        mine = np.zeros(n, bool)
        for m in members:
            mine[b["off"][m]:b["off"][m + 1]] = True
        got = _host(out)
        _same(got, exp, what, mine)
        _untouched(got, ~mine, what)
        inlist = np.zeros(M, bool)
        inlist[members] = True
        full = {k: getattr(out.full, k).cpu().numpy() for k in FIELDS}
        _same(full, own, what + ", full", inlist)
        _untouched(full, ~inlist, what + ", full")

    out = _sentinels(n, M)
    _run(b, plan=batch.Plan.for_markets(b["off"], listed, _dev()), out=out, check=True)
    check(out, listed, "listed")
    # the same through the C entry's plain list: one launch sized by max_len
    short = listed[lens[listed] <= 64]
    out = _sentinels(n, M)
    _raw(_T(b["off"]), M, _T(b["sid"]), _T(b["prob"]), _table(b), _T(short.astype(np.int32)), 64, out, out.full)
    check(out, short, "plain list")
    N.check_faults(_dev(), "market list")


# ----------------------------------------------------------------------------- large table
def test_large_table_uses_the_whole_sid():
    """2^20 + 8 rows: the sid takes more than 16 bits, in either kernel."""
    S = (1 << 20) + 8
    small = _batch((40, 300), 8, 10, p_zero=0.0)
    exp = _expected(small)  # the top 8 rows hold the small table: same order, same values
    relconf = torch.zeros((S, 2), dtype=torch.float64, device=_dev())
    relconf[S - 8:, 0] = _T(small["rel"])
    relconf[S - 8:, 1] = _T(small["conf"])
    bits = torch.zeros((S + 31) // 32, dtype=torch.int32, device=_dev())
    table = batch.SourceTable(relconf, bits, range(S))
    assert table.n == S
    sid = _T((small["sid"].astype(np.int64) + (S - 8)).astype(np.int32))
    for kw in (dict(offsets_host=small["off"]), dict(max_len=512)):
        res = batch.leave_one_out(_T(small["off"]), sid, _T(small["prob"]), table, check=True, **kw)
        _same(_host(res), exp, f"large table {kw}")


# ----------------------------------------------------------------------------- rejection
def test_too_long_markets_and_bad_sids_are_reported():
    b = _batch((5, 4097, 3), 10, 11)
    args = (_T(b["off"]), _T(b["sid"]), _T(b["prob"]), _table(b))
    N.check_faults(_dev(), "clean slate")
    with pytest.raises(ValueError, match="market 1 has 4097 signals"):
        batch.leave_one_out(*args, offsets_host=b["off"])
    with pytest.raises(ValueError, match="market 1 has 4097 signals"):
        batch.leave_one_out(*args)  # Plan.build_device: the host learns the lengths
    with pytest.raises(ValueError, match="market 1 has 4097 signals"):
        batch.leave_one_out(*args, plan=batch.Plan.build(b["off"], _dev()))
    N.check_faults(_dev(), "refused on the host")
    # a bound without host lengths: the market is left untouched and the fault word raised
    for lens, bound, who in (((5, 70, 3, 64), 64, "one launch"), ((5, 4097, 3, 64), 4096, "device plan")):
        b = _batch(lens, 10, 12)
        n = len(b["sid"])
        long_ = np.zeros(n, bool)
        long_[5:5 + lens[1]] = True
        rest = dict(b, off=_offsets((5, 0, 3, 64)), sid=b["sid"][~long_], prob=b["prob"][~long_])
        out = _sentinels(n, 4)
        _run(b, max_len=bound, out=out)
        with pytest.raises(N.BCEError):
            N.check_faults(_dev(), who)
        got = _host(out)
        _untouched(got, long_, who)
        _same({k: got[k][~long_] for k in FIELDS}, _expected(rest), who)
        full = {k: getattr(out.full, k).cpu().numpy() for k in FIELDS}
        _untouched(full, np.array([False, True, False, False]), who + ", full")
        own = orc.consensus_csr(rest["off"], rest["sid"], rest["prob"], b["rel"], b["conf"], b["present"])
        _same(full, {k: own[k] for k in FIELDS}, who + ", full", np.array([0, 2, 3]))
    N.check_faults(_dev(), "fault word is cleared")
    # a sid outside the table: its row read is clamped, the sid fault raised
    b = _batch((5, 70, 3), 10, 13)
    for bad in (10, -1, 2 ** 31 - 1):
        for where in (2, 40):
            sid = b["sid"].copy()
            sid[where] = bad
            res = _run(dict(b, sid=sid), offsets_host=b["off"])
            with pytest.raises(N.BCEError, match="sid"):
                N.check_faults(_dev(), "bad sid")
            exp = _expected(dict(b, sid=np.where(np.arange(len(sid)) == where, 9, sid).astype(np.int32)))
            _same(_host(res), exp, f"clamped {bad}")
    N.check_faults(_dev(), "fault word is cleared")


# G lanes per market: the first 64 / G markets share the first wave; the too-long one is not its first
SAME_WAVE_LENS = {8: (5, 8, 9, 3, 0, 1, 8, 7, 2, 8, 6, 4), 16: (16, 17, 0, 9, 1, 16, 12, 3, 15, 2, 16, 8)}


@pytest.mark.parametrize("G", sorted(SAME_WAVE_LENS))
def test_too_long_market_shares_a_wave_with_valid_ones(G):
    """A dozen markets under max_len = G: one wave of the short kernel holds a too-long market (not
    its first), an empty one and valid ones.  The neighbours (their ``full`` rows too) are
    bit-exact, the too-long market keeps what ``out`` held, and the fault word reads kFaultTooLong
    (4)."""
    lens = SAME_WAVE_LENS[G]
    bad = int(np.argmax(np.array(lens) > G))
    per_wave = 64 // G
    assert 0 < bad < per_wave and 0 in lens[:per_wave] and sum(0 < x <= G for x in lens[:per_wave]) >= 2
    b = _batch(lens, 10, 20 + G)
    n = len(b["sid"])
    long_ = np.zeros(n, bool)
    long_[b["off"][bad]:b["off"][bad + 1]] = True
    rest = dict(b, off=_offsets([0 if m == bad else x for m, x in enumerate(lens)]), sid=b["sid"][~long_],
                prob=b["prob"][~long_])
    out = _sentinels(n, len(lens))
    N.check_faults(_dev(), "clean slate")
    _run(b, max_len=G, out=out)
    with pytest.raises(N.BCEError, match="device fault 4"):
        N.check_faults(_dev(), "too long in the wave")
    got = _host(out)
    _untouched(got, long_, "same wave")
    _same({k: got[k][~long_] for k in FIELDS}, _expected(rest), "same wave")
    full = {k: getattr(out.full, k).cpu().numpy() for k in FIELDS}
    is_bad = np.arange(len(lens)) == bad
    _untouched(full, is_bad, "same wave, full")
    own = orc.consensus_csr(rest["off"], rest["sid"], rest["prob"], b["rel"], b["conf"], b["present"])
    _same(full, {k: own[k] for k in FIELDS}, "same wave, full", ~is_bad)
    N.check_faults(_dev(), "fault word is cleared")


# ----------------------------------------------------------------------------- walks
def _walk_fixture(golden_dir, name):
    from bayesian_engine.timeutil import iso_to_us

    g = json.load(open(os.path.join(golden_dir, name)))
    names = g["names"]
    S = len(names)
    off, sid, prob, outcome = [0], [], [], []
    for mk in g["markets"]:
        for s, p in mk["signals"]:
            sid.append(s)
            prob.append(float(p))
        off.append(len(sid))
        outcome.append(-1 if mk["outcome"] is None else int(mk["outcome"]))
    rel, conf = np.full(S, 0.5), np.full(S, 0.25)
    t_us, present = np.full(S, orc.NO_TIMESTAMP, np.int64), np.zeros(S, np.uint8)
    for nm, r, c, ts in g["seeds"]:
        s = names.index(nm)
        rel[s], conf[s], t_us[s], present[s] = float(r), float(c), iso_to_us(ts), 1
    csr = (_T(np.array(off, np.int64)), _T(np.array(sid, np.int32)), _T(np.array(prob)))
    return g, csr, _T(np.array(outcome, np.int8)), S, (rel, conf, t_us, present)


def _rtable(state):
    rel, conf, t_us, present = state
    return batch.ReliabilityTable(_T(rel), _T(conf), _T(t_us), _T(present), [""] * len(rel))


@pytest.mark.parametrize("name", ["walk_forward_small.json", "walk_lag_small.json"])
def test_walk_leave_one_out_on_the_walk_fixtures(golden_dir, name):
    g, (off, sid, prob), outcome, S, state = _walk_fixture(golden_dir, name)
    if "forecast_times_us" in g:
        resolve = [0 if t is None else t for t in g["resolve_times_us"]]
        plan = batch.WalkPlan.build_lagged(off, sid, prob, outcome, S, _T(np.array(g["forecast_times_us"], np.int64)),
                                           _T(np.array(resolve, np.int64)))
        times = ()
    else:
        plan = batch.WalkPlan.build(off, sid, prob, outcome, S)
        times = (_T(np.array(g["times_us"], np.int64)),)
    table = _rtable(state)
    loo = batch.walk_leave_one_out(plan, table, *times, offsets=off, prob=prob, check=True)
    wt, _ = batch.walk_trace(plan, _rtable(state), *times)
    direct = batch.leave_one_out(off, plan.pairs.esid, prob, wt, check=True)
    walk = batch.walk_forward(plan, _rtable(state), *times, offsets=off, prob=prob, commit=False)
    for k in FIELDS:
        assert torch.equal(getattr(loo, k), getattr(direct, k)), k
        assert torch.equal(getattr(loo.full, k), getattr(direct.full, k)), k
        assert torch.equal(getattr(loo.full, k), getattr(walk, k)), k
    for x, before in zip((table.rel, table.conf, table.t_us, table.present), state):  # nothing is committed
        assert x.cpu().numpy().tobytes() == np.asarray(before, x.cpu().numpy().dtype).tobytes()
    # the entry table against the oracle, signal by signal
    E = plan.pairs.n_entries
    b = dict(off=off.cpu().numpy(), sid=plan.pairs.esid.cpu().numpy(), prob=prob.cpu().numpy(),
             rel=wt.relconf[:E, 0].cpu().numpy().copy(), conf=wt.relconf[:E, 1].cpu().numpy().copy(),
             present=np.ones(E, np.uint8))
    _same(_host(loo), _expected(b), name)
    # ... and the reference's own numbers for every market's full consensus
    full = {k: getattr(loo.full, k).cpu().numpy() for k in FIELDS}
    for m, r in enumerate(g["results"]):
        assert (r["consensus"] is None) == bool(full["total_weight"][m] == 0), m
        assert r["consensus"] is None or repr(float(full["consensus"][m])) == r["consensus"], m
        assert repr(float(full["confidence"][m])) == r["confidence"], m
    N.check_faults(_dev(), name)


# ----------------------------------------------------------------------------- scoring
def _same_score(r, ref, what):
    torch.cuda.synchronize()
    for k in ("counts", "sums", "bin_n", "bin_pos", "bin_psum"):
        g = getattr(r, k).cpu().numpy()
        e = ref[k] if isinstance(ref, dict) else getattr(ref, k).cpu().numpy()
        assert g.shape == e.shape and np.array_equal(g, e), (what, k)


def test_score_leave_one_out_both_modes():
    rng = np.random.default_rng(14)
    lens = rng.integers(0, 7, 2500)
    M, S = len(lens), 8
    b = _batch(lens, S, 15, p_zero=0.3)
    b["sid"][b["off"][:-1][lens > 0]] = 0  # source 0 opens every market: a group longer than a score segment
    off, sid = _T(b["off"]), _T(b["sid"])
    loo = batch.leave_one_out(off, sid, _T(b["prob"]), _table(b), offsets_host=b["off"], check=True)
    exp = _expected(b)
    own = orc.consensus_csr(b["off"], b["sid"], b["prob"], b["rel"], b["conf"], b["present"])
    outcome = rng.choice(np.array([-1, 0, 1], np.int8), M, p=[0.15, 0.45, 0.4])
    market = np.repeat(np.arange(M), lens)
    full_null = (own["total_weight"] == 0) | (lens == 0)
    valid = (exp["total_weight"] != 0) & ~full_null[market]
    assert (~valid).sum() > 50 and (exp["total_weight"] == 0).sum() > 20
    pos = np.arange(len(market)) - b["off"][:-1][market]
    for per in ("pair", "signal"):
        lists = []
        for s in range(S):
            mine = np.flatnonzero(b["sid"] == s)
            if per == "pair":  # the source's first signal in every market
                earlier = np.array([(b["sid"][p - pos[p]:p] == s).any() for p in mine], bool)
                mine = mine[~earlier]
            lists.append(mine)
        assert len(lists[0]) > batch.SCORE_SEG if per == "pair" else True
        goff = _offsets([len(x) for x in lists])
        pidx = np.concatenate(lists)
        got = batch.score_leave_one_out(loo, off, sid, _T(outcome), S, per=per)
        ref = score_ref(dict(goff=goff, pidx=pidx, oidx=None, value=exp["consensus"], outcome=outcome[market],
                             valid=valid, base=own["consensus"][market], B=10, eps=1e-15))
        _same_score(got, ref, per)
        by_hand = batch.score(batch.ScorePlan.groups(_T(goff), _T(pidx)), _T(exp["consensus"]), _T(outcome[market]),
                              valid=_T(valid), base=_T(own["consensus"][market]))
        _same_score(got, by_hand, per + ", by hand")
        assert got.has_base and got.skill.shape == (S,)
    inf = loo.influence(off).cpu().numpy()
    want = np.where(valid, own["consensus"][market] - exp["consensus"], np.nan)
    assert np.array_equal(inf, want, equal_nan=True)
    N.check_faults(_dev(), "score_leave_one_out")


# ----------------------------------------------------------------------------- drop-in layer
FIELDS_OF_ROW = ["sourceId", "consensus", "confidence", "totalWeight", "sourceCount", "influence"]


def _row_of(name, res, full):
    cons = res["consensus"]
    fc = full["consensus"]
    return {"sourceId": name, "consensus": cons, "confidence": res["confidence"],
            "totalWeight": res["normalization"]["totalWeight"], "sourceCount": res["normalization"]["sourceCount"],
            "influence": None if cons is None or fc is None else fc - cons}


def test_market_leave_one_out_against_the_fixture_and_the_reduced_calls(golden_dir):
    from bayesian_engine.core import compute_consensus
    from bayesian_engine.market import Market, MarketId, MarketStore

    g = load_fixture(golden_dir)[0]
    table = fixture_table(g)
    store = MarketStore()
    for i, mk in enumerate(g["markets"]):
        market = store.create_market(MarketId(f"l:m{i}"))
        for name, p in mk["signals"]:
            market.add_signal({"sourceId": name, "probability": float(p)})
        got = market.leave_one_out(table)
        assert market.consensus_result is None and len(got) == len(mk["leave_out"])
        full = compute_consensus(market.signals, table)
        for row, r in zip(got, mk["leave_out"]):
            assert list(row) == FIELDS_OF_ROW and row["sourceId"] == r["sourceId"]
            assert (None if row["consensus"] is None else repr(row["consensus"])) == r["consensus"], (i, r)
            assert (repr(row["confidence"]), repr(row["totalWeight"]), row["sourceCount"]) == \
                (r["confidence"], r["totalWeight"], r["sourceCount"]), (i, r)
            rest = [s for s in market.signals if s["sourceId"] != r["sourceId"]]
            assert row == _row_of(r["sourceId"], compute_consensus(rest, table), full), (i, r)
            assert type(row["sourceCount"]) is int and type(row["totalWeight"]) is float
    assert Market(id=MarketId("l:none")).leave_one_out() == []
    # all open markets in one batch, cold-start table: the per-market calls
    store.get_market(MarketId("l:m3")).resolve(True)  # not open: left out
    everything = store.compute_all_leave_one_out()
    assert list(everything) == [f"l:m{i}" for i in range(len(g["markets"])) if i != 3]
    assert everything["l:m0"] == []
    for key, rows in everything.items():
        market = store.get_market(MarketId(key))
        assert rows == market.leave_one_out(), key
        assert market.consensus_result is None
    N.check_faults(_dev(), "market leave-one-out")


def test_store_leave_one_out_on_market_cases():
    """compute_all_leave_one_out with a reliability store, against per-market calls: every reduced
    market computed on its own, in a store of its own, from the same rows at the same "now"."""
    import bayesian_engine.decay as dmod
    from bayesian_engine.market import MarketId, MarketStatus, MarketStore
    from bayesian_engine.reliability import SQLiteReliabilityStore

    epoch = datetime(1970, 1, 1, tzinfo=timezone.utc)
    seen = 0
    for case in load_json("market_cases.json"):
        store = SQLiteReliabilityStore(":memory:")
        for row in case["rows"]:
            store._conn.execute("INSERT INTO sources VALUES (?,?,?,?,?)", tuple(row))
        ms = MarketStore()
        for mk in case["markets"]:
            m = ms.create_market(MarketId(mk["marketId"]))
            for s in mk["signals"]:
                m.add_signal(s)
            if mk["resolved"]:
                m.resolve(True)
        now = epoch + timedelta(microseconds=case["now_us"])

        class _Frozen(datetime):
            @classmethod
            def now(cls, tz=None):
                return now

        old = dmod.datetime
        dmod.datetime = _Frozen
        try:
            got = ms.compute_all_leave_one_out(store)
            assert all(m.consensus_result is None for m in ms.list_markets())
            cold = ms.compute_all_leave_one_out(None)
            everything = ms.compute_all_consensus(store)
            for m in ms.list_markets(status=MarketStatus.OPEN):
                key = str(m.id)
                assert cold[key] == m.leave_one_out(), key
                full = everything[key]
                ids = sorted({s["sourceId"] for s in m.signals})
                assert [r["sourceId"] for r in got[key]] == ids, key
                for row in got[key]:
                    alone = MarketStore()
                    reduced = alone.create_market(MarketId(key))
                    for s in m.signals:
                        if s["sourceId"] != row["sourceId"]:
                            reduced.add_signal(s)
                    res = alone.compute_all_consensus(store)[key]
                    if not reduced.signals:  # core.py:88-96
                        res = dict(res, normalization={"totalWeight": 0.0, "sourceCount": 0})
                    assert row == _row_of(row["sourceId"], res, full), (key, row)
                    seen += 1
        finally:
            dmod.datetime = old
        assert list(got) == [str(m.id) for m in ms.list_markets(status=MarketStatus.OPEN)]
        store.close()
    assert seen > 60
    N.check_faults(_dev(), "market cases")


def test_source_influence_against_score_leave_one_out():
    from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore, SourceScore

    rng = np.random.default_rng(21)
    ms = MarketStore()
    names = [f"s{i}" for i in range(7)]
    lens = rng.integers(0, 9, 60)
    lens[:3] = (0, 1, 8)
    for i, n in enumerate(lens):
        m = ms.create_market(MarketId(("x:" if i % 3 else "y:") + f"m{i}"))
        for _ in range(n):
            m.add_signal({"sourceId": names[int(rng.integers(0, 7))], "probability": float(rng.random())})
        if i % 4:
            m.resolve(bool(rng.random() < 0.5))
    agg = CrossMarketAggregator(ms)
    for patterns in (None, ["x:*"]):
        got = agg.source_influence(patterns)
        markets = [m for m in ms.list_markets() if m.signals and (patterns is None or str(m.id).startswith("x:"))]
        order = {}
        for m in markets:
            for s in m.signals:
                order.setdefault(s["sourceId"], len(order))
        assert list(got) == list(order) and all(isinstance(v, SourceScore) for v in got.values())
        # the same arrays by hand: ranks over (market, sorted sourceId), the cold-start table
        off = _offsets([len(m.signals) for m in markets])
        esid, gsid, base = [], [], 0
        for m in markets:
            ids = sorted({s["sourceId"] for s in m.signals})
            esid += [base + ids.index(s["sourceId"]) for s in m.signals]
            gsid += [order[s["sourceId"]] for s in m.signals]
            base += len(ids)
        prob = np.array([s["probability"] for m in markets for s in m.signals])
        code = np.array([(1 if m.outcome else 0) if m.outcome is not None else -1 for m in markets], np.int8)
        table = batch.SourceTable.from_arrays(_T(np.full(base, 0.5)), _T(np.full(base, 0.25)),
                                              _T(np.zeros(base, np.uint8)))
        loo = batch.leave_one_out(_T(off), _T(np.array(esid, np.int32)), _T(prob), table, offsets_host=off, check=True)
        ss = batch.score_leave_one_out(loo, _T(off), _T(np.array(gsid, np.int32)), _T(code), len(order), per="pair")
        for i, name in enumerate(order):
            v = got[name]
            want = (name, int(ss.n_scored[i]), float(ss.brier[i]), float(ss.log_loss[i]), float(ss.accuracy[i]),
                    float(ss.skill[i]))
            assert np.array_equal(np.array((v.n, v.brier, v.log_loss, v.accuracy, v.skill)), np.array(want[1:]),
                                  equal_nan=True) and v.source_id == name, name
        assert sum(v.n for v in got.values()) > 30
    assert agg.source_influence(["nothing:*"]) == {}
    N.check_faults(_dev(), "source influence")
