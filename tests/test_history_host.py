"""CPU checks of the consensus history: the restatement the kernels follow
(tests/history_ref.py) against the fixture recorded from the reference and against the oracle on
the expanded batch; ``history_at`` and the item lists of ``score_history`` on CPU tensors; the
argument checks of bce_consensus_history, which need no GPU."""
import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from history_ref import FIELDS, expand, fixture_points, history_ref, load_fixture
from oracle import oracle as orc
from score_ref import score_ref


def _oracle_points(off, sid, prob, rel, conf, present):
    off2, sid2, prob2 = expand(off, sid, prob)
    exp = orc.consensus_csr(off2, sid2, prob2, rel, conf, present)
    return {k: exp[k] for k in FIELDS}


def _issue_batch():
    """11 markets of lengths 0, 1, 2, 7, 31, 32, 33, 63, 64, 65, 100 over 9 sources with repeats, two
    of reliability 0.0, 5% of the probabilities at 1.25, one market opening with zero-weight sources."""
    rng = np.random.default_rng(7)
    lens = np.array([0, 1, 2, 7, 31, 32, 33, 63, 64, 65, 100])
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    sid = rng.integers(0, 9, n).astype(np.int32)
    sid[off[3]:off[3] + 3] = (2, 5, 2)  # the 7-signal market opens with zero-weight sources only
    prob = rng.random(n)
    prob[rng.random(n) < 0.05] = 1.25
    rel, conf = rng.uniform(0.1, 1.0, 9), rng.random(9)
    rel[[2, 5]] = 0.0
    return off, sid, prob, rel, conf, np.ones(9, np.uint8)


def test_restatement_equals_the_reference_fixture(golden_dir):
    g, off, sid, prob, rel, conf, _ = load_fixture(golden_dir)
    got = history_ref(off, sid, prob, rel, conf)
    points = fixture_points(g)
    assert len(points) == len(sid) == 112
    nulls = 0
    for p, (cons, confd, tot, count) in enumerate(points):
        null = cons is None
        nulls += null
        assert null == (got["total_weight"][p] == 0.0), p
        assert (got["consensus"][p] == 0.0) if null else (repr(float(got["consensus"][p])) == cons), p
        assert repr(float(got["confidence"][p])) == confd, p
        assert repr(float(got["total_weight"][p])) == tot, p
        assert int(got["n_unique"][p]) == count, p
    assert nulls == 8


def test_restatement_equals_the_oracle_on_the_expanded_batch(golden_dir):
    batches = [load_fixture(golden_dir)[1:], _issue_batch()]
    for off, sid, prob, rel, conf, present in batches:
        got = history_ref(off, sid, prob, rel, conf)
        exp = _oracle_points(off, sid, prob, rel, conf, present)
        for k in FIELDS:
            assert np.array_equal(got[k], exp[k]), k
    assert (got["total_weight"] == 0).sum() >= 3 and len(sid) == 398  # at least the zero-weight opening


def test_expand():
    off = np.array([0, 3, 3, 5], np.int64)
    off2, sid2, prob2 = expand(off, np.array([7, 8, 9, 1, 2], np.int32), np.arange(5.0))
    assert off2.tolist() == [0, 1, 3, 6, 7, 9]
    assert sid2.tolist() == [7, 7, 8, 7, 8, 9, 1, 1, 2]
    assert prob2.tolist() == [0, 0, 1, 0, 1, 2, 3, 3, 4]


# ---------------------------------------------------------------------------------- history_at
OFF = torch.tensor([0, 3, 3, 5, 6])
ARRIVAL = torch.tensor([10, 50, 90, 20, 20, 70])


def test_history_at_per_market():
    before = batch.history_at(OFF, ARRIVAL, torch.tensor([9, 0, 19, 69]))
    assert before.dtype == torch.int64 and before.tolist() == [-1, -1, -1, -1]
    exactly = batch.history_at(OFF, ARRIVAL, torch.tensor([50, 50, 20, 70]))
    assert exactly.tolist() == [1, -1, 4, 5]  # equal arrivals: the last of them
    after = batch.history_at(OFF, ARRIVAL, torch.tensor([1000, 1000, 21, 71]))
    assert after.tolist() == [2, -1, 4, 5]
    between = batch.history_at(OFF, ARRIVAL, torch.tensor([89, 5, 20, 0]))
    assert between.tolist() == [1, -1, 4, -1]


def test_history_at_grid_and_long_markets():
    at = torch.tensor([[9, 10, 11, 90], [0, 1, 2, 3], [19, 20, 21, 22], [69, 70, 71, 10 ** 9]])
    assert batch.history_at(OFF, ARRIVAL, at).tolist() == [[-1, 0, 0, 2], [-1] * 4, [-1, 4, 4, 4], [-1, 5, 5, 5]]
    rng = np.random.default_rng(3)
    lens = np.array([0, 1, 2, 3, 4, 5, 127, 128, 129, 1000, 0])
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    arrival = np.concatenate([np.sort(rng.integers(0, 500, n)) for n in lens])
    at = rng.integers(-5, 510, (len(lens), 9))
    got = batch.history_at(torch.from_numpy(off), torch.from_numpy(arrival), torch.from_numpy(at)).numpy()
    for m in range(len(lens)):
        for k in range(at.shape[1]):
            n = int((arrival[off[m]:off[m + 1]] <= at[m, k]).sum())
            assert got[m, k] == (off[m] + n - 1 if n else -1), (m, k)
    none = batch.history_at(torch.tensor([0, 0]), torch.zeros(0, dtype=torch.int64), torch.tensor([5]))
    assert none.tolist() == [-1]


def test_history_at_refuses_decreasing_arrivals():
    down = ARRIVAL.clone()
    down[2] = 49
    with pytest.raises(ValueError, match="signal 2 \\(market 0\\)"):
        batch.history_at(OFF, down, torch.tensor([0, 0, 0, 0]))
    assert batch.history_at(OFF, down, torch.tensor([0, 0, 0, 0]), check=False).shape == (4,)
    # a drop from one market to the next is no error: 90 -> 20 and 20 -> 70 stand in ARRIVAL
    batch.history_at(OFF, ARRIVAL, torch.tensor([0, 0, 0, 0]))
    with pytest.raises(ValueError, match="at_us"):
        batch.history_at(OFF, ARRIVAL, torch.tensor([0, 0, 0]))
    with pytest.raises(ValueError, match="arrival_us"):
        batch.history_at(OFF, ARRIVAL.int(), torch.tensor([0, 0, 0, 0]))


# ------------------------------------------------------------------------- score_history's items
def test_history_items_against_score_ref():
    """The item lists of score_history(points=None), scored by tests/score_ref.py, equal the
    plain statement: per group, every member market's points in member, then position order."""
    rng = np.random.default_rng(5)
    lens = np.array([3, 0, 5, 1, 4, 2])
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    goff = np.array([0, 3, 3, 8], np.int64)
    members = np.array([4, 1, 0, 5, 5, 2, 0, 3], np.int64)  # an empty group, a duplicate, an overlap
    plan = batch.ScorePlan.groups(torch.from_numpy(goff), torch.from_numpy(members))
    items = batch._history_items(torch.from_numpy(off), plan)
    want, want_off = [], [0]
    for g in range(len(goff) - 1):
        for m in members[goff[g]:goff[g + 1]]:
            want += list(range(off[m], off[m + 1]))
        want_off.append(len(want))
    assert items.pidx.tolist() == want and items.group_offsets.tolist() == want_off and items.oidx is None
    assert items.n_segments == 3
    market = batch._market_of_point(torch.from_numpy(off), n).numpy()
    assert market.tolist() == np.repeat(np.arange(len(lens)), lens).tolist()
    value = rng.random(n)
    valid = (rng.random(n) < 0.8).astype(np.uint8)
    outcome = np.array([1, 0, -1, 1, 0, 1], np.int8)
    a = score_ref(dict(goff=items.group_offsets.numpy(), pidx=items.pidx.numpy(), oidx=None, value=value,
                       outcome=outcome[market], valid=valid, base=None, B=10, eps=1e-15))
    fx = dict(goff=items.group_offsets.numpy(), pidx=items.pidx.numpy(), oidx=None, value=value,
              outcome=outcome[market], valid=np.ones(n, np.uint8), base=None, B=10, eps=1e-15)
    # the same items scored against the MARKET arrays (oidx = the market of every point)
    b = score_ref(dict(fx, goff=np.array(want_off), pidx=np.array(want, np.int64), oidx=market[want],
                       outcome=outcome, valid=np.ones(len(lens), np.uint8)))
    c = score_ref(fx)
    for k in ("counts", "sums", "bin_n", "bin_pos", "bin_psum"):
        assert np.array_equal(c[k], b[k]), k
    # with the null mask: a null point moves from scored to null, an unresolved one stays unresolved
    assert np.array_equal(a["counts"][:, 2], b["counts"][:, 2])
    assert np.array_equal(a["counts"][:, 0] + a["counts"][:, 3], b["counts"][:, 0])
    assert a["counts"][:, 3].sum() > 0 and a["counts"][1].sum() == 0


# ------------------------------------------------------------------------------ the C entry
def _call(**over):
    a = dict(offsets=1, n_markets=1, sid=1, prob=1, n_signals=1, relconf=16, bits=None, n_sources=1, list=None,
             n_list=0, bins_host=None, bins_dev=None, max_len=8, cons=1, conf=1, tot=1, nu=1, stream=None)
    a.update(over)
    return N.load_library().bce_consensus_history(*a.values())


def test_argument_errors_need_no_gpu():
    """Every refusal comes before anything touches the GPU (the pointers here are never read)."""
    lib = N.load_library()
    assert lib.bce_consensus_history(None, 5, None, None, 0, None, None, 0, None, 0, None, None, 32,
                                     None, None, None, None, None) == -1
    assert b"history" in lib.bce_last_error() and b"offsets" in lib.bce_last_error()
    for over in (dict(offsets=None), dict(sid=None), dict(prob=None), dict(relconf=None), dict(cons=None),
                 dict(conf=None), dict(tot=None), dict(nu=None), dict(n_markets=-1), dict(n_signals=-1),
                 dict(n_sources=-1), dict(n_list=-1), dict(max_len=-1), dict(max_len=4097), dict(relconf=8),
                 dict(bins_host=1), dict(bins_host=1, bins_dev=1, list=1)):
        assert _call(**over) == -1, over
        assert b"history" in lib.bce_last_error(), over
    assert _call(n_markets=0) == 0 and _call(n_signals=0, sid=None, prob=None, cons=None) == 0  # nothing to do


def test_names_are_reachable():
    for name in ("HistoryResult", "consensus_history", "history_at", "score_history", "walk_history",
                 "HISTORY_MAX_LEN"):
        assert getattr(batch, name) is getattr(batch.history, name), name
    assert batch.HISTORY_MAX_LEN == 4096
    assert "bce_consensus_history" in N.EXPORTED
    from bayesian_engine.market import Market, MarketStore
    assert callable(Market.consensus_history) and callable(MarketStore.compute_all_history)
    assert "history" in batch.__doc__.split("listed before it:")[1]


def test_history_result_on_cpu_tensors():
    h = batch.HistoryResult(*(torch.tensor(x, dtype=torch.float64) for x in ([0.5, 0.0, 0.7, 0.2], [0.1, 0.0, 0.3, 0.4],
                                                                                 [1.0, 0.0, 2.0, 3.0])),
                            torch.tensor([1, 1, 2, 1], dtype=torch.int32))
    assert h.is_null().tolist() == [False, True, False, False]
    last = h.last(torch.tensor([0, 2, 2, 3, 4]))
    assert last.consensus.tolist() == [0.0, 0.0, 0.7, 0.2] and last.n_unique.tolist() == [1, 0, 2, 1]
    assert last.total_weight.tolist() == [0.0, 0.0, 2.0, 3.0] and last.n_unique.dtype == torch.int32
    assert last.is_null(torch.tensor([0, 2, 2, 3, 4])).tolist() == [True, True, False, False]
    with pytest.raises(ValueError, match="max_len"):
        batch.consensus_history(torch.tensor([0, 1]), torch.zeros(1, dtype=torch.int32), torch.zeros(1), None,
                                max_len=4097)
    with pytest.raises(ValueError, match="market 1 has 4097 signals"):
        batch.consensus_history(None, None, None, None, offsets_host=np.array([0, 3, 4100, 4101]))
