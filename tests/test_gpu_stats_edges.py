"""bce_agreement_stats (agreement_kernel, csrc/stats.hip) against a reference of its own:
orc.agreement_stats, cross-checked here with np.add.at over (prob >= 0.5) == (outcome != 0).
Counts are integers: every comparison is ==.  Every sid lies in [0, n_sources).
"""
import numpy as np
import pytest

from oracle import oracle as orc

S = 97  # sources: every source collects atomics from many lanes of one wave


def _reference(offsets, sid, prob, outcome, n_sources):
    """(correct, total): the oracle, checked against a numpy restatement of market.py:279-304."""
    correct, total = orc.agreement_stats(offsets, sid, prob, outcome, n_sources)
    lens = np.diff(offsets)
    o = np.repeat(np.asarray(outcome, np.int8), lens)
    n = int(offsets[-1])
    live = o >= 0
    hit = live & ((np.asarray(prob[:n]) >= 0.5) == (o != 0))
    c2, t2 = np.zeros(n_sources, np.int64), np.zeros(n_sources, np.int64)
    np.add.at(t2, sid[:n][live], 1)
    np.add.at(c2, sid[:n][hit], 1)
    assert np.array_equal(correct, c2) and np.array_equal(total, t2)
    return correct, total


def _run(offsets, sid, prob, outcome, n_sources, correct=None, total=None):
    import torch

    from bayesian_engine import batch

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    if correct is not None:
        correct, total = T(correct.astype(np.int32)), T(total.astype(np.int32))
    c, t = batch.agreement_stats(T(offsets), T(sid), T(prob), T(outcome), n_sources, correct, total)
    torch.cuda.synchronize()
    return c.cpu().numpy(), t.cpu().numpy()


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


EDGE_PROBS = np.array([0.5, np.nextafter(0.5, 0.0), np.nan, -0.0, 1.5, -3.0, 0.0, 1.0, np.nextafter(0.5, 1.0)])


def _length_batch():
    """Market lengths around the 64-lane stride, each with outcomes 0, 1 and -1; duplicates of a
    source inside a market (97 sources, up to 1000 signals) count once per signal."""
    rng = np.random.default_rng(97)
    lens = np.repeat([0, 1, 63, 64, 65, 128, 129, 1000], 3)
    outcome = np.tile(np.array([0, 1, -1], np.int8), 8)
    off = _offsets(lens)
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    edge = rng.random(n) < 0.3
    prob[edge] = rng.choice(EDGE_PROBS, int(edge.sum()))
    return off, sid, prob, outcome


@pytest.mark.gpu
def test_agreement_market_lengths_around_the_lane_stride():
    off, sid, prob, outcome = _length_batch()
    exp_c, exp_t = _reference(off, sid, prob, outcome, S)
    assert exp_t.sum() == np.diff(off)[outcome >= 0].sum() and exp_t.max() > 10
    c, t = _run(off, sid, prob, outcome, S)
    assert np.array_equal(t, exp_t) and np.array_equal(c, exp_c)


@pytest.mark.gpu
def test_agreement_probability_edges_against_every_outcome():
    """0.5 predicts true, nextafter(0.5, 0) and NaN predict false; an outcome of 2 reads as true
    (o != 0), -1 skips the market.  One market per (probability, outcome), one source per market,
    so every count is a statement about one comparison."""
    outs = np.array([-1, 0, 1, 2], np.int8)
    P, O = len(EDGE_PROBS), len(outs)
    prob = np.repeat(EDGE_PROBS, O)
    outcome = np.tile(outs, P)
    off = _offsets(np.ones(P * O, np.int64))
    sid = np.arange(P * O, dtype=np.int32)
    exp_c, exp_t = _reference(off, sid, prob, outcome, P * O)
    c, t = _run(off, sid, prob, outcome, P * O)
    assert np.array_equal(t, exp_t) and np.array_equal(c, exp_c)
    # the rule itself, spelled out
    pred = np.array([True, False, False, False, True, False, False, True, True])
    assert np.array_equal(t.reshape(P, O), np.tile(outs >= 0, (P, 1)).astype(np.int32))
    assert np.array_equal(c.reshape(P, O), ((pred[:, None] == (outs != 0)[None, :]) & (outs >= 0)[None, :]))


@pytest.mark.gpu
def test_agreement_whole_batch_unresolved_leaves_the_counts_untouched():
    off, sid, prob, _ = _length_batch()
    outcome = np.full(len(off) - 1, -1, np.int8)
    c0, t0 = np.arange(S) * 3 + 1, np.arange(S) * 5 + 2
    c, t = _run(off, sid, prob, outcome, S, c0, t0)
    assert np.array_equal(c, c0) and np.array_equal(t, t0)


@pytest.mark.gpu
def test_agreement_capped_grid_every_wave_strides_twice():
    """M = 2 * 64 * CUs + 37 markets of 0..3 signals: the launch is capped at 16 workgroups of
    four waves per CU, so every wave takes at least two markets."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = 2 * 64 * cus + 37
    rng = np.random.default_rng(cus)
    off = _offsets(rng.integers(0, 4, M))
    n = int(off[-1])
    sid = rng.integers(0, S, n).astype(np.int32)
    prob = rng.random(n)
    prob[::7] = 0.5
    outcome = rng.choice(np.array([-1, 0, 1], np.int8), M)
    exp_c, exp_t = _reference(off, sid, prob, outcome, S)
    c, t = _run(off, sid, prob, outcome, S)
    assert np.array_equal(t, exp_t) and np.array_equal(c, exp_c)


@pytest.mark.gpu
def test_agreement_accumulates_across_calls_and_onto_preloaded_counts():
    off, sid, prob, outcome = _length_batch()
    exp_c, exp_t = _reference(off, sid, prob, outcome, S)
    h = (len(off) - 1) // 2
    a = int(off[h])
    c, t = _run(off[:h + 1], sid[:a], prob[:a], outcome[:h], S)
    assert 0 < t.sum() < exp_t.sum()
    c, t = _run(off[h:] - a, sid[a:], prob[a:], outcome[h:], S, c, t)
    assert np.array_equal(t, exp_t) and np.array_equal(c, exp_c)
    c0, t0 = np.arange(S) * 3 + 1, np.arange(S) * 5 + 2
    c, t = _run(off, sid, prob, outcome, S, c0, t0)
    assert np.array_equal(t, exp_t + t0) and np.array_equal(c, exp_c + c0)
