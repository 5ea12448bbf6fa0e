"""CPU checks of the walk-forward plan's integer half (batch.WalkPlan.order on CPU tensors, no
kernel): the entry list and the queries against a plain numpy restatement, the argument errors,
and the oracle composition the GPU suite compares against (tests/walk_ref.py) against the fixture
recorded from the reference itself."""
import json
import os

import numpy as np
import pytest
import torch

from bayesian_engine import batch
from bayesian_engine.timeutil import NO_TIMESTAMP, iso_to_us
from walk_ref import walk_ref


def _restate(off, sid, outcome, S):
    """(usid, emarket, esid, qstart, qpos, qentry, qlast, slast) by loops over the batch."""
    sid = np.clip(np.asarray(sid, np.int64), 0, S - 1)
    M = len(off) - 1
    usid, emarket, esid = [], [], np.zeros(len(sid), np.int32)
    for m in range(M):
        a, b = off[m], off[m + 1]
        for s in sorted(set(sid[a:b].tolist())):
            for i in range(a, b):
                if sid[i] == s:
                    esid[i] = len(usid)
            usid.append(s)
            emarket.append(m)
    E = len(usid)
    qstart, qpos, qentry = [0], [], []
    qlast, slast = np.full(E, -1, np.int32), np.full(S, -1, np.int64)
    for s in range(S):
        pos, last = 0, -1
        for e in range(E):  # entries ascend by market
            if usid[e] != s:
                continue
            qpos.append(pos)
            qentry.append(e)
            qlast[e] = last
            m = emarket[e]
            if outcome[m] >= 0:
                pos += int((sid[off[m]:off[m + 1]] == s).sum())
                last = m
        qstart.append(len(qpos))
        slast[s] = last
    return (np.array(usid, np.int32), np.array(emarket, np.int32), esid, np.array(qstart, np.int64),
            np.array(qpos, np.int64), np.array(qentry, np.int32), qlast, slast)


def _order(off, sid, prob, outcome, S):
    T = lambda a, dt: torch.tensor(np.asarray(a, dt))  # noqa: E731
    return batch.WalkPlan.order(T(off, np.int64), T(sid, np.int32), T(prob, np.float64), T(outcome, np.int8), S)


def _check(off, sid, outcome, S, n_clamped=0):
    pairs, qstart, qpos, qentry, qlast, slast, nc = _order(off, sid, np.full(len(sid), 0.5), outcome, S)
    usid, emarket, esid, eqstart, eqpos, eqentry, eqlast, eslast = _restate(off, sid, outcome, S)
    E = len(usid)
    assert pairs.n_entries == E and pairs.n_markets == len(off) - 1 and pairs.n_sources == S
    assert np.array_equal(pairs.usid[:E].numpy(), usid) and np.array_equal(pairs.emarket[:E].numpy(), emarket)
    assert np.array_equal(pairs.esid.numpy(), esid)
    for name, got, exp in (("qstart", qstart, eqstart), ("qpos", qpos, eqpos), ("qentry", qentry, eqentry),
                           ("qlast", qlast, eqlast), ("slast", slast, eslast)):
        assert got.numpy().dtype == exp.dtype, name
        assert np.array_equal(got.numpy(), exp), name
    assert nc == n_clamped
    return qpos.numpy(), qlast.numpy()


def test_small_batch_by_hand():
    off = [0, 3, 5, 5, 8]
    sid = [2, 0, 2, 1, 2, 0, 0, 2]
    qpos, qlast = _check(off, sid, [1, -1, 0, 1], 4)
    # source 0: market 0 (1 bit), market 3; source 1: market 1; source 2: markets 0 (2 bits), 1, 3
    assert qpos.tolist() == [0, 1, 0, 0, 2, 2]
    assert qlast.tolist() == [-1, -1, -1, 0, 0, 0]  # by entry


@pytest.mark.parametrize("seed", range(4))
def test_random_batches(seed):
    rng = np.random.default_rng(seed)
    M, S = int(rng.integers(1, 30)), int(rng.integers(1, 12))
    lens = rng.integers(0, 9, M)
    off = np.zeros(M + 1, np.int64)
    off[1:] = np.cumsum(lens)
    sid = rng.integers(0, S, int(off[-1]))
    outcome = rng.integers(-1, 2, M)
    _check(off.tolist(), sid, outcome, S)


def test_edges():
    _check([0, 0], [], [1], 3)                       # one empty market
    _check([0, 2], [1, 1], [-1], 2)                  # M = 1, unresolved
    _check([0, 2, 4], [1, 1, 1, 1], [1, 0], 2)       # duplicates only
    _check([0, 1, 2, 3], [0, 0, 0], [-1, -1, -1], 1)  # no chain at all
    # sids outside [0, S) are clamped and counted, resolved market or not
    _check([0, 2, 4], [0, 7, -3, 1], [1, -1], 2, n_clamped=2)


def test_argument_errors():
    ok = dict(off=[0, 2, 3], sid=[0, 1, 0], prob=[0.5, 0.5, 0.5], outcome=[1, -1], S=2)

    def run(**kw):
        a = {**ok, **kw}
        return _order(a["off"], a["sid"], a["prob"], a["outcome"], a["S"])

    run()
    for bad in (0, -1, 1 << 31, "x"):
        with pytest.raises(ValueError, match="n_sources"):
            run(S=bad)
    with pytest.raises(ValueError, match="one entry per market"):
        run(outcome=[1])
    with pytest.raises(ValueError, match="offsets"):
        run(off=[0, 2, 4])
    with pytest.raises(ValueError, match="offsets"):
        run(off=[0, 3, 2])
    with pytest.raises(ValueError, match="differ in length"):
        run(prob=[0.5])
    with pytest.raises(ValueError, match="int8"):
        batch.WalkPlan.order(torch.tensor([0, 1]), torch.tensor([0], dtype=torch.int32),
                             torch.tensor([0.5], dtype=torch.float64), torch.tensor([1], dtype=torch.int64), 1)


def test_oracle_composition_reproduces_the_reference_fixture(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "walk_forward_small.json")))
    names = g["names"]
    S = len(names)
    off, sid, prob = [0], [], []
    for mk in g["markets"]:
        sid += [s for s, _ in mk["signals"]]
        prob += [float(p) for _, p in mk["signals"]]
        off.append(len(sid))
    outcome = [-1 if mk["outcome"] is None else int(mk["outcome"]) for mk in g["markets"]]
    rel, conf = np.full(S, 0.5), np.full(S, 0.25)
    t_us, present = np.full(S, NO_TIMESTAMP, np.int64), np.zeros(S, np.uint8)
    for name, r, c, ts in g["seeds"]:
        s = names.index(name)
        rel[s], conf[s], t_us[s], present[s] = float(r), float(c), iso_to_us(ts), 1
    assert len(g["markets"]) == 10 and S == 6 and (t_us[present == 1] == NO_TIMESTAMP).sum() == 1
    assert -1 in outcome[1:-1] and len(set(g["times_us"])) < 10 and (np.diff(g["times_us"]) < 0).any()
    exp, state = walk_ref(off, sid, prob, outcome, S, rel, conf, t_us, present, g["times_us"])
    R = lambda x: repr(float(x))  # noqa: E731
    for m, r in enumerate(g["results"]):
        a, u = off[m], int(exp["n_unique"][m])
        assert R(exp["consensus"][m]) == r["consensus"] and R(exp["confidence"][m]) == r["confidence"], m
        assert R(exp["total_weight"][m]) == r["totalWeight"], m
        assert [[R(x), R(y)] for x, y in zip(exp["rel_read"][a:a + u], exp["conf_read"][a:a + u])] == \
            [x[1:] for x in r["read"]], m
        assert [[names[i & 0x7FFFFFFF], R(x), R(y)] for i, x, y in
                zip(exp["usid"][a:a + u], exp["weight"][a:a + u], exp["nweight"][a:a + u])] == r["sourceWeights"], m
    final = {n: (r, c, ts) for n, r, c, ts in g["final"]}
    for s, n in enumerate(names):
        assert (R(state[0][s]), R(state[1][s]), int(state[2][s])) == (*final[n][:2], iso_to_us(final[n][2])), n
