"""CPU: the oracle's orc_aggregate_groups against tests/aggregate_ref.py (the reference's
aggregate_consensus with Python floats, ``sum`` and ``sorted``) on the groups of
tests/test_gpu_aggregate_edges.py, bit for bit, the sign of a zero median included.
"""
import numpy as np
import pytest

from aggregate_ref import aggregate_ref, aggregate_ref_groups, order_sensitive, same_bits
from oracle import oracle as orc
from test_gpu_aggregate_edges import M, SIGNED_ZERO_LISTS, build_batch, check_against, reference


@pytest.mark.parametrize("nonfinite", [False, True], ids=["main", "nonfinite"])
def test_oracle_equals_aggregate_ref_on_the_edge_batch(nonfinite):
    fx = build_batch(nonfinite)
    ref, oracle = reference(nonfinite)
    assert len(fx["names"]) == len(set(fx["names"]))
    check_against(oracle, ref, fx, np.arange(len(fx["names"])), "oracle vs aggregate_ref", ref["median_known"])
    mem = fx["members"][:fx["goff"][-1]]
    assert ((mem < 0) | (mem >= M)).any() == (not nonfinite)  # the out-of-range members are in the main batch


def test_aggregate_ref_signed_zero_lists():
    """The six lists of the issue through aggregate_ref and the oracle: sorted(...)[k // 2]."""
    exp = [-0.0, 0.0, -0.0, -0.0, 0.0, -0.0]
    for lst, e in zip(SIGNED_ZERO_LISTS, exp):
        cons = np.array(lst)
        one = np.ones(len(lst))
        r = aggregate_ref(range(len(lst)), cons, one, one)
        assert same_bits([r["median"]], [e]) and same_bits([sorted(lst)[len(lst) // 2]], [e]), lst
        o = orc.aggregate_groups(np.array([0, len(lst)]), np.arange(len(lst)), cons, one, one.astype(np.uint8))
        assert same_bits(o["median"], [e]), lst


def test_oracle_median_of_random_signed_zero_groups():
    """Zeros of random sign around a few negatives, up to 5001 members: the oracle's order is
    its comparator's (value, then position), not the sort routine's."""
    rng = np.random.default_rng(300)
    cons = np.array([0.0, -0.0, -1.0, 1.0, -5e-324, 5e-324])
    lens = np.concatenate([rng.integers(1, 40, 250), rng.integers(1000, 5002, 49), [5001]])
    goff = np.zeros(len(lens) + 1, np.int64)
    goff[1:] = np.cumsum(lens)
    members = rng.choice(6, int(goff[-1]), p=[0.44, 0.44, 0.05, 0.03, 0.02, 0.02]).astype(np.int64)
    one = np.ones(6)
    ref = aggregate_ref_groups(goff, members, cons, one, one.astype(np.uint8))
    out = orc.aggregate_groups(goff, members, cons, one, one.astype(np.uint8))
    assert same_bits(out["median"], ref["median"])
    zero = ref["median"] == 0
    assert zero.sum() > 200 and 0.2 < np.signbit(ref["median"][zero]).mean() < 0.8


def test_reference_sums_depend_on_member_order():
    """On the reference alone: in at least half of the groups with three or more kept members
    sum(conf) over the reversed list differs, so a kernel that reorders a chain cannot pass."""
    fx = build_batch()
    ref, _ = reference()
    big = [g for g in range(len(fx["names"])) if ref["n_included"][g] >= 3]
    sens = [g for g in big if order_sensitive(fx["members"][fx["goff"][g]:fx["goff"][g + 1]], fx["conf"], fx["has"])]
    assert len(big) >= 100 and 2 * len(sens) >= len(big), (len(sens), len(big))
    lens = [g for g in big if fx["names"][g].startswith("len")]
    assert 2 * sum(g in set(sens) for g in lens) >= len(lens)
