"""CPU pin of the planned launch's schedule (csrc/plan_host.hpp plan_schedule, through
bce_plan_schedule): which launches bce_consensus_planned / bce_consensus_planned_device make for
a plan, in which order, on which stream, and whether the side stream is forked.

The expected rows are literals.  They were printed once by the decision block of
bce_consensus_planned (lo[] merges, few(), merged_away, the three-pass order, the fork
condition) and the kOrderDev loop of bce_consensus_planned_device as they stood before
plan_schedule existed, copied into a stand-alone program with sharding._RESIDENT in place of the
occupancy queries -- not by plan_schedule."""
import numpy as np
import pytest

from bayesian_engine import _native as N
from bayesian_engine.sharding import _RESIDENT, plan_schedule

# (what the case is, mode, markets per bin or None for the device plan,
#  launches (b0, b1, side) in issue order, fork)
CASES = [
    ('every bin full, bin 12 too', 'fast', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 7680, 6144, 3072, 3072, 3],
     [(12, 12, 0), (10, 10, 0), (11, 11, 0), (9, 9, 0), (8, 8, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('every bin full, bin 12 too', 'exact', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 7680, 6144, 3072, 3072, 3],
     [(12, 12, 0), (10, 11, 0), (8, 9, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(8..9) one below 6 x resident[9], all in bin 9', 'fast', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 0, 6143, 3072, 3072, 0],
     [(10, 10, 0), (11, 11, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (8, 9, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(8..9) at 6 x resident[9], all in bin 9', 'fast', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 0, 6144, 3072, 3072, 0],
     [(10, 10, 0), (11, 11, 0), (9, 9, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(8..9) one below 6 x resident[9], all in bin 8', 'fast', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 6143, 0, 3072, 3072, 0],
     [(10, 10, 0), (11, 11, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (8, 9, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(8..9) at 6 x resident[9], all in bin 8', 'fast', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 6144, 0, 3072, 3072, 0],
     [(10, 10, 0), (11, 11, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (8, 8, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(10..11) one below 6 x resident[11], all in bin 11', 'fast', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 7680, 6144, 0, 3071, 0],
     [(9, 9, 0), (8, 8, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (10, 11, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(10..11) at 6 x resident[11], all in bin 11', 'fast', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 7680, 6144, 0, 3072, 0],
     [(11, 11, 0), (9, 9, 0), (8, 8, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(10..11) one below 6 x resident[11], all in bin 10', 'fast', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 7680, 6144, 3071, 0, 0],
     [(9, 9, 0), (8, 8, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (10, 11, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(10..11) at 6 x resident[11], all in bin 10', 'fast', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 7680, 6144, 3072, 0, 0],
     [(10, 10, 0), (9, 9, 0), (8, 8, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(4..6) one below 6 x resident[6]', 'fast', [1000, 1000, 1000, 1000, 8192, 8192, 8191, 12288, 7680, 6144, 3072, 3072, 0],
     [(10, 10, 0), (11, 11, 0), (9, 9, 0), (8, 8, 0), (7, 7, 0), (4, 6, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(4..6) at 6 x resident[6]', 'fast', [1000, 1000, 1000, 1000, 8192, 8192, 8192, 12288, 7680, 6144, 3072, 3072, 0],
     [(10, 10, 0), (11, 11, 0), (9, 9, 0), (8, 8, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('cnt(4..6) one below 6 x resident[6]', 'exact', [1000, 1000, 1000, 1000, 8192, 8192, 8191, 12288, 7680, 6144, 3072, 3072, 0],
     [(10, 11, 0), (8, 9, 0), (7, 7, 0), (4, 6, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('bin 7 small, not merged', 'fast', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 100, 7680, 6144, 3072, 3072, 0],
     [(10, 10, 0), (11, 11, 0), (9, 9, 0), (8, 8, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (7, 7, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('bin 7 small, not merged', 'exact', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 100, 7680, 6144, 3072, 3072, 0],
     [(10, 11, 0), (8, 9, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (7, 7, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('bins 9 and 11 small in exact (merged launches move back)', 'exact', [1000, 1000, 1000, 1000, 30720, 24576, 24576, 12288, 10, 10, 0, 7, 0],
     [(7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (10, 11, 0), (8, 9, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('a shard: every wide bin small', 'fast', [50, 0, 70, 0, 100, 100, 100, 100, 100, 100, 100, 100, 0],
     [(10, 11, 0), (8, 9, 0), (7, 7, 0), (4, 6, 0), (2, 2, 1), (0, 0, 1)], True),
    ('a shard: every wide bin small', 'exact', [50, 0, 70, 0, 100, 100, 100, 100, 100, 100, 100, 100, 0],
     [(10, 11, 0), (8, 9, 0), (7, 7, 0), (4, 6, 0), (2, 2, 1), (0, 0, 1)], True),
    ('only short markets', 'fast', [5, 6, 7, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0],
     [(3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], False),
    ('only wide markets', 'fast', [0, 0, 0, 0, 30720, 24576, 24576, 12288, 7680, 6144, 3072, 3072, 0],
     [(10, 10, 0), (11, 11, 0), (9, 9, 0), (8, 8, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0)], False),
    ('only wide markets', 'exact', [0, 0, 0, 0, 30720, 24576, 24576, 12288, 7680, 6144, 3072, 3072, 0],
     [(10, 11, 0), (8, 9, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0)], False),
    ('empty plan', 'fast', [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
     [], False),
    ('empty plan', 'exact', [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
     [], False),
    ('bin 12 and one short bin', 'fast', [10, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2],
     [(12, 12, 0), (0, 0, 1)], True),
    ('bin 12 alone', 'exact', [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2],
     [(12, 12, 0)], False),
    ('device plan', 'fast', None,
     [(10, 10, 0), (11, 11, 0), (9, 9, 0), (8, 8, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
    ('device plan', 'exact', None,
     [(10, 11, 0), (8, 9, 0), (7, 7, 0), (6, 6, 0), (5, 5, 0), (4, 4, 0), (3, 3, 1), (2, 2, 1), (1, 1, 1), (0, 0, 1)], True),
]


def test_cases_sit_on_the_merge_thresholds():
    """The literals above were chosen against sharding._RESIDENT: 6 x resident of the wide bins."""
    assert [6 * _RESIDENT[b] for b in range(4, 12)] == CASES[0][2][4:12]


@pytest.mark.parametrize("what,mode,counts,launches,fork", CASES, ids=[f"{c[1]}-{c[0]}" for c in CASES])
def test_plan_schedule(what, mode, counts, launches, fork):
    bin_start = None if counts is None else np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    assert plan_schedule(bin_start, mode) == (launches, fork)


def test_plan_schedule_rejects_bad_arguments():
    L = N.load_library()
    res, rows = np.zeros(N.NBINS, np.int64), np.zeros((N.NBINS, 3), np.int32)
    n, fork = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert L.bce_plan_schedule(None, 7, N.ptr(res), N.ptr(rows), N.ptr(n), N.ptr(fork)) == -1
    assert b"plan_schedule: bad mode 7" in L.bce_last_error()
    assert L.bce_plan_schedule(None, N.MODE_FAST, None, N.ptr(rows), N.ptr(n), N.ptr(fork)) == -1
