"""CPU checks of the update-rule sweep: the plain-Python expected-value loop of
tests/update_sweep_ref.py reproduces the fixture recorded from the reference under four update
rules (``==`` on every float), batch.update_steps' values, errors and pin-run bound, and the
argument checks of bce_settle_trace_grid, which need no GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from bayesian_engine import _native as N
from bayesian_engine import batch
from update_sweep_ref import check_point, load_fixture, update_one, update_sweep_ref

POINTS = [(0.15, 0.10), (0.05, 0.10), (0.30, 0.20), (0.0, 0.10)]
LAG_POINTS = [(0.05, 0.10), (0.30, 0.20)]
# every step the GPU tests sweep: the fixture's, the lane-mapping grids' and the long path's
GRID_STEPS = sorted({min(c, r) for r, c in POINTS} | {0.25, 0.1, 0.02, 0.01, 0.0, 1.0} |
                    {round(0.004 * (k + 1), 3) for k in range(64)})


def test_ref_reproduces_the_fixture(golden_dir):
    u, (g, csr, state, times), _ = load_fixture(golden_dir)
    assert [(float(p["learning_rate"]), float(p["max_step"])) for p in u["points"]] == POINTS
    for p, (rate, cap) in zip(u["points"], POINTS):
        out, final = update_sweep_ref(*csr, *state, times, rate, cap)
        check_point(p, g, csr, out, final)


def test_ref_reproduces_the_lagged_fixture(golden_dir):
    u, _, (g, csr, state, forecast, resolve) = load_fixture(golden_dir)
    assert [(float(p["learning_rate"]), float(p["max_step"])) for p in u["lag_points"]] == LAG_POINTS
    for p, (rate, cap) in zip(u["lag_points"], LAG_POINTS):
        out, final = update_sweep_ref(*csr, *state, forecast, rate, cap, resolve_time_us=resolve)
        check_point(p, g, csr, out, final)


def test_update_steps_values():
    assert batch.UPDATE_MAX_POINTS == N.UPDATE_MAX_POINTS == 64
    d, s = batch.update_steps([0.15, 0.05, 0.30, 0.0], [0.10, 0.10, 0.20, 0.10])
    assert d.dtype == np.float64 and s.dtype == np.int64
    assert d.tolist() == [0.10, 0.05, 0.20, 0.0] and s.tolist() == [11, 21, 6, 0]
    d, s = batch.update_steps([0.15, 0.05, 0.30])  # one cap for all: the reference's
    assert d.tolist() == [0.10, 0.05, 0.10] and s.tolist() == [11, 21, 11]
    d, s = batch.update_steps(0.15)
    assert d.tolist() == [0.10] and s.tolist() == [11]
    d, s = batch.update_steps(np.array([1.0, 2.0, 0.25, 2.0 ** -20, 2.0 ** -21]), 5.0)
    assert d.tolist() == [1.0, 2.0, 0.25, 2.0 ** -20, 2.0 ** -21] and s.tolist() == [2, 2, 5, 2 ** 20 + 1, 0]
    # pairs, not a product; the step is the reference's capped delta, selected and never computed
    for rate, cap in POINTS + [(0.3, 0.0), (1e-3, 7.0)]:
        d, _ = batch.update_steps([rate], [cap])
        up = max(-cap, min(cap, rate * 1.0))
        down = max(-cap, min(cap, rate * -1.0))
        assert (float(d[0]), -float(d[0])) == (up, down) or (up == 0.0 and down == 0.0 and d[0] == 0.0)


@pytest.mark.parametrize("args, exc", [
    (([],), ValueError),
    (([0.1, 0.2], [0.1]), ValueError),
    (([0.1], [0.1, 0.2]), ValueError),
    (([-0.1],), ValueError),
    (([0.1], -0.1), ValueError),
    (([float("nan")],), ValueError),
    (([0.1], [float("nan")]), ValueError),
    (([float("inf")],), ValueError),
    (([0.1], float("inf")), ValueError),
    (([1e301], 1e302), ValueError),
    ((["0.1"],), TypeError),
    (("0.1",), TypeError),
    (([0.1], "0.1"), TypeError),
    (([None],), TypeError),
    ((None,), TypeError),
    (([True],), TypeError),
    (([0.1], [[0.1]]), TypeError),
])
def test_update_steps_errors(args, exc):
    with pytest.raises(exc):
        batch.update_steps(*args)


def test_pin_run_holds_for_every_swept_step():
    """sync_run equal outcomes from the far end land exactly on 1.0 / 0.0: the update is monotone
    in r, so 0.0 upward and 1.0 downward are the worst starts."""
    delta, sync = batch.update_steps(GRID_STEPS, 10.0)
    assert delta.tolist() == GRID_STEPS
    for d, n in zip(delta.tolist(), sync.tolist()):
        if d == 0.0:
            assert n == 0
            continue
        assert n == math.ceil(1.0 / d) + 1
        up, down = 0.0, 1.0
        for _ in range(n):
            up, _c = update_one(up, 0.25, True, d, 10.0)
            down, _c = update_one(down, 0.25, False, d, 10.0)
        assert up == 1.0 and down == 0.0, (d, n, up, down)


def test_argument_errors_need_no_gpu():
    lib = N.load_library()
    step = np.array([0.1], np.float64)
    sync = np.array([11], np.int64)

    def call(n_points, step_p, sync_p):
        # no chain, no entry, one source: only the grid arguments are looked at
        return lib.bce_settle_trace_grid(None, 0, None, None, 0, 0, None, 0, 256, 1, None, None, None, 0.5, 0.25,
                                         None, None, None, 0, step_p, sync_p, n_points, None, None, None)

    assert call(1, N.ptr(step), N.ptr(sync)) == 0
    for n_points in (0, 65):
        assert call(n_points, N.ptr(step), N.ptr(sync)) == -1
        assert b"n_points" in lib.bce_last_error()
    assert call(1, None, N.ptr(sync)) == -1
    assert b"step" in lib.bce_last_error()
    assert call(1, N.ptr(step), None) == -1
    assert b"sync_run" in lib.bce_last_error()
    bad = (C.c_double * 3)()
    rc = lib.bce_settle_trace_grid(None, 0, None, None, 0, 0, None, 0, 256, 0, None, None, None, 0.5, 0.25, None, None,
                                   None, 0, bad, N.ptr(sync), 1, None, None, None)
    assert rc == -1 and b"shape" in lib.bce_last_error()
