"""CPU checks of the CSR re-estimation: the expected-value helper against a fixture made by
the reference itself, the C ABI symbols, and the builder's host-side rejections."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from reestimate_csr_ref import reference_rounds

SYMBOLS = ("bce_reestimate_csr_compile", "bce_reestimate_csr_consensus", "bce_reestimate_csr_agreement",
           "bce_reestimate_csr_weights")


def test_helper_reproduces_reference_fixture(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "reestimate_csr_small.json")))
    prob = np.array([float(x) for x in g["prob"]])
    w_init = np.array([float(x) for x in g["w_init"]])
    lens = np.diff(g["offsets"])
    assert (lens == 0).any() and len(lens) == 12 and g["n_sources"] == 8
    rounds = reference_rounds(g["offsets"], g["sid"], prob, g["n_sources"], len(g["rounds"]), w=w_init)
    assert len(rounds) == 4
    for got, exp in zip(rounds, g["rounds"]):
        assert [repr(float(x)) for x in got.cons] == exp["cons"]
        assert got.null.tolist() == exp["null"]
        assert got.outcome.tolist() == exp["outcome"]
        assert got.correct.tolist() == exp["correct"]
        assert got.total.tolist() == exp["total"]
        assert [repr(float(x)) for x in got.w] == exp["w"]
    first = g["rounds"][0]
    # the fixture exercises what it says: a null non-empty market, a skipped valid-consensus market
    assert any(n and ln for n, ln in zip(first["null"], lens))
    assert any(o == -1 and not n for o, n in zip(first["outcome"], first["null"]))


def test_library_exports_and_binds_the_entry_points():
    lib = N.load_library()
    raw = C.CDLL(N.LIB_PATH)
    for name in SYMBOLS:
        assert name in N.EXPORTED, name
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(N._SIGS[name][1])
    assert lib.bce_abi_version() == 3
    # argument errors need no GPU
    assert lib.bce_reestimate_csr_weights(0, None, None, None, None) == -1
    assert lib.bce_reestimate_csr_consensus(None, 5, None, None, None, None, None, 3, None, None, None, None) == -1
    assert b"NULL" in lib.bce_last_error()
    assert lib.bce_reestimate_csr_compile(None, 1, None, None, 1, None, None, 3, 1 << 31, None, None, None, None,
                                          None, None) == -1
    assert b"2^31" in lib.bce_last_error()


def test_builder_rejects_on_the_host():
    build = batch.ReestimateCsrPlan.build
    # one source with 65536 signals in one market: the 16-bit vote counts cannot hold it
    n = 65536
    off = torch.tensor([0, 2, 2 + n], dtype=torch.int64)
    sid = torch.cat([torch.tensor([0, 1]), torch.full((n,), 3)]).to(torch.int32)
    prob = torch.full((n + 2,), 0.25, dtype=torch.float64)
    with pytest.raises(ValueError, match="65535"):
        build(off, sid, prob, 5)
    # 2^31 markets (a meta tensor: the shape alone decides)
    big = torch.empty((1 << 31) + 1, dtype=torch.int64, device="meta")
    none = torch.empty(0, dtype=torch.int32, device="meta")
    with pytest.raises(ValueError, match="markets"):
        build(big, none, none.to(torch.float64), 5)
    ok_off = torch.tensor([0, 1, 3], dtype=torch.int64)
    ok_sid = torch.tensor([0, 1, 2], dtype=torch.int32)
    ok_prob = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    with pytest.raises(ValueError, match="n_sources"):
        build(ok_off, ok_sid, ok_prob, 0)
    with pytest.raises(ValueError, match="length"):
        build(ok_off, ok_sid, ok_prob[:2], 3)
    with pytest.raises(ValueError, match="offsets"):
        build(torch.tensor([0, 2, 1, 3]), ok_sid, ok_prob, 3)
    with pytest.raises(ValueError, match="offsets"):
        build(torch.tensor([0, 1, 2]), ok_sid, ok_prob, 3)


def test_order_is_market_then_sid_with_input_order_kept():
    # the integer half of the builder runs anywhere: 65535 signals of one source are accepted
    off = torch.tensor([0, 4, 4, 7], dtype=torch.int64)
    sid = torch.tensor([2, 0, 2, 9, 1, 1, 0], dtype=torch.int32)  # 9 is clamped to S - 1 = 3
    prob = torch.zeros(7, dtype=torch.float64)
    key, perm, group_start, uoffsets = batch._reestimate_csr_order(off, sid, prob, 4)
    assert key.tolist() == [0, 2, 2, 3, 8, 9, 9]
    assert perm.tolist() == [1, 0, 2, 3, 6, 4, 5]
    assert group_start.tolist() == [0, 1, 3, 4, 5, 7]
    assert uoffsets.tolist() == [0, 3, 3, 5]
    n = 65535
    off = torch.tensor([0, n], dtype=torch.int64)
    _, _, gs, uo = batch._reestimate_csr_order(off, torch.zeros(n, dtype=torch.int32),
                                               torch.zeros(n, dtype=torch.float64), 2)
    assert gs.tolist() == [0, n] and uo.tolist() == [0, 1]
