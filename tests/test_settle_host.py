"""CPU checks of batch settlement: the two lemmas the chunked chain kernel rests on (through the
oracle's arithmetic), the expected-value helper against a fixture made by the reference itself,
the C ABI symbols, the builder's host-side rejections and the market layer's gather."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from bayesian_engine import _native as N
from bayesian_engine import batch
from oracle import oracle as orc
from settle_ref import chains, fixture_scope, settle_ref


def _steps(r, c, bits):
    """(rel, conf) after every step of one source's chain, by orc.outcome_update."""
    rel, conf = np.array([r], np.float64), np.array([c], np.float64)
    t, pres = np.zeros(1, np.int64), np.ones(1, np.uint8)
    out = []
    for b in bits:
        rel, conf, t, pres = orc.outcome_update(rel, conf, t, pres, np.array([1 | (int(b) << 1)], np.uint8), 0)
        out.append((float(rel[0]), float(conf[0])))
    return out


def test_eleven_equal_outcomes_pin_the_reliability():
    up = _steps(0.0, 0.25, [1] * 11)
    assert up[9][0] == 0.9999999999999999 and up[9][0] != 1.0   # ten steps do not reach the clamp
    assert up[10][0] == 1.0
    down = _steps(1.0, 0.25, [0] * 11)
    assert down[9][0] == 1.3877787807814457e-16 and down[9][0] != 0.0
    assert down[10][0] == 0.0
    # any start is inside [0, 1] after one step (NaN and out-of-range values are clamped), and a
    # step is monotone in r: 11 equal outcomes after it give exactly 1.0 / 0.0
    for r0 in (0.37, 1.7, -0.3, float("nan"), 0.0, 1.0, 0.9999999999999999, 1.3877787807814457e-16):
        for first in (0, 1):
            one = _steps(r0, 0.25, [first])[0][0]
            assert 0.0 <= one <= 1.0, (r0, first, one)
            assert _steps(r0, 0.25, [first] + [1] * 11)[-1][0] == 1.0
            assert _steps(r0, 0.25, [first] + [0] * 11)[-1][0] == 0.0


def test_confidence_reaches_a_bitwise_fixed_point():
    conf = [c for _, c in _steps(0.5, 0.25, [1] * 400)]
    first = next(k for k in range(1, len(conf)) if conf[k] == conf[k - 1])
    assert first == 331                      # the 332nd step is the first to change nothing
    assert conf[first] == 0.9999999999999996
    assert all(c == conf[first] for c in conf[first:])
    assert all(a < b for a, b in zip(conf[:first - 1], conf[1:first]))
    for c0 in (1.0, 0.0, 0.9999):
        tail = [c for _, c in _steps(0.5, c0, [0] * 400)]
        assert tail[-1] == tail[-2] and tail[-1] <= 1.0


def test_helper_reproduces_reference_fixture(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "settle_small.json")))
    prob = np.array([float(x) for x in g["prob"]])
    S = g["n_sources"]
    assert S == 8 and len(g["outcome"]) == 12 and -1 in g["outcome"] and 0.5 in prob
    assert max(g["total"]) >= 25
    ch = chains(g["offsets"], g["sid"], prob, g["outcome"], S)
    assert ch.total.tolist() == g["total"] and ch.correct.tolist() == g["correct"]
    for scope in ("domain", "global"):
        (rel, conf, present), (erel, econf, epresent) = fixture_scope(g, scope)
        assert present.any() and not present.all()
        t0 = np.where(present, 5, orc.NO_TIMESTAMP).astype(np.int64)
        r, c, t, p, total, correct = settle_ref(g["offsets"], g["sid"], prob, g["outcome"], S, rel, conf, t0,
                                                present, 77)
        assert [repr(float(x)) for x in r] == [repr(float(x)) for x in erel], scope
        assert [repr(float(x)) for x in c] == [repr(float(x)) for x in econf], scope
        assert p.tolist() == epresent.tolist(), scope            # which rows exist
        assert np.array_equal(t == 77, ch.total > 0)             # only touched rows are stamped
    # the fixture exercises what it says: both clamps (src-0 ends at 0.0 after reaching 1.0), a
    # stored 1.0, 0.0 and confidence 1.0, a source seen only in the unresolved market
    seeds = {(s["scope"], s["reliability"]) for s in g["seeds"]} | {("conf", s["confidence"]) for s in g["seeds"]}
    assert ("domain", "1.0") in seeds and ("domain", "0.0") in seeds and ("conf", "1.0") in seeds
    assert g["final"]["domain"]["src-0"][0] == "0.0" and g["total"][7] == 0


def test_library_exports_and_binds_the_entry_points():
    lib = N.load_library()
    raw = C.CDLL(N.LIB_PATH)
    for name in ("bce_settle_compile", "bce_settle_apply"):
        assert name in N.EXPORTED, name
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(N._SIGS[name][1])
    assert lib.bce_abi_version() == 3
    # argument errors need no GPU
    assert lib.bce_settle_compile(None, 4, None, None, None, None, 4, None, 2, 3, None, None, None) == -1
    assert b"NULL" in lib.bce_last_error()
    assert lib.bce_settle_compile(None, 4, None, None, None, None, 4, None, 1 << 31, 3, None, None, None) == -1
    assert b"2^31" in lib.bce_last_error()
    assert lib.bce_settle_compile(None, 0, None, None, None, None, 4, None, 2, 3, None, None, None) == 0
    assert lib.bce_settle_apply(None, 64, None, None, 2, 3, None, 0, 64, 5, None, None, None, None, 0, 0.5, 0.25,
                                None, None) == -1
    assert b"long-chain" in lib.bce_last_error()
    assert lib.bce_settle_apply(None, 0, None, None, 0, 0, None, 0, 64, 5, None, None, None, None, 0, 0.5, 0.25,
                                None, None) == 0


def test_builder_rejects_on_the_host():
    build = batch.SettlePlan.build
    off = torch.tensor([0, 1, 3], dtype=torch.int64)
    sid = torch.tensor([0, 1, 2], dtype=torch.int32)
    prob = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    out = torch.tensor([1, -1], dtype=torch.int8)
    with pytest.raises(ValueError, match="one entry per market"):
        build(off, sid, prob, out[:1], 3)
    with pytest.raises(ValueError, match="one entry per market"):
        build(off, sid, prob, torch.tensor([1, 0, 1], dtype=torch.int8), 3)
    with pytest.raises(ValueError, match="int8"):
        build(off, sid, prob, out.to(torch.int32), 3)
    with pytest.raises(ValueError, match="int8"):
        build(off, sid, prob, out.to(torch.bool), 3)
    for bad in (0, -4):
        with pytest.raises(ValueError, match="n_sources"):
            build(off, sid, prob, out, bad)
    with pytest.raises(ValueError, match="n_sources"):
        build(off, sid, prob, out, 1 << 31)
    with pytest.raises(ValueError, match="length"):
        build(off, sid, prob[:2], out, 3)
    with pytest.raises(ValueError, match="offsets"):
        build(torch.tensor([0, 2, 1]), sid, prob, out, 3)
    big = torch.empty((1 << 31) + 1, dtype=torch.int64, device="meta")
    none = torch.empty(0, dtype=torch.int32, device="meta")
    with pytest.raises(ValueError, match="markets"):
        build(big, none, none.to(torch.float64), torch.empty(1 << 31, dtype=torch.int8, device="meta"), 5)


def test_order_is_sid_then_market_then_position():
    # the integer half of the builder runs anywhere
    off = torch.tensor([0, 4, 6, 6, 9], dtype=torch.int64)
    sid = torch.tensor([2, 0, 2, 9, 1, 2, 0, 2, 0], dtype=torch.int32)  # 9 is clamped to S - 1 = 3
    prob = torch.zeros(9, dtype=torch.float64)
    outcome = torch.tensor([1, -1, 0, 0], dtype=torch.int8)  # market 1 is unresolved, market 2 empty
    market, perm, key, total, start, order, lens_desc = batch._settle_order(off, sid, prob, outcome, 4)
    assert market.tolist() == [0, 0, 0, 0, 1, 1, 3, 3, 3]
    assert perm.tolist() == [1, 6, 8, 0, 2, 7, 3]
    assert key.tolist() == [0, 0, 0, 2, 2, 2, 3]
    assert total.tolist() == [3, 0, 3, 1] and start.tolist() == [0, 3, 3, 6, 7]
    assert order.tolist() == [0, 2, 3] and lens_desc.tolist() == [3, 3, 1]  # longest first, ties by rank
    plan = batch.SettlePlan(None, start, order, total, None, 7, 4, lens_desc)
    assert plan.chunks(2, 64)[0] == 2 and plan.chunks(2, 64)[2] == 2
    assert plan.chunks(1 << 62, 64) == (0, None, 0)
    with pytest.raises(ValueError, match="chunk_bits"):
        plan.chunks(2, 32)


def test_settle_resolved_gathers_like_summarize_sources():
    from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore

    class Stub:
        def __init__(self):
            self.calls = []

        def settle_markets(self, markets, domain=None, update_global=False, dry_run=False, now=None):
            self.calls.append(([(list(s), o) for s, o in markets], domain, update_global, dry_run))
            return "summary"

    store = MarketStore()
    sig = lambda name, p: {"sourceId": name, "probability": p}  # noqa: E731
    store.add_signal(MarketId("crypto:a"), sig("x", 0.9))
    store.add_signal(MarketId("sports:b"), sig("y", 0.2))
    store.add_signal(MarketId("crypto:c"), sig("x", 0.4))
    store.add_signal(MarketId("crypto:c"), sig("z", 0.6))
    store.add_signal(MarketId("crypto:open"), sig("x", 0.5))
    store.add_signal(MarketId("crypto:noout"), sig("y", 0.5))
    store.add_signal(MarketId("crypto:d"), sig("z", 0.1))
    store.get_market(MarketId("crypto:c")).resolve(False)
    store.get_market(MarketId("sports:b")).resolve(True)
    store.get_market(MarketId("crypto:a")).resolve(True)
    store.get_market(MarketId("crypto:d")).resolve(True)
    m = store.get_market(MarketId("crypto:noout"))
    m.resolve(True)
    m.outcome = None  # RESOLVED without an outcome: left out, as summarize_sources leaves it out
    agg = CrossMarketAggregator(store)
    stub = Stub()
    assert agg.settle_resolved(stub) == "summary"
    assert agg.settle_resolved(stub, domain="crypto", update_global=True, patterns=["crypto:*"], dry_run=True) == "summary"
    everything, filtered = stub.calls
    # list_markets order (insertion), not resolution order
    assert everything == ([([sig("x", 0.9)], True), ([sig("y", 0.2)], True),
                           ([sig("x", 0.4), sig("z", 0.6)], False), ([sig("z", 0.1)], True)], None, False, False)
    assert filtered == ([([sig("x", 0.9)], True), ([sig("x", 0.4), sig("z", 0.6)], False), ([sig("z", 0.1)], True)],
                        "crypto", True, True)
