"""The glob kernels (bce_glob_match / bce_glob_count / bce_glob_fill) and the device route of the
pattern filters, bit for bit against fnmatch and against the host route."""
import functools
import warnings

import numpy as np
import pytest
import torch

import glob_ref
from bayesian_engine import _native as N
from bayesian_engine import batch
from bayesian_engine.market import CrossMarketAggregator, MarketId, MarketStore
from bayesian_engine.reliability_abstraction import NamespacedReliabilityStore

pytestmark = pytest.mark.gpu

PATTERN_TILE = 32  # csrc/glob.hip kGlobPT
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _dev():
    return torch.device("cuda", 0)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _match(names, pats, sentinel_rows=2):
    """Device bitmap, one row per pattern given, the rows behind the bitmap checked untouched."""
    nt = batch.NameTable.from_strings(names, _dev())
    gs = batch.GlobSet.compile(pats)
    nw = (len(names) + 63) // 64
    buf = torch.full((gs.n + sentinel_rows, nw), SENTINEL, dtype=torch.int64, device=_dev())
    bits = batch.glob_match(nt, gs, out=buf[:gs.n])
    N.check_faults(_dev(), "glob_match")
    assert (buf[gs.n:] == SENTINEL).all()
    return gs, bits, _u64(bits)[gs.index]


@functools.lru_cache(maxsize=None)
def _case(seed, M, P):
    names, pats = glob_ref.random_case(seed, M, P)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        table = glob_ref.oracle(names, pats)
        if P >= 40:
            glob_ref.check_balanced(table)
        return names, pats, glob_ref.oracle_bits(names, pats)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 129, 1000])
@pytest.mark.parametrize("P", [1, 3, PATTERN_TILE + 1, 65])
def test_match_random_cases(M, P):
    names, pats, exp = _case(M % 5, M, P)
    _, _, got = _match(names, pats)
    assert np.array_equal(got, exp)  # the padding bits of the last word are zero in both


@pytest.mark.parametrize("P", [None, 1, 3, PATTERN_TILE + 1])
def test_match_edge_lists(P):
    names = glob_ref.edge_names()  # the empty name, '\n', 63 / 64 / 65 / 300 bytes
    assert {65, 300} <= {len(n.encode("utf-8", "surrogatepass")) for n in names}
    pats = glob_ref.EDGE_PATTERNS if P is None else (glob_ref.EDGE_PATTERNS * 2)[5:5 + P]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        exp = glob_ref.oracle_bits(names, pats)
    gs, _, got = _match(names, pats)
    assert not gs.declined
    assert np.array_equal(got, exp)


def test_match_declined_and_long_programs():
    """Rows of declined patterns are uploaded; a tile whose programs exceed the LDS staging budget
    (more than 2048 ops) reads them from global memory."""
    big = ["a" * 200 + chr(0x100 + i) + "*" for i in range(12)]  # 12 x 202 ops in one tile
    over = "a" * (batch.GLOB_MAX_OPS + 1)
    pats = ["a*"] + big + [over, "*b"]
    names = glob_ref.edge_names() + ["a" * 200 + chr(0x100 + 3) + "tail", over, "a" * 200 + chr(0x100)]
    gs, _, got = _match(names, pats)
    assert [gs.patterns[r] for r in gs.declined] == [over]
    assert np.array_equal(got, glob_ref.oracle_bits(names, pats))


def _bitmap(M, P, seed):
    """A random bitmap with an empty row (1) and a full row (2), padding bits zero."""
    rng = np.random.default_rng(seed)
    dense = rng.random((P, M)) < rng.choice([0.01, 0.3, 0.9], (P, 1))
    if P > 2:
        dense[1] = False
        dense[2] = True
    pad = np.zeros((P, ((M + 63) // 64) * 64), np.uint8)
    pad[:, :M] = dense
    words = np.packbits(pad, axis=1, bitorder="little").view(np.uint64).reshape(P, -1)
    return words, torch.from_numpy(words.view(np.int64).copy()).to(_dev())


@pytest.mark.parametrize("M,P", [(1, 3), (63, 4), (64, 5), (65, 5), (1000, 7), (4097 * 64 + 5, 3)])
def test_count_and_fill(M, P):
    words, bits = _bitmap(M, P, M)
    rows = [0, 2, 1, 0, P - 1, 2] if P > 2 else [0]  # rows listed twice, the empty and the full row
    groups = [0, 2, 2, 3, len(rows)]                   # an empty group among them
    goff, members = batch.glob_members(bits, M, torch.tensor(rows, dtype=torch.int64, device=_dev()), groups)
    cnt = batch.glob_count(bits, M, torch.tensor(rows, dtype=torch.int64, device=_dev()))
    N.check_faults(_dev(), "glob_members")
    exp = [glob_ref.expand(words[r], M) for r in rows]
    assert cnt.cpu().tolist() == [len(e) for e in exp]
    off = np.concatenate([[0], np.cumsum([len(e) for e in exp])])
    assert goff.cpu().tolist() == [int(off[g]) for g in groups]
    assert np.array_equal(members.cpu().numpy(), np.concatenate(exp))
    assert len(exp[1]) == M and len(exp[2]) == 0


def test_count_and_fill_no_slots():
    _, bits = _bitmap(100, 3, 0)
    goff, members = batch.glob_members(bits, 100, torch.zeros(0, dtype=torch.int64, device=_dev()), [0, 0])
    N.check_faults(_dev(), "glob_members")
    assert goff.cpu().tolist() == [0, 0] and members.numel() == 0


def test_malformed_inputs_raise_the_fault_word():
    """A row outside [0, P), decreasing name offsets and a class index outside its table: no
    match, the fault word set, nothing written outside the outputs."""
    L = N.require_gpu()
    _, bits = _bitmap(100, 3, 1)
    cnt = batch.glob_count(bits, 100, torch.tensor([0, 3, -1], dtype=torch.int64, device=_dev()))
    with pytest.raises(N.BCEError):
        N.check_faults(_dev(), "glob_count")
    assert cnt.cpu().tolist()[1:] == [0, 0]
    nt = batch.NameTable.from_strings(["ab", "cd", "ef"], _dev())
    gs = batch.GlobSet.compile(["*", "[a]*"])
    nt.off = torch.tensor([0, 4, 2, 6], dtype=torch.int64, device=_dev())  # name 1 runs backwards
    out = _u64(batch.glob_match(nt, gs))
    with pytest.raises(N.BCEError):
        N.check_faults(_dev(), "glob_match")
    assert out[:, 0].tolist() == [0b101, 0b001]
    nt = batch.NameTable.from_strings(["ab", "cd"], _dev())
    gs.cls_off = gs.cls_off[:1]  # no class left: index 0 is outside the table
    out = _u64(batch.glob_match(nt, gs))
    with pytest.raises(N.BCEError):
        N.check_faults(_dev(), "glob_match")
    assert out[:, 0].tolist() == [0b11, 0]
    N.check_faults(_dev(), "the fault word is cleared by the check")


def _store(n=300):
    rng = np.random.default_rng(5)
    cats = ["crypto", "sports", "politics", "weather-é"]
    ms = MarketStore()
    for i in range(n):
        mid = f"{cats[i % 4]}:{'btc' if i % 3 else 'eth'}:q-{i:04d}"
        m = ms.create_market(MarketId(mid))
        for j in range(int(rng.integers(0, 5))):
            m.add_signal({"sourceId": f"s{int(rng.integers(0, 9))}", "probability": float(np.round(rng.random(), 3))})
        if i % 7 != 0 and not mid.startswith("weather"):  # 'weather-é:*' markets have no consensus
            m.consensus_result = {"consensus": float(np.round(rng.random(), 4)),
                                  "confidence": float(np.round(rng.random(), 4))}
        elif i % 14 == 0:
            m.consensus_result = {"consensus": None, "confidence": 0.0}
        if i % 5 in (1, 2, 3) and m.signals:
            m.resolve(bool(rng.integers(0, 2)))
        if i % 10 == 1:
            m.outcome = None
    return ms


PATTERN_LISTS = [["crypto:*"], ["crypto:*", "*:eth:*"], ["*"], ["nothing:*"], [], ["weather-é:*"],
                 ["*:q-00[0-4]?", "sports:???:q-0[!0]*", "crypto:*"], ["[cs]*:btc:*", "nothing", "*-é:eth:*1"],
                 ["crypto:*", "crypto:*"], ["weather-é:*", "nothing:*"]]


@pytest.mark.parametrize("method", ["weighted_average", "median", "majority"])
def test_aggregate_many_routes_agree(method):
    agg = CrossMarketAggregator(_store())
    host = agg.aggregate_many(PATTERN_LISTS, method, device_match=False)
    dev = agg.aggregate_many(PATTERN_LISTS, method, device_match=True)
    N.check_faults(_dev(), "aggregate_many")
    assert dev == host
    assert [type(d.get("consensus")) for d in dev] == [type(d.get("consensus")) for d in host]
    assert host[0]["consensus"] is not None and host[3]["marketsIncluded"] == 0 and host[5]["consensus"] is None
    assert host[5]["marketsIncluded"] > 0
    assert agg.aggregate_many(PATTERN_LISTS, method) == host  # None: by size (here the device route)


def test_aggregate_many_in_several_bitmap_runs(monkeypatch):
    from bayesian_engine import market
    agg = CrossMarketAggregator(_store())
    host = agg.aggregate_many(PATTERN_LISTS, "median", device_match=False)
    monkeypatch.setattr(market, "GLOB_BITMAP_BUDGET", 3 * 5 * 8)  # 3 rows of 300 ids at a time
    assert agg.aggregate_many(PATTERN_LISTS, "median", device_match=True) == host
    N.check_faults(_dev(), "aggregate_many")


def test_aggregate_many_routes_agree_on_exceptions_and_empties():
    agg = CrossMarketAggregator(_store())
    for route in (False, True):
        with pytest.raises(ValueError, match="Unknown aggregation method: mean"):
            agg.aggregate_many(PATTERN_LISTS, "mean", device_match=route)
    quiet = [["weather-é:*"], ["nothing"], []]
    host = agg.aggregate_many(quiet, "mean", device_match=False)  # no consensus anywhere: no error
    assert agg.aggregate_many(quiet, "mean", device_match=True) == host
    assert agg.aggregate_many([], device_match=True) == [] == agg.aggregate_many([], device_match=False)
    late = _store(70)
    agg = CrossMarketAggregator(late)
    before = agg.aggregate_many([["crypto:*"]], device_match=True)
    m = late.create_market(MarketId("crypto:late"))  # the cached name table is rebuilt
    m.consensus_result = {"consensus": 1.0, "confidence": 1.0}
    after = agg.aggregate_many([["crypto:*"]], device_match=True)
    assert after == agg.aggregate_many([["crypto:*"]], device_match=False) != before


def test_pattern_filters_routes_agree(tmp_path):
    ms = _store()
    agg = CrossMarketAggregator(ms)
    for patterns in (["crypto:*"], ["*:eth:*", "sports:*", "nothing"], ["nothing"], ["*"]):
        assert agg.summarize_sources(patterns, device_match=True) == agg.summarize_sources(patterns, device_match=False)
        assert agg.reestimate_sources(3, patterns, device_match=True) == \
            agg.reestimate_sources(3, patterns, device_match=False)
        got = []
        for route in (True, False):
            st = NamespacedReliabilityStore(str(tmp_path / f"r{len(got)}-{abs(hash(tuple(patterns)))}.db"))
            s = agg.settle_resolved(st, domain="x", update_global=True, patterns=patterns, dry_run=True,
                                    device_match=route)
            got.append(({k: (v.reliability, v.confidence) for k, v in s.records.items()},
                        {k: (v.reliability, v.confidence) for k, v in s.global_records.items()}, s.total, s.correct))
            st.close()
        assert got[0] == got[1]
    assert agg.summarize_sources(["crypto:*"], device_match=True)
    N.check_faults(_dev(), "pattern filters")
    hit = ms.match_any(["sports:*", "*:q-0000"])
    assert hit.tolist() == [m.id.matches("sports:*") or m.id.matches("*:q-0000") for m in ms.list_markets()]
