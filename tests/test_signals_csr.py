"""CPU pin of the two host helpers every store layer goes through (bayesian_engine/core.py):
signals_csr, from lists of signal dicts to the CSR arrays of a batch, and consensus_dict, one
market of a batched result as compute_consensus's dict.

The expected values are literals.  They were printed once by the loops as they stood before the
helpers existed -- _batched_consensus (ranks per market), NamespacedReliabilityStore.walk_forward
and settle_markets (ranks over the batch, the consensus and the settlement rule),
summarize_sources (first-seen ranks), and the dict blocks of _batched_consensus and walk_forward
fed a fabricated result -- with the batch calls behind them replaced by a recorder, not by the
helpers."""
import json

import numpy as np
import pytest

from bayesian_engine import batch
from bayesian_engine.core import consensus_dict, signals_csr
from bayesian_engine.market import _FirstSeen

# a duplicate source, an int probability, an empty market
FULL = [[{"sourceId": "b", "probability": 0.7}, {"sourceId": "a", "probability": 0.2}, {"sourceId": "b", "probability": 1}],
        [],
        [{"sourceId": "c", "probability": 0.9}, {"sourceId": "a", "probability": 0.4}]]
# ... and a missing probability
MISSING = [FULL[0], [], [{"sourceId": "c"}, {"sourceId": "a", "probability": 0.4}]]


def per_market():
    """The caller's side of _batched_consensus: ranks of the market's own, behind the markets before."""
    base = [0]

    def rank(mpos, signals):
        ids = sorted({s["sourceId"] for s in signals})
        b = base[0]
        base[0] += len(ids)
        return {sid: b + i for i, sid in enumerate(ids)}
    return rank


def batch_wide(lists):
    return batch.intern(s["sourceId"] for signals in lists for s in signals)


def check(got, offsets, sid, prob):
    off, s, p = got
    assert (off.dtype, s.dtype, p.dtype) == (np.int64, np.int32, np.float64)
    assert off.tolist() == offsets and s.tolist() == sid and p.tolist() == prob


def test_ranks_per_market():
    check(signals_csr(FULL, per_market()), [0, 3, 3, 5], [1, 0, 1, 3, 2], [0.7, 0.2, 1.0, 0.9, 0.4])
    check(signals_csr([FULL[0], FULL[2]], per_market()), [0, 3, 5], [1, 0, 1, 3, 2], [0.7, 0.2, 1.0, 0.9, 0.4])


def test_ranks_over_the_batch():
    check(signals_csr(FULL, batch_wide(FULL)), [0, 3, 3, 5], [1, 0, 1, 2, 0], [0.7, 0.2, 1.0, 0.9, 0.4])
    check(signals_csr(MISSING, batch_wide(MISSING), settlement=True),
          [0, 3, 3, 5], [1, 0, 1, 2, 0], [0.7, 0.2, 1.0, 0.5, 0.4])


def test_ranks_first_seen():
    order = _FirstSeen()
    check(signals_csr(MISSING, order, settlement=True), [0, 3, 3, 5], [0, 1, 0, 2, 1], [0.7, 0.2, 1.0, 0.5, 0.4])
    assert list(order) == ["b", "a", "c"]


def test_no_markets():
    check(signals_csr([], {}), [0], [], [])


def test_missing_probability_under_the_consensus_rule():
    for rank in (per_market(), batch_wide(MISSING)):
        with pytest.raises(KeyError) as e:
            signals_csr(MISSING, rank)
        assert e.value.args == ("probability",)


@pytest.mark.parametrize("bad, settlement, message", [
    ("x", False, "unsupported operand type(s) for +: 'int' and 'str'"),
    ("x", True, "'>=' not supported between instances of 'str' and 'float'"),
    (None, False, "unsupported operand type(s) for +: 'int' and 'NoneType'"),
    (None, True, "'>=' not supported between instances of 'NoneType' and 'float'"),
])
def test_probability_that_is_no_number(bad, settlement, message):
    lists = [[{"sourceId": "a", "probability": 0.5}, {"sourceId": "b", "probability": bad}]]
    with pytest.raises(TypeError) as e:
        signals_csr(lists, {"a": 0, "b": 1}, settlement=settlement)
    assert str(e.value) == message


def test_the_first_bad_signal_raises():
    # market 0 holds a bad probability, market 1 a signal without a sourceId
    lists = [[{"sourceId": "a", "probability": 0.5}, {"sourceId": "b", "probability": "x"}], [{"probability": 0.1}]]
    with pytest.raises(TypeError, match="for \\+"):  # the ranks of market 1 are built when it is reached
        signals_csr(lists, per_market())
    with pytest.raises(TypeError, match=">="):
        signals_csr(lists, _FirstSeen(), settlement=True)
    with pytest.raises(KeyError) as e:  # ranks over the batch: the caller's interning meets market 1 first
        signals_csr(lists, batch_wide(lists), settlement=True)
    assert e.value.args == ("sourceId",)
    # inside one signal the sourceId is read before the probability
    lists = [[{"sourceId": "a", "probability": 0.5}, {"probability": "x"}]]
    for rank, settlement in ((_FirstSeen(), True), (per_market(), False)):
        with pytest.raises(KeyError) as e:
            signals_csr(lists, rank, settlement=settlement)
        assert e.value.args == ("sourceId",)


# A fabricated result of two markets (offsets 0, 3, 5): b is a cold source of the first, the
# second has no consensus (total weight 0).
CONS, CONF, TOT = np.array([0.6123456789, 0.5]), np.array([0.3333333333333333, 0.9]), np.array([1.1, 0.0])
WEIGHT = np.array([0.1, 1.0, 0.0, 0.0, 0.0])
NWEIGHT = np.array([0.09090909090909091, 0.9090909090909091, 0.0, 0.5, 0.5])
COLD_SOURCE = {
    "schemaVersion": "1.0.0", "consensus": 0.6123456789, "confidence": 0.3333333333333333,
    "sourceWeights": [{"sourceId": "a", "weight": 0.1, "normalizedWeight": 0.09090909090909091},
                      {"sourceId": "b", "weight": 1.0, "normalizedWeight": 0.9090909090909091}],
    "normalization": {"totalWeight": 1.1, "sourceCount": 2},
    "diagnostics": {"status": "computed", "sources": 3, "uniqueSources": 2, "coldStartSources": ["b"]},
    "marketId": "cat:m0"}
COLD_SOURCE_JSON = (
    '{"schemaVersion": "1.0.0", "consensus": 0.6123456789, "confidence": 0.3333333333333333, "sourceWeights": '
    '[{"sourceId": "a", "weight": 0.1, "normalizedWeight": 0.09090909090909091}, {"sourceId": "b", "weight": 1.0, '
    '"normalizedWeight": 0.9090909090909091}], "normalization": {"totalWeight": 1.1, "sourceCount": 2}, '
    '"diagnostics": {"status": "computed", "sources": 3, "uniqueSources": 2, "coldStartSources": ["b"]}, '
    '"marketId": "cat:m0"}')
NULL_CONSENSUS = {
    "schemaVersion": "1.0.0", "consensus": None, "confidence": 0.0,
    "sourceWeights": [{"sourceId": "a", "weight": 0.0, "normalizedWeight": 0.5},
                      {"sourceId": "c", "weight": 0.0, "normalizedWeight": 0.5}],
    "normalization": {"totalWeight": 0.0, "sourceCount": 2},
    "diagnostics": {"status": "computed", "sources": 2, "uniqueSources": 2, "coldStartSources": []}}
NULL_CONSENSUS_JSON = (
    '{"schemaVersion": "1.0.0", "consensus": null, "confidence": 0.0, "sourceWeights": [{"sourceId": "a", '
    '"weight": 0.0, "normalizedWeight": 0.5}, {"sourceId": "c", "weight": 0.0, "normalizedWeight": 0.5}], '
    '"normalization": {"totalWeight": 0.0, "sourceCount": 2}, "diagnostics": {"status": "computed", "sources": 2, '
    '"uniqueSources": 2, "coldStartSources": []}}')


def test_dict_of_a_market_with_a_cold_source():
    got = consensus_dict(["a", "b"], WEIGHT[0:2], NWEIGHT[0:2], CONS[0], CONF[0], TOT[0], 3, ["b"], "cat:m0")
    assert got == COLD_SOURCE
    assert json.dumps(got) == COLD_SOURCE_JSON


def test_dict_of_a_market_without_consensus():
    # as walk_forward renders it: no marketId, every source fetched
    got = consensus_dict(["a", "c"], WEIGHT[3:5], NWEIGHT[3:5], CONS[1], CONF[1], TOT[1], 2, [])
    assert got == NULL_CONSENSUS
    assert json.dumps(got) == NULL_CONSENSUS_JSON
    # as MarketStore renders it: the marketId last
    got = consensus_dict(["a", "c"], WEIGHT[3:5], NWEIGHT[3:5], CONS[1], CONF[1], TOT[1], 2, [], "cat:m1")
    assert got == dict(NULL_CONSENSUS, marketId="cat:m1")
    assert json.dumps(got) == NULL_CONSENSUS_JSON[:-1] + ', "marketId": "cat:m1"}'
