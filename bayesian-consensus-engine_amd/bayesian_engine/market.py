"""Drop-in for ``bayesian_engine.market`` (reference src/bayesian_engine/market.py).

The multi-market layer is where the batched engine pays off:

* ``MarketStore.compute_all_consensus`` (market.py:200-221) -- instead of a Python loop of
  per-market ``compute_consensus`` calls, ALL open markets become one CSR batch and one
  consensus launch.  With a reliability store, every (source, market) pair the batch
  needs is fetched in bulk and decayed on the GPU in one launch (the reference's
  per-signal ``get_reliability(..., apply_decay=True)``, market.py:208-219).  Ranks are
  interned over (market position, sourceId) so each market's rank order is Python
  ``sorted()`` order of its sourceIds -- results are identical to the reference's.
* ``CrossMarketAggregator.summarize_sources`` (market.py:256-321) -- the per-source
  correct/total counts run in the ``bce_agreement_stats`` kernel (exact int atomics).

* ``CrossMarketAggregator.aggregate_consensus`` (market.py:340-408) --
  weighted_average / median / majority over member groups in the ``bce_aggregate_groups``
  kernel (list-order sums, exact radix-select median); ``aggregate_many`` does many
  pattern lists in one launch.

Metadata (MarketId glob matching, status, category summaries) is host Python with the
reference's semantics.
"""
from __future__ import annotations

import fnmatch
import math
from dataclasses import dataclass, field
from datetime import datetime, timezone
from enum import Enum
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from . import _native as N
from . import batch
from .config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM, DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY, MAX_UPDATE_STEP
from .core import compute_consensus, consensus_dict, signals_csr
from .reliability import SQLiteReliabilityStore
from .reliability_abstraction import NamespacedReliabilityStore, _check_boot
from . import decay as _decay
from .timeutil import NO_TIMESTAMP, dt_to_us, iso_to_us, us_to_iso

__all__ = ["MarketId", "MarketStatus", "Market", "MarketStore", "SourcePerformance", "BacktestScore", "SourceScore",
           "WalkScore", "CrossMarketAggregator"]

# device_match=None: (markets) x (patterns) from which the pattern filters take the GPU route when
# a GPU is visible.  Measured crossover (tools/bench_glob.py part (e), name table cached): the
# device route is clear of the fnmatch loop in every repetition from 1792 pairs up (0.77 against
# 1.16 ms) and behind it at 448 (0.73 against 0.49 ms); rounded up to a power of two.  None = never.
DEVICE_MATCH_MIN_PAIRS: Optional[int] = 2048
# aggregate_many's device route: bytes of match bitmap held at once (more patterns: several runs)
GLOB_BITMAP_BUDGET = 4 << 30


@dataclass(frozen=True)
class MarketId:
    """Unique identifier for a market or question (market.py:41-82)."""

    value: str

    def __post_init__(self):
        if not self.value or not self.value.strip():
            raise ValueError("Market ID cannot be empty")

    def __str__(self) -> str:
        return self.value

    def __repr__(self) -> str:
        return f"MarketId({self.value!r})"

    @property
    def category(self) -> Optional[str]:
        if ":" in self.value:
            return self.value.split(":")[0]
        return None

    @property
    def parts(self) -> List[str]:
        return self.value.split(":")

    def matches(self, pattern: str) -> bool:
        return fnmatch.fnmatch(self.value, pattern)


class MarketStatus(str, Enum):
    OPEN = "open"
    CLOSED = "closed"
    RESOLVED = "resolved"


@dataclass
class Market:
    """A market with metadata and signals (market.py:93-134)."""

    id: MarketId
    status: MarketStatus = MarketStatus.OPEN
    signals: List[Dict[str, Any]] = field(default_factory=list)
    consensus_result: Optional[Dict[str, Any]] = None
    outcome: Optional[bool] = None
    created_at: str = field(default_factory=lambda: datetime.now(timezone.utc).isoformat())
    resolved_at: Optional[str] = None
    metadata: Dict[str, Any] = field(default_factory=dict)

    def add_signal(self, signal: Dict[str, Any]) -> None:
        if self.status != MarketStatus.OPEN:
            raise ValueError(f"Cannot add signal to {self.status} market")
        self.signals.append(signal)

    def compute_consensus(self, source_reliability: Optional[Dict[str, Dict[str, float]]] = None) -> Dict[str, Any]:
        if not self.signals:
            return _empty_market_result(self)
        result = compute_consensus(self.signals, source_reliability)
        result["marketId"] = str(self.id)
        self.consensus_result = result
        return result

    def consensus_history(self, source_reliability: Optional[Dict[str, Dict[str, float]]] = None
                          ) -> List[Dict[str, Any]]:
        """The consensus after every signal arrived, in one launch (``batch.consensus_history``):
        entry k is ``{"signals": k + 1, "sourceId": that of signal k, "consensus": a float or None,
        "confidence", "totalWeight", "sourceCount"}``, equal to the corresponding fields of
        ``compute_consensus(self.signals[:k + 1], source_reliability)`` -- what calling
        ``add_signal`` and ``compute_consensus`` in turn would have returned (market.py:104-115).
        An empty market gives ``[]``; ``consensus_result`` is not touched."""
        if not self.signals:
            return []
        rel = source_reliability or {}
        ids = sorted({s["sourceId"] for s in self.signals})  # core.py:103
        rank = {sid: i for i, sid in enumerate(ids)}
        off, sid, prob = signals_csr([self.signals], rank)
        rows = [rel.get(i, {}) for i in ids]  # core.py:110-112
        N.require_gpu()
        T = batch.to_device(N.device())
        table = batch.SourceTable.from_arrays(
            T(np.array([float(r.get("reliability", DEFAULT_RELIABILITY)) for r in rows], np.float64)),
            T(np.array([float(r.get("confidence", DEFAULT_CONFIDENCE)) for r in rows], np.float64)),
            T(np.array([i in rel for i in ids], np.uint8)), ids)
        h = batch.consensus_history(T(off), T(sid), T(prob), table, offsets_host=off, check=True)
        return _history_rows(self.signals, *(x.cpu().numpy() for x in (h.consensus, h.confidence, h.total_weight,
                                                                       h.n_unique)))

    def leave_one_out(self, source_reliability: Optional[Dict[str, Dict[str, float]]] = None
                      ) -> List[Dict[str, Any]]:
        """What the consensus would be without each source, in one launch
        (``batch.leave_one_out``): one entry per sourceId in sorted() order, ``{"sourceId",
        "consensus": a float or None, "confidence", "totalWeight", "sourceCount", "influence"}``.
        The first four equal the corresponding fields of ``compute_consensus([s for s in
        self.signals if s["sourceId"] != sourceId], source_reliability)`` -- dropping the only source
        gives the values of a market without signals (core.py:88-96).  ``influence`` is the market's
        consensus minus that consensus, None where either is None.  An empty market gives ``[]``;
        ``consensus_result`` is not touched."""
        if not self.signals:
            return []
        rel = source_reliability or {}
        ids = sorted({s["sourceId"] for s in self.signals})  # core.py:103
        rank = {sid: i for i, sid in enumerate(ids)}
        off, sid, prob = signals_csr([self.signals], rank)
        rows = [rel.get(i, {}) for i in ids]  # core.py:110-112
        N.require_gpu()
        T = batch.to_device(N.device())
        table = batch.SourceTable.from_arrays(
            T(np.array([float(r.get("reliability", DEFAULT_RELIABILITY)) for r in rows], np.float64)),
            T(np.array([float(r.get("confidence", DEFAULT_CONFIDENCE)) for r in rows], np.float64)),
            T(np.array([i in rel for i in ids], np.uint8)), ids)
        loo = batch.leave_one_out(T(off), T(sid), T(prob), table, offsets_host=off, check=True)
        return _leave_one_out_rows(ids, sid, *_loo_host(loo), 0, 0, len(sid))

    def resolve(self, outcome: bool) -> None:
        self.outcome = outcome
        self.status = MarketStatus.RESOLVED
        self.resolved_at = datetime.now(timezone.utc).isoformat()


def _empty_market_result(market: Market) -> Dict[str, Any]:
    return {"schemaVersion": "1.0.0", "consensus": None, "confidence": 0.0, "marketId": str(market.id)}


class MarketStore:
    """In-memory store for markets (market.py:137-221)."""

    def __init__(self):
        self._markets: Dict[str, Market] = {}
        self._names: Optional[batch.NameTable] = None  # the ids in list_markets order, in HBM

    def create_market(self, market_id: MarketId, metadata: Optional[Dict[str, Any]] = None) -> Market:
        key = str(market_id)
        if key in self._markets:
            raise ValueError(f"Market {market_id} already exists")
        market = Market(id=market_id, metadata=metadata or {})
        self._markets[key] = market
        self._names = None
        return market

    def get_market(self, market_id: MarketId) -> Optional[Market]:
        return self._markets.get(str(market_id))

    def get_or_create(self, market_id: MarketId) -> Market:
        market = self.get_market(market_id)
        if market is None:
            market = self.create_market(market_id)
        return market

    def add_signal(self, market_id: MarketId, signal: Dict[str, Any]) -> Market:
        market = self.get_or_create(market_id)
        market.add_signal(signal)
        return market

    def list_markets(self, status: Optional[MarketStatus] = None, pattern: Optional[str] = None) -> List[Market]:
        markets = list(self._markets.values())
        if status is not None:
            markets = [m for m in markets if m.status == status]
        if pattern is not None:
            markets = [m for m in markets if m.id.matches(pattern)]
        return markets

    def name_table(self) -> "batch.NameTable":
        """The ids of every market in ``list_markets()`` order, packed in HBM for the glob kernel;
        cached, rebuilt after a market is created."""
        N.require_gpu()
        if self._names is None or self._names.n != len(self._markets):
            self._names = batch.NameTable.from_strings(list(self._markets), N.device())
        return self._names

    def match_many(self, patterns: List[str]):
        """Every pattern against every market id in one launch (``batch.glob_match``):
        ``(globs, bits)``.  Row ``globs.index[i]`` of ``bits`` holds, at the market's position in
        ``list_markets()``, whether ``market.id.matches(patterns[i])`` (market.py:74-82)."""
        globs = batch.GlobSet.compile(patterns)
        return globs, batch.glob_match(self.name_table(), globs)

    def match_any(self, patterns: List[str]) -> np.ndarray:
        """bool [n_markets] in ``list_markets()`` order: the id matches any of the patterns."""
        globs, bits = self.match_many(patterns)
        rows = torch.tensor(sorted(set(globs.index)), dtype=torch.int64, device=bits.device)
        return batch.glob_mask(batch.glob_any(bits, rows), len(self._markets)).cpu().numpy()

    def compute_all_consensus(self, reliability_store: Optional[SQLiteReliabilityStore] = None, *,
                              pair_table: bool = False, domain_of=None) -> Dict[str, Dict[str, Any]]:
        """Consensus for all open markets in ONE batched launch (market.py:200-221).

        ``pair_table=True`` (with a store) reads the (source, market) rows through
        ``load_pair_table`` and ``batch.consensus_pairs``: chunked SQL, a sparse table in HBM and
        one lookup launch instead of a query per market and a host loop per pair.  Same dicts.

        ``domain_of`` (a callable ``Market -> Optional[str]``, or ``"category"`` for
        ``market.id.category``) needs a :class:`NamespacedReliabilityStore` (else ``TypeError``)
        and reads every source of every market through its fallback chain,
        ``get_reliability(sid, market_id=str(market.id), domain=domain_of(market),
        apply_decay=True)``, the markets of all domains in one batch (the pair-table route)."""
        if domain_of is not None:
            if not isinstance(reliability_store, NamespacedReliabilityStore):
                raise TypeError("domain_of= needs a NamespacedReliabilityStore "
                                f"(got {type(reliability_store).__name__})")
            domain_of = _domain_fn(domain_of)
        markets = self.list_markets(status=MarketStatus.OPEN)
        busy = [m for m in markets if m.signals]
        computed: Dict[str, Dict[str, Any]] = {}
        if busy and domain_of is not None:
            computed = _batched_consensus_pairs(busy, reliability_store, domain_of)
        elif busy and pair_table and reliability_store is not None:
            computed = _batched_consensus_pairs(busy, reliability_store)
        elif busy:
            computed = _batched_consensus(busy, reliability_store)
        results: Dict[str, Dict[str, Any]] = {}
        for market in markets:
            key = str(market.id)
            if not market.signals:
                results[key] = _empty_market_result(market)
            else:
                res = computed[key]
                market.consensus_result = res
                results[key] = res
        return results

    def compute_all_history(self, reliability_store: Optional[SQLiteReliabilityStore] = None
                            ) -> Dict[str, List[Dict[str, Any]]]:
        """``Market.consensus_history`` for all open markets in ONE batched launch: market id ->
        the list of its entries (``[]`` for a market without signals).  The table is the one
        ``compute_all_consensus`` reads: with a store, every (source, market) pair fetched and
        decayed at "now" (market.py:208-219).  No market's ``consensus_result`` is touched."""
        markets = self.list_markets(status=MarketStatus.OPEN)
        busy = [m for m in markets if m.signals]
        computed = _batched_history(busy, reliability_store) if busy else {}
        return {str(m.id): computed.get(str(m.id), []) for m in markets}

    def compute_all_leave_one_out(self, reliability_store: Optional[SQLiteReliabilityStore] = None
                                  ) -> Dict[str, List[Dict[str, Any]]]:
        """``Market.leave_one_out`` for all open markets in ONE batched launch: market id -> the
        list of its entries (``[]`` for a market without signals), over the table
        ``compute_all_consensus`` reads (:meth:`compute_all_history`).  No market's
        ``consensus_result`` is touched."""
        markets = self.list_markets(status=MarketStatus.OPEN)
        busy = [m for m in markets if m.signals]
        computed = _batched_leave_one_out(busy, reliability_store) if busy else {}
        return {str(m.id): computed.get(str(m.id), []) for m in markets}


def _domain_fn(domain_of):
    """``domain_of=``: a callable ``Market -> Optional[str]``, or "category" (MarketId.category)."""
    if domain_of == "category":
        return lambda market: market.id.category
    if not callable(domain_of):
        raise TypeError(f"domain_of must be a callable Market -> Optional[str] or 'category' (got {domain_of!r})")
    return domain_of


class _FirstSeen(dict):
    """sourceId -> rank in first-seen order: looking up a new id ranks it."""

    def __missing__(self, key):
        self[key] = rank = len(self)
        return rank


def _batched_table(markets: List[Market], store: Optional[SQLiteReliabilityStore]):
    """The batch ``_batched_consensus``, ``_batched_history`` and ``_batched_leave_one_out`` run on:
    CSR over the markets, ranks
    over (market position, sorted sourceId), and the consensus table over those ranks -- with a
    store, every (source, market) pair fetched and decayed at "now".  Returns ``(per_market_ids,
    off, (offsets, sid, prob) on the device, table)``."""
    per_market_ids: List[List[str]] = []
    key_names: List[str] = []

    def rank_market(mpos, signals):
        ids = sorted({s["sourceId"] for s in signals})
        base = len(key_names)
        per_market_ids.append(ids)
        key_names.extend(ids)
        return {sid: base + i for i, sid in enumerate(ids)}

    off, sid, prob = signals_csr([m.signals for m in markets], rank_market)
    S = len(key_names)
    dev = N.device()
    N.require_gpu()
    T = batch.to_device(dev)
    rel = np.full(max(S, 2), DEFAULT_RELIABILITY)
    conf = np.full(max(S, 2), DEFAULT_CONFIDENCE)
    present = np.zeros(max(S, 2), np.uint8)
    if store is not None:
        # every sourceId gets a dict entry (market.py:209-219): none is cold-start
        present[:S] = 1
        pairs = [(sid, str(m.id)) for m, ids in zip(markets, per_market_ids) for sid in ids]
        rows = store.fetch_pairs(pairs)
        t_us = np.full(max(S, 2), NO_TIMESTAMP, np.int64)
        for k, pair in enumerate(pairs):
            row = rows.get(pair)
            if row is not None:
                rel[k], conf[k], t_us[k] = row[0], row[1], iso_to_us(row[2])
        rt = batch.ReliabilityTable(T(rel[:S]), T(conf[:S]), T(t_us[:S]), T(present[:S]), key_names)
        # get_reliability(apply_decay=True) for every pair, "now" read like decay.py:136-137
        table = rt.consensus_table(dt_to_us(_decay.datetime.now(timezone.utc)))
    else:
        table = batch.SourceTable.from_arrays(T(rel[:S]), T(conf[:S]), T(present[:S]), key_names)
    return per_market_ids, off, (T(off), T(sid), T(prob)), table


def _batched_consensus(markets: List[Market], store: Optional[SQLiteReliabilityStore]) -> Dict[str, Dict[str, Any]]:
    """One consensus launch over the batch of :func:`_batched_table`."""
    per_market_ids, off, csr, table = _batched_table(markets, store)
    res = batch.consensus(*csr, table, validate=False, check=True)
    return _render_markets(markets, per_market_ids, off, res)


def _history_rows(signals, cons, confd, tot, nu) -> List[Dict[str, Any]]:
    """``Market.consensus_history``'s entries from one market's slices of a HistoryResult."""
    rows = []
    for k, s in enumerate(signals):
        null = tot[k] == 0  # core.py:131
        rows.append({"signals": k + 1, "sourceId": s["sourceId"], "consensus": None if null else float(cons[k]),
                     "confidence": 0.0 if null else float(confd[k]), "totalWeight": float(tot[k]),
                     "sourceCount": int(nu[k])})
    return rows


def _batched_history(markets: List[Market], store: Optional[SQLiteReliabilityStore]) -> Dict[str, List[Dict[str, Any]]]:
    """One history launch (``batch.consensus_history``) over the batch of :func:`_batched_table`."""
    _, off, csr, table = _batched_table(markets, store)
    h = batch.consensus_history(*csr, table, offsets_host=off, check=True)
    cons, confd, tot, nu = (x.cpu().numpy() for x in (h.consensus, h.confidence, h.total_weight, h.n_unique))
    return {str(m.id): _history_rows(m.signals, cons[a:b], confd[a:b], tot[a:b], nu[a:b])
            for m, a, b in zip(markets, off[:-1], off[1:])}


def _loo_host(loo):
    """A :class:`batch.LeaveOneOutResult` as host arrays: the four per-signal ones, then the full
    consensus and total weight per market."""
    return tuple(x.cpu().numpy() for x in (loo.consensus, loo.confidence, loo.total_weight, loo.n_unique,
                                           loo.full.consensus, loo.full.total_weight))


def _leave_one_out_rows(ids, sid, cons, confd, tot, nu, full_cons, full_tot, mpos, a, b) -> List[Dict[str, Any]]:
    """``Market.leave_one_out``'s entries for the market at batch position ``mpos`` with signals
    ``[a, b)``: ``ids`` its sourceIds in sorted() order, ``sid`` the batch's ranks (ascending with
    ``ids`` inside the market); a source's values are read at its first signal."""
    first: Dict[int, int] = {}
    for p in range(a, b):
        first.setdefault(int(sid[p]), p)
    full_null = full_tot[mpos] == 0  # core.py:131
    rows = []
    for name, s in zip(ids, sorted(first)):
        p = first[s]
        null = tot[p] == 0  # nothing left, or no weight left
        rows.append({"sourceId": name, "consensus": None if null else float(cons[p]),
                     "confidence": 0.0 if null else float(confd[p]), "totalWeight": float(tot[p]),
                     "sourceCount": int(nu[p]),
                     "influence": None if null or full_null else float(full_cons[mpos] - cons[p])})
    return rows


def _batched_leave_one_out(markets: List[Market], store: Optional[SQLiteReliabilityStore]
                           ) -> Dict[str, List[Dict[str, Any]]]:
    """One launch (``batch.leave_one_out``) over the batch of :func:`_batched_table`."""
    per_market_ids, off, csr, table = _batched_table(markets, store)
    loo = batch.leave_one_out(*csr, table, offsets_host=off, check=True)
    host = _loo_host(loo)
    sid = csr[1].cpu().numpy()
    return {str(m.id): _leave_one_out_rows(ids, sid, *host, mpos, int(off[mpos]), int(off[mpos + 1]))
            for mpos, (m, ids) in enumerate(zip(markets, per_market_ids))}


def _render_markets(markets: List[Market], per_market_ids, offsets, res) -> Dict[str, Dict[str, Any]]:
    """The dicts of a batch: market i's sorted sourceIds are ``per_market_ids[i]`` and its unique
    slots start at ``offsets[i]``; a set sign bit of ``usid`` marks a cold-start source."""
    cons, confd, tot, usid, weight, nweight = (x.cpu().numpy() for x in (
        res.consensus, res.confidence, res.total_weight, res.usid, res.weight, res.nweight))
    out = {}
    for mpos, (market, ids) in enumerate(zip(markets, per_market_ids)):
        a, b = offsets[mpos], offsets[mpos] + len(ids)
        out[str(market.id)] = consensus_dict(ids, weight[a:b], nweight[a:b], cons[mpos], confd[mpos], tot[mpos],
                                             len(market.signals), [s for s, r in zip(ids, usid[a:b]) if r < 0],
                                             str(market.id))
    return out


def _batched_consensus_pairs(markets: List[Market], store, domain_of=None) -> Dict[str, Dict[str, Any]]:
    """_batched_consensus with a store, through the pair table: sources ranked once over the
    batch, the (source, market) rows loaded by ``load_pair_table`` and looked up on the GPU
    (``batch.consensus_pairs``, store mode: every sourceId is in the dict, market.py:209-219).

    With ``domain_of`` the store is a NamespacedReliabilityStore and the lookup is its
    ``get_reliability(sid, market_id=str(market.id), domain=domain_of(market), apply_decay=True)``:
    the rows of the batch's domains are a second pair table over the domain index and every
    market carries its domain (``batch.consensus_pairs(domains=, market_domain=)``)."""
    rank = batch.intern(s["sourceId"] for m in markets for s in m.signals)
    names = list(rank)
    off, sid, prob = signals_csr([m.signals for m in markets], rank)
    N.require_gpu()
    dev = N.device()
    T = batch.to_device(dev)
    namespaced = {}
    if domain_of is not None:
        doms = [domain_of(m) for m in markets]
        drank = {d: i for i, d in enumerate(dict.fromkeys(d for d in doms if d))}
        namespaced = dict(
            namespaced=True,
            domains=store._store.load_pair_table([f"__domain__:{d}" for d in drank], names, device=dev),
            market_domain=T(np.array([drank[d] if d else -1 for d in doms], np.int32)),
            global_scope=store._scope(store.GLOBAL_MARKET_ID, names, dev)[0])
        store = store._store
    pairs = store.load_pair_table([str(m.id) for m in markets], names, device=dev)
    # get_reliability(apply_decay=True) for every pair, "now" read like decay.py:136-137
    now_us = dt_to_us(_decay.datetime.now(timezone.utc))
    pc = batch.consensus_pairs(T(off), T(sid), T(prob), pairs, now_us, validate=False, check=True, **namespaced)
    uoff = pc.plan.uoffsets.cpu().numpy()
    esrc = pc.plan.usid.cpu().numpy()
    # sorted(): entries ascend with the rank
    ids = [[names[s] for s in esrc[uoff[mpos]:uoff[mpos + 1]]] for mpos in range(len(markets))]
    return _render_markets(markets, ids, off, pc.result)


@dataclass
class SourcePerformance:
    """Aggregated performance of a source across markets (market.py:224-241)."""

    source_id: str
    total_markets: int
    correct_predictions: int
    wrong_predictions: int
    reliability: float
    markets: List[str] = field(default_factory=list)

    @property
    def accuracy(self) -> float:
        total = self.correct_predictions + self.wrong_predictions
        if total == 0:
            return 0.0
        return self.correct_predictions / total


@dataclass
class BacktestScore:
    """The forecasts of one group of markets against their outcomes (``score_walk`` /
    ``sweep_decay``): ``n`` scored markets, mean Brier score, mean log loss, accuracy of the
    ``>= 0.5`` vote and expected calibration error (None where ``n == 0``); ``calibration`` one row
    per non-empty bin: ``{"bin", "lo", "hi", "n", "mean_forecast", "observed"}``; the markets
    left out are counted in ``n_unresolved`` / ``n_null`` (no consensus) / ``n_bad`` (a forecast
    outside [0, 1]).  ``params``: the grid point of a sweep."""

    n: int
    brier: Optional[float]
    log_loss: Optional[float]
    accuracy: Optional[float]
    ece: Optional[float]
    calibration: List[Dict[str, Any]] = field(default_factory=list)
    n_unresolved: int = 0
    n_null: int = 0
    n_bad: int = 0
    params: Optional[Dict[str, float]] = None

    @classmethod
    def empty(cls, n_bins: int, params: Optional[Dict[str, float]] = None) -> "BacktestScore":
        return cls(0, None, None, None, None, [], 0, 0, 0, params)

    @classmethod
    def from_result(cls, r: "batch.ScoreResult") -> List["BacktestScore"]:
        """One per group of a 2-D :class:`batch.ScoreResult`."""
        counts = r.counts.cpu().numpy()
        brier, ll, acc, ece = (x.cpu().numpy() for x in (r.brier, r.log_loss, r.accuracy, r.ece))
        mean, obs = (x.cpu().numpy() for x in r.calibration)
        bin_n = r.bin_n.cpu().numpy()
        B = bin_n.shape[1]
        out = []
        for g in range(counts.shape[0]):
            n = int(counts[g, 0])
            rows = [{"bin": b, "lo": b / B, "hi": (b + 1) / B, "n": int(bin_n[g, b]),
                     "mean_forecast": float(mean[g, b]), "observed": float(obs[g, b])}
                    for b in range(B) if bin_n[g, b]]
            val = lambda x: float(x[g]) if n else None  # noqa: E731
            out.append(cls(n, val(brier), val(ll), val(acc), val(ece), rows, int(counts[g, 2]), int(counts[g, 3]),
                           int(counts[g, 4])))
        return out


@dataclass
class SourceScore:
    """One source's own signals against the outcomes (``score_walk(sources=True)``): ``n`` scored
    signals, mean Brier score, mean log loss, accuracy, and ``skill`` = its Brier score minus the
    consensus's over the same signals (negative: better than the consensus); NaN where n == 0."""

    source_id: str
    n: int
    brier: float
    log_loss: float
    accuracy: float
    skill: float


@dataclass
class WalkScore:
    """``CrossMarketAggregator.score_walk``: the whole history, one score per pattern list, per
    domain, and per source."""

    overall: BacktestScore
    groups: List[BacktestScore]
    domains: Dict[str, BacktestScore]
    sources: Dict[str, SourceScore]


@dataclass
class DecayRow:
    """One grid point of a :class:`DecayComparison`: ``n`` scored markets, the point estimate
    ``value`` of the metric with its percentile interval ``[lo, hi]``, the paired difference
    ``diff`` against the reference point (this point minus the reference, under the same
    resamples) with ``[diff_lo, diff_hi]``, ``p_better`` = the share of replicates in which this
    point is strictly better than the reference, ``p_best`` = the share in which it is the best
    of the grid.  None where nothing was scored."""

    params: Dict[str, float]
    n: int
    value: Optional[float]
    lo: Optional[float]
    hi: Optional[float]
    diff: Optional[float]
    diff_lo: Optional[float]
    diff_hi: Optional[float]
    p_better: Optional[float]
    p_best: Optional[float]


@dataclass
class DecayComparison:
    """``CrossMarketAggregator.compare_decay``: one :class:`DecayRow` per grid point (row-major,
    ``min_rel`` fastest), ``best`` = the index of the best point estimate (None where nothing was
    scored) and ``reference`` = the index every ``diff`` / ``p_better`` is taken against."""

    rows: List[DecayRow]
    best: Optional[int]
    reference: Optional[int]
    metric: str
    level: float
    n_boot: int
    seed: int
    block: int


COMPARE_METRICS = ("brier", "log_loss", "accuracy", "skill")


def _compare_arguments(what, store, half_life_days, min_rel, n_boot, block, metric, level, reference):
    """The checked arguments of a decay comparison: ``(half_life_days, min_rel)``."""
    hl, mr, _ = _sweep_arguments(what, store, half_life_days, min_rel, 10)
    _check_boot(n_boot, block)
    if isinstance(reference, bool) or not (reference is None or isinstance(reference, (int, np.integer))):
        raise TypeError(f"reference must be a grid index or None (got {type(reference).__name__})")
    if reference is not None and not 0 <= reference < len(hl) * len(mr):
        raise ValueError(f"reference must be a grid index in [0, {len(hl) * len(mr)}) (got {reference})")
    if metric not in COMPARE_METRICS:
        raise ValueError(f"metric must be one of {COMPARE_METRICS} (got {metric!r})")
    if metric == "skill":
        raise ValueError("metric 'skill' needs a base forecast: a decay comparison has none")
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must be in (0, 1) (got {level})")
    return hl, mr


def _comparison(run, hl, mr, metric, level, reference, n_boot, seed, block, params=None) -> "DecayComparison":
    """The :class:`DecayComparison` of a store's ``(scores, boot)`` (None: no signals); ``params``:
    the grid points where they are not the decay grid alone."""
    if params is None:
        params = [{"half_life_days": h, "min_rel": m} for h in hl for m in mr]
    level = float(level)
    if run is None:
        rows = [DecayRow(p, 0, None, None, None, None, None, None, None, None) for p in params]
        return DecayComparison(rows, None, reference, metric, level, n_boot, seed, block)
    _, boot = run
    point = boot.point(metric)[0].cpu().numpy()
    n = boot.W[0, 0].cpu().numpy()
    finite = ~np.isnan(point)
    best = None
    if finite.any():
        key = np.where(finite, -point if metric == "accuracy" else point, np.inf)
        best = int(np.argmin(key))  # the first of equal point estimates
    ref = best if reference is None else int(reference)
    lo, hi = (x[0].cpu().numpy() for x in boot.interval(metric, level))
    p_best = boot.p_best(metric)[0].cpu().numpy()
    none = [None] * len(params)
    d = d_lo = d_hi = p_better = none
    if ref is not None:
        dd, dl, dh = boot.diff(metric, ref, level)
        d, d_lo, d_hi = dd[0, 0].cpu().numpy(), dl[0].cpu().numpy(), dh[0].cpu().numpy()
        p_better = boot.p_better(metric, ref)[0].cpu().numpy()
    val = lambda x, k: None if x[k] is None or math.isnan(float(x[k])) else float(x[k])  # noqa: E731
    rows = [DecayRow(p, int(n[k]), val(point, k), val(lo, k), val(hi, k), val(d, k), val(d_lo, k), val(d_hi, k),
                     val(p_better, k), val(p_best, k)) for k, p in enumerate(params)]
    return DecayComparison(rows, best, ref, metric, level, n_boot, seed, block)


def _keyed_results(keyed, results) -> Dict[str, Dict[str, Any]]:
    """The result dicts of a walk keyed by ``str(market.id)``, in walk order."""
    out = {}
    for (_, _, m, _), r in zip(keyed, results):
        r["marketId"] = str(m.id)
        out[str(m.id)] = r
    return out


def _sweep_arguments(what: str, store, half_life_days, min_rel, n_bins):
    """The checked arguments of a decay sweep: ``(half_life_days, min_rel, n_bins)``."""
    if not isinstance(store, NamespacedReliabilityStore):
        raise TypeError(f"{what} needs a NamespacedReliabilityStore (got {type(store).__name__})")
    try:
        hl, mr = [float(x) for x in half_life_days], [float(x) for x in min_rel]
    except TypeError:
        raise TypeError("half_life_days and min_rel must be sequences of numbers") from None
    if not hl or not mr:
        raise ValueError(f"{what} needs at least one half_life_days and one min_rel")
    if any(not h > 0 for h in hl):
        raise ValueError(f"half_life_days must be > 0 (got {hl})")
    if any(not 0.0 <= m <= 1.0 for m in mr):
        raise ValueError(f"min_rel must be in [0, 1] (got {mr})")
    B = int(n_bins)
    if not 1 <= B <= batch.SCORE_MAX_BINS:
        raise ValueError(f"n_bins must be in [1, {batch.SCORE_MAX_BINS}] (got {n_bins})")
    return hl, mr, B


def _update_arguments(what: str, store, learning_rate, max_step, half_life_days, min_rel, n_bins):
    """The checked arguments of an update-rule sweep: ``(params, half_life_days, min_rel,
    n_bins)``, ``params`` one dict per grid point, the update point slowest."""
    hl, mr, B = _sweep_arguments(what, store, half_life_days, min_rel, n_bins)
    batch.update_steps(learning_rate, max_step)  # TypeError / ValueError
    lr = [float(x) for x in np.atleast_1d(np.asarray(learning_rate, np.float64))]
    ms = [float(x) for x in np.atleast_1d(np.asarray(max_step, np.float64))]
    if len(ms) == 1:
        ms = ms * len(lr)
    params = [{"learning_rate": r, "max_step": c, "half_life_days": h, "min_rel": m}
              for r, c in zip(lr, ms) for h in hl for m in mr]
    return params, hl, mr, B


def _sweep_rows(scores, hl, mr, B, params=None) -> List["BacktestScore"]:
    """One :class:`BacktestScore` per grid point of a store sweep (None: a history without
    signals); ``params``: the grid points where they are not the decay grid alone."""
    if params is None:
        params = [{"half_life_days": h, "min_rel": m} for h in hl for m in mr]
    if scores is None:
        return [BacktestScore.empty(B, p) for p in params]
    flat = batch.ScoreResult(*(getattr(scores, k)[:, 0] for k in ("counts", "sums", "bin_n", "bin_pos", "bin_psum")))
    rows = BacktestScore.from_result(flat)
    for r, p in zip(rows, params):
        r.params = p
    return rows


class CrossMarketAggregator:
    """Aggregate data across multiple markets (market.py:244-408)."""

    def __init__(self, market_store: MarketStore):
        self._store = market_store

    def _device_route(self, n_patterns: int, device_match: Optional[bool]) -> bool:
        """``device_match``: True / False force the GPU glob kernels / the fnmatch loop; None picks
        the GPU once (markets) x (patterns) reaches DEVICE_MATCH_MIN_PAIRS.  Without a visible GPU
        None keeps the fnmatch loop, so the calls that never reach a kernel (nothing matched, a
        store of one's own behind settle_resolved) still need none; True raises NativeUnavailable."""
        if device_match is not None:
            return bool(device_match)
        if DEVICE_MATCH_MIN_PAIRS is None or not torch.cuda.is_available():
            return False
        return len(self._store._markets) * n_patterns >= DEVICE_MATCH_MIN_PAIRS

    def _select(self, status: Optional[MarketStatus], patterns: Optional[List[str]],
                device_match: Optional[bool], with_signals: bool = False) -> List[Market]:
        """list_markets(status), optionally only markets with signals, filtered by "matches any
        pattern", order kept; on the device route the pattern filter is one launch over every id
        (MarketStore.match_any)."""
        if not patterns or not self._device_route(len(patterns), device_match):
            markets = self._store.list_markets(status=status)
            if with_signals:
                markets = [m for m in markets if m.signals]
            if patterns:
                markets = [m for m in markets if any(m.id.matches(p) for p in patterns)]
            return markets
        hit = self._store.match_any(patterns)
        return [m for m, h in zip(self._store.list_markets(), hit)
                if h and (status is None or m.status == status) and (m.signals or not with_signals)]

    def summarize_sources(self, patterns: Optional[List[str]] = None,
                          device_match: Optional[bool] = None) -> Dict[str, SourcePerformance]:
        markets = self._select(MarketStatus.RESOLVED, patterns, device_match)
        markets = [m for m in markets if m.outcome is not None]
        order = _FirstSeen()  # a sourceId is ranked when its signal is reached, as the reference's dict fills
        off, sid, prob = signals_csr([m.signals for m in markets], order, settlement=True)
        names = list(order)
        market_lists: List[List[str]] = [[] for _ in names]
        for market, a, b in zip(markets, off[:-1], off[1:]):
            for s in sid[a:b]:
                market_lists[s].append(str(market.id))
        outcome = [1 if market.outcome else 0 for market in markets]
        results: Dict[str, SourcePerformance] = {}
        if not names:
            return results
        N.require_gpu()
        T = batch.to_device(N.device())
        correct, total = batch.agreement_stats(T(off), T(sid), T(prob), T(np.array(outcome, np.int8)), len(names))
        correct = correct.cpu().numpy()
        total = total.cpu().numpy()
        for i, sid in enumerate(names):
            c, t = int(correct[i]), int(total[i])
            w = t - c
            results[sid] = SourcePerformance(sid, t, c, w, c / (c + w) if (c + w) > 0 else 0.5, market_lists[i])
        return results

    def reestimate_sources(self, iters: int = 10, patterns: Optional[List[str]] = None,
                           prior: float = 0.5, device_match: Optional[bool] = None) -> Dict[str, SourcePerformance]:
        """Learned source reliabilities over every market that has signals, resolved or not:
        ``iters`` rounds of consensus <-> reliability (batch.reestimate_csr), every source
        starting at ``prior``.  A RESOLVED market with an outcome is scored against that outcome,
        as summarize_sources does; any other market against its own consensus vote
        (``consensus >= 0.5``), and is left out of a round in which it has no consensus or holds
        a probability outside [0, 1].  Sources are interned in sorted() order, so every
        consensus sums in compute_consensus's order (core.py:103).  ``reliability`` is the
        weight after the last round; the counts and market lists are the last round's, laid
        out as summarize_sources lays them out."""
        markets = self._select(None, patterns, device_match, with_signals=True)
        results: Dict[str, SourcePerformance] = {}
        if not markets:
            return results
        rank = batch.intern(signal["sourceId"] for m in markets for signal in m.signals)
        off, sid, prob = signals_csr([m.signals for m in markets], rank, settlement=True)
        known: List[int] = []
        for market in markets:
            resolved = market.status == MarketStatus.RESOLVED and market.outcome is not None
            known.append((1 if market.outcome else 0) if resolved else -1)
        N.require_gpu()
        T = batch.to_device(N.device())
        plan = batch.ReestimateCsrPlan.build(T(off), T(sid), T(prob), len(rank))
        r = batch.reestimate_csr(plan, iters, w0=prior, known=T(np.array(known, np.int8)))
        w = r.w.cpu().numpy()
        correct = r.correct.cpu().numpy()
        total = r.total.cpu().numpy()
        outcome = r.outcome.cpu().numpy()
        market_lists: Dict[str, List[str]] = {}
        for market, o in zip(markets, outcome):
            if o < 0:
                continue
            for signal in market.signals:
                market_lists.setdefault(signal["sourceId"], []).append(str(market.id))
        for sid, lst in market_lists.items():
            c, t = int(correct[rank[sid]]), int(total[rank[sid]])
            results[sid] = SourcePerformance(sid, t, c, t - c, float(w[rank[sid]]), lst)
        return results

    def settle_resolved(self, store, domain: Optional[str] = None, update_global: bool = False,
                        patterns: Optional[List[str]] = None, dry_run: bool = False, market_scope: bool = False,
                        device_match: Optional[bool] = None, domain_of=None):
        """Commit every RESOLVED market with an outcome to the reliability store: the markets
        summarize_sources counts over, in the same order (list_markets, the pattern filter, then
        ``outcome is not None``), passed as ``(signals, outcome)`` to
        ``store.settle_markets`` (:class:`NamespacedReliabilityStore`), which applies
        ``update_reliability`` per signal at the domain or global scope in one compiled batch.
        ``market_scope=True`` passes ``str(market.id)`` for every resolved market, so the rows
        keyed by (source, market) are settled instead (``update_reliability(market_id=...)``, what
        the reference's ``report-outcome --market-id`` writes).  Returns the store's summary: the
        records and the ``total`` / ``correct`` counts per source (per pair at market scope).
        ``domain_of`` (as in ``compute_all_consensus``; together with ``domain=``, ``ValueError``)
        settles every market at the scope of its own domain: ``domains=[domain_of(m), ...]``."""
        if domain_of is not None:
            if domain is not None:
                raise ValueError("domain= (one for the batch) and domain_of= (one per market) exclude each other")
            domain_of = _domain_fn(domain_of)
        markets = self._select(MarketStatus.RESOLVED, patterns, device_match)
        markets = [m for m in markets if m.outcome is not None]
        if domain_of is not None:
            return store.settle_markets([(m.signals, m.outcome) for m in markets], update_global=update_global,
                                        dry_run=dry_run, domains=[domain_of(m) for m in markets],
                                        market_ids=[str(m.id) for m in markets] if market_scope else None)
        if market_scope:
            return store.settle_markets([(m.signals, m.outcome) for m in markets], domain=domain,
                                        update_global=update_global, dry_run=dry_run,
                                        market_ids=[str(m.id) for m in markets])
        return store.settle_markets([(m.signals, m.outcome) for m in markets], domain=domain,
                                    update_global=update_global, dry_run=dry_run)

    def walk_forward(self, store, patterns: Optional[List[str]] = None, domain: Optional[str] = None,
                     dry_run: bool = False, device_match: Optional[bool] = None, domain_of=None,
                     update_global: bool = False, market_scope: bool = False, lagged: bool = False):
        """A back-test over the store's history: every market with signals (selected as
        reestimate_sources selects them), ordered by (time, store position) -- ``resolved_at`` for
        a RESOLVED market with an outcome, ``created_at`` otherwise -- is scored with the
        reliabilities as they stood after the markets before it were settled and decayed to its
        own time, then settled itself if it is resolved; unresolved markets read and commit
        nothing (``store.walk_forward``, :class:`NamespacedReliabilityStore`).  Returns
        ``(results, summary)``: the consensus dict of every market keyed by ``str(market.id)``, in
        walk order, and the store's settle summary.

        ``domain_of`` (as in ``settle_resolved``; together with ``domain=``, ``ValueError``) walks
        a history that spans domains: every market is read with the fallback market -> domain ->
        global -> cold start and settled at the scope of its own domain, ``update_global`` as
        ``update_reliability`` takes it (``store.walk_forward_namespaced``); ``market_scope=True``
        passes ``str(market.id)`` so that seeded (source, market) rows are read first.  Without
        ``domain_of`` the two flags are not used.

        ``lagged=True`` keeps a market's two events apart: every market is forecast at
        ``created_at`` and a resolved one settled at ``resolved_at``, the order is (``created_at``,
        store position), and a market reads only the outcomes that had arrived by its forecast
        (``store.walk_forward(resolve_times=)``).  A resolved market whose ``resolved_at`` is
        missing or earlier than its ``created_at`` is a ``ValueError`` that names it.  The lagged
        walk here is single-scope: together with ``domain_of=``, ``ValueError``
        (:meth:`walk_forward_namespaced` walks a history that spans domains with lag)."""
        if lagged and domain_of is not None:
            raise ValueError("lagged=True walks one scope: it cannot be combined with domain_of= "
                             "(walk_forward_namespaced(lagged=True) does that)")
        if domain_of is not None:
            if domain is not None:
                raise ValueError("domain= (one for the batch) and domain_of= (one per market) exclude each other")
            return self.walk_forward_namespaced(store, _domain_fn(domain_of), patterns, update_global, market_scope,
                                                dry_run=dry_run, device_match=device_match)
        keyed, batch_markets, stamps, resolve_stamps = self._walk_history(patterns, device_match, lagged)
        if lagged:
            results, summary = store.walk_forward(batch_markets, stamps, domain=domain, dry_run=dry_run,
                                                  resolve_times=resolve_stamps)
        else:
            results, summary = store.walk_forward(batch_markets, stamps, domain=domain, dry_run=dry_run)
        return _keyed_results(keyed, results), summary

    def walk_forward_namespaced(self, store, domain_of, patterns: Optional[List[str]] = None,
                                update_global: bool = False, market_scope: bool = False, lagged: bool = False,
                                dry_run: bool = False, device_match: Optional[bool] = None):
        """:meth:`walk_forward` over a history that spans domains (``domain_of`` as there: a
        callable or "category"), immediate or ``lagged``: every market is read with the fallback
        market -> domain -> global -> cold start as the rows stood at its forecast, and a
        resolved one is settled at the scope of its own domain (``update_global`` as
        ``update_reliability`` takes it; ``market_scope=True`` reads seeded (source, market) rows
        first).  ``lagged=False`` returns exactly what ``walk_forward(domain_of=)`` returns;
        ``lagged=True`` forecasts every market at ``created_at`` and settles it at
        ``resolved_at``, so no read sees an outcome that had not arrived
        (``store.walk_forward_namespaced(resolve_times=)``).  Returns ``(results, summary)`` as
        :meth:`walk_forward`; ``score_walk`` takes the results."""
        if not isinstance(store, NamespacedReliabilityStore):
            raise TypeError(f"walk_forward_namespaced needs a NamespacedReliabilityStore (got {type(store).__name__})")
        keyed, batch_markets, stamps, resolve_stamps, kw = self._namespaced_history(
            domain_of, patterns, update_global, market_scope, lagged, device_match)
        results, summary = store.walk_forward_namespaced(batch_markets, stamps, dry_run=dry_run,
                                                         resolve_times=resolve_stamps, **kw)
        return _keyed_results(keyed, results), summary

    def _namespaced_history(self, domain_of, patterns, update_global, market_scope, lagged, device_match):
        """:meth:`_walk_history` plus the keyword arguments the namespaced store methods share."""
        if domain_of is None:
            raise ValueError("domain_of is needed: a callable market -> domain, or \"category\"")
        domain_of = _domain_fn(domain_of)
        keyed, batch_markets, stamps, resolve_stamps = self._walk_history(patterns, device_match, lagged)
        kw = dict(domains=[domain_of(m) for _, _, m, _ in keyed],
                  market_ids=[str(m.id) for _, _, m, _ in keyed] if market_scope else None,
                  update_global=update_global)
        return keyed, batch_markets, stamps, resolve_stamps, kw

    def _walk_history(self, patterns: Optional[List[str]], device_match: Optional[bool], lagged: bool = False):
        """The markets of a back-test in walk order: ``(keyed, batch_markets, stamps,
        resolve_stamps)`` with ``keyed`` = ``(time_us, store position, market, resolved)`` sorted
        by (time, position), ``batch_markets`` the ``(signals, outcome or None)`` pairs and
        ``stamps`` the ISO times.  ``lagged``: the time is ``created_at`` for every market, and
        ``resolve_stamps`` holds ``resolved_at`` of the resolved ones (else it is None)."""
        markets = self._select(None, patterns, device_match, with_signals=True)
        keyed = []
        for pos, m in enumerate(markets):
            resolved = m.status == MarketStatus.RESOLVED and m.outcome is not None
            stamp = m.resolved_at if resolved and m.resolved_at and not lagged else m.created_at
            t = iso_to_us(stamp)
            if t == NO_TIMESTAMP:
                raise ValueError(f"market {m.id}: no usable time ({stamp!r})")
            if lagged and resolved:
                r = iso_to_us(m.resolved_at) if m.resolved_at else NO_TIMESTAMP
                if r == NO_TIMESTAMP:
                    raise ValueError(f"market {m.id}: resolved without a usable resolved_at ({m.resolved_at!r})")
                if r < t:
                    raise ValueError(f"market {m.id}: resolved_at {m.resolved_at!r} is earlier than created_at "
                                     f"{m.created_at!r}")
            keyed.append((t, pos, m, resolved))
        keyed.sort(key=lambda k: k[:2])
        batch_markets = [(m.signals, m.outcome if resolved else None) for _, _, m, resolved in keyed]
        stamps = [us_to_iso(t) for t, _, _, _ in keyed]
        resolve_stamps = [m.resolved_at if resolved else None for _, _, m, resolved in keyed] if lagged else None
        return keyed, batch_markets, stamps, resolve_stamps

    def score_walk(self, results: Dict[str, Dict[str, Any]], pattern_lists: Optional[List[List[str]]] = None,
                   domain_of=None, n_bins: int = 10, sources: bool = True,
                   device_match: Optional[bool] = None) -> "WalkScore":
        """How good were the forecasts of a back-test?  ``results`` is the dict ``walk_forward``
        returns (market id -> consensus dict, in walk order); every market is scored against the
        store's own outcome (a RESOLVED market with an outcome; any other counts as unresolved):
        Brier score, log loss, accuracy (the ``>= 0.5`` vote, market.py:298-301), expected
        calibration error and the calibration rows, all summed on the GPU in one launch
        (``batch.score``, reproducible to the bit).  Returns a :class:`WalkScore`:

        ``overall``  the whole history;
        ``groups``   one :class:`BacktestScore` per pattern list (the markets of ``results`` that
                     match, per pattern in store order, duplicates kept as ``aggregate_many`` keeps
                     them; ``device_match`` as there: the member lists come from the glob kernels);
        ``domains``  with ``domain_of`` (a callable or "category"), one per domain, first seen first;
        ``sources``  with ``sources=True``, a :class:`SourceScore` per sourceId, interned in
                     first-seen order as ``summarize_sources`` does, every signal counted;
                     ``skill`` is the source's Brier score minus the consensus's on the markets it
                     forecast (markets without a consensus are left out of a source's scores)."""
        if not isinstance(results, dict):
            raise TypeError(f"results must be the dict walk_forward returns (got {type(results).__name__})")
        B = int(n_bins)
        if not 1 <= B <= batch.SCORE_MAX_BINS:
            raise ValueError(f"n_bins must be in [1, {batch.SCORE_MAX_BINS}] (got {n_bins})")
        if domain_of is not None:
            domain_of = _domain_fn(domain_of)
        if pattern_lists is not None and any(isinstance(p, str) for p in pattern_lists):
            raise TypeError("pattern_lists must be a list of pattern lists")
        pattern_lists = [list(p) for p in pattern_lists] if pattern_lists else []
        position = {key: i for i, key in enumerate(self._store._markets)}
        missing = [key for key in results if key not in position]
        if missing:
            raise KeyError(f"results names markets the store does not hold: {missing[:3]}")
        walk = [self._store._markets[key] for key in results]
        spos = np.array([position[key] for key in results], np.int64)
        Ms, Mw = len(position), len(walk)
        empty = BacktestScore.empty(B)
        if not walk:
            return WalkScore(empty, [empty for _ in pattern_lists], {}, {})
        code = np.array([(1 if m.outcome else 0) if m.status == MarketStatus.RESOLVED and m.outcome is not None
                         else -1 for m in walk], np.int8)
        cons_w = np.array([float(r["consensus"]) if r.get("consensus") is not None else 0.0
                           for r in results.values()], np.float64)
        valid_w = np.array([r.get("consensus") is not None for r in results.values()], np.uint8)
        # market groups index the arrays by store position (the glob kernels emit those)
        outcome = np.full(Ms, -1, np.int8)
        cons = np.zeros(Ms, np.float64)
        valid = np.zeros(Ms, np.uint8)
        outcome[spos], cons[spos], valid[spos] = code, cons_w, valid_w
        lists: List[np.ndarray] = [spos]
        dnames: List[str] = []
        if domain_of is not None:
            by_domain: Dict[str, List[int]] = {}
            for m, p in zip(walk, spos):
                d = domain_of(m)
                if d:
                    by_domain.setdefault(d, []).append(int(p))
            dnames = list(by_domain)
            lists += [np.array(by_domain[d], np.int64) for d in dnames]
        n_patterns = sum(len(p) for p in pattern_lists)
        N.require_gpu()
        dev = N.device()
        T = batch.to_device(dev)
        on_device = bool(n_patterns) and self._device_route(n_patterns, device_match)
        if not on_device:
            for patterns in pattern_lists:
                lists.append(np.array([position[str(m.id)] for pattern in patterns
                                       for m in self._store.list_markets(pattern=pattern)
                                       if str(m.id) in results], np.int64))
        goff = np.zeros(len(lists) + 1, np.int64)
        goff[1:] = np.cumsum([len(x) for x in lists])
        goff_t, members = T(goff), T(np.concatenate(lists))
        if on_device:
            globs, bits = self._store.match_many([p for patterns in pattern_lists for p in patterns])
            slot_groups = np.zeros(len(pattern_lists) + 1, np.int64)
            slot_groups[1:] = np.cumsum([len(patterns) for patterns in pattern_lists])
            rows = torch.tensor(globs.index, dtype=torch.int64, device=dev)
            pgoff, pmem = batch.glob_members(bits, Ms, rows, slot_groups)
            inres = torch.zeros(Ms, dtype=torch.bool, device=dev)
            inres[T(spos)] = True
            keep = inres[pmem]  # only the markets of the back-test
            run = torch.zeros(pmem.numel() + 1, dtype=torch.int64, device=dev)
            torch.cumsum(keep, 0, out=run[1:])
            goff_t = torch.cat([goff_t, goff_t[-1] + run[pgoff[1:]]])
            members = torch.cat([members, pmem[keep]])
        plan = batch.ScorePlan.groups(goff_t, members)
        ms = batch.score(plan, T(cons), T(outcome), valid=T(valid), n_bins=B)
        rows_ = BacktestScore.from_result(ms)
        nd = len(dnames)
        out = WalkScore(rows_[0], rows_[1 + nd:], dict(zip(dnames, rows_[1:1 + nd])), {})
        if sources:
            order = _FirstSeen()
            off, sid, prob = signals_csr([m.signals for m in walk], order, settlement=True)
            names = list(order)
            splan = batch.ScorePlan.by_source(T(off), T(sid), len(names))
            ss = batch.score_sources(splan, T(prob), T(code), consensus=T(cons_w), valid=T(valid_w), n_bins=B)
            n, brier, ll, acc, skill = (x.cpu().numpy() for x in (ss.n_scored, ss.brier, ss.log_loss, ss.accuracy,
                                                                   ss.skill))
            out.sources = {name: SourceScore(name, int(n[i]), float(brier[i]), float(ll[i]), float(acc[i]),
                                             float(skill[i])) for i, name in enumerate(names)}
        N.check_faults(dev, "score_walk")
        return out

    def source_influence(self, patterns: Optional[List[str]] = None,
                         reliability_store: Optional[SQLiteReliabilityStore] = None,
                         n_bins: int = 10) -> Dict[str, SourceScore]:
        """Was the consensus better or worse for having each source?  Over the selected markets
        that have signals (as ``reestimate_sources`` selects them), every market's consensus is
        computed with and without each of its sources in one launch (``batch.leave_one_out``, over
        the table ``compute_all_consensus`` reads) and scored against the store's own outcome, read
        as ``score_walk`` reads it.  Returns a :class:`SourceScore` per sourceId, interned in
        first-seen order as ``summarize_sources`` does, one item per (market, source)
        (``batch.score_leave_one_out(per="pair")``): ``n`` the scored markets of the source,
        ``brier`` / ``log_loss`` / ``accuracy`` those of the consensus WITHOUT the source, and
        ``skill`` that Brier score minus the full consensus's over the same markets -- positive:
        the consensus is worse without the source."""
        B = int(n_bins)
        if not 1 <= B <= batch.SCORE_MAX_BINS:
            raise ValueError(f"n_bins must be in [1, {batch.SCORE_MAX_BINS}] (got {n_bins})")
        markets = self._select(None, patterns, None, with_signals=True)
        if not markets:
            return {}
        code = np.array([(1 if m.outcome else 0) if m.status == MarketStatus.RESOLVED and m.outcome is not None
                         else -1 for m in markets], np.int8)
        order = _FirstSeen()
        gsid = np.array([order[s["sourceId"]] for m in markets for s in m.signals], np.int32)
        names = list(order)
        _, off, csr, table = _batched_table(markets, reliability_store)
        dev = N.device()
        T = batch.to_device(dev)
        loo = batch.leave_one_out(*csr, table, offsets_host=off, check=True)
        ss = batch.score_leave_one_out(loo, csr[0], T(gsid), T(code), len(names), per="pair", n_bins=B)
        n, brier, ll, acc, skill = (x.cpu().numpy() for x in (ss.n_scored, ss.brier, ss.log_loss, ss.accuracy,
                                                               ss.skill))
        N.check_faults(dev, "source_influence")
        return {name: SourceScore(name, int(n[i]), float(brier[i]), float(ll[i]), float(acc[i]), float(skill[i]))
                for i, name in enumerate(names)}

    def sweep_decay(self, store, half_life_days, min_rel, patterns: Optional[List[str]] = None,
                    domain: Optional[str] = None, n_bins: int = 10,
                    device_match: Optional[bool] = None, lagged: bool = False) -> List["BacktestScore"]:
        """The back-test of ``walk_forward(store, patterns, domain, dry_run=True)`` for every point
        of a grid of decay parameters: one whole-history :class:`BacktestScore` per
        ``(half_life_days[i], min_rel[j])``, row-major (``params`` names the point).  The
        settlement trace does not depend on the decay parameters, so it runs once
        (``store.sweep_decay``, ``batch.walk_sweep``); nothing is written to the store.  The
        single-scope walk only: a history that spans domains (``walk_forward(domain_of=)``) is
        swept by :meth:`sweep_decay_namespaced`.  ``lagged`` as in ``walk_forward``."""
        hl, mr, B = _sweep_arguments("sweep_decay", store, half_life_days, min_rel, n_bins)
        _, batch_markets, stamps, resolve_stamps = self._walk_history(patterns, device_match, lagged)
        scores = store.sweep_decay(batch_markets, stamps, hl, mr, domain=domain, n_bins=B,
                                   resolve_times=resolve_stamps)
        return _sweep_rows(scores, hl, mr, B)

    def sweep_decay_namespaced(self, store, half_life_days, min_rel, domain_of, patterns: Optional[List[str]] = None,
                               update_global: bool = False, market_scope: bool = False, lagged: bool = False,
                               n_bins: int = 10, device_match: Optional[bool] = None) -> List["BacktestScore"]:
        """:meth:`sweep_decay` over the namespaced walk: the back-test of
        ``walk_forward_namespaced(store, domain_of, ..., dry_run=True)``, immediate or ``lagged``,
        for every point of the grid, one whole-history :class:`BacktestScore` per point
        (``params`` names it).  Both chain families are traced once
        (``store.sweep_decay_namespaced``, ``batch.walk_sweep_scoped``); nothing is written."""
        hl, mr, B = _sweep_arguments("sweep_decay_namespaced", store, half_life_days, min_rel, n_bins)
        _, batch_markets, stamps, resolve_stamps, kw = self._namespaced_history(
            domain_of, patterns, update_global, market_scope, lagged, device_match)
        scores = store.sweep_decay_namespaced(batch_markets, stamps, hl, mr, n_bins=B, resolve_times=resolve_stamps,
                                              **kw)
        return _sweep_rows(scores, hl, mr, B)

    def compare_decay(self, store, half_life_days, min_rel, patterns: Optional[List[str]] = None,
                      domain: Optional[str] = None, lagged: bool = False, device_match: Optional[bool] = None,
                      n_boot: int = 1000, seed: int = 0, block: int = 1, metric: str = "brier", level: float = 0.95,
                      reference: Optional[int] = None) -> "DecayComparison":
        """:meth:`sweep_decay` with the question a sweep leaves open: is the best grid point
        better than the others, or is the difference noise?  The same walk and sweep, then a
        paired Poisson bootstrap over the markets on the GPU (``store.compare_decay``,
        ``batch.score_bootstrap``): every grid point is re-scored under the same ``n_boot``
        resamples (``seed``; ``block`` consecutive markets of the walk are resampled together, for
        a history whose neighbours depend on each other).  Returns a :class:`DecayComparison` for
        ``metric`` ("brier", "log_loss" or "accuracy"): per grid point the estimate with its
        ``level`` percentile interval, the paired difference against ``reference`` (a grid index;
        default: the point with the best estimate) with its interval, and the shares of
        replicates in which the point beats the reference / is the best of the grid."""
        hl, mr = _compare_arguments("compare_decay", store, half_life_days, min_rel, n_boot, block, metric, level,
                                    reference)
        _, batch_markets, stamps, resolve_stamps = self._walk_history(patterns, device_match, lagged)
        run = store.compare_decay(batch_markets, stamps, hl, mr, domain=domain, resolve_times=resolve_stamps,
                                  n_boot=n_boot, seed=seed, block=block)
        return _comparison(run, hl, mr, metric, level, reference, n_boot, seed, block)

    def compare_decay_namespaced(self, store, half_life_days, min_rel, domain_of,
                                 patterns: Optional[List[str]] = None, update_global: bool = False,
                                 market_scope: bool = False, lagged: bool = False,
                                 device_match: Optional[bool] = None, n_boot: int = 1000, seed: int = 0,
                                 block: int = 1, metric: str = "brier", level: float = 0.95,
                                 reference: Optional[int] = None) -> "DecayComparison":
        """:meth:`compare_decay` over the namespaced walk (the arguments of
        :meth:`sweep_decay_namespaced`, then those of :meth:`compare_decay`)."""
        hl, mr = _compare_arguments("compare_decay_namespaced", store, half_life_days, min_rel, n_boot, block,
                                    metric, level, reference)
        _, batch_markets, stamps, resolve_stamps, kw = self._namespaced_history(
            domain_of, patterns, update_global, market_scope, lagged, device_match)
        run = store.compare_decay_namespaced(batch_markets, stamps, hl, mr, resolve_times=resolve_stamps,
                                             n_boot=n_boot, seed=seed, block=block, **kw)
        return _comparison(run, hl, mr, metric, level, reference, n_boot, seed, block)

    def sweep_update(self, store, learning_rate, max_step=MAX_UPDATE_STEP, half_life_days=(DECAY_HALF_LIFE_DAYS,),
                     min_rel=(DECAY_MINIMUM,), patterns: Optional[List[str]] = None, domain: Optional[str] = None,
                     n_bins: int = 10, device_match: Optional[bool] = None,
                     lagged: bool = False) -> List["BacktestScore"]:
        """:meth:`sweep_decay` over the update rule: you edited ``_BASE_LEARNING_RATE`` /
        ``MAX_UPDATE_STEP`` to tune the engine -- this is the back-test of ``walk_forward(store,
        patterns, domain, dry_run=True)`` as if they were ``(learning_rate[i], max_step[i])``
        (pairs; ``max_step`` one number for all or one per point), for every update point and
        every point of the decay grid: one whole-history :class:`BacktestScore` per point,
        update point slowest, ``min_rel`` fastest (``params`` names it: ``learning_rate``,
        ``max_step``, ``half_life_days``, ``min_rel``).  All update points are traced in one
        launch (``store.sweep_update``, ``batch.walk_sweep_update``); nothing is written to the
        store.  The single-scope walk only."""
        params, hl, mr, B = _update_arguments("sweep_update", store, learning_rate, max_step, half_life_days,
                                              min_rel, n_bins)
        _, batch_markets, stamps, resolve_stamps = self._walk_history(patterns, device_match, lagged)
        scores = store.sweep_update(batch_markets, stamps, learning_rate, max_step, hl, mr, domain=domain, n_bins=B,
                                    resolve_times=resolve_stamps)
        return _sweep_rows(scores, hl, mr, B, params)

    def compare_update(self, store, learning_rate, max_step=MAX_UPDATE_STEP, half_life_days=(DECAY_HALF_LIFE_DAYS,),
                       min_rel=(DECAY_MINIMUM,), patterns: Optional[List[str]] = None, domain: Optional[str] = None,
                       lagged: bool = False, device_match: Optional[bool] = None, n_boot: int = 1000, seed: int = 0,
                       block: int = 1, metric: str = "brier", level: float = 0.95,
                       reference: Optional[int] = None) -> "DecayComparison":
        """:meth:`compare_decay` over the grid of :meth:`sweep_update`: the same walk and sweep,
        then the paired bootstrap over the markets (``store.compare_update``).  Returns a
        :class:`DecayComparison` whose rows carry the four ``params`` of :meth:`sweep_update`."""
        params, hl, mr, _ = _update_arguments("compare_update", store, learning_rate, max_step, half_life_days,
                                              min_rel, 10)
        _check_boot(n_boot, block)
        if isinstance(reference, bool) or not (reference is None or isinstance(reference, (int, np.integer))):
            raise TypeError(f"reference must be a grid index or None (got {type(reference).__name__})")
        if reference is not None and not 0 <= reference < len(params):
            raise ValueError(f"reference must be a grid index in [0, {len(params)}) (got {reference})")
        if metric not in COMPARE_METRICS or metric == "skill":
            raise ValueError(f"metric must be one of {COMPARE_METRICS[:3]} (got {metric!r})")
        if not 0.0 < float(level) < 1.0:
            raise ValueError(f"level must be in (0, 1) (got {level})")
        _, batch_markets, stamps, resolve_stamps = self._walk_history(patterns, device_match, lagged)
        run = store.compare_update(batch_markets, stamps, learning_rate, max_step, hl, mr, domain=domain,
                                   resolve_times=resolve_stamps, n_boot=n_boot, seed=seed, block=block)
        return _comparison(run, hl, mr, metric, level, reference, n_boot, seed, block, params)

    def summarize_category(self, category: str) -> Dict[str, Any]:
        markets = self._store.list_markets(pattern=f"{category}:*")
        resolved = [m for m in markets if m.status == MarketStatus.RESOLVED]
        open_markets = [m for m in markets if m.status == MarketStatus.OPEN]
        return {"category": category, "total_markets": len(markets), "resolved": len(resolved),
                "open": len(open_markets), "markets": [str(m.id) for m in markets]}

    def aggregate_consensus(self, patterns: List[str], method: str = "weighted_average") -> Dict[str, Any]:
        """Cross-market aggregation (market.py:338-408), computed by bce_aggregate_groups."""
        return self.aggregate_many([patterns], method)[0]

    def aggregate_many(self, pattern_lists: List[List[str]], method: str = "weighted_average",
                       device_match: Optional[bool] = None) -> List[Dict[str, Any]]:
        """aggregate_consensus for many pattern lists in ONE kernel launch: each list is a
        member group (markets in list_markets order per pattern, duplicates kept,
        market.py:355-357); the sums run in that order on the GPU (bit-exact).

        ``device_match`` (see ``_device_route``): the member groups come from the glob kernels
        (``MarketStore.match_many`` + ``batch.glob_members``) instead of one fnmatch call per
        (pattern, market) pair; same dicts."""
        n_patterns = sum(len(patterns) for patterns in pattern_lists)
        if n_patterns and self._device_route(n_patterns, device_match):
            return self._aggregate_many_device(pattern_lists, method)
        groups: List[List[int]] = []
        index: Dict[str, int] = {}
        cons: List[float] = []
        conf: List[float] = []
        has: List[int] = []
        for patterns in pattern_lists:
            members: List[int] = []
            for pattern in patterns:
                for market in self._store.list_markets(pattern=pattern):
                    key = str(market.id)
                    if key not in index:
                        index[key] = len(cons)
                        res = market.consensus_result
                        ok = bool(res) and res.get("consensus") is not None  # market.py:369-370
                        cons.append(float(res["consensus"]) if ok else 0.0)
                        conf.append(float(res.get("confidence", 0.5)) if ok else 0.0)
                        has.append(1 if ok else 0)
                    members.append(index[key])
            groups.append(members)
        empty = {"schemaVersion": "1.0.0", "consensus": None, "confidence": 0.0}
        if not any(has[m] for g in groups for m in g):
            return [dict(empty, marketsIncluded=len(g)) for g in groups]
        if method not in ("weighted_average", "median", "majority"):
            for g in groups:  # the reference raises only once a group has consensuses
                if any(has[m] for m in g):
                    raise ValueError(f"Unknown aggregation method: {method}")
        N.require_gpu()
        dev = N.device()
        T = batch.to_device(dev)
        goff = np.zeros(len(groups) + 1, np.int64)
        goff[1:] = np.cumsum([len(g) for g in groups])
        flat = np.array([m for g in groups for m in g], np.int64)
        r = batch.aggregate(T(goff), T(flat if flat.size else np.zeros(1, np.int64)), T(np.array(cons, np.float64)),
                            T(np.array(conf, np.float64)), T(np.array(has, np.uint8)), median=method == "median")
        pick = {"weighted_average": r.wavg, "median": r.median, "majority": r.majority}[method].cpu().numpy()
        mconf = r.mean_conf.cpu().numpy()
        k = r.n_included.cpu().numpy()
        out = []
        for gi, g in enumerate(groups):
            if not g:
                out.append(dict(empty, marketsIncluded=0))
            elif k[gi] == 0:
                out.append(dict(empty, marketsIncluded=len(g)))
            else:
                out.append({"schemaVersion": "1.0.0", "consensus": float(pick[gi]), "confidence": float(mconf[gi]),
                            "marketsIncluded": int(k[gi]), "method": method})
        return out

    def _aggregate_many_device(self, pattern_lists: List[List[str]], method: str) -> List[Dict[str, Any]]:
        """aggregate_many with the member groups built in HBM: one match launch over every id,
        count + fill into ``group_offsets`` / ``members``.  The value arrays are indexed by store
        position (the host route indexes them in first-seen order; no output depends on it)."""
        markets = self._store.list_markets()
        M = len(markets)
        # the bitmap is (patterns) x ceil(M / 64) words: pattern lists are taken in runs whose bitmap
        # stays inside GLOB_BITMAP_BUDGET, each run matched and expanded on its own
        per_run = max(GLOB_BITMAP_BUDGET // (8 * ((M + 63) // 64) or 1), 1)
        runs, n = [[]], 0
        for patterns in pattern_lists:
            if runs[-1] and n + len(patterns) > per_run:
                runs.append([])
                n = 0
            runs[-1].append(patterns)
            n += len(patterns)
        goffs, mems, base = [], [], 0
        for run in runs:
            globs, bits = self._store.match_many([p for patterns in run for p in patterns])
            slot_groups = np.zeros(len(run) + 1, np.int64)
            slot_groups[1:] = np.cumsum([len(patterns) for patterns in run])
            rows = torch.tensor(globs.index, dtype=torch.int64, device=bits.device)
            goff, mem = batch.glob_members(bits, M, rows, slot_groups)
            goffs.append(goff[(1 if goffs else 0):] + base)
            mems.append(mem)
            base += mem.numel()
            del bits
        goff, members = torch.cat(goffs), torch.cat(mems)
        dev = goff.device
        sizes = np.diff(goff.cpu().numpy())
        cons = np.zeros(max(M, 1), np.float64)
        conf = np.zeros(max(M, 1), np.float64)
        has = np.zeros(max(M, 1), np.uint8)
        if members.numel():
            # the matched markets in first-seen order: the order the host route reads their results in
            srt, idx = torch.sort(members, stable=True)
            head = torch.ones_like(srt, dtype=torch.bool)
            head[1:] = srt[1:] != srt[:-1]
            seen = srt[head][torch.argsort(idx[head])]
            for m in seen.cpu().tolist():
                res = markets[m].consensus_result
                if bool(res) and res.get("consensus") is not None:  # market.py:369-370
                    cons[m] = float(res["consensus"])
                    conf[m] = float(res.get("confidence", 0.5))
                    has[m] = 1
        empty = {"schemaVersion": "1.0.0", "consensus": None, "confidence": 0.0}
        if not has.any():
            return [dict(empty, marketsIncluded=int(n)) for n in sizes]
        if method not in ("weighted_average", "median", "majority"):
            raise ValueError(f"Unknown aggregation method: {method}")  # some group has a consensus
        T = batch.to_device(dev)
        r = batch.aggregate(goff, members, T(cons), T(conf), T(has), median=method == "median")
        pick = {"weighted_average": r.wavg, "median": r.median, "majority": r.majority}[method].cpu().numpy()
        mconf = r.mean_conf.cpu().numpy()
        k = r.n_included.cpu().numpy()
        out = []
        for gi, n in enumerate(sizes):
            if k[gi] == 0:
                out.append(dict(empty, marketsIncluded=int(n)))
            else:
                out.append({"schemaVersion": "1.0.0", "consensus": float(pick[gi]), "confidence": float(mconf[gi]),
                            "marketsIncluded": int(k[gi]), "method": method})
        return out
