"""Drop-in for ``bayesian_engine.reliability_abstraction`` (reference
src/bayesian_engine/reliability_abstraction.py): namespace-aware reliability with the
fallback chain market -> domain -> global -> cold start.

The per-source API (``get_reliability``, ``update_reliability``, ``set_global_reliability``)
keeps the reference's names, arguments, records and fallback order, on top of this
package's :class:`SQLiteReliabilityStore` (whose decay runs on the GPU).  The batched
path, :meth:`NamespacedReliabilityStore.resolve`, loads the three scopes of a whole rank
space from SQLite once and resolves every source in ONE launch of
``bce_namespace_resolve`` (decay + precedence + consensus-table packing fused), so the
table a consensus batch gathers from is built without a per-source Python loop.
"""
from __future__ import annotations

import sqlite3
from dataclasses import dataclass
from datetime import datetime, timezone
from enum import Enum
from typing import List, Optional, Protocol, Sequence, Tuple, runtime_checkable

import numpy as np
import torch

from . import _native as N
from . import batch
from .config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM, DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY, MAX_UPDATE_STEP
from .core import _no_signals as core_no_signals, consensus_dict, signals_csr
from .reliability import SQLiteReliabilityStore
from .timeutil import NO_TIMESTAMP, dt_to_us, iso_to_us, us_to_iso

__all__ = ["ReliabilityNamespace", "NamespacedReliabilityRecord", "ReliabilityProvider",
           "NamespacedReliabilityStore", "SettleSummary"]


class ReliabilityNamespace(str, Enum):
    """Namespace levels for reliability tracking (reliability_abstraction.py:33-38)."""

    GLOBAL = "global"
    DOMAIN = "domain"
    MARKET = "market"


@dataclass(frozen=True)
class NamespacedReliabilityRecord:
    """Reliability record with namespace context (reliability_abstraction.py:41-51)."""

    source_id: str
    namespace: ReliabilityNamespace
    namespace_value: str
    reliability: float
    confidence: float
    updated_at: str
    is_fallback: bool


@dataclass(frozen=True)
class SettleSummary:
    """What :meth:`NamespacedReliabilityStore.settle_markets` did, per touched source: the record
    of the settled scope, the global record when it was updated as well, and the
    summarize_sources counts of the batch (signals in resolved markets, and how many agreed)."""

    records: dict
    global_records: dict
    total: dict
    correct: dict


@runtime_checkable
class ReliabilityProvider(Protocol):
    """Protocol for reliability data providers (reliability_abstraction.py:54-81)."""

    def get_reliability(self, source_id: str, namespace: ReliabilityNamespace,
                        namespace_value: str) -> Optional[NamespacedReliabilityRecord]:
        ...

    def update_reliability(self, source_id: str, namespace: ReliabilityNamespace, namespace_value: str,
                           outcome_correct: bool) -> NamespacedReliabilityRecord:
        ...


def _namespaced(r, namespace: ReliabilityNamespace, value: str) -> NamespacedReliabilityRecord:
    """A settled :class:`ReliabilityRecord` as the record of its namespace."""
    return NamespacedReliabilityRecord(r.source_id, namespace, value, r.reliability, r.confidence, r.updated_at, False)


def _outcome_codes(markets) -> np.ndarray:
    """int8 per ``(signals, outcome)``: -1 unresolved (None), else the outcome's truth."""
    return np.array([-1 if o is None else (1 if o else 0) for _, o in markets], np.int8)


def _walk_times_us(markets, times, resolve_times):
    """``(forecast or market times, resolve times or None)`` of a walk as int64 microseconds.
    ``resolve_times`` has one entry per market; those of unresolved markets are not looked at."""
    times = list(times)
    if len(times) != len(markets):
        raise ValueError(f"times has {len(times)} entries for {len(markets)} markets")
    t_us = np.array([_as_us(t) for t in times], np.int64)
    if (t_us == NO_TIMESTAMP).any():
        raise ValueError("a market time is empty or unparseable")
    return t_us, None if resolve_times is None else _resolve_times_us(markets, resolve_times)


def _as_us(t) -> int:
    """An ISO string or a datetime as int64 microseconds (NO_TIMESTAMP: empty or unparseable)."""
    return iso_to_us(t) if isinstance(t, str) else dt_to_us(t)


def _resolve_times_us(markets, resolve_times) -> np.ndarray:
    """One resolve time per market as int64 microseconds; those of unresolved markets are not
    looked at (0)."""
    resolve_times = list(resolve_times)
    if len(resolve_times) != len(markets):
        raise ValueError(f"resolve_times has {len(resolve_times)} entries for {len(markets)} markets")
    r_us = np.array([0 if o is None else (NO_TIMESTAMP if r is None else _as_us(r))
                     for (_, o), r in zip(markets, resolve_times)], np.int64)
    if (r_us == NO_TIMESTAMP).any():
        raise ValueError("the resolve time of a resolved market is empty or unparseable")
    return r_us


def _check_market_ids(market_ids, M: int) -> None:
    """One truthy, distinct market id per market."""
    if len(market_ids) != M:
        raise ValueError(f"market_ids has {len(market_ids)} entries for {M} markets")
    if not all(market_ids):
        raise ValueError("every market id must be truthy (a falsy one selects another scope)")
    if len(set(market_ids)) != M:
        raise ValueError("duplicate market id in market_ids")


@dataclass
class _WalkBatch:
    """A history compiled for a walk: the interned source ``names``, the host ``offsets`` and the
    device ``off`` / ``prob`` of its CSR batch, the ``plan`` with its ``mtime`` (None for a lagged
    plan) and, loaded by the store, ``table`` -- the walked scope, or ``__global__`` of a
    namespaced walk, which also has the domain names and scope keys, the domain and market-scope
    pair tables (``ptable`` None without market ids) and ``ghas``: the global row has a stamp."""

    names: list
    offsets: np.ndarray
    off: torch.Tensor
    prob: torch.Tensor
    plan: object
    mtime: Optional[torch.Tensor]
    table: Optional["batch.ReliabilityTable"] = None
    dnames: Optional[list] = None
    dkeys: Optional[list] = None
    dtable: Optional["batch.PairTable"] = None
    ptable: Optional["batch.PairTable"] = None
    ghas: Optional[torch.Tensor] = None

    @classmethod
    def compile(cls, markets, t_us, r_us, market_domain=None, n_domains=0, **kw):
        """The batch of normalised ``markets`` without its tables, None for a history without
        signals: the sources interned in sorted() order, the CSR batch on the current device and
        its :class:`batch.WalkPlan` -- with ``market_domain`` its :class:`batch.WalkScopePlan`
        (``kw``: ``update_global``) -- lagged, with its own times, where ``r_us`` is given."""
        rank = batch.intern(s["sourceId"] for signals, _ in markets for s in signals)
        if not rank:
            return None
        offsets, sid, prob = signals_csr([signals for signals, _ in markets], rank)
        N.require_gpu()
        T = batch.to_device(N.device())
        off, sid, prob, outcome = T(offsets), T(sid), T(prob), T(_outcome_codes(markets))
        if market_domain is None:
            kind, args = batch.WalkPlan, (off, sid, prob, outcome, len(rank))
        else:
            kind, args = batch.WalkScopePlan, (off, sid, prob, outcome, T(market_domain), len(rank), n_domains)
        if r_us is None:
            plan, mtime = kind.build(*args, **kw), T(t_us)
        else:
            plan, mtime = kind.build_lagged(*args, T(t_us), T(r_us), **kw), None
        return cls(list(rank), offsets, off, prob, plan, mtime)


def _walk_dicts(markets, offsets, names, res, pairs) -> list:
    """The per-market ``compute_consensus``-shaped dicts of a walk-forward result whose ``usid``
    holds entry indices of ``pairs``."""
    cons, confd, tot = (x.cpu().numpy() for x in (res.consensus, res.confidence, res.total_weight))
    n_unique, usid = res.n_unique.cpu().numpy(), res.usid.cpu().numpy()
    weight, nweight = res.weight.cpu().numpy(), res.nweight.cpu().numpy()
    esrc = pairs.usid.cpu().numpy()
    results = []
    for m, (signals, _) in enumerate(markets):
        if not signals:
            results.append(core_no_signals())
            continue
        a, b = offsets[m], offsets[m] + int(n_unique[m])
        ids = [names[esrc[e & 0x7FFFFFFF]] for e in usid[a:b]]
        results.append(consensus_dict(ids, weight[a:b], nweight[a:b], cons[m], confd[m], tot[m], len(signals),
                                      []))  # every source was fetched: none is cold
    return results


def _domain_counts(domains, markets):
    """summarize_sources' ``total`` / ``correct`` keyed ``(source_id, domain-or-None)``."""
    total: dict = {}
    correct: dict = {}
    for d, (signals, out) in zip(domains, markets):
        if out is None:
            continue
        for s in signals:
            k = (s["sourceId"], d if d else None)
            total[k] = total.get(k, 0) + 1
            correct[k] = correct.get(k, 0) + int((s.get("probability", 0.5) >= 0.5) == bool(out))
    return total, correct


# scope code (bce_namespace_resolve) -> (namespace, is_fallback)
_SCOPE_NS = {batch.NS_MARKET: (ReliabilityNamespace.MARKET, False),
             batch.NS_DOMAIN: (ReliabilityNamespace.DOMAIN, True),
             batch.NS_GLOBAL: (ReliabilityNamespace.GLOBAL, True)}


def _check_boot(n_boot, block) -> None:
    """The bootstrap arguments of the ``compare_decay`` methods."""
    for name, x in (("n_boot", n_boot), ("block", block)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise TypeError(f"{name} must be an int (got {type(x).__name__})")
        if x < 1:
            raise ValueError(f"{name} must be >= 1 (got {x})")


class NamespacedReliabilityStore:
    """Reliability store with namespace-aware fallback chain (reliability_abstraction.py:84-291).

    Fallback order: market-specific, domain-specific, global, cold-start defaults.
    """

    GLOBAL_MARKET_ID = "__global__"

    def __init__(self, db_path: str = ":memory:"):
        self._store = SQLiteReliabilityStore(db_path)

    # ------------------------------------------------------------------ reference API
    def get_reliability(self, source_id: str, market_id: Optional[str] = None, domain: Optional[str] = None,
                        apply_decay: bool = True) -> NamespacedReliabilityRecord:
        """reliability_abstraction.py:119-188."""
        if market_id:
            record = self._store.get_reliability(source_id, market_id, apply_decay)
            if record.updated_at:
                return NamespacedReliabilityRecord(source_id, ReliabilityNamespace.MARKET, market_id,
                                                   record.reliability, record.confidence, record.updated_at, False)
        if domain:
            record = self._store.get_reliability(source_id, f"__domain__:{domain}", apply_decay)
            if record.updated_at:
                return NamespacedReliabilityRecord(source_id, ReliabilityNamespace.DOMAIN, domain,
                                                   record.reliability, record.confidence, record.updated_at, True)
        record = self._store.get_reliability(source_id, self.GLOBAL_MARKET_ID, apply_decay)
        if record.updated_at:
            return NamespacedReliabilityRecord(source_id, ReliabilityNamespace.GLOBAL, "global",
                                               record.reliability, record.confidence, record.updated_at, True)
        return NamespacedReliabilityRecord(source_id, ReliabilityNamespace.GLOBAL, "cold-start",
                                           DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE, "", True)

    def update_reliability(self, source_id: str, outcome_correct: bool, market_id: Optional[str] = None,
                           domain: Optional[str] = None, update_global: bool = False) -> NamespacedReliabilityRecord:
        """reliability_abstraction.py:190-240."""
        namespace, namespace_value, target = self._update_scope(domain, market_id)
        record = self._store.update_reliability(source_id, target, outcome_correct)
        if update_global and namespace != ReliabilityNamespace.GLOBAL:
            self._store.update_reliability(source_id, self.GLOBAL_MARKET_ID, outcome_correct)
        return NamespacedReliabilityRecord(source_id, namespace, namespace_value, record.reliability,
                                           record.confidence, record.updated_at, False)

    def _update_scope(self, domain: Optional[str], market_id: Optional[str] = None):
        """``(namespace, namespace_value, scope key)`` an update goes to (reliability_abstraction.py:211-216)."""
        if market_id:
            return ReliabilityNamespace.MARKET, market_id, market_id
        if domain:
            return ReliabilityNamespace.DOMAIN, domain, f"__domain__:{domain}"
        return ReliabilityNamespace.GLOBAL, "global", self.GLOBAL_MARKET_ID

    def set_global_reliability(self, source_id: str, reliability: float,
                               confidence: float) -> NamespacedReliabilityRecord:
        """reliability_abstraction.py:242-283: upsert through a fresh connection to the
        same path (as the reference does; for ":memory:" that is a separate database)."""
        now = datetime.now(timezone.utc).isoformat()
        conn = sqlite3.connect(self._store._db_path)
        conn.execute(
            "INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at) "
            "VALUES (?, ?, ?, ?, ?) ON CONFLICT(source_id, market_id) "
            "DO UPDATE SET reliability = excluded.reliability, confidence = excluded.confidence, "
            "updated_at = excluded.updated_at",
            (source_id, self.GLOBAL_MARKET_ID, reliability, confidence, now),
        )
        conn.commit()
        conn.close()
        return NamespacedReliabilityRecord(source_id, ReliabilityNamespace.GLOBAL, "global", reliability,
                                           confidence, now, False)

    def close(self) -> None:
        self._store.close()

    def __enter__(self) -> "NamespacedReliabilityStore":
        return self

    def __exit__(self, *exc_info: object) -> None:
        self.close()

    # ------------------------------------------------------------------ batched path (f3)
    def _scope(self, key: str, names: Sequence[str], dev) -> Tuple[batch.ScopeTable, List[str]]:
        rows = self._store._conn.execute(
            "SELECT source_id, reliability, confidence, updated_at FROM sources WHERE market_id = ?",
            (key,)).fetchall()
        idx = {n: i for i, n in enumerate(names)}
        S = len(names)
        rel = np.full(S, DEFAULT_RELIABILITY)
        conf = np.full(S, DEFAULT_CONFIDENCE)
        t_us = np.full(S, NO_TIMESTAMP, np.int64)
        has = np.zeros(S, np.uint8)
        stamps = [""] * S
        for sid, r, c, ts in rows:
            i = idx.get(sid)
            if i is None or not ts:  # the reference only takes rows with a truthy updated_at
                continue
            rel[i], conf[i], t_us[i], has[i], stamps[i] = r, c, iso_to_us(ts), 1, ts
        T = batch.to_device(dev)
        return batch.ScopeTable(T(rel), T(conf), T(t_us), T(has)), stamps

    def resolve(self, names: Sequence[str], market_id: Optional[str] = None, domain: Optional[str] = None,
                apply_decay: bool = True, now: Optional[datetime] = None, mark_cold: bool = False,
                device=None):
        """get_reliability(sid, market_id, domain, apply_decay) for every sid of ``names`` in
        one kernel launch.  Returns (SourceTable for batch.consensus, scope codes u8[S],
        per-source updated_at strings of the chosen rows)."""
        N.require_gpu()
        dev = device or N.device()
        names = list(names)
        keys = [market_id if market_id else None, f"__domain__:{domain}" if domain else None,
                self.GLOBAL_MARKET_ID]
        scopes, stamps = [], []
        for key in keys:
            if key is None:
                scopes.append(None)
                stamps.append(None)
            else:
                sc, st = self._scope(key, names, dev)
                scopes.append(sc)
                stamps.append(st)
        now_us = dt_to_us(now or datetime.now(timezone.utc))
        table, scope = batch.namespace_resolve(scopes, now_us, apply_decay=apply_decay, mark_cold=mark_cold,
                                               names=names)
        code = scope.cpu().numpy()
        chosen = [stamps[c][i] if c < 3 else "" for i, c in enumerate(code)]
        return table, scope, chosen

    def settle_markets(self, markets: Sequence[tuple], domain: Optional[str] = None, update_global: bool = False,
                       dry_run: bool = False, now: Optional[datetime] = None,
                       market_ids: Optional[Sequence[str]] = None,
                       domains: Optional[Sequence[Optional[str]]] = None) -> "SettleSummary":
        """``update_reliability(sid, correct, domain=domain, update_global=update_global)`` for
        every signal of every resolved market, in list order, as ONE compiled batch.

        ``markets`` is a sequence of ``(signals, outcome)``: the reference's signal dicts and the
        market's outcome (``None``: the market is skipped); ``correct`` is ``(probability >= 0.5)
        == outcome`` with a missing probability read as 0.5 (market.py:298-301).  Sources are
        interned in sorted() order, one :class:`batch.SettlePlan` is built and applied to the
        ``__domain__:<domain>`` scope, or to ``__global__`` when ``domain`` is None; with
        ``update_global`` and a domain the same plan is applied a second time to ``__global__``
        (reliability_abstraction.py:225-229).  ``dry_run`` computes the records and writes nothing.

        ``market_ids`` (one truthy, distinct id per entry of ``markets``, else ``ValueError``)
        settles at MARKET scope instead, as ``update_reliability(sid, correct, market_id=m, ...)``
        chooses it (:211-216; ``domain`` is ignored there, as in the reference): every (source,
        market) pair has a row of its own and its chain is that market's signals of the source
        (:meth:`SQLiteReliabilityStore.settle_pairs`).  The summary's ``records`` / ``total`` /
        ``correct`` are then keyed by ``(source_id, market_id)``; with ``update_global`` the
        source-scope plan also settles ``__global__``.

        ``domains`` (one entry per market, falsy = no domain; together with ``domain=``,
        ``ValueError``; ignored with ``market_ids``, as ``domain`` is) gives every market a domain
        of its own: per signal ``update_reliability(sid, correct, domain=domains[i],
        update_global=update_global)``.  A market with a domain settles ``__domain__:<d>``
        (:meth:`SQLiteReliabilityStore.settle_domains`, distinct domains interned in first-seen
        order), one without settles ``__global__`` directly, and with ``update_global`` every
        resolved signal reaches ``__global__`` exactly once (:211-229).  ``records`` / ``total`` /
        ``correct`` are keyed ``(source_id, domain)``, ``domain`` None for the signals of markets
        without one (their record is the final ``__global__`` row); ``global_records`` has every
        source whose global row was written."""
        markets = [(list(signals), outcome) for signals, outcome in markets]
        if domains is not None:
            if domain is not None:
                raise ValueError("domain= (one for the batch) and domains= (one per market) exclude each other")
            domains = list(domains)
            if len(domains) != len(markets):
                raise ValueError(f"domains has {len(domains)} entries for {len(markets)} markets")
        if market_ids is not None:
            market_ids = list(market_ids)
            _check_market_ids(market_ids, len(markets))
        rank = batch.intern(s["sourceId"] for signals, _ in markets for s in signals)
        names = list(rank)
        offsets, sid, prob = signals_csr([signals for signals, _ in markets], rank, settlement=True)
        outcomes = _outcome_codes(markets)
        namespace, value, target = self._update_scope(domain)
        if not names:
            return SettleSummary({}, {}, {}, {})
        N.require_gpu()
        dev = N.device()
        T = batch.to_device(dev)
        if domains is not None and market_ids is None:
            return self._settle_per_domain(markets, domains, names, offsets, sid, prob, outcomes, update_global,
                                           dry_run, now or datetime.now(timezone.utc))
        plan = batch.SettlePlan.build(T(offsets), T(sid), T(prob), T(outcomes), len(names))
        now = now or datetime.now(timezone.utc)
        if market_ids is not None:
            mids = [str(m) for m in market_ids]
            precs = self._store.settle_pairs(mids, names, offsets, sid, prob, outcomes, dry_run=dry_run, now=now)
            records = {k: _namespaced(r, ReliabilityNamespace.MARKET, k[1]) for k, r in precs.items()}
            global_records = self._settle_global(names, plan, dry_run, now) if update_global else {}
            ptotal = dict.fromkeys(records, 0)
            pcorrect = dict.fromkeys(records, 0)
            for mid, (signals, outcome) in zip(mids, markets):
                if outcome is None:
                    continue
                for s in signals:
                    k = (s["sourceId"], mid)
                    ptotal[k] += 1
                    pcorrect[k] += int((s.get("probability", 0.5) >= 0.5) == bool(outcome))
            return SettleSummary(records, global_records, ptotal, pcorrect)
        recs = self._store.settle(target, names, plan, dry_run=dry_run, now=now)
        records = {sid: _namespaced(r, namespace, value) for sid, r in recs.items()}
        global_records = {}
        if update_global and namespace != ReliabilityNamespace.GLOBAL:
            global_records = self._settle_global(names, plan, dry_run, now)
        total = plan.total.cpu().numpy()
        correct = plan.correct.cpu().numpy()
        return SettleSummary(records, global_records, {sid: int(total[rank[sid]]) for sid in records},
                             {sid: int(correct[rank[sid]]) for sid in records})

    def _settle_global(self, names, plan, dry_run, now) -> dict:
        """``plan`` applied to ``__global__``: the records of the touched sources."""
        grecs = self._store.settle(self.GLOBAL_MARKET_ID, names, plan, dry_run=dry_run, now=now)
        return {sid: _namespaced(r, ReliabilityNamespace.GLOBAL, "global") for sid, r in grecs.items()}

    def _settle_per_domain(self, markets, domains, names, offsets, sid, prob, outcome, update_global,
                           dry_run, now) -> "SettleSummary":
        """settle_markets(domains=...): the domain rows through settle_domains, then ONE global
        chain per source -- the signals of the markets without a domain, or with ``update_global``
        every resolved signal (no second global update where the target already is global,
        reliability_abstraction.py:225-229) -- through the existing settle."""
        dnames = list(dict.fromkeys(d for d in domains if d))
        drank = {d: i for i, d in enumerate(dnames)}
        market_domain = np.array([drank[d] if d else -1 for d in domains], np.int32)
        dev = N.device()
        T = batch.to_device(dev)
        records = {}
        if dnames:
            of_key = {f"__domain__:{d}": d for d in dnames}
            precs = self._store.settle_domains(list(of_key), names, offsets, sid, prob, outcome, market_domain,
                                               dry_run=dry_run, now=now)
            for (s, key), r in precs.items():
                records[(s, of_key[key])] = _namespaced(r, ReliabilityNamespace.DOMAIN, of_key[key])
        gout = outcome if update_global else np.where(market_domain < 0, outcome, np.int8(-1)).astype(np.int8)
        global_records = {}
        if bool((gout >= 0).any()):
            gplan = batch.SettlePlan.build(T(offsets), T(sid), T(prob), T(gout), len(names))
            global_records = self._settle_global(names, gplan, dry_run, now)
        total, correct = _domain_counts(domains, markets)
        for k in total:
            if k[1] is None:
                records[k] = global_records[k[0]]
        return SettleSummary(records, global_records, total, correct)

    def walk_forward(self, markets: Sequence[tuple], times: Sequence, domain: Optional[str] = None,
                     dry_run: bool = False, resolve_times: Optional[Sequence] = None):
        """The reference run online over a chronological batch, as ONE compiled batch
        (:func:`batch.walk_forward`): market i is scored by ``compute_consensus`` with every source
        fetched by ``get_reliability(sid, scope, apply_decay=True)`` at ``times[i]``, then, if its
        outcome is not None, ``update_reliability(sid, scope, (probability >= 0.5) == outcome)``
        runs for every signal and stamps the row with ``times[i]``.  ``markets`` is a sequence of
        ``(signals, outcome)`` as in :meth:`settle_markets`, ``times`` ISO strings or datetimes
        (one per market); the scope is ``__domain__:<domain>``, or ``__global__`` without a
        domain.  The scope is loaded once (``load_table``), the sources interned in sorted()
        order, and the final rows of the touched sources written back with one ``executemany``
        unless ``dry_run``.  Returns ``(results, summary)``: one dict per market shaped like
        ``compute_consensus``'s, and the :class:`SettleSummary` of the settled scope.

        ``resolve_times`` (one entry per market, as ``times``; ignored for unresolved markets)
        separates the two events of a market: it is scored at ``times[i]`` and its updates run,
        and stamp the rows, at ``resolve_times[i]`` -- the reference as an event loop sorted by
        (time, market, forecast before resolution), so a market does not see outcomes that had
        not arrived when it was forecast.  ``times`` must then be in order and no resolve time
        earlier than its market's time (``ValueError``); rows written back carry the resolve time
        of their last settling market."""
        namespace, value, target = self._update_scope(domain)
        markets, b = self._scope_walk(markets, times, target, resolve_times)
        if b is None:
            return [core_no_signals() for _ in markets], SettleSummary({}, {}, {}, {})
        names, plan, table = b.names, b.plan, b.table
        res = table.walk_forward(plan, b.mtime, offsets=b.off, prob=b.prob, validate=False)
        N.check_faults(b.off.device, "walk_forward")
        results = _walk_dicts(markets, b.offsets, names, res, plan.pairs)
        return results, self._walked_summary(names, plan.settle, table, namespace, value, target, dry_run)

    def _walked_summary(self, names, splan, table, namespace, value, target, dry_run) -> SettleSummary:
        """What a committed walk of one scope leaves behind: the final rows of the touched sources
        of ``splan`` read from ``table``, written back with one ``executemany`` unless ``dry_run``,
        as the :class:`SettleSummary` of the scope."""
        touched = sorted(int(x) for x in splan.order.cpu().numpy())
        rel, conf, stamp_us = table.rel.cpu().numpy(), table.conf.cpu().numpy(), table.t_us.cpu().numpy()
        total, correct = splan.total.cpu().numpy(), splan.correct.cpu().numpy()
        records = {names[i]: NamespacedReliabilityRecord(names[i], namespace, value, float(rel[i]), float(conf[i]),
                                                         us_to_iso(int(stamp_us[i])), False) for i in touched}
        if not dry_run and records:
            self._store._upsert((r.source_id, target, r.reliability, r.confidence, r.updated_at)
                                for r in records.values())
        return SettleSummary(records, {}, {names[i]: int(total[i]) for i in touched},
                             {names[i]: int(correct[i]) for i in touched})

    def walk_history_live(self, markets: Sequence[tuple], arrival_times: Sequence[Sequence],
                          resolve_times: Sequence, domain: Optional[str] = None, dry_run: bool = False):
        """The consensus history of every market with the reliabilities re-read at every arrival
        (:func:`batch.walk_history_live`): the reference run online as an event loop -- signal k
        of market i arrives at ``arrival_times[i][k]`` and ``compute_consensus(signals[:k + 1])``
        runs with every source fetched by ``get_reliability(sid, scope, apply_decay=True)`` at
        that time; a market whose outcome is not None runs ``update_reliability`` per signal at
        ``resolve_times[i]`` and stamps the rows with it.  ``markets`` as in :meth:`walk_forward`
        (any order); ``arrival_times`` one sequence of ISO strings or datetimes per market, one per
        signal, not decreasing; ``resolve_times`` one per market (ignored for unresolved markets),
        no earlier than the market's last arrival.  Returns ``(histories, summary)``: per market
        one row per signal shaped like ``Market.consensus_history``'s, and the
        :class:`SettleSummary` of the scope, whose rows are written back unless ``dry_run``."""
        namespace, value, target = self._update_scope(domain)
        markets = [(list(signals), outcome) for signals, outcome in markets]
        arrival_times = [list(a) for a in arrival_times]
        if len(arrival_times) != len(markets):
            raise ValueError(f"arrival_times has {len(arrival_times)} entries for {len(markets)} markets")
        for m, ((signals, _), a) in enumerate(zip(markets, arrival_times)):
            if len(a) != len(signals):
                raise ValueError(f"arrival_times[{m}] has {len(a)} entries for {len(signals)} signals")
        a_us = np.array([_as_us(t) for a in arrival_times for t in a], np.int64)
        if (a_us == NO_TIMESTAMP).any():
            raise ValueError("an arrival time is empty or unparseable")
        r_us = _resolve_times_us(markets, resolve_times)
        rank = batch.intern(s["sourceId"] for signals, _ in markets for s in signals)
        if not rank:
            return [[] for _ in markets], SettleSummary({}, {}, {}, {})
        names = list(rank)
        offsets, sid, prob = signals_csr([signals for signals, _ in markets], rank)
        N.require_gpu()
        T = batch.to_device(N.device())
        off, dsid, dprob = T(offsets), T(sid), T(prob)
        plan = batch.LivePlan.build(off, dsid, dprob, T(_outcome_codes(markets)), len(names), T(a_us), T(r_us))
        table = self._store.load_table(target, names, device=off.device)
        h = batch.walk_history_live(plan, table, offsets=off, sid=dsid, prob=dprob, offsets_host=offsets, commit=True)
        N.check_faults(off.device, "walk_history_live")
        cons, confd, tot, nu = (x.cpu().numpy() for x in (h.consensus, h.confidence, h.total_weight, h.n_unique))
        from .market import _history_rows
        histories = [_history_rows(signals, cons[a:b], confd[a:b], tot[a:b], nu[a:b])
                     for (signals, _), a, b in zip(markets, offsets[:-1], offsets[1:])]
        return histories, self._walked_summary(names, plan.settle, table, namespace, value, target, dry_run)

    def sweep_decay(self, markets: Sequence[tuple], times: Sequence, half_life_days: Sequence[float],
                    min_rel: Sequence[float], domain: Optional[str] = None, n_bins: int = 10,
                    resolve_times: Optional[Sequence] = None):
        """:meth:`walk_forward` as a dry run for every point of a grid of decay parameters, each
        scored against the batch's outcomes (:func:`batch.walk_sweep`: the settlement trace does
        not depend on the decay parameters and runs once).  Nothing is written.  Returns the
        :class:`batch.ScoreResult` of the whole history with a leading grid dimension
        ``[len(half_life_days) * len(min_rel), 1, ...]`` (``min_rel`` fastest), or None for a
        history without signals.  ``resolve_times`` as :meth:`walk_forward`."""
        b = self._scope_walk(markets, times, self._update_scope(domain)[2], resolve_times)[-1]
        run = self._sweep_run(b, half_life_days, min_rel, n_bins, False, "sweep_decay")
        return None if run is None else run[0]

    def _scope_walk(self, markets, times, target, resolve_times):
        """What :meth:`walk_forward` and the single-scope sweeps share: ``(markets, batch)`` with
        ``markets`` normalised and ``batch`` the :class:`_WalkBatch` of the interned history, its
        compiled :class:`batch.WalkPlan` (lagged where ``resolve_times`` is given) and the loaded
        scope; None for a history without signals."""
        markets = [(list(signals), outcome) for signals, outcome in markets]
        b = _WalkBatch.compile(markets, *_walk_times_us(markets, times, resolve_times))
        if b is not None:
            b.table = self._store.load_table(target, b.names, device=b.off.device)
        return markets, b

    @staticmethod
    def _sweep_run(b, half_life_days, min_rel, n_bins, keep_consensus, what):
        """What the four sweep methods share: :func:`batch.walk_sweep` or, for the batch of a
        namespaced walk, :func:`batch.walk_sweep_scoped`.  ``(scores, kept, outcome)`` with
        ``kept`` the ``[K, M]`` consensus and null mask (``keep_consensus``) and ``outcome`` the
        int8[M] device tensor; None for no batch (a history without signals)."""
        if b is None:
            return None
        kw = dict(offsets=b.off, prob=b.prob, half_life_days=half_life_days, min_rel=min_rel, n_bins=n_bins,
                  keep_consensus=keep_consensus)
        if b.dtable is None:
            scores, kept = batch.walk_sweep(b.plan, b.table, b.mtime, **kw)
        else:
            scores, kept = batch.walk_sweep_scoped(b.plan, b.dtable, b.table, b.mtime, pairs=b.ptable,
                                                   global_has=b.ghas, **kw)
        N.check_faults(b.off.device, what)
        return scores, kept, b.plan.outcome

    @staticmethod
    def _compare(scores, kept, outcome, n_boot, seed, block, what):
        """The bootstrap of a sweep's kept consensus: one group of all markets, one set per grid
        point, ``unit = market // block``."""
        cons, nulls = kept
        M = outcome.numel()
        dev = cons.device
        boot = batch.score_bootstrap(batch.ScorePlan.whole(M, device=dev), cons, outcome, valid=~nulls,
                                     unit=batch.boot_units(M, block, device=dev), n_boot=n_boot, seed=seed)
        N.check_faults(dev, what)
        return scores, boot

    def compare_decay(self, markets: Sequence[tuple], times: Sequence, half_life_days: Sequence[float],
                      min_rel: Sequence[float], domain: Optional[str] = None,
                      resolve_times: Optional[Sequence] = None, n_boot: int = 1000, seed: int = 0, block: int = 1):
        """:meth:`sweep_decay` with a paired bootstrap over the markets: is the difference between
        two grid points more than noise?  The same plan and the same :func:`batch.walk_sweep`
        (``keep_consensus=True``), then :func:`batch.score_bootstrap` over one group of all
        markets with one forecast set per grid point, every set under the same ``n_boot``
        resamples (``seed``; ``block`` consecutive markets of the walk are resampled together).
        Nothing is written.  Returns ``(scores, boot)``: the :class:`batch.ScoreResult` of
        :meth:`sweep_decay` and a :class:`batch.BootstrapResult` ``[n_boot + 1, 1, K, ...]``, or
        None for a history without signals."""
        _check_boot(n_boot, block)
        b = self._scope_walk(markets, times, self._update_scope(domain)[2], resolve_times)[-1]
        run = self._sweep_run(b, half_life_days, min_rel, 10, True, "compare_decay")
        return None if run is None else self._compare(*run, n_boot, seed, block, "compare_decay")

    @staticmethod
    def _update_run(b, learning_rate, max_step, half_life_days, min_rel, n_bins, keep_consensus, what):
        """:meth:`_sweep_run` with the update rule as the slowest axis (:func:`batch.walk_sweep_update`)."""
        if b is None:
            return None
        scores, kept = batch.walk_sweep_update(b.plan, b.table, b.mtime, offsets=b.off, prob=b.prob,
                                               learning_rate=learning_rate, max_step=max_step,
                                               half_life_days=half_life_days, min_rel=min_rel, n_bins=n_bins,
                                               keep_consensus=keep_consensus)
        N.check_faults(b.off.device, what)
        return scores, kept, b.plan.outcome

    def sweep_update(self, markets: Sequence[tuple], stamps: Sequence, learning_rate, max_step=MAX_UPDATE_STEP,
                     half_life_days: Sequence[float] = (DECAY_HALF_LIFE_DAYS,),
                     min_rel: Sequence[float] = (DECAY_MINIMUM,), domain: Optional[str] = None, n_bins: int = 10,
                     resolve_times: Optional[Sequence] = None):
        """:meth:`sweep_decay` over the update rule itself: :meth:`walk_forward` as a dry run as if
        ``_BASE_LEARNING_RATE`` / ``MAX_UPDATE_STEP`` were ``(learning_rate[i], max_step[i])`` --
        pairs, ``max_step`` one number for all or one per point (:func:`batch.update_steps`) --
        for every update point and every point of the decay grid, each scored against the
        batch's outcomes (:func:`batch.walk_sweep_update`: all update points are traced in one
        launch).  Nothing is written.  Returns the :class:`batch.ScoreResult` of the whole history
        with a leading grid dimension ``[K * len(half_life_days) * len(min_rel), 1, ...]`` (update
        point slowest, ``min_rel`` fastest), or None for a history without signals.  ``stamps`` /
        ``resolve_times`` are :meth:`walk_forward`'s ``times`` / ``resolve_times``."""
        batch.update_steps(learning_rate, max_step)  # the argument errors, before anything is loaded
        b = self._scope_walk(markets, stamps, self._update_scope(domain)[2], resolve_times)[-1]
        run = self._update_run(b, learning_rate, max_step, half_life_days, min_rel, n_bins, False, "sweep_update")
        return None if run is None else run[0]

    def compare_update(self, markets: Sequence[tuple], stamps: Sequence, learning_rate, max_step=MAX_UPDATE_STEP,
                       half_life_days: Sequence[float] = (DECAY_HALF_LIFE_DAYS,),
                       min_rel: Sequence[float] = (DECAY_MINIMUM,), domain: Optional[str] = None,
                       resolve_times: Optional[Sequence] = None, n_boot: int = 1000, seed: int = 0, block: int = 1):
        """:meth:`sweep_update` with the paired bootstrap of :meth:`compare_decay`: the same sweep
        (``keep_consensus=True``) into :func:`batch.score_bootstrap`, one forecast set per grid
        point.  Nothing is written.  Returns ``(scores, boot)`` or None for a history without
        signals."""
        _check_boot(n_boot, block)
        batch.update_steps(learning_rate, max_step)
        b = self._scope_walk(markets, stamps, self._update_scope(domain)[2], resolve_times)[-1]
        run = self._update_run(b, learning_rate, max_step, half_life_days, min_rel, 10, True, "compare_update")
        return None if run is None else self._compare(*run, n_boot, seed, block, "compare_update")

    def _namespaced_walk(self, markets, times, domains, market_ids, update_global, resolve_times):
        """What :meth:`walk_forward_namespaced` and :meth:`sweep_decay_namespaced` share: the
        argument checks, the interned batch, the compiled :class:`batch.WalkScopePlan` (lagged
        where ``resolve_times`` is given) and the three loaded scopes, as a :class:`_WalkBatch`;
        None for a history without signals (``markets`` / ``domains`` normalised either way, as
        the first two items of the returned tuple)."""
        markets = [(list(signals), outcome) for signals, outcome in markets]
        M = len(markets)
        t_us, r_us = _walk_times_us(markets, times, resolve_times)
        domains = [domains] * M if isinstance(domains, str) or domains is None else list(domains)
        if len(domains) != M:
            raise ValueError(f"domains has {len(domains)} entries for {M} markets")
        if market_ids is not None:
            market_ids = [str(m) for m in market_ids]
            _check_market_ids(market_ids, M)
        dnames = list(dict.fromkeys(d for d in domains if d))
        drank = {d: i for i, d in enumerate(dnames)}
        market_domain = np.array([drank[d] if d else -1 for d in domains], np.int32)
        b = _WalkBatch.compile(markets, t_us, r_us, market_domain, len(dnames), update_global=update_global)
        if b is None:
            return markets, domains, None
        names, dev = b.names, b.off.device
        b.dnames, b.dkeys = dnames, [f"__domain__:{d}" for d in dnames]
        b.dtable = self._store.load_pair_table(b.dkeys, names, device=dev)
        b.ptable = self._store.load_pair_table(market_ids, names, device=dev) if market_ids is not None else None
        b.table = self._store.load_table(self.GLOBAL_MARKET_ID, names, device=dev)
        stamps = self._store.fetch_pairs([(n, self.GLOBAL_MARKET_ID) for n in names])
        b.ghas = batch.to_device(dev)(np.array([1 if stamps.get((n, self.GLOBAL_MARKET_ID), (0, 0, ""))[2] else 0
                                                for n in names], np.uint8))
        return markets, domains, b

    def walk_forward_namespaced(self, markets: Sequence[tuple], times: Sequence, domains=None,
                                market_ids: Optional[Sequence[str]] = None, update_global: bool = False,
                                dry_run: bool = False, resolve_times: Optional[Sequence] = None):
        """:meth:`walk_forward` for a history that spans domains, with the fallback chain at
        every read, as ONE compiled batch (:func:`batch.walk_forward_scoped`): market i is scored
        by ``compute_consensus`` with every source fetched by ``get_reliability(sid,
        market_id=market_ids[i], domain=domains[i], apply_decay=True)`` at ``times[i]``, then, if
        its outcome is not None, ``update_reliability(sid, correct, domain=domains[i],
        update_global=update_global)`` runs for every signal and stamps the rows it writes with
        ``times[i]``.  ``domains`` is one entry per market (falsy = none) or one string for all;
        ``market_ids`` (optional, truthy and distinct, else ``ValueError``) are used for the read
        only: market-scope rows are priors and are not settled here.  Sources are interned in
        sorted() order and domains in first-seen order; the market and domain rows are loaded
        with ``load_pair_table``, ``__global__`` with ``load_table``, and the touched domain and
        global rows written back with one ``executemany``, each with its own ``updated_at``,
        unless ``dry_run``.  Returns ``(results, summary)``: one dict per market shaped like
        ``compute_consensus``'s, and a :class:`SettleSummary` keyed as
        ``settle_markets(domains=)`` keys it (``(source_id, domain-or-None)``).

        ``resolve_times`` as in :meth:`walk_forward`: market i is scored at ``times[i]`` and its
        updates run, and stamp the rows of its scopes, at ``resolve_times[i]``, so a scope that
        had no truthy stamp when a market was forecast is skipped by that read even if an
        earlier-listed market creates it later (:meth:`batch.WalkScopePlan.build_lagged`); rows
        written back carry the resolve time of their last settling market, per scope."""
        markets, domains, b = self._namespaced_walk(markets, times, domains, market_ids, update_global,
                                                    resolve_times)
        if b is None:
            return [core_no_signals() for _ in markets], SettleSummary({}, {}, {}, {})
        names, dnames, dkeys, plan, gtable, dev = b.names, b.dnames, b.dkeys, b.plan, b.table, b.off.device
        res = batch.walk_forward_scoped(plan, b.dtable, gtable, b.mtime, offsets=b.off, prob=b.prob, pairs=b.ptable,
                                        global_has=b.ghas, validate=False)
        N.check_faults(dev, "walk_forward_namespaced")
        results = _walk_dicts(markets, b.offsets, names, res, plan.pairs)
        records, global_records, rows = {}, {}, []
        F = plan.dplan.n_entries
        if F and plan.dsettle.n_touched:  # every touched chain has a row in the new table: read them back
            r = batch.pair_resolve(plan.dplan.uoffsets, plan.dplan.usid, res.domains, 0, mode="raw",
                                   emarket=plan.dplan.emarket)
            touched = torch.nonzero(res.domain_total[:F] > 0).flatten()
            cols = [x[touched].cpu().numpy() for x in (plan.dplan.emarket, plan.dplan.usid, r.rel, r.conf, r.t_us)]
            for d, s, x, c, t in zip(*cols):
                rec = NamespacedReliabilityRecord(names[int(s)], ReliabilityNamespace.DOMAIN, dnames[int(d)],
                                                  float(x), float(c), us_to_iso(int(t)), False)
                records[(rec.source_id, rec.namespace_value)] = rec
                rows.append((rec.source_id, dkeys[int(d)], rec.reliability, rec.confidence, rec.updated_at))
        gtouched = sorted(int(x) for x in plan.gsettle.order.cpu().numpy())
        rel, conf, stamp_us = gtable.rel.cpu().numpy(), gtable.conf.cpu().numpy(), gtable.t_us.cpu().numpy()
        for i in gtouched:
            rec = NamespacedReliabilityRecord(names[i], ReliabilityNamespace.GLOBAL, "global", float(rel[i]),
                                              float(conf[i]), us_to_iso(int(stamp_us[i])), False)
            global_records[names[i]] = rec
            rows.append((rec.source_id, self.GLOBAL_MARKET_ID, rec.reliability, rec.confidence, rec.updated_at))
        N.check_faults(dev, "walk_forward_namespaced")
        total, correct = _domain_counts(domains, markets)
        for k in total:
            if k[1] is None:
                records[k] = global_records[k[0]]
        if not dry_run and rows:
            self._store._upsert(rows)
        return results, SettleSummary(records, global_records, total, correct)

    def sweep_decay_namespaced(self, markets: Sequence[tuple], times: Sequence, half_life_days: Sequence[float],
                               min_rel: Sequence[float], domains=None, market_ids: Optional[Sequence[str]] = None,
                               update_global: bool = False, n_bins: int = 10,
                               resolve_times: Optional[Sequence] = None):
        """:meth:`walk_forward_namespaced` as a dry run for every point of a grid of decay
        parameters, each scored against the batch's outcomes (:func:`batch.walk_sweep_scoped`:
        neither chain family depends on the decay parameters, so both are traced once).  Nothing
        is written.  Returns the :class:`batch.ScoreResult` of the whole history with a leading
        grid dimension ``[len(half_life_days) * len(min_rel), 1, ...]`` (``min_rel`` fastest), or
        None for a history without signals.  ``resolve_times`` as :meth:`walk_forward_namespaced`."""
        b = self._namespaced_walk(markets, times, domains, market_ids, update_global, resolve_times)[-1]
        run = self._sweep_run(b, half_life_days, min_rel, n_bins, False, "sweep_decay_namespaced")
        return None if run is None else run[0]

    def compare_decay_namespaced(self, markets: Sequence[tuple], times: Sequence, half_life_days: Sequence[float],
                                 min_rel: Sequence[float], domains=None, market_ids: Optional[Sequence[str]] = None,
                                 update_global: bool = False, resolve_times: Optional[Sequence] = None,
                                 n_boot: int = 1000, seed: int = 0, block: int = 1):
        """:meth:`compare_decay` over the namespaced walk: the plan and sweep of
        :meth:`sweep_decay_namespaced`, then the same paired bootstrap.  Returns ``(scores,
        boot)`` or None for a history without signals."""
        _check_boot(n_boot, block)
        b = self._namespaced_walk(markets, times, domains, market_ids, update_global, resolve_times)[-1]
        run = self._sweep_run(b, half_life_days, min_rel, 10, True, "compare_decay_namespaced")
        return None if run is None else self._compare(*run, n_boot, seed, block, "compare_decay_namespaced")

    def get_reliability_many(self, names: Sequence[str], market_id: Optional[str] = None,
                             domain: Optional[str] = None, apply_decay: bool = True,
                             now: Optional[datetime] = None) -> List[NamespacedReliabilityRecord]:
        """Records identical to per-source get_reliability, from one resolve() launch."""
        table, scope, stamps = self.resolve(names, market_id, domain, apply_decay, now)
        rc = table.relconf[:len(names)].cpu().numpy()
        code = scope.cpu().numpy()
        out = []
        for i, sid in enumerate(names):
            c = int(code[i])
            if c == batch.NS_COLD:
                out.append(NamespacedReliabilityRecord(sid, ReliabilityNamespace.GLOBAL, "cold-start",
                                                       DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE, "", True))
                continue
            ns, fb = _SCOPE_NS[c]
            value = market_id if c == batch.NS_MARKET else domain if c == batch.NS_DOMAIN else "global"
            out.append(NamespacedReliabilityRecord(sid, ns, value, float(rc[i, 0]), float(rc[i, 1]), stamps[i], fb))
        return out
