"""Drop-in for ``bayesian_engine.reliability`` (reference src/bayesian_engine/reliability.py).

SQLite stays on the host as the system of record (same schema, same SQL, autocommit,
WAL: reliability.py:36-79, 221-264).  The arithmetic of the hot path runs on the GPU:

* ``get_reliability(..., apply_decay=True)`` -- decay of the stored value via
  ``bce_decay_apply`` (reliability.py:114-123);
* ``compute_update`` / ``update_reliability`` -- the capped +-MAX_UPDATE_STEP step and
  the confidence growth via ``bce_outcome_update`` (reliability.py:161-173).

Bulk paths for millions of sources:

* :meth:`SQLiteReliabilityStore.load_table` -- ``SELECT ... ORDER BY source_id`` (SQLite
  BINARY collation == code-point order == the engine's rank order) into a dense HBM
  table (rel, conf, updated_at as int64 microseconds, present);
* :meth:`SQLiteReliabilityStore.decayed_view` -- ``get_reliability(apply_decay=True)``
  for every row of a scope in one launch;
* :meth:`SQLiteReliabilityStore.apply_outcomes` -- one outcome per source: one GPU launch,
  then one ``executemany`` upsert in a single transaction (``dry_run`` = no write-back);
* :meth:`SQLiteReliabilityStore.settle` -- any number of outcomes per source: a compiled batch
  of resolved markets (``batch.SettlePlan``) applied to one domain or global scope;
* :meth:`SQLiteReliabilityStore.load_pair_table` / :meth:`SQLiteReliabilityStore.settle_pairs` --
  the market-scope rows of a batch of markets as a sparse HBM table (``batch.PairTable``), and
  the same settlement at market scope, where every (source, market) pair has a row of its own;
* :meth:`SQLiteReliabilityStore.settle_domains` -- that settlement one scope up, for a batch whose
  markets belong to different domains: the ``__domain__:<d>`` rows are a ``batch.PairTable`` over
  the domain index and every market names its domain.
"""
from __future__ import annotations

import sqlite3
from dataclasses import dataclass
from datetime import datetime, timezone
from pathlib import Path
from typing import Dict, List, Mapping, Optional, Sequence, Union

import numpy as np
import torch

from . import _native as N
from . import batch
from .config import (
    BASE_LEARNING_RATE,
    DECAY_HALF_LIFE_DAYS,
    DECAY_MINIMUM,
    DEFAULT_CONFIDENCE,
    DEFAULT_RELIABILITY,
    MAX_UPDATE_STEP,
)
from .decay import apply_reliability_decay, days_since_update
from .timeutil import NO_TIMESTAMP, dt_to_us, iso_to_us, iso_to_us_many, us_to_iso

__all__ = ["ReliabilityRecord", "SQLiteReliabilityStore", "DEFAULT_RELIABILITY", "DEFAULT_CONFIDENCE",
           "MAX_UPDATE_STEP", "DECAY_HALF_LIFE_DAYS", "DECAY_MINIMUM"]

_BASE_LEARNING_RATE: float = BASE_LEARNING_RATE

_CREATE_TABLE_SQL = """
CREATE TABLE IF NOT EXISTS sources (
    source_id   TEXT    NOT NULL,
    market_id   TEXT    NOT NULL,
    reliability REAL    NOT NULL DEFAULT 0.5,
    confidence  REAL    NOT NULL DEFAULT 0.5,
    updated_at  TEXT    NOT NULL,
    PRIMARY KEY (source_id, market_id)
);
"""

_UPSERT_SQL = """
INSERT INTO sources (source_id, market_id, reliability, confidence, updated_at)
VALUES (?, ?, ?, ?, ?)
ON CONFLICT(source_id, market_id)
DO UPDATE SET reliability = excluded.reliability,
              confidence  = excluded.confidence,
              updated_at  = excluded.updated_at
"""


@dataclass(frozen=True)
class ReliabilityRecord:
    """Immutable snapshot of a source's reliability data (reliability.py:48-56)."""

    source_id: str
    market_id: str
    reliability: float
    confidence: float
    updated_at: str


def _as_tensor(a, dev, dtype) -> torch.Tensor:
    """An array or a tensor as a tensor of ``dtype`` on ``dev``."""
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).to(dev, dtype)


def _csr_tensors(dev, offsets, sid, prob, outcome):
    return (_as_tensor(offsets, dev, torch.int64), _as_tensor(sid, dev, torch.int32),
            _as_tensor(prob, dev, torch.float64), _as_tensor(outcome, dev, torch.int8))


def _update_one_gpu(r: float, c: float, correct: bool) -> tuple:
    """reliability.py:163-173 for one row, through the batched update kernel."""
    N.require_gpu()
    dev = N.device()
    rel = torch.tensor([float(r)], dtype=torch.float64, device=dev)
    conf = torch.tensor([float(c)], dtype=torch.float64, device=dev)
    t = torch.zeros(1, dtype=torch.int64, device=dev)
    pres = torch.ones(2, dtype=torch.uint8, device=dev)
    flags = torch.tensor([1 | (2 if correct else 0)], dtype=torch.uint8, device=dev)
    batch.outcome_update(rel, conf, t, pres, flags, 0)
    return float(rel[0].item()), float(conf[0].item())


class SQLiteReliabilityStore:
    """SQLite-backed store for per-source, per-market reliability scores."""

    def __init__(self, db_path: Union[str, Path] = ":memory:") -> None:
        self._db_path = str(db_path)
        self._conn: sqlite3.Connection = sqlite3.connect(self._db_path, isolation_level=None)
        self._conn.execute("PRAGMA journal_mode=WAL")
        self._conn.execute("PRAGMA foreign_keys=ON")
        self._conn.row_factory = sqlite3.Row
        self._ensure_schema()

    # ------------------------------------------------------------------ reference API
    def get_reliability(self, source_id: str, market_id: str, apply_decay: bool = False) -> ReliabilityRecord:
        row = self._conn.execute(
            "SELECT source_id, market_id, reliability, confidence, updated_at "
            "FROM sources WHERE source_id = ? AND market_id = ?",
            (source_id, market_id),
        ).fetchone()
        if row is not None:
            reliability = row["reliability"]
            updated_at = row["updated_at"]
            if apply_decay and updated_at:
                elapsed_days = days_since_update(updated_at)
                if elapsed_days > 0:
                    reliability = apply_reliability_decay(reliability, elapsed_days, DECAY_HALF_LIFE_DAYS,
                                                          DECAY_MINIMUM)
            return ReliabilityRecord(row["source_id"], row["market_id"], reliability, row["confidence"],
                                     updated_at)
        return ReliabilityRecord(source_id, market_id, DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE, "")

    def compute_update(self, source_id: str, market_id: str, outcome_correct: bool) -> ReliabilityRecord:
        current = self.get_reliability(source_id, market_id)
        new_r, new_c = _update_one_gpu(current.reliability, current.confidence, bool(outcome_correct))
        now = datetime.now(timezone.utc).isoformat()
        return ReliabilityRecord(source_id, market_id, new_r, new_c, now)

    def update_reliability(self, source_id: str, market_id: str, outcome_correct: bool,
                           dry_run: bool = False) -> ReliabilityRecord:
        result = self.compute_update(source_id, market_id, outcome_correct)
        if dry_run:
            return result
        self._conn.execute(_UPSERT_SQL, (source_id, market_id, result.reliability, result.confidence,
                                         result.updated_at))
        return result

    def list_sources(self, market_id: Optional[str] = None) -> List[ReliabilityRecord]:
        if market_id is not None:
            rows = self._conn.execute(
                "SELECT source_id, market_id, reliability, confidence, updated_at "
                "FROM sources WHERE market_id = ? ORDER BY source_id",
                (market_id,),
            ).fetchall()
        else:
            rows = self._conn.execute(
                "SELECT source_id, market_id, reliability, confidence, updated_at "
                "FROM sources ORDER BY source_id, market_id",
            ).fetchall()
        return [ReliabilityRecord(r["source_id"], r["market_id"], r["reliability"], r["confidence"],
                                  r["updated_at"]) for r in rows]

    def close(self) -> None:
        self._conn.close()

    def __enter__(self) -> "SQLiteReliabilityStore":
        return self

    def __exit__(self, *exc_info: object) -> None:
        self.close()

    def _ensure_schema(self) -> None:
        self._conn.executescript(_CREATE_TABLE_SQL)

    def _upsert(self, rows) -> None:
        """Rows ``(source_id, market_id, reliability, confidence, updated_at)`` in one transaction."""
        with self._conn:
            self._conn.execute("BEGIN")
            self._conn.executemany(_UPSERT_SQL, rows)

    # ------------------------------------------------------------------ bulk paths (f1)
    def load_table(self, market_id: str, names: Optional[Sequence[str]] = None,
                   device=None) -> batch.ReliabilityTable:
        """Dense HBM table for one scope.  ``names`` (sorted) fixes the rank space (e.g. all
        sourceIds of a batch); absent rows get the baked cold-start values."""
        rows = self._conn.execute(
            "SELECT source_id, reliability, confidence, updated_at FROM sources "
            "WHERE market_id = ? ORDER BY source_id", (market_id,)).fetchall()
        if names is None:
            names = [r[0] for r in rows]
        idx = {n: i for i, n in enumerate(names)}
        S = len(names)
        rel = np.full(S, DEFAULT_RELIABILITY)
        conf = np.full(S, DEFAULT_CONFIDENCE)
        t_us = np.full(S, NO_TIMESTAMP, np.int64)
        present = np.zeros(S, np.uint8)
        if rows:
            pos = np.fromiter((idx.get(r[0], -1) for r in rows), np.int64, len(rows))
            keep = pos >= 0
            cols = list(zip(*rows))
            p = pos[keep]
            rel[p] = np.asarray(cols[1], np.float64)[keep]
            conf[p] = np.asarray(cols[2], np.float64)[keep]
            t_us[p] = iso_to_us_many(cols[3])[keep]
            present[p] = 1
        dev = device or N.device()
        T = batch.to_device(dev)
        return batch.ReliabilityTable(T(rel), T(conf), T(t_us), T(present), list(names))

    def decayed_view(self, table: batch.ReliabilityTable, now: Optional[datetime] = None) -> torch.Tensor:
        """get_reliability(apply_decay=True).reliability for every source of ``table``."""
        return table.view(dt_to_us(now or datetime.now(timezone.utc)))

    def apply_outcomes(self, market_id: str, outcomes: Mapping[str, bool], dry_run: bool = False,
                       now: Optional[datetime] = None) -> Dict[str, ReliabilityRecord]:
        """update_reliability for many sources at once (one outcome each)."""
        names = sorted(outcomes)
        table = self.load_table(market_id, names)
        S = len(names)
        flags = np.zeros(S, np.uint8)
        for i, n in enumerate(names):
            flags[i] = 1 | (2 if outcomes[n] else 0)
        now_us = dt_to_us(now or datetime.now(timezone.utc))
        dflags = torch.from_numpy(flags).to(table.rel.device)
        batch.outcome_update(table.rel, table.conf, table.t_us, table.present, dflags, now_us)
        rel = table.rel[:S].cpu().numpy()
        conf = table.conf[:S].cpu().numpy()
        stamp = us_to_iso(now_us)
        out = {n: ReliabilityRecord(n, market_id, float(rel[i]), float(conf[i]), stamp) for i, n in enumerate(names)}
        if not dry_run and S:
            self._upsert((n, market_id, float(rel[i]), float(conf[i]), stamp) for i, n in enumerate(names))
        return out

    def settle(self, market_id: str, names: Sequence[str], plan: "batch.SettlePlan", dry_run: bool = False,
               now: Optional[datetime] = None) -> Dict[str, ReliabilityRecord]:
        """update_reliability for every signal of a compiled batch of resolved markets
        (:class:`batch.SettlePlan` over the rank space ``names``), any number of outcomes per
        source, in the reference's loop order: one load_table, the chain kernels, then one
        ``executemany`` upsert of the touched rows in a single transaction.  ``market_id`` is a
        domain (``__domain__:<d>``) or the global scope key; market-level rows, keyed by
        (source, market), are settled by :meth:`settle_pairs`.  Returns the touched sources'
        records."""
        names = list(names)
        if len(names) != plan.n_sources:
            raise ValueError(f"the plan ranks {plan.n_sources} sources, names has {len(names)}")
        table = self.load_table(market_id, names, device=plan.order.device)
        now_us = dt_to_us(now or datetime.now(timezone.utc))
        table.settle(plan, now_us)
        touched = plan.order.cpu().numpy()
        rel = table.rel.cpu().numpy()
        conf = table.conf.cpu().numpy()
        N.check_faults(plan.order.device, "settle")
        stamp = us_to_iso(now_us)
        out = {names[i]: ReliabilityRecord(names[i], market_id, float(rel[i]), float(conf[i]), stamp)
               for i in sorted(int(x) for x in touched)}
        if not dry_run and out:
            self._upsert((r.source_id, market_id, r.reliability, r.confidence, stamp) for r in out.values())
        return out

    _IN_CHUNK = 900  # host parameters per statement (SQLite's default limit is 999)

    def load_pair_table(self, market_ids: Sequence[str], names: Sequence[str], device=None) -> batch.PairTable:
        """The market-scope rows of ``market_ids`` as a :class:`batch.PairTable`: row i of the
        batch is ``market_ids[i]`` (distinct, else ``ValueError``), sources are ranked by ``names``
        (sorted) and rows of other sources are dropped.  ``market_id IN (...)`` in chunks, never
        one statement per market.  ``device="cpu"`` needs no GPU."""
        market_ids = [str(m) for m in market_ids]
        mrank = {m: i for i, m in enumerate(market_ids)}
        if len(mrank) != len(market_ids):
            raise ValueError("duplicate market id in market_ids")
        srank = {n: i for i, n in enumerate(names)}
        mk: List[int] = []
        sd: List[int] = []
        rel: List[float] = []
        conf: List[float] = []
        stamps: List[str] = []
        for k in range(0, len(market_ids), self._IN_CHUNK):
            chunk = market_ids[k:k + self._IN_CHUNK]
            q = ("SELECT source_id, market_id, reliability, confidence, updated_at FROM sources "
                 f"WHERE market_id IN ({','.join('?' * len(chunk))})")
            for sid, mid, r, c, ts in self._conn.execute(q, chunk):
                s = srank.get(sid)
                if s is None:
                    continue
                mk.append(mrank[mid])
                sd.append(s)
                rel.append(r)
                conf.append(c)
                stamps.append(ts)
        dev = device if device is not None else N.device()
        T = batch.to_device(dev)
        has = np.fromiter((1 if ts else 0 for ts in stamps), np.uint8, len(stamps))
        return batch.PairTable.from_rows(T(np.asarray(mk, np.int64)), T(np.asarray(sd, np.int32)),
                                         T(np.asarray(rel, np.float64)), T(np.asarray(conf, np.float64)),
                                         T(iso_to_us_many(stamps)), T(has), len(market_ids), max(len(srank), 1))

    def settle_pairs(self, market_ids: Sequence[str], names: Sequence[str], offsets, sid, prob, outcome,
                     dry_run: bool = False, now: Optional[datetime] = None) -> Dict[tuple, ReliabilityRecord]:
        """``update_reliability(source, market_id, correct)`` for every signal of every market of
        the CSR batch with ``outcome >= 0``, at MARKET scope, in the reference's loop order:
        :meth:`load_pair_table`, :func:`batch.settle_pairs`, then one ``executemany`` upsert of the
        touched pairs in a single transaction (``dry_run``: no write).  ``offsets`` / ``sid`` /
        ``prob`` / ``outcome`` are arrays or tensors; market i is ``market_ids[i]``, ranks index
        ``names``.  Returns ``{(source_id, market_id): record}`` of the touched pairs."""
        N.require_gpu()
        dev = N.device()
        market_ids = [str(m) for m in market_ids]
        offsets, sid, prob, outcome = _csr_tensors(dev, offsets, sid, prob, outcome)
        if offsets.numel() != len(market_ids) + 1:
            raise ValueError("offsets must have len(market_ids) + 1 entries")
        pairs = self.load_pair_table(market_ids, names, device=dev)
        plan = batch.PairPlan.build(offsets, sid, prob, pairs.n_sources)
        return self._settle_keyed(market_ids, names, plan, pairs, batch.settle_pairs, offsets, prob, outcome,
                                  "settle_pairs", dry_run, now)

    def settle_domains(self, domain_keys: Sequence[str], names: Sequence[str], offsets, sid, prob, outcome,
                       market_domain, dry_run: bool = False,
                       now: Optional[datetime] = None) -> Dict[tuple, ReliabilityRecord]:
        """:meth:`settle_pairs` one scope up, for a batch whose markets belong to different
        domains: ``update_reliability(source, domain_keys[market_domain[m]], correct)`` for every
        signal of every market ``m`` with ``outcome >= 0`` and ``market_domain[m] >= 0``, in the
        reference's loop order.  ``domain_keys`` are the scope keys as stored (``__domain__:<d>``,
        distinct); their rows come from :meth:`load_pair_table` with the domain index in the
        market's place, :func:`batch.settle_domains` applies the chains, and the touched (source,
        domain key) rows are written by one ``executemany`` in a single transaction (``dry_run``:
        no write).  Returns ``{(source_id, domain_key): record}`` of the touched pairs."""
        N.require_gpu()
        dev = N.device()
        domain_keys = [str(k) for k in domain_keys]
        offsets, sid, prob, outcome = _csr_tensors(dev, offsets, sid, prob, outcome)
        domains = self.load_pair_table(domain_keys, names, device=dev)
        plan = batch.DomainPlan.build(offsets, sid, _as_tensor(market_domain, dev, torch.int32), domains.n_sources,
                                      len(domain_keys))
        return self._settle_keyed(domain_keys, names, plan, domains, batch.settle_domains, offsets, prob, outcome,
                                  "settle_domains", dry_run, now)

    def _settle_keyed(self, keys: List[str], names: Sequence[str], plan: "batch.PairPlan", table: "batch.PairTable",
                      settle, offsets, prob, outcome, what: str, dry_run: bool,
                      now: Optional[datetime]) -> Dict[tuple, ReliabilityRecord]:
        """The body of :meth:`settle_pairs` / :meth:`settle_domains`: ``settle`` (the function of
        :mod:`batch` of that name) applies the chains to ``table``, whose market index ranks
        ``keys``; the touched rows are read back per entry of ``plan`` and upserted."""
        names = list(names)
        now_us = dt_to_us(now or datetime.now(timezone.utc))
        settled, splan = settle(plan, table, offsets, prob, outcome, now_us)
        E = plan.n_entries
        if not E:  # an empty batch, or (domains) no signal in a market with a domain
            return {}
        # every touched pair now has a row: read them back per entry
        r = batch.pair_resolve(plan.uoffsets, plan.usid, settled, now_us, mode="raw", emarket=plan.emarket)
        touched = torch.nonzero(splan.total[:E] > 0).flatten()
        ek = plan.emarket[touched].cpu().numpy()
        us = plan.usid[touched].cpu().numpy()
        rel = r.rel[touched].cpu().numpy()
        conf = r.conf[touched].cpu().numpy()
        N.check_faults(offsets.device, what)
        stamp = us_to_iso(now_us)
        out = {(names[int(s)], keys[int(k)]): ReliabilityRecord(names[int(s)], keys[int(k)], float(x), float(c), stamp)
               for k, s, x, c in zip(ek, us, rel, conf)}
        if not dry_run and out:
            self._upsert((r_.source_id, r_.market_id, r_.reliability, r_.confidence, stamp) for r_ in out.values())
        return out

    def fetch_pairs(self, pairs: Sequence[tuple]) -> Dict[tuple, tuple]:
        """Rows for (source_id, market_id) pairs -> {(sid, mid): (rel, conf, updated_at)}."""
        out = {}
        by_market: Dict[str, List[str]] = {}
        for s, m in pairs:
            by_market.setdefault(m, []).append(s)
        for m, sids in by_market.items():
            for k in range(0, len(sids), 900):
                chunk = sids[k:k + 900]
                q = ("SELECT source_id, reliability, confidence, updated_at FROM sources WHERE market_id = ? "
                     f"AND source_id IN ({','.join('?' * len(chunk))})")
                for sid, r, c, ts in self._conn.execute(q, [m, *chunk]):
                    out[(sid, m)] = (r, c, ts)
        return out
