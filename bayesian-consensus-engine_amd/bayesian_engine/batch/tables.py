"""The tables every subsystem shares, the entry buffers, and the argument checks of the builders."""
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from .. import _native as N
from ..config import DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY
from .elementwise import decay_view


def intern(ids: Iterable[str]) -> Dict[str, int]:
    """Rank ids in Python ``sorted()`` (code-point) order: integer order == str order."""
    return {s: i for i, s in enumerate(sorted(set(ids)))}


def to_device(dev):
    """``T = to_device(dev)``: ``T(a)`` is the numpy array ``a`` as a tensor on ``dev``."""
    return lambda a: torch.from_numpy(a).to(dev)


@dataclass
class SourceTable:
    """Dense per-source table resident in HBM, in the consensus kernel's layout.

    relconf [S, 2] fp64: interleaved {reliability, confidence} -> one 16-B gather per
    unique source; bits [ceil(S/32)] int32: present bitmask ("sourceId is a key of the
    reliability dict", core.py:167-170).  Cold-start defaults are baked into relconf.
    """

    relconf: torch.Tensor
    bits: torch.Tensor
    names: List[str]
    t_us: Optional[torch.Tensor] = None

    @property
    def n(self) -> int:
        return len(self.names)

    @property
    def rel(self) -> torch.Tensor:
        return self.relconf[:, 0]

    @property
    def conf(self) -> torch.Tensor:
        return self.relconf[:, 1]

    @classmethod
    def from_arrays(cls, rel: torch.Tensor, conf: torch.Tensor, present: Optional[torch.Tensor],
                    names: Optional[Sequence[str]] = None, t_us: Optional[torch.Tensor] = None) -> "SourceTable":
        """Pack device arrays with bce_table_pack (one launch)."""
        L = N.require_gpu()
        S = rel.numel()
        dev = rel.device
        relconf = torch.empty((max(S, 1), 2), dtype=torch.float64, device=dev)
        bits = torch.zeros(max((S + 31) // 32, 1), dtype=torch.int32, device=dev)
        rel = rel.to(torch.float64).contiguous()
        conf = conf.to(torch.float64).contiguous()
        pres = present.to(torch.uint8).contiguous() if present is not None else None
        N.check(L.bce_table_pack(S, N.ptr(rel), N.ptr(conf), N.ptr(pres), N.ptr(relconf), N.ptr(bits),
                                 N.stream(dev)), "bce_table_pack")
        return cls(relconf, bits, list(names) if names is not None else [""] * S, t_us)

    @classmethod
    def from_dict(cls, names: Sequence[str], source_reliability: Optional[dict], device=None) -> "SourceTable":
        """core.py:110-112 semantics: a key present (even with a partial dict) is not cold."""
        S = len(names)
        rel = np.full(max(S, 1), DEFAULT_RELIABILITY, np.float64)
        conf = np.full(max(S, 1), DEFAULT_CONFIDENCE, np.float64)
        present = np.zeros(max(S, 1), np.uint8)
        sr = source_reliability or {}
        for i, n in enumerate(names):
            if n in sr:
                present[i] = 1
                d = sr.get(n, {})  # a None value raises AttributeError, as core.py:110-111 does
                r = d.get("reliability", DEFAULT_RELIABILITY)
                c = d.get("confidence", DEFAULT_CONFIDENCE)
                acc = 0.0
                acc += r  # same TypeError as core.py:120 for non-numbers
                rel[i] = float(r)
                conf[i] = float(c)
        dev = device or N.device()
        T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        return cls.from_arrays(T(rel[:S]), T(conf[:S]), T(present[:S]), names)


@dataclass
class ReliabilityTable:
    """Store-side table (SoA) for the streaming decay / outcome-update kernels.

    rel, conf fp64[S], t_us int64[S] (updated_at as microseconds, NO_TIMESTAMP if
    falsy/unparseable), present u8[S] (a row exists).  Absent rows hold the baked
    cold-start values (0.5, 0.25, NO_TIMESTAMP), reliability.py:133-140.
    """

    rel: torch.Tensor
    conf: torch.Tensor
    t_us: torch.Tensor
    present: torch.Tensor
    names: List[str]

    @property
    def n(self) -> int:
        return len(self.names)

    def view(self, now_us: int) -> torch.Tensor:
        """get_reliability(apply_decay=True).reliability of every source."""
        return decay_view(self.rel, self.t_us, now_us, present=self.present)

    def consensus_table(self, now_us: Optional[int] = None, all_present: bool = True) -> "SourceTable":
        """Packed consensus table; reliability decayed at ``now_us`` when given.  Callers that
        fetch every source through get_reliability (market.py:209-219, cli.py:37-44) put
        every sourceId in the dict, hence ``all_present``."""
        rel = self.view(now_us) if now_us is not None else self.rel
        return SourceTable.from_arrays(rel, self.conf, None if all_present else self.present, self.names)
    # ``settle`` / ``walk_forward``: attached in settle.py / walk.py, where those functions live


@dataclass
class ScopeTable:
    """One namespace scope of the store (rows of one market_id key) over a rank space:
    rel, conf fp64[S], t_us int64[S] (NO_TIMESTAMP = unparseable), has u8[S] = a row with a
    truthy updated_at exists (the ``if record.updated_at`` test)."""

    rel: torch.Tensor
    conf: torch.Tensor
    t_us: torch.Tensor
    has: torch.Tensor


NS_MARKET, NS_DOMAIN, NS_GLOBAL, NS_COLD = 0, 1, 2, 3


# ---------------------------------------------------------------------------------------
# market scope: the (source, market) rows of the store as a sparse table in HBM
# ---------------------------------------------------------------------------------------
@dataclass
class PairTable:
    """The market-scope rows of a batch of markets, CSR by market over the batch's market index:
    ``poffsets`` int64[M+1] (the row range of every market), ``psid`` int32[P] (source ranks,
    strictly ascending inside a market), ``rel`` / ``conf`` fp64[P], ``t_us`` int64[P]
    (NO_TIMESTAMP where ``updated_at`` is falsy or unparseable), ``has`` u8[P] (``updated_at`` is
    truthy: the ``if record.updated_at`` test).  Only rows that exist are stored."""

    poffsets: torch.Tensor
    psid: torch.Tensor
    rel: torch.Tensor
    conf: torch.Tensor
    t_us: torch.Tensor
    has: torch.Tensor
    n_markets: int
    n_sources: int

    @property
    def n_rows(self) -> int:
        return int(self.psid.numel())

    @classmethod
    def empty(cls, n_markets: int, n_sources: int, device=None) -> "PairTable":
        dev = device if device is not None else N.device()
        z = lambda dt: torch.zeros(0, dtype=dt, device=dev)  # noqa: E731
        return cls(torch.zeros(int(n_markets) + 1, dtype=torch.int64, device=dev), z(torch.int32),
                   z(torch.float64), z(torch.float64), z(torch.int64), z(torch.uint8), int(n_markets),
                   int(n_sources))

    @classmethod
    def from_rows(cls, market: torch.Tensor, sid: torch.Tensor, rel: torch.Tensor, conf: torch.Tensor,
                  t_us: torch.Tensor, has: torch.Tensor, n_markets: int, n_sources: int) -> "PairTable":
        """Rows in any order (tensors of one device, CPU included: torch only, no kernel) sorted
        into the table.  A duplicate (market, sid), or an index outside the batch, ``ValueError``."""
        M, S = int(n_markets), int(n_sources)
        if M < 0 or M >= (1 << 31):
            raise ValueError(f"n_markets must be in [0, 2^31) (got {n_markets})")
        if not 0 < S < (1 << 31):
            raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources})")
        P = market.numel()
        if not all(x.numel() == P for x in (sid, rel, conf, t_us, has)):
            raise ValueError("the row arrays differ in length")
        dev = market.device
        if P == 0:
            return cls.empty(M, S, dev)
        mk = market.to(torch.int64)
        sd = sid.to(torch.int64)
        if int(mk.min()) < 0 or int(mk.max()) >= M:
            raise ValueError("a row's market index is outside [0, n_markets)")
        if int(sd.min()) < 0 or int(sd.max()) >= S:
            raise ValueError("a row's source rank is outside [0, n_sources)")
        key, perm = torch.sort(mk * S + sd)
        if P > 1 and bool((key[1:] == key[:-1]).any()):
            raise ValueError("duplicate (market, sid) row")
        poffsets = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        poffsets[1:] = torch.cumsum(torch.bincount(mk, minlength=M), 0)
        return cls(poffsets, sd[perm].to(torch.int32), rel.to(torch.float64)[perm].contiguous(),
                   conf.to(torch.float64)[perm].contiguous(), t_us.to(torch.int64)[perm].contiguous(),
                   has.to(torch.uint8)[perm].contiguous(), M, S)


# ---------------------------------------------------------------------------------------
# what the builders and the launches share: entry buffers and argument checks
# ---------------------------------------------------------------------------------------
def _entry_buffers(E: int, dev):
    """``(relconf [E, 2], present words (zeroed), u8[E])`` over E entries, at least one row each."""
    E1 = max(E, 1)
    return (torch.empty((E1, 2), dtype=torch.float64, device=dev),
            torch.zeros(max((E + 31) // 32, 1), dtype=torch.int32, device=dev),
            torch.empty(E1, dtype=torch.uint8, device=dev))


def _check_csr(offsets: torch.Tensor, sid: torch.Tensor, n_sources: int, *, too_many: Optional[str] = None,
               prob: Optional[torch.Tensor] = None, outcome: Optional[torch.Tensor] = None,
               market_domain: Optional[torch.Tensor] = None, n_domains: Optional[int] = None,
               values: bool = True):
    """The shape of a CSR batch, for every builder (torch only, any device): returns ``(M, Nsig, S,
    offsets as int64, lens)`` or raises ``ValueError``.  ``too_many``: the caller's text for 2^31
    markets, formatted with M (None: the caller has no int32 market index); ``prob``, ``outcome``
    and ``market_domain`` / ``n_domains`` are checked where given.  ``values=False`` checks shapes
    and dtypes alone -- nothing is read from the device -- and returns None for the last two: for
    a caller whose builders check the offsets themselves."""
    M, Nsig = offsets.numel() - 1, sid.numel()
    try:
        S = int(n_sources)
    except (TypeError, ValueError):
        raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources!r})") from None
    if not 0 < S < (1 << 31):
        raise ValueError(f"n_sources must be in [1, 2^31) (got {n_sources})")
    if n_domains is not None and not 0 <= int(n_domains) < (1 << 31):
        raise ValueError(f"n_domains must be in [0, 2^31) (got {n_domains})")
    if M < 0 or offsets.dim() != 1:
        raise ValueError("offsets must be a 1-D tensor of n_markets + 1 entries")
    if too_many is not None and M >= (1 << 31):
        raise ValueError(too_many.format(M))
    if prob is not None and prob.numel() != Nsig:
        raise ValueError("sid and prob differ in length")
    if outcome is not None:
        if outcome.dtype != torch.int8:
            raise ValueError(f"outcome must be int8 (-1 unresolved, 0, 1), got {outcome.dtype}")
        if outcome.dim() != 1 or outcome.numel() != M:
            raise ValueError(f"outcome must have one entry per market ({M}), got {tuple(outcome.shape)}")
    if market_domain is not None and (market_domain.dim() != 1 or market_domain.numel() != M):
        raise ValueError(f"market_domain must have one entry per market ({M}), got {tuple(market_domain.shape)}")
    if not values:
        return M, Nsig, S, None, None
    offsets = offsets.to(torch.int64)
    lens = offsets[1:] - offsets[:-1]
    if (M and (int(offsets[0]) != 0 or int(offsets[-1]) != Nsig or int(lens.min()) < 0)) or (M == 0 and Nsig):
        raise ValueError("offsets must rise from 0 to len(sid)")
    return M, Nsig, S, offsets, lens


def _check_table(rel: torch.Tensor, conf: torch.Tensor, t_us: torch.Tensor, present: Optional[torch.Tensor],
                 S: int, rows: str = "the table must have n_sources rows") -> None:
    """A dense scope table against the ``n_sources`` of the plan that reads or writes it."""
    assert rel.dtype == torch.float64 and conf.dtype == torch.float64 and t_us.dtype == torch.int64, \
        "rel / conf must be fp64 and t_us int64"
    assert rel.numel() == S and conf.numel() == S and t_us.numel() == S, rows
    assert present is None or (present.dtype == torch.uint8 and present.numel() == S), "present must be u8[n_sources]"


def _check_market_time(market_time_us: torch.Tensor, M: int) -> None:
    if market_time_us.dtype != torch.int64 or market_time_us.dim() != 1 or market_time_us.numel() != M:
        raise ValueError(f"market_time_us must be int64 with one entry per market ({M})")
