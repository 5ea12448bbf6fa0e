"""Bootstrap of the back-test scores: intervals and paired comparisons."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _native as N
from .score import ScorePlan, _nan_div

BOOT_MAX_SETS = N.BOOT_MAX_SETS  # forecast sets of one launch (include/bce.h BCE_BOOT_MAX_SETS)
BOOT_TILE = N.BOOT_TILE          # items the kernel stages at a time
BOOT_COUNTS = ("W", "W_hit")
BOOT_METRICS = ("brier", "log_loss", "accuracy", "skill")  # what the comparisons rank
_HIGHER_IS_BETTER = ("accuracy",)
_ROW_BYTES = 5 * 8  # a scratch row per (segment, replicate, set): 2 counts and 3 sums


def _seed64(seed) -> int:
    """``seed`` (any Python int, taken modulo 2^64) as the int64 of the same bit pattern."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise TypeError(f"seed must be an int (got {type(seed).__name__})")
    s = int(seed) & (2 ** 64 - 1)
    return s - 2 ** 64 if s >= 2 ** 63 else s


def boot_weights(seed: int, replicates, units) -> torch.Tensor:
    """The bootstrap weights ``w(r, u)`` of bce_boot_weights_host as a CPU int32 tensor
    ``[len(replicates), len(units)]`` (include/bce.h: Poisson(1) in 0..21 from an integer hash of
    ``(seed, r, u)``; replicate 0 is all ones).  ``units`` are any int64 values.  Needs no GPU."""
    reps = np.ascontiguousarray(np.asarray(replicates, dtype=np.int64).reshape(-1))
    us = np.ascontiguousarray(np.asarray(units, dtype=np.int64).reshape(-1))
    if reps.size and int(reps.min()) < 0:
        raise ValueError("replicates must be >= 0")
    w = np.zeros((reps.size, us.size), np.int32)
    N.check(N.lib().bce_boot_weights_host(_seed64(seed), N.ptr(reps if reps.size else None), reps.size,
                                          N.ptr(us if us.size else None), us.size, N.ptr(w if w.size else None)),
            "bce_boot_weights_host")
    return torch.from_numpy(w)


def boot_units(n_markets: int, block: int = 1, device=None) -> torch.Tensor:
    """``arange(n_markets) // block``: the resampling units of a block bootstrap over a history in
    time order (``block = 1``: every market on its own)."""
    if int(n_markets) < 0 or int(block) < 1:
        raise ValueError(f"boot_units needs n_markets >= 0 and block >= 1 (got {n_markets}, {block})")
    return torch.arange(int(n_markets), dtype=torch.int64, device=device) // int(block)


def _metric_name(metric: str) -> str:
    if metric not in BOOT_METRICS + ("brier_base",):
        raise ValueError(f"metric must be one of {BOOT_METRICS + ('brier_base',)} (got {metric!r})")
    return metric


@dataclass
class BootstrapResult:
    """:func:`score_bootstrap`: ``counts`` int64[R + 1, G, K, 2] (BOOT_COUNTS: the resampled number
    of scored items and of hits) and ``sums`` fp64[R + 1, G, K, 3] (SCORE_SUMS) of K forecast sets
    over G groups; row 0 is the sample itself, rows 1.. the replicates, the same resample for
    every set.  Everything below is torch only, so it also works on CPU tensors.  A metric is
    ``[R + 1, G, K]`` and NaN where ``W == 0``; a NaN replicate is left out of every statistic."""

    counts: torch.Tensor
    sums: torch.Tensor
    has_base: bool = False

    @property
    def n_boot(self) -> int:
        return int(self.counts.shape[0]) - 1

    @property
    def W(self) -> torch.Tensor:
        return self.counts[..., 0]

    @property
    def brier(self) -> torch.Tensor:
        return _nan_div(self.sums[..., 0], self.W)

    @property
    def log_loss(self) -> torch.Tensor:
        return _nan_div(self.sums[..., 1], self.W)

    @property
    def brier_base(self) -> torch.Tensor:
        return _nan_div(self.sums[..., 2], self.W)

    @property
    def accuracy(self) -> torch.Tensor:
        return _nan_div(self.counts[..., 1], self.W)

    @property
    def skill(self) -> torch.Tensor:
        """``brier - brier_base``: negative = better than the base forecast on the same items."""
        if not self.has_base:
            raise ValueError("skill needs score_bootstrap(base=...)")
        return self.brier - self.brier_base

    def metric(self, metric: str) -> torch.Tensor:
        return getattr(self, _metric_name(metric))

    def point(self, metric: str) -> torch.Tensor:
        """The metric of the sample itself: row 0, ``[G, K]``."""
        return self.metric(metric)[0]

    @staticmethod
    def _limits(x: torch.Tensor, level: float) -> Tuple[torch.Tensor, torch.Tensor]:
        if not 0.0 < float(level) < 1.0:
            raise ValueError(f"level must be in (0, 1) (got {level})")
        if x.shape[0] == 0:
            nan = torch.full(x.shape[1:], float("nan"), dtype=torch.float64, device=x.device)
            return nan, nan.clone()
        a = (1.0 - float(level)) / 2.0
        q = torch.nanquantile(x, torch.tensor([a, 1.0 - a], dtype=torch.float64, device=x.device), dim=0)
        return q[0], q[1]

    def interval(self, metric: str, level: float = 0.95) -> Tuple[torch.Tensor, torch.Tensor]:
        """Percentile limits ``(lo, hi)`` over the replicates, each ``[G, K]`` (``torch.quantile``'s
        linear interpolation; NaN where every replicate is NaN)."""
        return self._limits(self.metric(metric)[1:], level)

    def stderr(self, metric: str) -> torch.Tensor:
        """The standard deviation of the metric over the replicates (n - 1 in the denominator),
        ``[G, K]``; NaN with fewer than two."""
        x = self.metric(metric)[1:]
        ok = ~torch.isnan(x)
        n = ok.sum(0).to(torch.float64)
        z = torch.where(ok, x, torch.zeros_like(x))
        mean = z.sum(0) / n.clamp(min=1.0)
        ss = (torch.where(ok, x - mean, torch.zeros_like(x)) ** 2).sum(0)
        return torch.where(n > 1, (ss / (n - 1).clamp(min=1.0)).sqrt(), torch.full_like(mean, float("nan")))

    def diff(self, metric: str, ref: int, level: float = 0.95):
        """The paired difference against set ``ref``: ``(d, lo, hi)`` with ``d[r, g, k] = metric[r,
        g, k] - metric[r, g, ref]`` under the same resample (row 0: the difference of the point
        estimates) and the percentile limits of rows 1.., each ``[G, K]``."""
        x = self.metric(metric)
        d = x - x[..., self._set(ref)].unsqueeze(-1)
        lo, hi = self._limits(d[1:], level)
        return d, lo, hi

    def _set(self, ref: int) -> int:
        K = int(self.counts.shape[2])
        if isinstance(ref, bool) or not isinstance(ref, (int, np.integer)):
            raise TypeError(f"ref must be an int (got {type(ref).__name__})")
        if not 0 <= int(ref) < K:
            raise ValueError(f"ref must be a set index in [0, {K}) (got {ref})")
        return int(ref)

    def p_better(self, metric: str, ref: int) -> torch.Tensor:
        """The share of replicates in which a set is STRICTLY better than set ``ref`` (lower for
        brier, log_loss and skill, higher for accuracy), ``[G, K]``, over the replicates in which
        both are defined; NaN where there is none.  A tie counts for neither."""
        x = self.metric(metric)[1:]
        y = x[..., self._set(ref)].unsqueeze(-1)
        both = ~torch.isnan(x) & ~torch.isnan(y)
        won = (x > y) if metric in _HIGHER_IS_BETTER else (x < y)
        return _nan_div((won & both).sum(0), both.sum(0))

    def p_best(self, metric: str) -> torch.Tensor:
        """The share of replicates in which each set is the best one, ``[G, K]``: ties go to the
        lowest index, a NaN set never wins, and a replicate in which every set is NaN is left out
        (NaN where none remains), so the shares of a group add up to 1."""
        x = self.metric(metric)[1:]
        nan = torch.isnan(x)
        worst = torch.full_like(x, float("inf"))
        key = torch.where(nan, worst, -x if metric in _HIGHER_IS_BETTER else x)
        top = (key == key.min(-1, keepdim=True).values) & ~nan
        first = top & (top.to(torch.int64).cumsum(-1) == 1)
        return _nan_div(first.sum(0), (~nan).any(-1).sum(0).unsqueeze(-1).expand(first.shape[1:]))


def score_bootstrap(plan: ScorePlan, value: torch.Tensor, outcome: torch.Tensor, *,
                    valid: Optional[torch.Tensor] = None, base: Optional[torch.Tensor] = None,
                    unit: Optional[torch.Tensor] = None, n_boot: int = 1000, seed: int = 0, eps: float = 1e-15,
                    scratch_budget: int = 256 << 20) -> BootstrapResult:
    """The sums of :func:`score` under ``n_boot`` Poisson-bootstrap resamples of the markets, for
    K forecast sets that share every resample (bce_score_bootstrap; rows 0 .. n_boot, row 0 the
    sample itself).  ``value`` is fp64 ``[M']`` or ``[K, M']`` (item i of set k reads ``value[k,
    pidx[i]]``), ``outcome`` int8[M], ``valid`` u8 / bool ``[M]`` or ``[K, M]``, ``base`` fp64[M]
    and ``unit`` int64[M] (the resampling unit of every market; None: the market itself,
    :func:`boot_units` for blocks) are shared by the sets.  The weights are an integer function of
    ``(seed, replicate, unit)`` and the summation shape is fixed (include/bce.h), so every bit of
    the result follows from the arguments: the sets are tiled by BOOT_MAX_SETS and the replicates
    so that the scratch stays under ``scratch_budget`` bytes, and no tiling changes a bit.  No
    host synchronisation; bad indices raise the device fault word as in :func:`score`."""
    if isinstance(n_boot, bool) or not isinstance(n_boot, (int, np.integer)):
        raise TypeError(f"n_boot must be an int (got {type(n_boot).__name__})")
    if n_boot < 0:
        raise ValueError(f"n_boot must be >= 0 (got {n_boot})")
    R1 = int(n_boot) + 1
    if not float(eps) >= 0.0:
        raise ValueError(f"eps must be >= 0 (got {eps})")
    if int(scratch_budget) < 1:
        raise ValueError(f"scratch_budget must be positive (got {scratch_budget})")
    seed = _seed64(seed)
    if outcome.dtype != torch.int8 or outcome.dim() != 1:
        raise ValueError(f"outcome must be int8[M] (-1 unresolved, 0, 1), got {outcome.dtype}")
    if value.dtype != torch.float64 or value.dim() not in (1, 2):
        raise ValueError("value must be an fp64 tensor [M'] or [K, M']")
    value = (value.unsqueeze(0) if value.dim() == 1 else value).contiguous()
    K, n_values = int(value.shape[0]), int(value.shape[1])
    if K < 1:
        raise ValueError("value holds no forecast set")
    M = outcome.numel()
    valid_stride = 0
    if valid is not None:
        if valid.dim() == 2 and tuple(valid.shape) == (K, M):
            valid_stride = M
        elif valid.dim() != 1 or valid.numel() != M:
            raise ValueError(f"valid must be [{M}] or [{K}, {M}]")
        valid = valid.to(torch.uint8).contiguous()
    if base is not None:
        if base.dtype != torch.float64 or base.dim() != 1 or base.numel() != M:
            raise ValueError(f"base must be fp64 with one entry per market ({M})")
        base = base.contiguous()
    if unit is not None:
        if unit.dtype != torch.int64 or unit.dim() != 1 or unit.numel() != M:
            raise ValueError(f"unit must be int64 with one entry per market ({M})")
        unit = unit.contiguous()
    L = N.require_gpu()  # after the argument checks: those need no GPU
    dev = value.device
    G, n_seg, n_items = plan.n_groups, plan.n_segments, plan.n_items
    counts = torch.zeros((R1, G, K, 2), dtype=torch.int64, device=dev)
    sums = torch.zeros((R1, G, K, 3), dtype=torch.float64, device=dev)
    out = BootstrapResult(counts, sums, has_base=base is not None)
    if G == 0:
        return out
    outcome = outcome.contiguous()
    ks_max = min(K, BOOT_MAX_SETS)
    rep_tile = max(1, min(R1, int(scratch_budget) // (max(n_seg, 1) * ks_max * _ROW_BYTES)))
    if 256 <= rep_tile < R1:
        rep_tile -= rep_tile % 256  # whole workgroups of replicates
    scratch = torch.empty(n_seg * rep_tile * ks_max * _ROW_BYTES // 8, dtype=torch.int64, device=dev)
    direct = K <= BOOT_MAX_SETS  # a call's rows are a contiguous slice of the result
    for k0 in range(0, K, BOOT_MAX_SETS):
        ks = min(BOOT_MAX_SETS, K - k0)
        v = value[k0:k0 + ks]
        va = valid if valid is None or valid_stride == 0 else valid[k0:k0 + ks]
        for r0 in range(0, R1, rep_tile):
            nr = min(rep_tile, R1 - r0)
            c = counts[r0:r0 + nr] if direct else torch.empty((nr, G, ks, 2), dtype=torch.int64, device=dev)
            s = sums[r0:r0 + nr] if direct else torch.empty((nr, G, ks, 3), dtype=torch.float64, device=dev)
            sb = int(L.bce_boot_scratch_bytes(n_seg, nr, ks))
            N.check(L.bce_score_bootstrap(
                N.ptr(plan.group_offsets), G, N.ptr(plan.seg_start), N.ptr(plan.seg_group), n_seg,
                N.ptr(plan.pidx if n_items else None), N.ptr(plan.oidx if n_items else None), n_items,
                N.ptr(v if n_values else None), n_values, n_values, ks, N.ptr(outcome if M else None),
                N.ptr(va if M else None), valid_stride, N.ptr(base if M else None), N.ptr(unit if M else None), M,
                float(eps), seed, r0, nr, N.ptr(scratch), sb, N.ptr(c), N.ptr(s), N.stream(dev)),
                "bce_score_bootstrap")
            if not direct:
                counts[r0:r0 + nr, :, k0:k0 + ks] = c
                sums[r0:r0 + nr, :, k0:k0 + ks] = s
    return out
