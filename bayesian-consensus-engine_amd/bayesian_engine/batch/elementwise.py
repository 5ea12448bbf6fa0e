"""Streaming kernels over the reliability table: decayed view, outcome update, replay step."""
from typing import Optional

import numpy as np
import torch

from .. import _native as N
from ..config import DECAY_HALF_LIFE_DAYS, DECAY_MINIMUM, DEFAULT_CONFIDENCE, DEFAULT_RELIABILITY


def decay_view(rel: torch.Tensor, t_us: torch.Tensor, now_us: int, present: Optional[torch.Tensor] = None,
               half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM,
               default_rel: float = DEFAULT_RELIABILITY, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """get_reliability(apply_decay=True) for a whole table (reliability.py:110-131)."""
    L = N.require_gpu()
    n = rel.numel()
    view = out if out is not None else torch.empty(max(n, 2), dtype=torch.float64, device=rel.device)
    N.check(L.bce_decay_view(n, N.ptr(rel), N.ptr(t_us), N.ptr(present), int(now_us), float(half_life_days),
                             float(min_rel), float(default_rel), N.ptr(view), N.stream(rel.device)),
            "bce_decay_view")
    return view[:n]


def decay_apply(rel: Optional[torch.Tensor], elapsed_days: torch.Tensor,
                half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM,
                want_factor: bool = False):
    """decay.compute_decay_factor / apply_reliability_decay on arrays (decay.py:31-100)."""
    L = N.require_gpu()
    n = elapsed_days.numel()
    dev = elapsed_days.device
    out = torch.empty(n, dtype=torch.float64, device=dev) if rel is not None else None
    fac = torch.empty(n, dtype=torch.float64, device=dev) if want_factor else None
    N.check(L.bce_decay_apply(n, N.ptr(rel), N.ptr(elapsed_days), float(half_life_days), float(min_rel),
                              N.ptr(out), N.ptr(fac), N.stream(dev)), "bce_decay_apply")
    return out, fac


def outcome_update(rel: torch.Tensor, conf: torch.Tensor, t_us: torch.Tensor, present: torch.Tensor,
                   flags: torch.Tensor, now_us: int, default_rel: float = DEFAULT_RELIABILITY,
                   default_conf: float = DEFAULT_CONFIDENCE) -> None:
    """In-place update_reliability math for every participant (reliability.py:142-183).

    flags u8[S]: bit0 participates, bit1 correct (at most one outcome per source per call;
    :func:`settle` applies a whole batch of resolved markets, any number per source).
    """
    L = N.require_gpu()
    N.check(L.bce_outcome_update(rel.numel(), N.ptr(rel), N.ptr(conf), N.ptr(t_us), N.ptr(present),
                                 N.ptr(flags), int(now_us), float(default_rel), float(default_conf),
                                 N.stream(rel.device)), "bce_outcome_update")


def replay_step(rel, conf, t_us, present, flags2, now_us: int, view: torch.Tensor,
                half_life_days: float = DECAY_HALF_LIFE_DAYS, min_rel: float = DECAY_MINIMUM) -> None:
    """Config-4 step: decayed view at ``now_us`` then the outcome update, fused.

    flags2: 2 bits per source (bit0 participates, bit1 correct), 4 sources per byte.
    Absent rows must hold the baked cold-start values (rel 0.5, conf 0.25, t = NO_TIMESTAMP).
    """
    L = N.require_gpu()
    N.check(L.bce_replay_step(rel.numel(), N.ptr(rel), N.ptr(conf), N.ptr(t_us), N.ptr(present),
                              N.ptr(flags2), int(now_us), float(half_life_days), float(min_rel),
                              DEFAULT_RELIABILITY, DEFAULT_CONFIDENCE, N.ptr(view), N.stream(rel.device)),
            "bce_replay_step")


def pack_flags2(participate: np.ndarray, correct: np.ndarray) -> np.ndarray:
    """Host helper: (participate, correct) bool arrays -> the 2-bit packed flags2 layout."""
    S = len(participate)
    f = participate.astype(np.uint8) | (correct.astype(np.uint8) << 1)
    pad = (-S) % 4
    f = np.concatenate([f, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    return (f[:, 0] | (f[:, 1] << 2) | (f[:, 2] << 4) | (f[:, 3] << 6)).astype(np.uint8)
