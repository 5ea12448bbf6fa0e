"""Glob patterns over market ids (include/bce.h "market-id glob patterns")."""
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import _native as N

GLOB_MAX_OPS = 256    # include/bce.h BCE_GLOB_MAX_OPS
GLOB_MAX_RANGES = 64  # include/bce.h BCE_GLOB_MAX_RANGES
_GLOB_LIT, _GLOB_ANY, _GLOB_STAR, _GLOB_CLS = 0 << 29, 1 << 29, 2 << 29, 3 << 29
_GLOB_NEGATE = 1 << 28


class _GlobDeclined(Exception):
    """The pattern is left to fnmatch on the host."""


def _glob_bracket(pat: str, i: int, j: int):
    """The bracket expression pat[i:j] (``i`` just behind '[', ``j`` at the closing ']') as
    fnmatch.translate (CPython 3.10, fnmatch.py:110-151) turns it into a regex set, and that set
    as ``re`` reads it: ``("never" | "any" | "set", negate, [(lo, hi), ...])``."""
    stuff = pat[i:j]
    if "-" not in stuff:
        stuff = stuff.replace("\\", "\\\\")
    else:
        chunks = []
        k = i + 2 if pat[i] == "!" else i + 1
        while True:
            k = pat.find("-", k, j)
            if k < 0:
                break
            chunks.append(pat[i:k])
            i = k + 1
            k = k + 3
        chunk = pat[i:j]
        if chunk:
            chunks.append(chunk)
        else:
            chunks[-1] += "-"
        for k in range(len(chunks) - 1, 0, -1):  # "remove empty ranges"
            if chunks[k - 1][-1] > chunks[k][0]:
                chunks[k - 1] = chunks[k - 1][:-1] + chunks[k][1:]
                del chunks[k]
        stuff = "-".join(s.replace("\\", "\\\\").replace("-", "\\-") for s in chunks)
    for c in "&~|":
        stuff = stuff.replace(c, "\\" + c)
    if not stuff:
        return "never", False, []
    if stuff == "!":
        return "any", False, []
    negate = stuff[0] == "!"
    if negate:
        stuff = stuff[1:]
    elif stuff[0] in "^[":
        stuff = "\\" + stuff
    # the set as sre_parse reads it: every escape left is a backslash in front of punctuation (a
    # literal), an unescaped '-' between two members is a range, a trailing one a member
    toks = []
    k = 0
    while k < len(stuff):
        if stuff[k] == "\\":
            toks.append((ord(stuff[k + 1]), False))
            k += 2
        else:
            toks.append((ord(stuff[k]), stuff[k] == "-"))
            k += 1
    ranges = []
    k = 0
    while k < len(toks):
        lo = toks[k][0]
        k += 1
        if k < len(toks) and toks[k][1]:
            if k + 1 == len(toks):
                ranges += [(lo, lo), (0x2D, 0x2D)]
                break
            hi = toks[k + 1][0]
            k += 2
            if hi < lo:
                raise _GlobDeclined("bad character range")  # re.error in the reference
            ranges.append((lo, hi))
        else:
            ranges.append((lo, lo))
    return "set", negate, ranges


def _glob_compile_one(pat: str):
    """One pattern as ``[op]`` with classes still inline: an op is an int, or ``(negate, ranges)``.
    fnmatch.translate's scan (fnmatch.py:89-153); its second half only anchors the pieces between
    stars, which the iterative matcher does by construction."""
    ops: list = []
    i, n = 0, len(pat)
    while i < n:
        c = pat[i]
        i += 1
        if c == "*":
            if not ops or ops[-1] != _GLOB_STAR:
                ops.append(_GLOB_STAR)
        elif c == "?":
            ops.append(_GLOB_ANY)
        elif c == "[":
            j = i
            if j < n and pat[j] == "!":
                j += 1
            if j < n and pat[j] == "]":
                j += 1
            while j < n and pat[j] != "]":
                j += 1
            if j >= n:
                ops.append(_GLOB_LIT | 0x5B)
            else:
                kind, negate, ranges = _glob_bracket(pat, i, j)
                i = j + 1
                if kind == "any":
                    ops.append(_GLOB_ANY)
                elif kind == "never":
                    ops.append((False, ()))
                else:
                    ranges = sorted(set(ranges))
                    if len(ranges) > GLOB_MAX_RANGES:
                        raise _GlobDeclined("too many ranges")
                    ops.append((negate, tuple(ranges)))
        else:
            ops.append(_GLOB_LIT | ord(c))
    if len(ops) > GLOB_MAX_OPS:
        raise _GlobDeclined("too many ops")
    return ops


@dataclass
class NameTable:
    """Names packed for the matcher: UTF-8 bytes ('surrogatepass') and int64 offsets [M+1], on the
    host and -- when built with a device -- in HBM; ``strings`` serves the declined patterns."""

    strings: List[str]
    bytes_host: np.ndarray
    off_host: np.ndarray
    data: Optional[torch.Tensor] = None
    off: Optional[torch.Tensor] = None

    @property
    def n(self) -> int:
        return len(self.strings)

    @classmethod
    def from_strings(cls, names: Sequence[str], device=None) -> "NameTable":
        strings = list(names)
        enc = [s.encode("utf-8", "surrogatepass") for s in strings]
        off = np.zeros(len(enc) + 1, np.int64)
        if enc:
            np.cumsum(np.fromiter(map(len, enc), np.int64, len(enc)), out=off[1:])
        data = np.frombuffer(b"".join(enc), np.uint8)
        if data.size == 0:
            data = np.zeros(1, np.uint8)
        t = cls(strings, data, off)
        if device is not None:
            t.data = torch.from_numpy(data.copy()).to(device)
            t.off = torch.from_numpy(off).to(device)
        return t


@dataclass
class GlobSet:
    """Compiled patterns (host arrays, include/bce.h): ``patterns`` are the distinct patterns in
    first-seen order, ``index[i]`` the row of the i-th pattern given, ``declined`` the rows whose
    pattern is over a cap (or that fnmatch itself rejects) and is evaluated by fnmatch on the host."""

    patterns: List[str]
    index: List[int]
    prog: np.ndarray      # uint32 [n_ops]
    prog_off: np.ndarray  # int64 [P+1]
    cls_rng: np.ndarray   # uint32 [2 * n_rng]
    cls_off: np.ndarray   # int32 [n_cls+1]
    declined: List[int]

    @property
    def n(self) -> int:
        return len(self.patterns)

    @property
    def n_cls(self) -> int:
        return len(self.cls_off) - 1

    @classmethod
    def compile(cls, patterns: Sequence[str]) -> "GlobSet":
        row: Dict[str, int] = {}
        index = []
        for p in patterns:
            if p not in row:
                row[p] = len(row)
            index.append(row[p])
        classes: Dict[tuple, int] = {}
        prog: List[int] = []
        prog_off = [0]
        declined = []
        for p, r in row.items():
            try:
                ops = _glob_compile_one(p)
            except Exception:  # over a cap, or malformed for translate() itself: fnmatch answers (or raises)
                ops = None
                declined.append(r)
            for op in ops or ():
                if isinstance(op, tuple):
                    c = classes.setdefault(op[1], len(classes))
                    op = _GLOB_CLS | (_GLOB_NEGATE if op[0] else 0) | c
                prog.append(op)
            prog_off.append(len(prog))
        rng: List[int] = []
        cls_off = [0]
        for ranges in classes:  # insertion order == class index
            for lo, hi in ranges:
                rng += [lo, hi]
            cls_off.append(len(rng) // 2)
        return cls(list(row), index, np.array(prog, np.uint32), np.array(prog_off, np.int64),
                   np.array(rng, np.uint32), np.array(cls_off, np.int32), declined)


def _glob_host_row(names: NameTable, pattern: str) -> np.ndarray:
    """One bitmap row by fnmatch itself (a declined pattern): uint64 [ceil(M / 64)]."""
    import fnmatch

    M = names.n
    hit = np.zeros(((M + 63) // 64) * 64, np.uint8)
    hit[:M] = np.fromiter((fnmatch.fnmatchcase(s, pattern) for s in names.strings), np.uint8, M)
    return np.packbits(hit, bitorder="little").view(np.uint64)


def _np_or_dummy(a: np.ndarray, dtype) -> np.ndarray:
    return a if a.size else np.zeros(2, dtype)


def glob_match_host(names: NameTable, globs: GlobSet) -> np.ndarray:
    """The bitmap uint64 [P][ceil(M / 64)] by the CPU build of the matcher (bce_glob_match_host):
    no GPU.  Declined patterns are answered by fnmatch."""
    L = N.lib()
    M, P = names.n, globs.n
    bits = np.zeros((P, (M + 63) // 64), np.uint64)
    N.check(L.bce_glob_match_host(N.ptr(names.bytes_host), int(names.off_host[-1]), N.ptr(names.off_host), M,
                                  N.ptr(_np_or_dummy(globs.prog, np.uint32)), globs.prog.size,
                                  N.ptr(globs.prog_off), P, N.ptr(_np_or_dummy(globs.cls_rng, np.uint32)),
                                  globs.cls_rng.size // 2, N.ptr(globs.cls_off), globs.n_cls, N.ptr(bits)),
            "bce_glob_match_host")
    for r in globs.declined:
        bits[r] = _glob_host_row(names, globs.patterns[r])
    return bits


def glob_match(names: NameTable, globs: GlobSet, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Every pattern against every name in one launch (bce_glob_match): int64 [P][ceil(M / 64)]
    holding the 64-bit words, bit ``m % 64`` of word ``m // 64`` of row p set iff
    ``fnmatch.fnmatchcase(names[m], patterns[p])``.  Rows of declined patterns are computed by
    fnmatch on the host and uploaded."""
    L = N.require_gpu()
    if names.data is None:
        raise ValueError("glob_match needs a NameTable built with a device")
    dev = names.data.device
    M, P = names.n, globs.n
    nw = (M + 63) // 64
    bits = out if out is not None else torch.empty((P, nw), dtype=torch.int64, device=dev)
    assert bits.shape == (P, nw) and bits.dtype == torch.int64 and bits.is_contiguous()
    T = lambda a, dt: torch.from_numpy(_np_or_dummy(a, a.dtype).view(dt)).to(dev)  # noqa: E731
    prog, rng = T(globs.prog, np.int32), T(globs.cls_rng, np.int32)
    poff, coff = T(globs.prog_off, np.int64), T(globs.cls_off, np.int32)
    N.check(L.bce_glob_match(N.ptr(names.data), int(names.off_host[-1]), N.ptr(names.off), M, N.ptr(prog),
                             globs.prog.size, N.ptr(poff), P, N.ptr(rng), globs.cls_rng.size // 2, N.ptr(coff),
                             globs.n_cls, N.ptr(bits), N.stream(dev)), "bce_glob_match")
    for r in globs.declined:
        bits[r] = torch.from_numpy(_glob_host_row(names, globs.patterns[r]).view(np.int64)).to(dev)
    return bits


def glob_count(bits: torch.Tensor, n_names: int, rows: torch.Tensor) -> torch.Tensor:
    """Set bits of ``bits[rows[r]]`` per slot r (bce_glob_count): int64 [R]."""
    L = N.require_gpu()
    R = rows.numel()
    cnt = torch.empty(max(R, 1), dtype=torch.int64, device=bits.device)
    N.check(L.bce_glob_count(N.ptr(bits), n_names, bits.shape[0], N.ptr(rows), R, N.ptr(cnt),
                             N.stream(bits.device)), "bce_glob_count")
    return cnt[:R]


def glob_members(bits: torch.Tensor, n_names: int, rows: torch.Tensor, slot_groups) -> tuple:
    """Member lists for bce_aggregate_groups from the bitmap: slot r holds the set bit positions of
    row ``rows[r]`` ascending (store order), group g is the slots ``slot_groups[g] ..
    slot_groups[g+1]`` (int64 [G+1], host or device), so a group lists its patterns' matches in
    pattern order with duplicates kept (market.py:352-357).  Count, cumulative sum (torch; one
    host read sizes ``members``), fill.  Returns ``(group_offsets [G+1], members)``."""
    L = N.require_gpu()
    dev = bits.device
    R = rows.numel()
    cnt = glob_count(bits, n_names, rows)
    slot_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, out=slot_off[1:])
    total = int(slot_off[-1].item())
    members = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    N.check(L.bce_glob_fill(N.ptr(bits), n_names, bits.shape[0], N.ptr(rows), R, N.ptr(slot_off), total,
                            N.ptr(members), N.stream(dev)), "bce_glob_fill")
    sg = torch.as_tensor(slot_groups, dtype=torch.int64).to(dev)
    return slot_off[sg], members[:total]


def glob_any(bits: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """OR of the listed rows: one word row int64 [ceil(M / 64)] ("any of these patterns")."""
    sel = bits.index_select(0, rows)
    if sel.shape[0] == 0:
        return torch.zeros(bits.shape[1], dtype=torch.int64, device=bits.device)
    while sel.shape[0] > 1:
        h = sel.shape[0] // 2
        sel = torch.cat([sel[:h] | sel[h:2 * h], sel[2 * h:]])
    return sel[0]


def glob_mask(words: torch.Tensor, n_names: int) -> torch.Tensor:
    """A word row as bool [M]."""
    sh = torch.arange(64, dtype=torch.int64, device=words.device)
    return (((words.unsqueeze(1) >> sh) & 1) != 0).reshape(-1)[:n_names]
