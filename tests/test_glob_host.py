"""The glob matcher and the Python pattern compiler on the CPU (bce_glob_match_host: the same
csrc/glob_match.hpp the kernel includes, compiled for the host), bit for bit against fnmatch."""
import warnings

import numpy as np
import pytest

import glob_ref
from bayesian_engine import _native as N
from bayesian_engine import batch

CASES = [(s, M, P) for s in range(5) for (M, P) in ((65, 65), (129, 40), (1000, 65))]


def _host_bits(names, pats):
    nt = batch.NameTable.from_strings(names)
    gs = batch.GlobSet.compile(pats)
    bits = batch.glob_match_host(nt, gs)
    return gs, bits[gs.index]  # one row per pattern given


@pytest.mark.parametrize("seed,M,P", CASES)
def test_random_cases_match_fnmatch(seed, M, P):
    names, pats = glob_ref.random_case(seed, M, P)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)  # re's "possible nested set" on '[['
        glob_ref.check_balanced(glob_ref.oracle(names, pats))
        exp = glob_ref.oracle_bits(names, pats)
    gs, got = _host_bits(names, pats)
    assert not gs.declined
    assert np.array_equal(got, exp)


def test_edge_patterns_match_fnmatch():
    names, pats = glob_ref.edge_names(), glob_ref.EDGE_PATTERNS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        exp = glob_ref.oracle_bits(names, pats)
    gs, got = _host_bits(names, pats)
    assert not gs.declined
    assert gs.n == len(set(pats)) < len(pats)  # duplicates share a row
    bad = [(pats[p], names[m]) for p in range(len(pats)) for m in range(len(names))
           if ((got[p, m // 64] >> np.uint64(m % 64)) & np.uint64(1)) != ((exp[p, m // 64] >> np.uint64(m % 64)) & np.uint64(1))]
    assert not bad, bad[:10]
    assert np.array_equal(got, exp)  # the padding bits too


def test_declined_patterns_are_answered_by_fnmatch():
    names = glob_ref.edge_names()
    long_ops = "a" * (batch.GLOB_MAX_OPS + 1)
    at_cap = "a" * (batch.GLOB_MAX_OPS - 1) + "*"
    wide = "[" + "".join(chr(0x100 + 2 * i) for i in range(batch.GLOB_MAX_RANGES + 1)) + "]*"
    pats = ["a*", long_ops, long_ops + "*", at_cap, wide, "*a"]
    names = names + [long_ops, "a" * batch.GLOB_MAX_OPS, chr(0x100) + "x", chr(0x101)]
    gs, got = _host_bits(names, pats)
    assert [gs.patterns[r] for r in gs.declined] == [long_ops, long_ops + "*", wide]
    assert np.array_equal(got, glob_ref.oracle_bits(names, pats))


def test_program_layout():
    gs = batch.GlobSet.compile(["a?*[!b-c]", "**", "[x]", "[x]"])
    assert gs.index == [0, 1, 2, 2] and gs.prog_off.tolist() == [0, 4, 5, 6]
    assert gs.prog.tolist() == [ord("a"), 1 << 29, 2 << 29, (3 << 29) | (1 << 28) | 0, 2 << 29, (3 << 29) | 1]
    assert gs.cls_off.tolist() == [0, 1, 2] and gs.cls_rng.tolist() == [ord("b"), ord("c"), ord("x"), ord("x")]


def test_argument_errors():
    L = N.load_library()
    nt = batch.NameTable.from_strings(["ab", "c"])
    gs = batch.GlobSet.compile(["a*", "[c]"])
    bits = np.zeros((2, 1), np.uint64)

    def call(**kw):
        a = dict(nb=N.ptr(nt.bytes_host), n_bytes=3, noff=N.ptr(nt.off_host), M=2, prog=N.ptr(gs.prog), n_ops=3,
                 poff=N.ptr(gs.prog_off), P=2, rng=N.ptr(gs.cls_rng), n_rng=1, coff=N.ptr(gs.cls_off), n_cls=1,
                 bits=N.ptr(bits))
        a.update(kw)
        return L.bce_glob_match_host(*a.values())

    assert call() == 0 and bits[:, 0].tolist() == [1, 2]
    for kw in (dict(noff=None), dict(poff=None), dict(bits=None), dict(nb=None), dict(prog=None), dict(rng=None),
               dict(coff=None), dict(M=-1), dict(P=-1), dict(n_bytes=-1), dict(n_ops=-1), dict(n_rng=-1),
               dict(n_cls=-1),
               dict(n_bytes=2),   # the last name leaves the bytes
               dict(n_ops=2),     # the last program leaves the ops
               dict(n_cls=0),     # a class index outside its table
               dict(n_rng=0)):    # a class row outside the range table
        assert call(**kw) == -1, kw
        assert L.bce_last_error()
    off = np.array([0, 2, 1], np.int64)  # decreasing
    assert call(noff=N.ptr(off)) == -1
    assert call(poff=N.ptr(off)) == -1
    bad_kind = np.array([7 << 29, 0, 0], np.uint32)
    assert call(prog=N.ptr(bad_kind)) == -1
    # the device entry points check their arguments before touching a GPU
    assert L.bce_glob_match(None, 3, None, 2, None, 3, None, 2, None, 1, None, 1, None, None) == -1
    assert L.bce_glob_match(None, 3, None, -2, None, 3, None, 2, None, 1, None, 1, None, None) == -1
    assert L.bce_glob_count(None, 5, 1, None, 3, None, None) == -1
    assert L.bce_glob_count(None, 5, 1, None, -3, None, None) == -1
    assert L.bce_glob_fill(None, 5, 1, None, 3, None, 0, None, None) == -1
    assert L.bce_glob_fill(None, 5, 1, None, 3, None, -1, None, None) == -1
