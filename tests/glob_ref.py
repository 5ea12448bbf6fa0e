"""Helper for the glob tests (not a test): the case generator, the edge lists and the oracle,
which is ``fnmatch.fnmatchcase`` of the running interpreter."""
import fnmatch
import random

import numpy as np

ALPHABET = ["a", "b", ":", "-", "é", "€", "\U0001F600"]  # 1, 1, 1, 1, 2, 3, 4 bytes
PATTERN_EXTRA = ["*", "?", "[", "]", "!", "\\", "^"]

EDGE_PATTERNS = ["", "*", "**", "?", "[", "[]", "[!]", "[]]", "[!]]", "[a-]", "[-a]", "[z-a]", "[a-b-c]", "[\\]",
                 "[^a]", "[[a]", "a[", "*a*a*a", "?*?", "*€", "[é-€]", "\ud800", "*\ud800*", "[\ud800]",
                 # more of translate()'s bracket branches
                 "[!z-a]", "[!a-b]x", "[--a]", "[a&&b]", "[~|]", "[!^]", "[!!]", "[a-b-]", "[]-a]", "[ab-cz-ef]",
                 "a*", "*:*-*", "a?b", "[!]a", "[]", "*[ab]", "[a-b:]*[!a-b]"]


def edge_names():
    """The empty name, a newline, every member the edge patterns ask about, and names of 63, 64,
    65 and 300 bytes (one byte past the kernel's LDS slot, and far past it)."""
    names = ["", "\n", "a\nb", "a", "b", "c", "z", "-", "]", "[", "!", "\\", "^", "&", "~", "|", "a[", "[a", "[]",
             "aa", "aaa", "abaca", "baaa", "ab", "é", "€", "\U0001F600", "x€", "€x", "\ud800",
             "a\ud800b", "ā", "a:b-c", "ax", "cx", ":-", "a-", "d", "e", "f"]
    for n in (63, 64, 65, 300):
        names.append("a" * n)
        names.append("a" * (n - 3) + "€")           # ends in a 3-byte code point
        names.append("b" + "a" * (n - 2) + "b")
        names.append("é" * (n // 2) + "a" * (n % 2))
    return names


def random_case(seed: int, M: int, P: int):
    """(names, patterns) as the issue specifies them."""
    rng = random.Random(seed)
    names = ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(1, 12))) for _ in range(M)]
    pats = []
    for p in range(P):
        if p % 2 == 0:
            name = rng.choice(names)
            out = []
            i = 0
            while i < len(name):
                r = rng.random()
                c = name[i]
                if r < 0.15:
                    span = rng.randint(0, len(name) - i)  # the span may be empty, or the whole rest
                    out.append("*")
                    i += span
                    if span == 0:
                        out.append(c)
                        i += 1
                elif r < 0.30:
                    out.append("?")
                    i += 1
                elif r < 0.45:
                    out.append(rng.choice([f"[{c}x]", f"[!{c}]", "[a-b:]", "[!a-b]", f"[]{c}-]", f"[b-a{c}]"]))
                    i += 1
                else:
                    out.append(c)
                    i += 1
            if rng.random() < 0.2:
                out.append("*")
            pats.append("".join(out))
        else:
            pats.append("".join(rng.choice(ALPHABET + PATTERN_EXTRA) for _ in range(rng.randint(0, 8))))
    return names, pats


def oracle(names, pats):
    return [[fnmatch.fnmatchcase(n, p) for n in names] for p in pats]


def check_balanced(table):
    """Neither an all-false nor an all-true matcher passes a case of >= 40 patterns."""
    P = len(table)
    hit = sum(any(r) for r in table) / P
    miss = sum(not all(r) for r in table) / P
    rate = sum(map(sum, table)) / (P * len(table[0]))
    assert hit >= 0.3 and miss >= 0.3 and rate >= 0.01, (hit, miss, rate)


def oracle_bits(names, pats):
    """The oracle packed like the kernel's output: uint64 [P][ceil(M / 64)]."""
    M = len(names)
    out = np.zeros((len(pats), ((M + 63) // 64) * 64), np.uint8)
    for p, row in enumerate(oracle(names, pats)):
        out[p, :M] = row
    return np.packbits(out, axis=1, bitorder="little").view(np.uint64).reshape(len(pats), (M + 63) // 64)


def expand(bits_row, M):
    """Set bit positions of one uint64 row, ascending."""
    b = np.unpackbits(np.ascontiguousarray(bits_row).view(np.uint8), bitorder="little")[:M]
    return np.nonzero(b)[0].astype(np.int64)
