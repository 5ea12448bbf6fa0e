#!/usr/bin/env python3
"""Generate decay_edges.json by running the REFERENCE Python (test infrastructure only).

    PYTHONPATH=<reference>/src python3 tests/golden/gen_decay_edges.py

The edges of the decay arithmetic that decay_cases.json leaves out: exponents in every path of
libm's pow(2.0, y) (|y| < 2^-65, table boundaries, the special-case threshold at ratio 738.65,
subnormal and vanishing factors), non-finite and out-of-range reliabilities, and stamps up to
the widest span two datetimes can have, where the elapsed microseconds no longer fit a double.

Every double is stored as its 64-bit pattern in hex (NaN, -0.0 and subnormals survive); the
stamps are integers (microseconds since 1970).  The fixture holds data only, by column (pack()
below; tests/decay_ref.py edges() reads it back).

  ratios  the elapsed/half-life ratios the `days` section is built from
  days    two blocks of columns r, e, h, m, factor, out: compute_decay_factor(e, h),
          apply_reliability_decay(r, e, h, m)
  stamps  columns r, t_us, now_us, h, m, days, out: days_since_update(t, now) and
          decay_reliability_if_needed(r, t, now, h, m)[0], t and now as aware datetimes
  stamps_single_rounding_rows
          the number of `stamps` rows whose `out` differs from what float(n) / 1e6 (convert,
          then divide: two roundings) would give; the generator stops below 50
"""
from __future__ import annotations

import json
import math
import os
import struct
from datetime import datetime, timedelta, timezone

import numpy as np

import bayesian_engine.decay as ref

HERE = os.path.dirname(os.path.abspath(__file__))
EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)
INF, NAN = math.inf, math.nan


def hx(x: float) -> str:
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def us(dt: datetime) -> int:
    d = dt - EPOCH
    return (d.days * 86400 + d.seconds) * 10**6 + d.microseconds


def at(t_us: int) -> datetime:
    return EPOCH + timedelta(microseconds=t_us)


# ---------------------------------------------------------------------------------------
# days: (r, e, h, m)
# ---------------------------------------------------------------------------------------
HS = [1e-3, 1.0, 30.0, 1e5, 1e300, INF]
MS = [0.0, 0.1, 0.3, 1.0, 1.2]
RS = [0.0, -0.0, 5e-324, 0.1, 0.5, 1.0, 1.5, -0.3, 1e308, INF, NAN]


def ratios() -> list:
    out = [5e-324, 1e-300, 2.0**-66, 2.0**-65, 2.0**-64, 2.0**-54, 2.0**-53, 1.0, 2.0, 3.0]
    for k in (1, 63, 128, 129, 5000):  # exp table boundaries: exponent = -k/128
        x = k / 128
        out += [math.nextafter(x, 0.0), x, math.nextafter(x, INF)]
    out += [738.0, 738.6, 738.7, 739.0]  # |y ln2| = 512 at 738.65: libm's special-case path
    out += [1021.9999, 1022.0, 1022.5, 1050.3, 1073.0, 1074.0, 1074.5, 1075.0, 1076.0]  # subnormal factors
    out += [1e4, 1e300, INF]
    return out


def gen_days(rng) -> list:
    rows = []
    for ih, h in enumerate(HS):
        es = [q * h for q in ratios()] + [0.0, -0.0, -1.0, NAN, INF]
        for ie, e in enumerate(es):
            for ir, r in enumerate(RS):
                rows.append((r, e, h, MS[(ih + ie + ir) % len(MS)]))
    finite_h = [1e-3, 1.0, 30.0, 1e5]
    for i in range(2000):
        q = 2.0 ** rng.uniform(-70.0, 11.0)
        h = finite_h[i % 4]
        r = float(rng.uniform(0.0, 1.5)) if i % 8 else RS[(i // 8) % len(RS)]
        rows.append((r, q * h, h, MS[(i // 4) % len(MS)]))
    out = []
    for r, e, h, m in rows:
        f = ref.compute_decay_factor(e, h)
        d = ref.apply_reliability_decay(r, e, h, m)
        out.append([hx(r), hx(e), hx(h), hx(m), hx(f), hx(d)])
    return out


# ---------------------------------------------------------------------------------------
# stamps: (r, t_us, now_us, h, m)
# ---------------------------------------------------------------------------------------
NOW_A = us(datetime(2026, 3, 1, 12, 0, 0, 250000, tzinfo=timezone.utc))
NOW_Z = us(datetime(9999, 12, 31, 23, 59, 59, 999999, tzinfo=timezone.utc))
YEAR1 = us(datetime(1, 1, 1, tzinfo=timezone.utc))
WIDEST = NOW_Z - YEAR1
assert WIDEST == 315537897599999999
RM = [(1.0, 0.0), (0.8, 0.1)]
# half-lives for the old stamps: days / h must fall in [2, 50] so that the last bit of `days`
# reaches the factor (a few values only: every (now, h, m) is a launch)
OLD_HS = [100000.0 / 3.0, 52000.0, 73000.0, 100000.0]
NEAR_HS = [30.0, 1000.0]


def old_hs(n_us: int) -> list:
    days = n_us / 10**6 / 86400.0
    return [h for h in OLD_HS if 2.0 <= days / h <= 50.0]


def two_roundings(r, n_us, h, m):
    """What convert-then-divide arithmetic gives: float(n) rounds, / 1e6 rounds again."""
    e = max(0.0, float(n_us) / 1e6 / 86400.0)
    return r if e <= 0 else ref.apply_reliability_decay(r, e, h, m)


def gen_stamps(rng):
    cases = []  # (t_us, now_us, [h...])
    for now in (NOW_A, NOW_Z):
        for t in (now, now - 1, now - 10**6):
            cases.append((t, now, NEAR_HS))
    cases.append((NOW_A + 1, NOW_A, NEAR_HS))                     # 1 us in the future
    cases.append((NOW_A + 3 * 86400 * 10**6, NOW_A, NEAR_HS))     # three days in the future
    cases.append((0, NOW_A, NEAR_HS))                             # the epoch
    cases.append((us(datetime(1900, 1, 1, tzinfo=timezone.utc)), NOW_A, NEAR_HS))
    cases.append((us(datetime(1969, 12, 31, 23, 59, 59, 999999, tzinfo=timezone.utc)), NOW_A, NEAR_HS))
    cases.append((YEAR1, NOW_A, old_hs(NOW_A - YEAR1)))           # 0001-01-01 seen from today
    cases.append((YEAR1, NOW_Z, old_hs(WIDEST)))                  # the widest span
    cases.append((NOW_Z, YEAR1, NEAR_HS))                         # ... and backwards: 0 days
    for now in (NOW_A, NOW_Z):
        for n in (2**53 - 1, 2**53, 2**53 + 1):
            cases.append((now - n, now, old_hs(n)))
    for i in range(500):
        now = NOW_Z if i % 10 < 7 else NOW_A
        n = int(rng.integers(2**53, now - YEAR1, endpoint=True))
        hs = old_hs(n)
        cases.append((now - n, now, [hs[i % len(hs)]]))
    rows, differs = [], 0
    for t, now, hs in cases:
        assert hs, (t, now)
        for h in hs:
            for r, m in RM:
                days = ref.days_since_update(at(t), now=at(now))
                out, _ = ref.decay_reliability_if_needed(r, at(t), now=at(now), half_life_days=h,
                                                         min_reliability=m)
                differs += hx(out) != hx(two_roundings(r, now - t, h, m))
                rows.append([hx(r), t, now, hx(h), hx(m), hx(days), hx(out)])
    return rows, differs


B36 = "0123456789abcdefghijklmnopqrstuvwxyz"


def pack(col: list):
    """One column, the smaller of: as it is (doubles: the 16-digit patterns joined into one
    string; stamps: a list of integers), or its distinct values in first-seen order plus one
    base-36 index of `width` digits per row."""
    plain = "".join(col) if isinstance(col[0], str) else col
    uniq = list(dict.fromkeys(col))
    if len(uniq) > 36 * 36:
        return plain
    w = 1 if len(uniq) <= 36 else 2
    at = {v: k for k, v in enumerate(uniq)}
    coded = {"values": uniq, "width": w,
             "index": "".join(B36[at[v] // 36] * (w - 1) + B36[at[v] % 36] for v in col)}
    return coded if len(json.dumps(coded)) < len(json.dumps(plain)) else plain


def main() -> None:
    repo = os.path.dirname(os.path.dirname(HERE))
    assert not os.path.abspath(ref.__file__).startswith(repo), "must import the reference, not the build"
    days = gen_days(np.random.default_rng(53))
    stamps, differs = gen_stamps(np.random.default_rng(54))
    # the fixture must see the single rounding of n / 10**6: stop if it does not
    assert differs >= 50, f"only {differs} stamps rows tell n / 10**6 from float(n) / 1e6"
    pairs = {(r[2], r[3]) for r in days}
    groups = {(r[2], r[3], r[4]) for r in stamps}
    assert len(pairs) <= 40 and len(groups) <= 40, (len(pairs), len(groups))
    doc = {"ratios": pack([hx(q) for q in ratios()]),
           # two blocks, the grid and the 2000 random rows: the grid's few distinct values code well
           "days": [{k: pack(list(c)) for k, c in zip(("r", "e", "h", "m", "factor", "out"), zip(*rows))}
                    for rows in (days[:-2000], days[-2000:])],
           "stamps": {k: pack(list(c)) for k, c in zip(("r", "t_us", "now_us", "h", "m", "days", "out"),
                                                       zip(*stamps))},
           "stamps_single_rounding_rows": differs}
    path = os.path.join(HERE, "decay_edges.json")
    with open(path, "w", encoding="utf-8") as f:
        one = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
        block = lambda b: "{\n" + ",\n".join(f'  "{k}":{one(c)}' for k, c in b.items()) + "}"  # noqa: E731
        f.write('{"ratios":' + one(doc["ratios"]) + ',\n "days":[' + ",\n ".join(map(block, doc["days"]))
                + '],\n "stamps":' + block(doc["stamps"]) + f',\n "stamps_single_rounding_rows":{differs}}}\n')
    print(f"{path}: {len(days)} days rows ({len(pairs)} (h, m) pairs), {len(stamps)} stamps rows "
          f"({len(groups)} (now, h, m) groups, {differs} single-rounding rows), {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
