"""The decay edges on the CPU: the plain reference (tests/decay_ref.py), the oracle and the
package's host-side days against tests/golden/decay_edges.json, bit for bit.  No GPU needed."""
from datetime import datetime, timedelta, timezone

import numpy as np

import decay_ref as dr
from oracle import oracle as orc

EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)


def test_fixture_covers_what_it_claims():
    ed = dr.edges()
    d, s = ed.days, ed.stamps
    assert len(dr.groups(d.h, d.m)) <= 40 and len(dr.groups(s.now_us, s.h, s.m)) <= 40
    n = s.now_us.astype(object) - s.t_us.astype(object)
    assert sum(int(x) >= 2**53 for x in n) >= 500 and max(n) == 315537897599999999
    assert {2**53 - 1, 2**53, 2**53 + 1} <= set(n) and any(x < 0 for x in n) and any(x == 0 for x in n)
    assert ed.single_rounding_rows >= 50
    q = ed.ratios
    assert q.min() == 5e-324 and np.isinf(q.max()) and (np.abs(q - 738.65) < 0.1).sum() == 2
    assert ((q > 1022) & (q < 1075)).sum() >= 5 and (q < 2.0**-65).sum() >= 3
    # factors whose bits min_rel = 0.1 would hide are observed with min_rel = 0
    tiny = (d.factor > 0) & (d.factor < 2.0**-53)
    assert (tiny & (d.m == 0) & (d.r == 1.0)).any()


def test_decay_ref_matches_fixture():
    ed = dr.edges()
    d, s = ed.days, ed.stamps
    dr.assert_bits([dr.factor(e, h) for e, h in zip(d.e.tolist(), d.h.tolist())], d.factor, "factor")
    dr.assert_bits([dr.apply(*a) for a in zip(d.r.tolist(), d.e.tolist(), d.h.tolist(), d.m.tolist())],
                   d.out, "apply")
    dr.assert_bits([dr.days(t, now) for t, now in zip(s.t_us.tolist(), s.now_us.tolist())], s.days, "days")
    dr.assert_bits([dr.view(*a) for a in zip(s.r.tolist(), s.t_us.tolist(), s.now_us.tolist(), s.h.tolist(),
                                             s.m.tolist())], s.out, "view")


def test_fixture_sees_the_double_rounding():
    """float(n) / 1e6 (convert, then divide) is not n / 10**6 from 2**53 us on: the fixture must
    tell them apart in the decayed value itself, or the stamp tests prove nothing."""
    s = dr.edges().stamps
    two = [dr.apply(r, max(0.0, float(now - t) / 1e6 / 86400.0), h, m)
           for r, t, now, h, m in zip(s.r.tolist(), s.t_us.tolist(), s.now_us.tolist(), s.h.tolist(), s.m.tolist())]
    differ = int((dr.bits(two) != dr.bits(s.out)).sum())
    assert differ == dr.edges().single_rounding_rows and differ >= 50


def test_oracle_scalars_match_fixture():
    ed = dr.edges()
    d, s = ed.days, ed.stamps
    dr.assert_bits([orc.decay_factor(e, h) for e, h in zip(d.e.tolist(), d.h.tolist())], d.factor, "orc_decay_factor")
    dr.assert_bits([orc.apply_decay(*a) for a in zip(d.r.tolist(), d.e.tolist(), d.h.tolist(), d.m.tolist())],
                   d.out, "orc_apply_decay")
    dr.assert_bits([orc.days_since(now, t) for t, now in zip(s.t_us.tolist(), s.now_us.tolist())], s.days,
                   "orc_days_since")


def test_oracle_decay_view_matches_fixture():
    s = dr.edges().stamps
    for (now, h, m), idx in dr.groups(s.now_us, s.h, s.m):
        present = np.ones(len(idx), np.uint8)
        present[::5] = 0
        got = orc.decay_view(s.r[idx], s.t_us[idx], present, now, h, m, default_rel=0.5)
        dr.assert_bits(got, np.where(present != 0, s.out[idx], 0.5), f"orc_decay_view now={now} h={h} m={m}")


def test_oracle_namespace_lookup_matches_fixture():
    s = dr.edges().stamps
    for (now, h, m), idx in dr.groups(s.now_us, s.h, s.m):
        scopes = dr.poisoned_scopes(s.r[idx], s.t_us[idx])
        rel, conf, scope = orc.namespace_resolve(scopes, True, now, h, m)
        dr.assert_bits(rel, s.out[idx], f"orc_namespace_resolve now={now} h={h} m={m}")
        assert np.array_equal(scope, np.arange(len(idx)) % 3)
        for q in range(3):
            dr.assert_bits(conf[scope == q], scopes[q][1][scope == q], "conf")


def test_package_days_since_update_matches_fixture():
    from bayesian_engine.decay import days_since_update
    from bayesian_engine.timeutil import dt_to_us
    s = dr.edges().stamps
    at = lambda u: EPOCH + timedelta(microseconds=u)  # noqa: E731
    got = []
    for t, now in zip(s.t_us.tolist(), s.now_us.tolist()):
        assert dt_to_us(at(t)) == t
        got.append(days_since_update(at(t), now=at(now)))
    dr.assert_bits(got, s.days, "days_since_update")
