"""GPU checks of the decay arithmetic at its edges: every kernel that decays a stored reliability
(decay_apply, decay_view, replay_step, namespace_resolve, pair_resolve, scope_resolve, walk_read,
walk_scope_read) against tests/golden/decay_edges.json, the reference's own results for exponents
in every path of libm's pow(2.0, y), non-finite reliabilities and stamps up to the widest span two
datetimes can have.  Every comparison is on the 64-bit patterns.  The odd lengths run the tail
branches of decay_view_kernel and replay_step_kernel."""
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest
import torch

import decay_ref as dr
from bayesian_engine import _native as N
from bayesian_engine import batch
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 255, 256, 257, 511, 512, 513, 1025]
ODD = [1, 3, 5, 7, 513]
NOTS = int(orc.NO_TIMESTAMP)
EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)


def _dev():
    return torch.device("cuda", 0)


def _T(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev())


def _np(t):
    return t.cpu().numpy()


def _stamp_groups():
    s = dr.edges().stamps
    return s, dr.groups(s.now_us, s.h, s.m)


def _hm_groups():
    """The stamps rows by (h, m), each sorted by `now` (a walk's markets are chronological)."""
    s = dr.edges().stamps
    return s, [((h, m), idx[np.argsort(s.now_us[idx], kind="stable")]) for (h, m), idx in dr.groups(s.h, s.m)]


def _cycle(idx, n):
    return idx[(np.arange(n) + n) % len(idx)]


# ---------------------------------------------------------------------------------------
# elapsed days in: decay_apply
# ---------------------------------------------------------------------------------------
def test_decay_apply_factor_and_out_alone_and_together():
    d = dr.edges().days
    groups = dr.groups(d.h, d.m)
    assert len(groups) <= 40
    for (h, m), idx in groups:
        r, e = _T(d.r[idx]), _T(d.e[idx])
        what = f"h={h!r} m={m!r}"
        out, fac = batch.decay_apply(r, e, h, m, want_factor=True)
        dr.assert_bits(_np(fac), d.factor[idx], f"factor (with out) {what}")
        dr.assert_bits(_np(out), d.out[idx], f"out (with factor) {what}")
        out, fac = batch.decay_apply(r, e, h, m, want_factor=False)
        assert fac is None
        dr.assert_bits(_np(out), d.out[idx], f"out alone {what}")
        out, fac = batch.decay_apply(None, e, h, m, want_factor=True)
        assert out is None
        dr.assert_bits(_np(fac), d.factor[idx], f"factor alone {what}")


# ---------------------------------------------------------------------------------------
# stamps in: decay_view, replay_step, outcome_update
# ---------------------------------------------------------------------------------------
def test_decay_view_every_length_with_and_without_present():
    s, groups = _stamp_groups()
    rng = np.random.default_rng(3)
    for (now, h, m), idx in groups:
        rows = _cycle(idx, max(LENGTHS))  # every row of the group, then around again
        r, t = _T(s.r[rows]), _T(s.t_us[rows])
        for n in LENGTHS:
            what = f"now={now} h={h!r} m={m!r} n={n}"
            got = batch.decay_view(r[:n], t[:n], now, None, h, m, default_rel=0.5)
            dr.assert_bits(_np(got), s.out[rows[:n]], f"present=None {what}")
            present = (rng.random(n) < 0.8).astype(np.uint8)
            if n & 1:
                present[-1] = 0  # the tail branch reads its own present byte
            got = batch.decay_view(r[:n], t[:n], now, _T(present), h, m, default_rel=0.625)
            dr.assert_bits(_np(got), np.where(present != 0, s.out[rows[:n]], 0.625), f"present mask {what}")


def test_replay_step_decay_only_leaves_the_table_alone():
    s, groups = _stamp_groups()
    rng = np.random.default_rng(4)
    for (now, h, m), idx in groups:
        rows = _cycle(idx, max(LENGTHS))
        conf = rng.random(len(rows))
        present = (rng.random(len(rows)) < 0.5).astype(np.uint8)
        for n in LENGTHS:
            tab = [_T(s.r[rows[:n]]), _T(conf[:n]), _T(s.t_us[rows[:n]]), _T(present[:n])]
            view = torch.full((n,), -7.0, dtype=torch.float64, device=_dev())
            flags2 = torch.zeros((n + 3) // 4, dtype=torch.uint8, device=_dev())
            batch.replay_step(*tab, flags2, now, view, h, m)
            what = f"now={now} h={h!r} m={m!r} n={n}"
            dr.assert_bits(_np(view), s.out[rows[:n]], f"view {what}")
            dr.assert_bits(_np(tab[0]), s.r[rows[:n]], f"rel {what}")
            dr.assert_bits(_np(tab[1]), conf[:n], f"conf {what}")
            assert np.array_equal(_np(tab[2]), s.t_us[rows[:n]]), what
            assert np.array_equal(_np(tab[3]), present[:n]), what


def _absent_baked(r, conf, t, present):
    """Absent rows as the store bakes them (reliability.py:133-140)."""
    r, conf, t = r.copy(), conf.copy(), t.copy()
    r[present == 0], conf[present == 0], t[present == 0] = 0.5, 0.25, NOTS
    return r, conf, t


@pytest.mark.parametrize("n", ODD)
def test_replay_step_with_updates_at_odd_lengths(n):
    s, groups = _stamp_groups()
    rng = np.random.default_rng(5 + n)
    for (now, h, m), idx in groups:
        rows = _cycle(idx, n)
        present = (rng.random(n) < 0.7).astype(np.uint8)
        r, conf, t = _absent_baked(s.r[rows], rng.random(n), s.t_us[rows], present)
        part, correct = rng.random(n) < 0.6, rng.random(n) < 0.5
        part[-1] = True  # the tail source participates: its flag bits are read and acted on
        flags = part.astype(np.uint8) | (correct.astype(np.uint8) << 1)
        exp_view = orc.decay_view(r, t, np.ones(n, np.uint8), now, h, m)
        exp = orc.outcome_update(r, conf, t, present, flags, now)
        tab = [_T(r), _T(conf), _T(t), _T(present)]
        view = torch.full((n,), -7.0, dtype=torch.float64, device=_dev())
        batch.replay_step(*tab, _T(batch.pack_flags2(part, correct)), now, view, h, m)
        what = f"now={now} h={h!r} m={m!r} n={n}"
        live = present != 0
        dr.assert_bits(exp_view[live], s.out[rows][live], f"oracle view {what}")
        dr.assert_bits(_np(view), exp_view, f"view {what}")
        dr.assert_bits(_np(tab[0]), exp[0], f"rel {what}")
        dr.assert_bits(_np(tab[1]), exp[1], f"conf {what}")
        assert np.array_equal(_np(tab[2]), exp[2]) and np.array_equal(_np(tab[3]), exp[3]), what


@pytest.mark.parametrize("with_present", [True, False])
@pytest.mark.parametrize("n", ODD)
def test_outcome_update_at_odd_lengths(n, with_present):
    s = dr.edges().stamps
    rng = np.random.default_rng(50 + n)
    rows = rng.integers(0, len(s.r), n)
    present = (rng.random(n) < 0.7).astype(np.uint8) if with_present else np.ones(n, np.uint8)
    r, conf, t = s.r[rows].copy(), rng.random(n), s.t_us[rows].copy()
    part, correct = rng.random(n) < 0.6, rng.random(n) < 0.5
    part[-1] = True
    flags = part.astype(np.uint8) | (correct.astype(np.uint8) << 1)
    now = int(s.now_us[rows[0]])
    exp = orc.outcome_update(r, conf, t, present, flags, now)
    tab = [_T(r), _T(conf), _T(t), _T(present)]
    batch.outcome_update(tab[0], tab[1], tab[2], tab[3] if with_present else None, _T(flags), now)
    dr.assert_bits(_np(tab[0]), exp[0], "rel")
    dr.assert_bits(_np(tab[1]), exp[1], "conf")
    assert np.array_equal(_np(tab[2]), exp[2])
    assert np.array_equal(_np(tab[3]), exp[3] if with_present else present)


# ---------------------------------------------------------------------------------------
# the lookups: the stored row decays the same way whichever scope it is found in
# ---------------------------------------------------------------------------------------
def _scope(sc):
    return batch.ScopeTable(*(_T(a) for a in sc))


def _check_entries(table, scope, exp_rel, exp_conf, exp_scope, what):
    Q = len(exp_rel)
    rc = _np(table.relconf)[:Q]
    dr.assert_bits(rc[:, 0], exp_rel, f"reliability {what}")
    dr.assert_bits(rc[:, 1], exp_conf, f"confidence {what}")
    assert np.array_equal(_np(scope), exp_scope), what


def test_namespace_resolve_each_scope_wins_over_poison():
    s, groups = _stamp_groups()
    for (now, h, m), idx in groups:
        scopes = dr.poisoned_scopes(s.r[idx], s.t_us[idx])
        win = np.arange(len(idx)) % 3
        conf = np.choose(win, [sc[1] for sc in scopes])
        table, scope = batch.namespace_resolve([_scope(sc) for sc in scopes], now, apply_decay=True,
                                               half_life_days=h, min_rel=m)
        _check_entries(table, scope, s.out[idx], conf, win, f"now={now} h={h!r} m={m!r}")


def _pair_rows(sc, market, sid, M, S):
    rel, conf, t, has = sc
    return batch.PairTable.from_rows(_T(market, np.int64), _T(sid, np.int32), _T(rel), _T(conf), _T(t), _T(has), M, S)


def test_pair_resolve_store_and_namespaced():
    """One query per stored row: source i in market i % 3.  Store mode reads the pair row;
    namespaced mode falls through poisoned has = 0 rows to the domain and the global scope."""
    s, groups = _stamp_groups()
    M = 3
    for (now, h, m), idx in groups:
        n = len(idx)
        sid, market = np.arange(n), np.arange(n) % M
        order = np.argsort(market * n + sid, kind="stable")  # the table's and the queries' order
        what = f"now={now} h={h!r} m={m!r}"
        conf = 0.25 + 0.5 * np.random.default_rng(6).random(n)
        pt = _pair_rows((s.r[idx], conf, s.t_us[idx], np.ones(n, np.uint8)), market, sid, M, n)
        got = batch.pair_resolve(pt.poffsets, pt.psid, pt, now, mode="store", half_life_days=h, min_rel=m)
        assert bool(got.matched.all())
        _check_entries(got.table, got.scope, s.out[idx][order], conf[order], np.zeros(n), f"store {what}")
        win = (sid // M) % 3
        scopes = dr.poisoned_scopes(s.r[idx], s.t_us[idx], win)
        pt = _pair_rows(scopes[0], market, sid, M, n)
        got = batch.pair_resolve(pt.poffsets, pt.psid, pt, now, mode="namespaced", domain=_scope(scopes[1]),
                                 global_scope=_scope(scopes[2]), half_life_days=h, min_rel=m)
        exp_conf = np.choose(win, [sc[1] for sc in scopes])
        _check_entries(got.table, got.scope, s.out[idx][order], exp_conf[order], win[order], f"namespaced {what}")
    N.check_faults(_dev(), "pair_resolve")


def test_scope_resolve_market_domain_and_global_rows():
    """Source i in market i % 3; markets 0 and 2 belong to domain 1, market 1 to domain 0."""
    s, groups = _stamp_groups()
    M, D = 3, 2
    md = np.array([1, 0, 1], np.int32)
    for (now, h, m), idx in groups:
        n = len(idx)
        sid, market = np.arange(n), np.arange(n) % M
        order = np.argsort(market * n + sid, kind="stable")
        win = (sid // M) % 3
        scopes = dr.poisoned_scopes(s.r[idx], s.t_us[idx], win)
        pt = _pair_rows(scopes[0], market, sid, M, n)
        dt = _pair_rows(scopes[1], md[market], sid, D, n)
        lb, matched, dlb, dmatched, table, scope = batch.scope_resolve(
            pt.poffsets, pt.psid, pt, dt, _T(md), now, global_scope=_scope(scopes[2]), half_life_days=h, min_rel=m)
        assert bool(matched.all()) and bool(dmatched.all())
        exp_conf = np.choose(win, [sc[1] for sc in scopes])
        _check_entries(table, scope, s.out[idx][order], exp_conf[order], win[order], f"now={now} h={h!r} m={m!r}")
    N.check_faults(_dev(), "scope_resolve")


# ---------------------------------------------------------------------------------------
# the walks: one single-signal market per case, nothing resolved, the market's time is `now`
# ---------------------------------------------------------------------------------------
def test_walk_trace_reads_every_case_at_its_own_time():
    s, groups = _hm_groups()
    for (h, m), idx in groups:
        n = len(idx)
        assert bool((np.diff(s.now_us[idx]) >= 0).all())
        conf = 0.25 + 0.5 * np.random.default_rng(8).random(n)
        plan = batch.WalkPlan.build(_T(np.arange(n + 1, dtype=np.int64)), _T(np.arange(n, dtype=np.int32)),
                                    _T(np.full(n, 0.5)), _T(np.full(n, -1, np.int8)), n)
        assert plan.settle.n_touched == 0 and plan.pairs.n_entries == n
        table = batch.ReliabilityTable(_T(s.r[idx]), _T(conf), _T(s.t_us[idx]), _T(np.ones(n, np.uint8)), [""] * n)
        wt, exists = batch.walk_trace(plan, table, _T(s.now_us[idx]), half_life_days=h, min_rel=m)
        _check_entries(wt, exists, s.out[idx], conf, np.ones(n), f"h={h!r} m={m!r}")
    N.check_faults(_dev(), "walk_trace")


def test_walk_scope_trace_reads_the_domain_row_and_the_global_row():
    """Case i is market i with the single source i.  i % 3 == 0: the row lives in the market's
    domain; 1: the market has no domain, the row is global; 2: the domain row is poison with
    has = 0 and the global row is read."""
    s, groups = _hm_groups()
    D = 2
    for (h, m), idx in groups:
        n = len(idx)
        i = np.arange(n)
        kind = i % 3
        md = np.where(kind == 1, -1, i % D).astype(np.int32)
        win = np.where(kind == 0, 1, 2)  # NS_DOMAIN / NS_GLOBAL
        _, dom, glo = dr.poisoned_scopes(s.r[idx], s.t_us[idx], win)
        rows = kind != 1
        dt = _pair_rows(tuple(a[rows] for a in dom), md[rows], i[rows], D, n)
        gt = batch.ReliabilityTable(_T(glo[0]), _T(glo[1]), _T(glo[2]), _T(np.ones(n, np.uint8)), [""] * n)
        plan = batch.WalkScopePlan.build(_T(np.arange(n + 1, dtype=np.int64)), _T(i, np.int32), _T(np.full(n, 0.5)),
                                         _T(np.full(n, -1, np.int8)), _T(md), n, D)
        assert plan.dsettle.n_touched == 0 and plan.gsettle.n_touched == 0
        wt, scope = batch.walk_scope_trace(plan, dt, gt, _T(s.now_us[idx]), global_has=_T(glo[3]),
                                           half_life_days=h, min_rel=m)
        exp_conf = np.where(win == 1, dom[1], glo[1])
        _check_entries(wt, scope, s.out[idx], exp_conf, win, f"h={h!r} m={m!r}")
    N.check_faults(_dev(), "walk_scope_trace")


# ---------------------------------------------------------------------------------------
# days on the host (decay.decay_reliability_if_needed) and on the device (decay_view) agree
# ---------------------------------------------------------------------------------------
def test_host_days_and_device_days_agree():
    from bayesian_engine import decay
    s, groups = _stamp_groups()
    at = lambda u: EPOCH + timedelta(microseconds=int(u))  # noqa: E731
    host = np.empty(len(s.r))
    for i, (r, t, now, h, m) in enumerate(zip(s.r.tolist(), s.t_us.tolist(), s.now_us.tolist(), s.h.tolist(),
                                              s.m.tolist())):
        host[i], _ = decay.decay_reliability_if_needed(r, at(t), now=at(now), half_life_days=h, min_reliability=m)
    device = np.empty(len(s.r))
    for (now, h, m), idx in groups:
        device[idx] = _np(batch.decay_view(_T(s.r[idx]), _T(s.t_us[idx]), now, None, h, m))
    dr.assert_bits(host, device, "host days against device days")
    dr.assert_bits(device, s.out, "device against the fixture")
