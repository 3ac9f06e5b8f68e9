"""Conditional GP on the device (ABI 10: ewh_cond_gp, csrc/cond.hip) against
the criterion of tests/_cond_ref.py -- per fixture, floor = 4 x enterprise
order's worst near-row error; near rows: every unit within the floor; prior
rows: worst error <= max(enterprise order's worst, floor); status 0 -- and
properties that need no reference: batch-size independence bit for bit,
group relabelling, coefficient-only calls, ewh_lnl_batch bits unchanged by a
conditional call, in-place white noise, and the failure statuses.

Fixtures: c1_j1832 (326 TOAs: no multiple of 16 or 64; varying white noise),
c2_small (ECORR epochs), c3_small (fixed white noise, four pulsars of
different n_toa; again with delays on the first and last pulsar), c4_small
(13 blocks, three pulsars), c1_widefix (376 columns = 24 blocks, the lazily
kept Gram), c2_chromvary (the VALU process kernel)."""
import numpy as np
import pytest

import _cond_ref as cr
from conftest import load_golden

pytestmark = pytest.mark.gpu

CASES = [("c1_j1832", ()), ("c2_small", ()), ("c3_small", ()), ("c3_small", (0, -1)), ("c4_small", ()),
         ("c1_widefix", ()), ("c2_chromvary", ())]


def _call(eng):
    return lambda th, z, cg, ng: eng.cond_gp(th, z=z, col_group=cg, n_group=ng)


@pytest.mark.parametrize("name,dl", CASES, ids=[n + ("_delays" if d else "") for n, d in CASES])
def test_criterion(require_gpu, name, dl):
    cs = cr.case(name, dl)
    eng = cs.pta.engine()
    assert eng.cond_dims() == (cs.n_coef, int(cs.toa_off[-1]))
    coef, proc, status = cr.run_case(cs, _call(eng))
    cs.check(coef, proc, status, f"{name}{' +delays' if dl else ''} (device)")


def _x37(name):
    pta, z = load_golden(name, full=True)
    X = np.ascontiguousarray(z["theta"][np.arange(37) % len(z["theta"])])
    n_coef = sum(c.T.shape[1] for c in pta.signal_collections)
    zz = np.random.default_rng(7).standard_normal((37, n_coef))
    # groups: per pulsar 0 = timing model, 1 = the rest
    grp = np.concatenate([np.where(np.arange(c.T.shape[1]) < c.n_lead_const, 0, 1)
                          for c in pta.signal_collections]).astype(np.int32)
    return pta, X, zz, grp


@pytest.mark.parametrize("name", ["c3_small", "c1_j1832"])
def test_rows_do_not_depend_on_the_batch(require_gpu, name):
    pta, X, z, grp = _x37(name)
    eng = pta.engine()
    c37, y37, s37 = eng.cond_gp(X, z=z, col_group=grp, n_group=2)
    assert not s37.any()
    for B in (1, 5, 17):
        c, y, s = eng.cond_gp(X[:B], z=z[:B], col_group=grp, n_group=2)
        assert np.array_equal(c, c37[:B]) and np.array_equal(y, y37[:B]) and np.array_equal(s, s37[:, :B]), B


def test_groups_relabelled_alone_and_absent(require_gpu):
    pta, X, z, grp = _x37("c3_small")
    X, z = X[:9], z[:9]
    eng = pta.engine()
    c, y, _ = eng.cond_gp(X, z=z, col_group=grp, n_group=2)
    c_sw, y_sw, _ = eng.cond_gp(X, z=z, col_group=(1 - grp).astype(np.int32), n_group=2)
    assert np.array_equal(c, c_sw) and np.array_equal(y[:, 0], y_sw[:, 1]) and np.array_equal(y[:, 1], y_sw[:, 0])
    only1 = np.where(grp == 1, 0, -1).astype(np.int32)
    _, y1, _ = eng.cond_gp(X, z=z, col_group=only1, n_group=1)
    assert np.array_equal(y1[:, 0], y[:, 1])
    c0, y0, _ = eng.cond_gp(X, z=z)
    assert y0 is None and np.array_equal(c0, c)


@pytest.mark.parametrize("B", [5, 37])
def test_lnl_bits_unchanged_by_a_conditional_call(require_gpu, B):
    """B = 5: the latency path; B = 37: the batched route, replayed from its graph."""
    pta, X, z, grp = _x37("c3_small")
    before = [pta.get_lnlikelihood_batch(X[:B]) for _ in range(3)]      # eager, capture, replay
    pta.engine().cond_gp(X[:B], z=z[:B], col_group=grp, n_group=2)
    after = [pta.get_lnlikelihood_batch(X[:B]) for _ in range(3)]
    for a in before[1:] + after:
        assert np.array_equal(a, before[0])


def test_in_place_white_noise_equals_a_fresh_handle(require_gpu):
    pta, X, z, grp = _x37("c3_small")
    X, z = X[:6], z[:6]
    const = pta.constant_values()
    rng = np.random.default_rng(5)
    new = {k: (v * rng.uniform(0.95, 1.05) if k.endswith("_efac") else v + rng.uniform(-0.2, 0.2))
           for k, v in const.items() if k.endswith(("_efac", "_log10_tnequad", "_log10_ecorr"))}
    old = pta.engine().cond_gp(X, z=z, col_group=grp, n_group=2)
    pta.set_default_params(new)
    got = pta.engine().cond_gp(X, z=z, col_group=grp, n_group=2)
    fresh, _, _, _ = load_golden("c3_small")
    fresh.set_default_params(new)
    want = fresh.engine().cond_gp(X, z=z, col_group=grp, n_group=2)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert not np.array_equal(got[0], old[0])


@pytest.mark.parametrize("name", ["c3_small", "c1_j1832"])
@pytest.mark.parametrize("bad", [np.nan, -np.inf])
def test_bad_spectral_parameter_fails_its_row_only(require_gpu, name, bad):
    pta, X, z, grp = _x37(name)
    X, z = X[:7].copy(), z[:7]
    eng = pta.engine()
    clean = eng.cond_gp(X, z=z, col_group=grp, n_group=2)
    psr = pta.pulsars[0]
    j = pta.param_names.index(f"{psr}_red_noise_log10_A")
    X[3, j] = bad
    c, y, s = eng.cond_gp(X, z=z, col_group=grp, n_group=2)
    want = np.zeros_like(s)
    want[0, 3] = 1
    assert np.array_equal(s, want)
    m0, n0 = pta.signal_collections[0].T.shape[1], len(pta.signal_collections[0].psr.toas)
    assert np.isnan(c[3, :m0]).all() and np.isnan(y[3, :, :n0]).all()
    cm = np.ones_like(c, bool)
    cm[3, :m0] = False
    ym = np.ones_like(y, bool)
    ym[3, :, :n0] = False
    assert np.array_equal(c[cm], clean[0][cm]) and np.array_equal(y[ym], clean[1][ym])
