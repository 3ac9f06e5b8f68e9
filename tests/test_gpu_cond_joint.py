"""Joint conditional GP on the device (ABI 11: ewh_cond_joint,
csrc/cond_joint.hip) against the criterion of tests/_cond_joint_ref.py -- per
case, floor = 4 x enterprise order's worst near-row error; near rows: every
unit within the floor; prior rows: worst error <= max(enterprise order's
worst, floor); status 0 -- and properties that need no reference: rows bit for
bit across batch sizes and chunk bounds, group relabelling, coefficient-only
calls, ewh_lnl_batch bits unchanged by a joint call, and the failure statuses.

Cases: c5_small (Hellings-Downs, fixed white noise: the cached Gram in
descriptor order, mo = 42), c5_mono, c5_dipo (mo = 44), c5_varwn (the aligned
layout of varying white noise), mc_hd_mono (two processes in the term form,
the monopole on 6 of the 10 common columns), synth7 (7 pulsars, N_c = 126
across 16- and 64-column panels, n_col = 18, mo = 33 / 34 / 35: the masked
k-slice), and three wide variants of synth7 whose own blocks leave more than
one trailing tile per side of the Schur update and whose dense stage has more
than 256 rows: synth7_nc40 (nc = 40, mo = 31 / 32 / 33, n = 80: off-diagonal
Schur tiles on waves 1 and 2, a full last pivot panel beside two masked ones,
N_c = 280 -> 288), synth7_nc40_varwn (the same with varying white noise: 1, 0
and 15 inner pads, n = 80 / 80 / 96) and synth7_nc48_lead (nc = 48, mo = 11 /
12 / 13: a single pivot panel, N_c = 336 with no identity pad rows).  Every
case uses the first 4 prior and 4 near rows."""
import numpy as np
import pytest

import _cond_joint_ref as jr
from conftest import load_golden

pytestmark = pytest.mark.gpu

CASES = ["c5_small", "c5_mono", "c5_dipo", "c5_varwn", "mc_hd_mono", "synth7", "synth7_nc40", "synth7_nc40_varwn",
         "synth7_nc48_lead"]


def _call(eng, **kw):
    return lambda th, z, cg, ng: eng.cond_joint(th, z=z, col_group=cg, n_group=ng, **kw)


@pytest.mark.parametrize("name", CASES)
def test_criterion(require_gpu, name):
    cs = jr.case(name)
    assert cs.references()["ok"].all(), "the long-double reference fails on a row of this case"
    eng = cs.pta.engine()
    assert eng.cond_joint_dims() == (cs.n_coef, int(cs.toa_off[-1]))
    coef, proc, status = jr.run_case(cs, _call(eng))
    cs.check(coef, proc, status, f"{name} (device)")


def _x37(name):
    if name in jr.SYNTH:                                 # a synthesised case: its PTA and its 8 rows, tiled
        cs = jr.case(name)
        pta, X = cs.pta, np.ascontiguousarray(cs.X[np.arange(37) % len(cs.X)])
    else:
        pta, z = load_golden(name, full=True)
        keep = np.flatnonzero(np.isfinite(z["lnl"]))
        X = np.ascontiguousarray(z["theta"][keep[np.arange(37) % len(keep)]])
    n_coef = sum(c.T.shape[1] for c in pta.signal_collections)
    zz = np.random.default_rng(7).standard_normal((37, n_coef))
    # groups: per pulsar 0 = the common process's columns, 1 = the rest
    grp = np.concatenate([np.where(np.isin(np.arange(c.T.shape[1]), c.common_cols), 0, 1)
                          for c in pta.signal_collections]).astype(np.int32)
    return pta, X, zz, grp


@pytest.mark.parametrize("name", ["c5_small", "c5_varwn", "synth7_nc40", "synth7_nc40_varwn"])
def test_rows_do_not_depend_on_the_batch_or_the_chunk(require_gpu, name):
    pta, X, z, grp = _x37(name)
    eng = pta.engine()
    c37, y37, s37 = eng.cond_joint(X, z=z, col_group=grp, n_group=2)
    assert not s37.any()
    for B in (1, 5, 17):
        c, y, s = eng.cond_joint(X[:B], z=z[:B], col_group=grp, n_group=2)
        assert np.array_equal(c, c37[:B]) and np.array_equal(y, y37[:B]) and np.array_equal(s, s37[:, :B]), B
    for mc in (3, 1):                                    # eight rows across chunk bounds
        c, y, s = eng.cond_joint(X[:8], z=z[:8], col_group=grp, n_group=2, max_chunk=mc)
        assert np.array_equal(c, c37[:8]) and np.array_equal(y, y37[:8]) and np.array_equal(s, s37[:, :8]), mc


def test_groups_relabelled_alone_and_absent(require_gpu):
    pta, X, z, grp = _x37("c5_small")
    X, z = X[:9], z[:9]
    eng = pta.engine()
    c, y, _ = eng.cond_joint(X, z=z, col_group=grp, n_group=2)
    c_sw, y_sw, _ = eng.cond_joint(X, z=z, col_group=(1 - grp).astype(np.int32), n_group=2)
    assert np.array_equal(c, c_sw) and np.array_equal(y[:, 0], y_sw[:, 1]) and np.array_equal(y[:, 1], y_sw[:, 0])
    only1 = np.where(grp == 1, 0, -1).astype(np.int32)
    _, y1, _ = eng.cond_joint(X, z=z, col_group=only1, n_group=1)
    assert np.array_equal(y1[:, 0], y[:, 1])
    c0, y0, _ = eng.cond_joint(X, z=z)                   # a coefficient-only call
    assert y0 is None and np.array_equal(c0, c)
    cn, yn, _ = eng.cond_joint(X, z=z, col_group=grp, n_group=2, want_coef=False)
    assert cn is None and np.array_equal(yn, y)


def test_class_surface_on_the_device(require_gpu):
    from enterprise_warp_amd import JointConditionalGP
    pta, X, z, _ = _x37("c5_small")
    jg = JointConditionalGP(pta)
    mean = jg.get_mean_coefficients(X[0])
    proc = jg.get_mean_processes(pta.map_params(X[0]))
    for c in pta.signal_collections:
        a = mean[f"{c.name}_gw_coefficients"]
        assert a.shape == (len(c.common_cols),) and np.isfinite(a).all()
        np.testing.assert_allclose(proc[f"{c.name}_gw"], c.T[:, c.common_cols] @ a, rtol=1e-9, atol=1e-20)
    draws = jg.sample_coefficients(X[0], n=2, rng=4)
    assert len(draws) == 2 and sorted(draws[0]) == sorted(mean)


@pytest.mark.parametrize("B", [5, 37])
def test_lnl_bits_unchanged_by_a_joint_call(require_gpu, B):
    pta, X, z, grp = _x37("c5_small")
    before = [pta.get_lnlikelihood_batch(X[:B]) for _ in range(3)]      # eager, capture, replay
    pta.engine().cond_joint(X[:B], z=z[:B], col_group=grp, n_group=2)
    after = [pta.get_lnlikelihood_batch(X[:B]) for _ in range(3)]
    for a in before[1:] + after:
        assert np.array_equal(a, before[0])


def test_indefinite_orf_rows_are_status_3(require_gpu):
    """c5_noauto (no auto term: M_g indefinite on some rows): status 3 on
    every pulsar of exactly the golden's -inf rows, NaN there, the other rows
    equal to the same rows evaluated alone."""
    pta, z = load_golden("c5_noauto", full=True)
    X = np.ascontiguousarray(z["theta"])
    bad = ~np.isfinite(z["lnl"])
    assert bad.any() and not bad.all()
    n_coef = sum(c.T.shape[1] for c in pta.signal_collections)
    zz = np.random.default_rng(3).standard_normal((len(X), n_coef))
    grp = np.zeros(n_coef, np.int32)
    eng = pta.engine()
    c, y, s = eng.cond_joint(X, z=zz, col_group=grp, n_group=1)
    assert np.array_equal(s, np.where(bad, 3, 0)[None, :].repeat(len(pta.pulsars), 0))
    assert np.isnan(c[bad]).all() and np.isnan(y[bad]).all()
    assert np.isfinite(c[~bad]).all() and np.isfinite(y[~bad]).all()
    c1, y1, s1 = eng.cond_joint(X[~bad], z=zz[~bad], col_group=grp, n_group=1)
    assert not s1.any() and np.array_equal(c1, c[~bad]) and np.array_equal(y1, y[~bad])
    # the criterion on the rows the reference stands on, a non-zero status on the others
    cs = jr.case("c5_noauto")
    assert np.array_equal(~cs.references()["ok"], cs.inf_rows)
    coef, proc, status = jr.run_case(cs, _call(eng))
    cs.check(coef, proc, status, "c5_noauto (device)")


def test_nan_red_noise_parameter_fails_its_row_only(require_gpu):
    pta, X, z, grp = _x37("c5_small")
    X, z = X[:7].copy(), z[:7]
    eng = pta.engine()
    clean = eng.cond_joint(X, z=z, col_group=grp, n_group=2)
    j = pta.param_names.index(f"{pta.pulsars[1]}_red_noise_log10_A")
    X[3, j] = np.nan
    c, y, s = eng.cond_joint(X, z=z, col_group=grp, n_group=2)
    want = np.zeros_like(s)
    want[:, 3] = 3
    want[1, 3] = 1
    assert np.array_equal(s, want)
    assert np.isnan(c[3]).all() and np.isnan(y[3]).all()
    rows = np.arange(7) != 3
    assert np.array_equal(c[rows], clean[0][rows]) and np.array_equal(y[rows], clean[1][rows])


@pytest.mark.parametrize("signal", ["red_noise", "dm_gp"])
def test_nan_row_across_chunk_bounds(require_gpu, signal):
    """synth7_nc40, B = 7, a NaN log10_A of pulsar 1 in row 3, in chunks of 2
    (the last chunk holds one row, the failed row shares its chunk with a good
    one: the pstat / sfail / retained-factor offsets): row 3 fails alone, the
    other rows are bit for bit those of the clean call made in one chunk.
      dm_gp      the columns are pulsar 1's own: its own block fails, the
                 status pattern of test_nan_red_noise_parameter_fails_its_row_only
                 (1 on pulsar 1, 3 on the others)
      red_noise  here its 10 frequencies lie inside the 20 of the common
                 process, so the parameter enters M_g alone and no own block
                 fails: by include/ewarp_hip.h the sample "failed elsewhere",
                 3 on every pulsar (on c5_small red noise has own columns,
                 hence the 1 there)"""
    pta, X, z, grp = _x37("synth7_nc40")
    X, z = X[:7].copy(), z[:7]
    col = pta.signal_collections[1]
    own_block = not set(col.signal_cols[signal]) <= set(col.common_cols)
    assert own_block == (signal == "dm_gp")
    eng = pta.engine()
    clean = eng.cond_joint(X, z=z, col_group=grp, n_group=2)
    assert not clean[2].any()
    j = pta.param_names.index(f"{pta.pulsars[1]}_{signal}_log10_A")
    X[3, j] = np.nan
    c, y, s = eng.cond_joint(X, z=z, col_group=grp, n_group=2, max_chunk=2)
    want = np.zeros_like(s)
    want[:, 3] = 3
    if own_block:
        want[1, 3] = 1
    assert np.array_equal(s, want)
    assert np.isnan(c[3]).all() and np.isnan(y[3]).all()
    rows = np.arange(7) != 3
    assert np.array_equal(c[rows], clean[0][rows]) and np.array_equal(y[rows], clean[1][rows])


def test_uncorrelated_handle_is_invalid(require_gpu):
    from enterprise_warp_amd import _lib
    pta, th, _, _ = load_golden("c3_small")
    eng = pta.engine()
    with pytest.raises(_lib.EngineError, match="error -1:"):           # EWH_E_INVALID
        eng.cond_joint_dims()
    n_coef = sum(c.T.shape[1] for c in pta.signal_collections)
    theta = np.ascontiguousarray(th[:2], dtype=float)
    status = np.zeros((len(pta.pulsars), 2), np.int32)
    coef = np.zeros((2, n_coef))
    rc = eng.lib.ewh_cond_joint(eng.h, theta.ctypes.data_as(_lib._dp), 2, None, 0, None,
                                coef.ctypes.data_as(_lib._dp), None, status.ctypes.data_as(_lib._ip), 0)
    assert rc == -1
