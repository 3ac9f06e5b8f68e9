"""Conditional GP (ABI 10: ewh_cond_dims / ewh_cond_gp,
enterprise_warp_amd.condgp.ConditionalGP) on the CPU: the per-signal column
map, the enterprise-style methods' keys and shapes and the correlated refusal,
the host twin against the criterion of tests/_cond_ref.py (c1_j1832, c3_small,
c2_chromvary, c3_small with a dip + annual delay on pulsar 0; status 2 for a
NaN delay amplitude), and the reparametrisation identity the device relies on
(mean invariant, a draw with the same z reproduced, under T -> T A)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sl

import _cond_ref as cr
from conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "enterprise_warp_amd", "libewarp_cpu.so")


# ------------------------------------------------------------------ column map
def test_signal_column_map_merged_curn():
    pta, _, _, _ = load_golden("c3_small")
    for c in pta.signal_collections:
        sc = c.signal_cols
        nl, m = c.n_lead_const, c.T.shape[1]
        assert list(sc) == ["timing_model", "gw", "red_noise", "dm_gp"]
        assert sc["timing_model"] == list(range(nl))
        # gw is merged onto the first red-noise Fourier columns
        assert sc["gw"] == sc["red_noise"][:len(sc["gw"])] and len(sc["gw"]) < len(sc["red_noise"])
        assert sc["red_noise"] == c.gp_cols["red_noise"] and sc["gw"] == c.gp_cols["gw"]
        assert sorted(set(sum(sc.values(), []))) == list(range(m))      # every column has an owner


def test_signal_column_map_theta_dependent_basis():
    pta, _, _, _ = load_golden("c2_chromvary")
    c = pta.signal_collections[0]
    sc = c.signal_cols
    assert "chromatic_gp" in sc and "chromatic_gp" not in c.gp_cols     # gp_cols leaves it out, unchanged
    assert all(c.col_bgroup[j] >= 0 for j in sc["chromatic_gp"])
    assert all(c.col_bgroup[j] < 0 for k in ("timing_model", "red_noise", "dm_gp") for j in sc[k])
    assert sorted(sum(sc.values(), [])) == list(range(c.T.shape[1]))


def test_correlated_model_is_refused():
    from enterprise_warp_amd import ConditionalGP
    pta, _, _, _ = load_golden("c5_small")
    with pytest.raises(NotImplementedError):
        ConditionalGP(pta)


# ------------------------------------------------------------------------ twin
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "enterprise_warp_amd", "csrc"), "cpu"], check=True,
                       capture_output=True)
    path = str(tmp_path_factory.mktemp("cond") / "twin.npz")
    env = dict(os.environ, EWARP_BACKEND="cpu", OMP_NUM_THREADS="4")
    env.pop("EWARP_HIP_LIB", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "_cond_worker.py"), path], env=env, capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0 and "COND_WORKER_OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    return np.load(path)


def test_twin_exports_cond_entries():
    import ctypes
    from enterprise_warp_amd import _lib
    assert {"ewh_cond_dims", "ewh_cond_gp"} <= set(_lib.EXPORTS) and _lib.EWH_ABI_VERSION >= 10
    if os.path.exists(LIB):
        lib = ctypes.CDLL(LIB)
        assert hasattr(lib, "ewh_cond_dims") and hasattr(lib, "ewh_cond_gp")


@pytest.mark.parametrize("i", range(4))
def test_twin_meets_the_criterion(twin, i):
    from _cond_worker import CASES
    name, dl = CASES[i]
    cs = cr.case(name, dl)
    coef = [twin[f"c{i}_coef{k}"] for k in (0, 1)]
    proc = [{gi: twin[f"c{i}_proc{k}_{gi}"] for gi in range(len(cs.groups))} for k in (0, 1)]
    cs.check(coef, proc, list(twin[f"c{i}_status"]), f"{name}{' +delays' if dl else ''} (cpu twin)")


def test_twin_nan_delay_amplitude_is_status_2(twin):
    st = twin["nan_status"]
    want = np.zeros_like(st)
    want[0, 2] = 2                                    # pulsar 0 carries the delays
    assert np.array_equal(st, want)
    cs = cr.case("c3_small", (0,))
    bad, ok = twin["nan_coef_bad"], twin["nan_coef_ok"]
    m0, n0 = cs.m[0], cs.n_toa[0]
    assert np.isnan(bad[2, :m0]).all() and np.isnan(twin["nan_proc_bad"][2, 0, :n0]).all()
    mask = np.ones_like(bad, bool)
    mask[2, :m0] = False
    assert np.array_equal(bad[mask], ok[mask])        # every other unit unchanged
    pm = np.ones_like(twin["nan_proc_bad"], bool)
    pm[2, 0, :n0] = False
    assert np.array_equal(twin["nan_proc_bad"][pm], twin["nan_proc_ok"][pm])


# ------------------------------------------------------------------- API shape
def test_enterprise_style_methods_keys_and_shapes(monkeypatch):
    """Keys and shapes of the four methods (the engine call is replaced by the
    enterprise-order reference, so this runs without a device)."""
    from enterprise_warp_amd import ConditionalGP
    cs = cr.case("c3_small")
    pta = cs.pta
    cg = ConditionalGP(pta)
    ref = cs.references()

    class FakeEngine:
        def cond_dims(self):
            return cg.n_coef, cg.n_toa_total

        def cond_gp(self, theta, z=None, col_group=None, n_group=0, want_coef=True):
            B = len(theta)
            coef = np.zeros((B, cg.n_coef))
            for p in range(len(cs.psrs)):
                coef[:, cs.col_off[p]:cs.col_off[p + 1]] = ref["ent"][(p, 4)][0]
            if z is not None:
                coef = coef + 1e-9 * z
            proc = None
            if n_group:
                proc = np.zeros((B, n_group, cg.n_toa_total))
                for p in range(len(cs.psrs)):
                    T = ref["T"][(p, 4)]
                    for g in range(n_group):
                        cols = np.flatnonzero(col_group[cs.col_off[p]:cs.col_off[p + 1]] == g)
                        proc[:, g, cs.toa_off[p]:cs.toa_off[p + 1]] = \
                            coef[:, cs.col_off[p] + cols] @ T[:, cols].T
            return (coef if want_coef else None), proc, np.zeros((len(cs.psrs), B), np.int32)

    monkeypatch.setattr(cg, "_engine", lambda: FakeEngine())
    x = cs.X[4]
    names = [f"{c.name}_{s}" for c in pta.signal_collections for s in c.signal_cols]
    mc = cg.get_mean_coefficients(x)
    assert sorted(mc) == sorted(n + "_coefficients" for n in names)
    for c in pta.signal_collections:
        for s, cols in c.signal_cols.items():
            assert mc[f"{c.name}_{s}_coefficients"].shape == (len(cols),)
        # merged columns: gw reports the shared red-noise values
        k = len(c.signal_cols["gw"])
        assert np.array_equal(mc[f"{c.name}_gw_coefficients"], mc[f"{c.name}_red_noise_coefficients"][:k])
    one = cg.sample_coefficients(pta.map_params(x), n=1, rng=3)
    many = cg.sample_coefficients(x, n=3, rng=3)
    assert isinstance(one, dict) and isinstance(many, list) and len(many) == 3
    assert all(np.array_equal(one[k], many[0][k]) for k in one)        # the same seed: the same first draw
    mp = cg.get_mean_processes(x)
    assert sorted(mp) == sorted(names)
    for c in pta.signal_collections:
        for s in c.signal_cols:
            assert mp[f"{c.name}_{s}"].shape == (len(c.psr.toas),)
        T, a = ref["T"][(pta.pulsars.index(c.name), 4)], mc
        cols = c.signal_cols["red_noise"]
        np.testing.assert_allclose(mp[f"{c.name}_red_noise"], T[:, cols] @ a[f"{c.name}_red_noise_coefficients"],
                                   rtol=1e-12, atol=1e-22)
    sp = cg.sample_processes(x, n=2, rng=1)
    assert isinstance(sp, list) and len(sp) == 2 and sorted(sp[0]) == sorted(names)
    procs, status = cg.processes_batch(cs.X[:3], signals=["dm_gp"])
    assert sorted(procs) == sorted((c.name, "dm_gp") for c in pta.signal_collections) and status.shape == (4, 3)
    assert all(v.shape == (3, len(c.psr.toas)) for c in pta.signal_collections for v in [procs[(c.name, "dm_gp")]])
    assert cg.coefficients_batch(cs.X[:3]).shape == (3, cg.n_coef)


# ------------------------------------------------------------------ invariance
@pytest.mark.parametrize("name", ["c1_j1832", "c3_small"])
def test_mean_and_draw_invariant_under_reparametrisation(name):
    """coef_user = A coef_dev + [c_r; 0] with the same z, for T_dev = T A and
    r_dev = r - M c_r: the identity the device relies on, in numpy at 1e-9
    sigma on the near rows (C from the weighted least-squares projection the
    library applies, restated)."""
    cs = cr.case(name)
    ref = cs.references()
    from oracle.enterprise_ref import OraclePTA
    const = cs.pta.constant_values()
    ent = OraclePTA(cs.psrs, cs.pta.oracle_terms(), fixed_params=None)
    worst = 0.0
    for b in np.flatnonzero(cs.near):
        d = dict(const)
        d.update(cs.pta.map_params(cs.X[b]))
        for p, (pp, c) in enumerate(zip(ent.pulsars, cs.pta.signal_collections)):
            nl, m = c.n_lead_const, cs.m[p]
            T, r = np.asarray(pp.basis(d), float), np.asarray(pp.r, float)
            w0 = 1.0 / np.asarray(pp.sigma, float) ** 2
            M = T[:, :nl]
            C = np.linalg.solve(M.T @ (w0[:, None] * M), M.T @ (w0[:, None] * np.c_[T[:, nl:], r]))
            A = np.eye(m)
            A[:nl, nl:] = -C[:, :-1]
            pp2 = OraclePTA([cs.psrs[p]], [cs.pta.oracle_terms()[p]], fixed_params=None).pulsars[0]
            pp2.T = T @ A
            pp2.basis = lambda params, _T=pp2.T: _T
            pp2.r = r - M @ C[:, -1]
            TNT, TNr, _, _ = pp2.white_terms(d)
            cf = sl.cho_factor(TNT + np.diag(1.0 / pp.phi(d)), lower=True)
            z = cs.z[b, cs.col_off[p]:cs.col_off[p + 1]]
            shift = np.r_[C[:, -1], np.zeros(m - nl)]
            mean = A @ sl.cho_solve(cf, TNr) + shift
            draw = mean + A @ sl.solve_triangular(cf[0], z, lower=True, trans="T")
            worst = max(worst, cs.coef_err(p, b, mean, 0), cs.coef_err(p, b, draw, 1))
    print(f"{name}: reparametrised mean / draw vs near-exact, worst {worst:.3e} sigma")
    assert worst <= 1e-9
