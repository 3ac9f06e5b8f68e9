"""The correlated common process past 31 common columns (15 frequencies) and
the optimal statistic up to EWH_OS_MAX_COMMON_COLS, on the CPU: the fixtures
of tests/golden/make_corr_wide.py regenerate, the descriptor validation (shared
by the HIP library and its host twin, csrc/ewarp_desc.h) through the twin,
and the Python layer at the reference's default frequency count."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import load_golden, strict_tolerance
from enterprise_warp_amd import _lib, synth
from golden.make_corr_wide import CORR_WIDE_NAMES, build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TWIN = os.path.join(ROOT, "enterprise_warp_amd", "libewarp_cpu.so")
OS_CAP = 63            # EWH_OS_MAX_COMMON_COLS (include/ewarp_hip.h)


# --------------------------------------------------------------------------
# fixtures
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", CORR_WIDE_NAMES)
def test_fixture_regenerates(name):
    """The stored theta is the generator's; lnl (enterprise order) and
    lnl_exact (near-exact) equal the oracles' values now -- lnl to 1e-9
    relative as test_oracle.py holds the older fixtures, lnl_exact on two
    samples bit for bit --; near-truth draws satisfy |ent - exact| <= strict;
    every stored value is finite and the two references agree on it."""
    from oracle.ddref import DDReferencePTA
    from oracle.device_order_ref import DeviceOrderPTA
    from oracle.enterprise_ref import OraclePTA
    pta, z = load_golden(name, full=True)
    _, _, X = build(name)
    np.testing.assert_array_equal(z["theta"], X)
    for key in ("lnl", "lnl_dev", "lnl_exact"):
        assert np.all(np.isfinite(z[key])), key
    near = z["near"]
    assert near.sum() == 8 and (~near).sum() == 8
    assert np.all(np.abs(z["lnl"][near] - z["lnl_exact"][near]) <= strict_tolerance(z["lnl_exact"][near]))
    const_ = pta.constant_values()
    fixed = const_ if pta.white_fixed() else None
    psrs, terms = [c.psr for c in pta.signal_collections], pta.oracle_terms()
    ent = OraclePTA(psrs, terms, fixed_params=fixed)
    exact = (DeviceOrderPTA(psrs, terms, fixed, np.longdouble) if ent.correlated() else DDReferencePTA(psrs, terms))
    for i, x in enumerate(z["theta"]):
        d = dict(const_)
        d.update(pta.map_params(x))
        assert abs(ent.lnlikelihood(d) - z["lnl"][i]) <= 1e-9 * abs(z["lnl"][i])
        if i in (0, 8):
            assert exact.lnlikelihood(d) == z["lnl_exact"][i]


# --------------------------------------------------------------------------
# descriptor validation through the host twin
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin():
    if not os.path.exists(TWIN):
        subprocess.run(["make", "-C", os.path.join(ROOT, "enterprise_warp_amd", "csrc"), "cpu"], check=True,
                       capture_output=True)
    lib = C.CDLL(TWIN)
    lib.ewh_create.argtypes = [C.POINTER(_lib.PtaDesc), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p)]
    lib.ewh_create.restype = C.c_int
    lib.ewh_last_error.restype = C.c_char_p
    return lib


def _create(lib, n_common, kind, orf=True, n_col_common=None):
    """ewh_create on the smallest valid descriptor with n_common common
    columns: one pulsar, 4 TOAs, no other column.  Returns (rc, message)."""
    n = 4
    keep = []

    def dptr(a):
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_double))

    def iptr(a):
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_int32))
    cst = _lib.Pref(-1, 0, 0.0)
    slots = (_lib.Pref * 1)(_lib.Pref(-1, 0, 1.0))
    psr = _lib.PulsarDesc(
        n, n_common, 0, 0,
        dptr(np.ones((n, max(1, n_common)))), dptr(np.zeros(n)), dptr(np.full(n, 1e-6)),
        1, slots, iptr(np.zeros(n, np.int32)), iptr(np.full(n, -1, np.int32)),
        0, None, None, None, None,
        0, None, None, None,
        n_common,
        0, None, None)
    ncc = n_common if n_col_common is None else n_col_common
    cspec = (_lib.SpecEntry * max(1, ncc))()
    for g in range(ncc):
        cspec[g] = _lib.SpecEntry(_lib.SPEC_POWERLAW, g, _lib.Pref(-1, 0, -14.0), _lib.Pref(-1, 0, 4.0), cst,
                                  1e-8 * (1 + g // 2), 1e-8, 3.17e-8)
    common = _lib.CommonDesc(ncc, dptr(np.ones((1, 1))) if orf else None,
                             cspec if kind == _lib.COMMON_CORRELATED else None, kind)
    psrs = (_lib.PulsarDesc * 1)(psr)
    d = _lib.PtaDesc(_lib.EWH_ABI_VERSION, 1, 0, 1, psrs, C.pointer(common))
    h = C.c_void_p()
    ids = (C.c_int32 * 1)(0)
    rc = lib.ewh_create(C.byref(d), ids, 1, C.byref(h))
    assert rc != 0 and not h.value          # (the twin takes no common descriptor at all)
    return rc, lib.ewh_last_error().decode()


def test_wide_common_descriptor_passes_validation(twin):
    """32 common columns (16 frequencies) are a valid descriptor: the host
    twin reaches its own refusal of correlated handles (EWH_E_UNSUPPORTED,
    "device-only") instead of EWH_E_INVALID "need 1..31 columns"; so do 180."""
    for ncol in (31, 32, 63, 64, 180):
        rc, msg = _create(twin, ncol, _lib.COMMON_CORRELATED)
        assert rc == -4 and "device-only" in msg, (ncol, rc, msg)


def test_bad_common_descriptor_still_invalid(twin):
    rc, msg = _create(twin, 0, _lib.COMMON_CORRELATED)
    assert rc == -1, msg
    rc, msg = _create(twin, 32, _lib.COMMON_CORRELATED, orf=False)
    assert rc == -1 and "ORF" in msg, msg
    rc, msg = _create(twin, 32, _lib.COMMON_OPTSTAT, orf=False)
    assert rc == -1, msg
    rc, msg = _create(twin, 32, _lib.COMMON_CORRELATED, n_col_common=30)    # n_common != common->n_col
    assert rc == -1, msg


def test_optstat_cap_is_named(twin):
    """An optimal-statistic descriptor at the cap is valid (the twin's own
    refusal); one column above it is EWH_E_UNSUPPORTED naming the cap."""
    rc, msg = _create(twin, OS_CAP, _lib.COMMON_OPTSTAT)
    assert rc == -4 and "device-only" in msg, msg
    rc, msg = _create(twin, OS_CAP + 1, _lib.COMMON_OPTSTAT)
    assert rc == -4 and "EWH_OS_MAX_COMMON_COLS" in msg and str(OS_CAP) in msg and "device-only" not in msg, msg


# --------------------------------------------------------------------------
# Python layer
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_nfreqs_pta():
    """Two pulsars over 14.95 yr with `gwb: hd_vary_gamma` (no _nfreqs): the
    count comes from determine_nfreqs(common_signal=True) under the default
    red_general_freqs tobs_60days -- round(Tspan / 60 d - 1) = 90."""
    psrs = [synth.make_pulsar(f"J{i:04d}+1495", 260, tspan_yr=14.95, seed=1495 + i, epoch_size=4) for i in range(2)]
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    ns = synth.params_namespace(Tspan, True)
    wn = synth.white_noisedict(psrs, 1497)
    terms = {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend",
             "spin_noise": "powerlaw_10_nfreqs", "dm_noise": "powerlaw_10_nfreqs"}
    pta = synth.build_pta(psrs, terms, {"gwb": "hd_vary_gamma"}, ns, wn)
    truth = synth.truth_values(pta, 1498, white=wn)
    synth.simulate_residuals(pta, truth, 1499)
    return pta, truth


def test_default_frequency_count_gives_180_common_columns(default_nfreqs_pta):
    pta, _ = default_nfreqs_pta
    assert pta.correlated()
    cl = pta.common_layout()
    assert cl["n_col"] == 180 and len(cl["spec"]) == 180 and cl["orf"].shape == (2, 2)
    for L in pta.layout():
        assert L["n_common"] == 180


def test_oracle_matches_dense_covariance_at_180_columns(default_nfreqs_pta):
    """The enterprise-order route (Sigma = blockdiag(TNT) + Phi^-1) against the
    dense covariance C = N + T Phi T^T over all TOAs on one near-truth draw, at
    the tolerance of test_oracle.py::test_correlated_woodbury_matches_dense."""
    from oracle.dense_ref import dense_lnl_pta, woodbury_lnl_pta
    from oracle.enterprise_ref import OraclePTA
    pta, truth = default_nfreqs_pta
    o = OraclePTA([c.psr for c in pta.signal_collections], pta.oracle_terms())
    assert o.correlated()
    x = synth.near_draws(pta, truth, 1, 1500)[0]
    d = dict(pta.constant_values())
    d.update(pta.map_params(x))
    a = dense_lnl_pta(o, d, 1e-12)
    b = woodbury_lnl_pta(o, d, 1e-12)
    print(f"dense {a!r} woodbury {b!r} rel {abs(a - b) / abs(a):.3e}")
    assert abs(a - b) <= 1e-9 * abs(a)
