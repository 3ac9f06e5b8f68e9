"""Several correlated common processes and sampled-parameter ORFs on the CPU:
the Python layer (layout, names, refusals), the ABI-9 descriptor validation
(csrc/ewarp_desc.h) through the host twin, the CPU references of
tests/_common_ref.py and the fixtures of tests/golden/make_multi_common.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _common_ref import TermDeviceOrderPTA, TermOraclePTA
from conftest import load_golden
from enterprise_warp_amd import _lib, models, parameter, signals, synth
from enterprise_warp_amd.pta import PTA
from golden.make_multi_common import MG_COND_MIN, MULTI_NAMES, build, mg_condition, references

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TWIN = os.path.join(ROOT, "enterprise_warp_amd", "libewarp_cpu.so")
TERMS = {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend",
         "spin_noise": "powerlaw_10_nfreqs", "dm_noise": "powerlaw_10_nfreqs"}


def _pta(option, n_psr=3, n_toa=60, seed=700, term="gwb_multi", cls=None):
    rng = np.random.default_rng(seed)
    psrs = []
    for i in range(n_psr):
        v = rng.standard_normal(3)
        psrs.append(synth.make_pulsar(f"J{i:04d}+{seed:04d}", n_toa, seed=seed * 1000 + i, pos=v / np.linalg.norm(v),
                                      epoch_size=4))
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    ns = synth.params_namespace(Tspan, True)
    wn = synth.white_noisedict(psrs, seed + 1)
    return synth.build_pta(psrs, TERMS, {term: option}, ns, wn), psrs, ns, wn


# --------------------------------------------------------------------------
# Python layer
# --------------------------------------------------------------------------
def test_two_orfs_build_and_lay_out():
    """Fails without the feature: a second ORF raised NotImplementedError.
    HD 5 freqs + monopole 3: the union of the columns, two terms with the
    constant coefficient 1, the monopole's spectrum zero on its missing
    columns, one amplitude and gamma per sub-term."""
    pta, psrs, _, _ = _pta("hd_vary_gamma_5_nfreqs+mono_vary_gamma_3_nfreqs")
    assert pta.correlated()
    for name in ("gw_log10_A_hd", "gw_hd_gamma", "gw_log10_A_mono", "gw_mono_gamma"):
        assert name in pta.param_names
    c = pta.signal_collections[0]
    assert [x["name"] for x in c.commons] == ["gw_hd", "gw_mono"] and c.common is c.commons[0]
    assert len(c.common_cols) == 10 and c.commons[1]["cols"] == c.common_cols[:6]
    cl = pta.common_layout()
    assert cl["n_col"] == 10 and len(cl["terms"]) == 2 and cl["orf"] is None and cl["kind"] == "terms"
    hd, mono = cl["terms"]
    assert hd["coef"] == (-1, 1.0) and mono["coef"] == (-1, 1.0)
    pos = [p.pos for p in psrs]
    np.testing.assert_array_equal(hd["mat"], models.orf_matrix("hd", pos))
    np.testing.assert_array_equal(mono["mat"], models.orf_matrix("monopole", pos))
    assert [s[1] for s in mono["spec"]] == list(range(10))
    assert all(s[0] == _lib.SPEC_POWERLAW for s in mono["spec"][:6])
    assert all(s[0] == _lib.SPEC_CONST and s[2] == (-1, 0.0) for s in mono["spec"][6:])
    assert all(s[0] == _lib.SPEC_POWERLAW for s in hd["spec"])
    i_hd, i_mono = pta.param_names.index("gw_log10_A_hd"), pta.param_names.index("gw_log10_A_mono")
    assert hd["spec"][0][2] == (i_hd, 0.0) and mono["spec"][0][2] == (i_mono, 0.0)
    for L in pta.layout():
        assert L["n_common"] == 10


def test_four_subterms_names_and_curn_merges_as_own():
    pta, _, _, _ = _pta("vary_gamma_6_nfreqs+hd_vary_gamma_6_nfreqs+mono_vary_gamma_6_nfreqs+dipo_vary_gamma_4_nfreqs")
    for name in ("gw_log10_A", "gw_gamma", "gw_log10_A_hd", "gw_hd_gamma", "gw_log10_A_mono", "gw_mono_gamma",
                 "gw_log10_A_dipo", "gw_dipo_gamma"):
        assert name in pta.param_names
    cl = pta.common_layout()
    assert cl["n_col"] == 12 and [t["proc"] for t in cl["terms"]] == [0, 1, 2]
    assert [p["name"] for p in cl["procs"]] == ["gw_hd", "gw_mono", "gw_dipo"]
    # the CURN entries are the pulsars' own: in each pulsar's spec list on the common columns
    i_curn = pta.param_names.index("gw_log10_A")
    for L in pta.layout():
        m = L["T"].shape[1]
        own = [s for s in L["spec"] if s[1] >= m - 12 and s[2] == (i_curn, 0.0)]
        assert len(own) == 12


def test_binned_and_legendre_orf_terms():
    pta, psrs, _, _ = _pta("varorf_vary_gamma_5_nfreqs", n_psr=4)
    names = pta.param_names
    assert [f"gw_orf_bin_{i}" in names for i in range(7)] == [True] * 7
    assert "gw_log10_A_orf" in names and "gw_orf_gamma" in names
    cl = pta.common_layout()
    assert len(cl["terms"]) == 8 and cl["n_col"] == 10
    np.testing.assert_array_equal(cl["terms"][0]["mat"], np.eye(4))
    assert cl["terms"][0]["coef"] == (-1, 1.0)
    i0 = names.index("gw_orf_bin_0")
    assert [t["coef"] for t in cl["terms"][1:]] == [(i0 + i, 0.0) for i in range(7)]
    tot = sum(t["mat"] for t in cl["terms"][1:])
    np.testing.assert_array_equal(tot, 1.0 - np.eye(4))          # every pair in exactly one bin
    pos = np.array([p.pos for p in psrs])
    xi = np.degrees(np.arccos(np.clip(pos @ pos.T, -1, 1)))
    edges = models.BIN_ORF_EDGES_DEG
    for i, t in enumerate(cl["terms"][1:]):
        a, b = np.nonzero(t["mat"])
        assert np.all((xi[a, b] >= edges[i]) & (xi[a, b] < edges[i + 1]))
    assert all(t["spec"] is cl["terms"][0]["spec"] for t in cl["terms"])
    # Legendre up to l = 3
    pta, psrs, _, _ = _pta("legendreorf_3_vary_gamma_5_nfreqs", n_psr=4)
    cl = pta.common_layout()
    assert len(cl["terms"]) == 5 and "gw_orf_legendre_3" in pta.param_names
    pos = np.array([p.pos for p in psrs])
    cx = np.clip(pos @ pos.T, -1, 1)
    off = ~np.eye(4, dtype=bool)
    want = [np.ones_like(cx), cx, (3 * cx ** 2 - 1) / 2, (5 * cx ** 3 - 3 * cx) / 2]
    for ell in range(4):
        np.testing.assert_allclose(cl["terms"][1 + ell]["mat"], np.where(off, want[ell], 0.0), rtol=0, atol=1e-15)


def test_single_process_layout_keeps_its_keys():
    pta, psrs, _, _ = _pta("hd_vary_gamma_5_nfreqs", term="gwb")
    cl = pta.common_layout()
    assert cl["kind"] == "hd" and cl["n_col"] == 10 and len(cl["spec"]) == 10
    np.testing.assert_array_equal(cl["orf"], models.orf_matrix("hd", [p.pos for p in psrs]))
    assert cl["orf"].flags["C_CONTIGUOUS"] and len(cl["terms"]) == 1
    # the same model through gwb_multi: another signal name, the same layout form
    pta2, _, _, _ = _pta("hd_vary_gamma_5_nfreqs")
    cl2 = pta2.common_layout()
    assert cl2["kind"] == "hd" and "gw_log10_A_hd" in pta2.param_names
    np.testing.assert_array_equal(cl2["orf"], cl["orf"])


def test_gwb_is_unchanged_and_combines_two_orfs():
    pta, _, _, _ = _pta("hd_vary_gamma_5_nfreqs+mono_vary_gamma_3_nfreqs", term="gwb")
    assert pta.common_layout()["kind"] == "monopole"          # reference behaviour: the last term wins

    class Combining(models.StandardModels):
        combine_plus_terms = True
    _, psrs, ns, wn = _pta("hd_vary_gamma_5_nfreqs")
    m = signals.TimingModel() + Combining(psr=psrs, params=ns).gwb("hd_vary_gamma_5_nfreqs+mono_vary_gamma_3_nfreqs")
    mdl = [m + models.StandardModels(psr=p, params=ns).efac("by_backend")
           + models.StandardModels(psr=p, params=ns).spin_noise("powerlaw_10_nfreqs") for p in psrs]
    pta = PTA([x(p) for x, p in zip(mdl, psrs)])
    assert len(pta.common_layout()["terms"]) == 2 and "gw_log10_A_hd" in pta.param_names


def test_same_signal_name_is_refused():
    with pytest.raises(ValueError, match="named 'gw_hd'"):
        _pta("hd_vary_gamma_5_nfreqs+hd_vary_gamma_3_nfreqs")


def test_different_tspan_is_refused():
    _, psrs, ns, _ = _pta("hd_vary_gamma_5_nfreqs")
    pl = lambda n: signals.powerlaw(log10_A=parameter.Uniform(-18, -12)(n + "_A"),  # noqa: E731
                                    gamma=parameter.Uniform(0, 7)(n + "_g"))
    m = (signals.TimingModel() + signals.MeasurementNoise(efac=parameter.Constant(1.0))
         + signals.FourierBasisCommonGP(pl("a"), "hd", components=4, Tspan=ns.Tspan, name="a")
         + signals.FourierBasisCommonGP(pl("b"), "monopole", components=4, Tspan=0.9 * ns.Tspan, name="b"))
    with pytest.raises(NotImplementedError, match="Tspan"):
        m(psrs[0])


def test_term_count_of_a_wide_legendre_orf():
    """Legendre up to l = 16 is 18 terms, more than EWH_COMMON_MAX_TERMS: the
    layout states them (the engine refuses: test_gpu_multi_common.py)."""
    pta, _, _, _ = _pta("legendreorf_16_vary_gamma_3_nfreqs")
    assert len(pta.common_layout()["terms"]) == 18 > _lib.COMMON_MAX_TERMS


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


def _create(lib, n_term=2, mats=None, coef_idx=-1, legacy=False, kind=_lib.COMMON_CORRELATED, null_mat=False,
            null_spec=False, n_param=1, abi8_style=False):
    """ewh_create on a two-pulsar descriptor with 2 common columns and n_term
    terms.  Returns (rc, message)."""
    n, P, nc = 4, 2, 2
    keep = []

    def dptr(a):
        a = np.ascontiguousarray(a, dtype=float)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_double))

    def iptr(a):
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_int32))
    cst = _lib.Pref(-1, 0, 0.0)
    slots = (_lib.Pref * 1)(_lib.Pref(-1, 0, 1.0))
    psrs = (_lib.PulsarDesc * P)()
    for a in range(P):
        psrs[a] = _lib.PulsarDesc(
            n, nc, 0, 0,
            dptr(np.arange(n * nc).reshape(n, nc) + 1.0), dptr(np.zeros(n)), dptr(np.full(n, 1e-6)),
            1, slots, iptr(np.zeros(n, np.int32)), iptr(np.full(n, -1, np.int32)),
            0, None, None, None, None,
            0, None, None, None,
            nc,
            0, None, None)
    cspec = (_lib.SpecEntry * nc)()
    for g in range(nc):
        cspec[g] = _lib.SpecEntry(_lib.SPEC_POWERLAW, g, _lib.Pref(-1, 0, -14.0), _lib.Pref(-1, 0, 4.0), cst,
                                  1e-8, 1e-8, 3.17e-8)
    nt = max(1, n_term)
    terms = (_lib.CommonTerm * nt)()
    for t in range(nt):
        M = np.array([[1.0, 0.3], [0.3, 1.0]]) if mats is None else mats[t % len(mats)]
        terms[t] = _lib.CommonTerm(_lib.Pref(coef_idx, 0, 1.0), None if null_mat else dptr(M),
                                   None if null_spec else cspec)
    orf = dptr(np.eye(P))
    if abi8_style:        # four positional fields: the ABI-8 call sites
        common = _lib.CommonDesc(nc, orf, cspec, kind)
    else:
        common = _lib.CommonDesc(nc, orf if legacy else None, cspec if legacy else None, kind, n_term, terms)
    d = _lib.PtaDesc(_lib.EWH_ABI_VERSION, P, n_param, 1, psrs, C.pointer(common))
    h = C.c_void_p()
    ids = (C.c_int32 * 1)(0)
    rc = lib.ewh_create(C.byref(d), ids, 1, C.byref(h))
    assert rc != 0 and not h.value          # (the twin takes no common descriptor at all)
    return rc, lib.ewh_last_error().decode()


def test_valid_term_descriptors_reach_the_twins_refusal(twin):
    for kw in (dict(n_term=1), dict(n_term=2), dict(n_term=16), dict(n_term=2, coef_idx=0),
               dict(abi8_style=True), dict(n_term=0, legacy=True)):
        rc, msg = _create(twin, **kw)
        assert rc == -4 and "device-only" in msg, (kw, rc, msg)


@pytest.mark.parametrize("kw", [
    dict(n_term=17), dict(n_term=-1),                                  # n_term outside 0..16
    dict(n_term=2, legacy=True),                                       # terms together with the legacy pointers
    dict(n_term=2, null_mat=True), dict(n_term=2, null_spec=True),     # NULL matrix / spec
    dict(n_term=2, mats=[np.array([[1.0, 0.3], [0.2, 1.0]])]),         # asymmetric matrix
    dict(n_term=2, coef_idx=1), dict(n_term=2, coef_idx=0, n_param=0),  # coefficient index >= n_param
    dict(n_term=2, kind=_lib.COMMON_OPTSTAT),                          # terms on an OPTSTAT descriptor
    dict(n_term=0),                                                    # neither form
])
def test_bad_term_descriptor_is_invalid(twin, kw):
    rc, msg = _create(twin, **kw)
    assert rc == -1, (kw, rc, msg)


# --------------------------------------------------------------------------
# the CPU references of tests/_common_ref.py
# --------------------------------------------------------------------------
def _refs(pta):
    const = pta.constant_values()
    fixed = const if pta.white_fixed() else None
    return const, fixed, [c.psr for c in pta.signal_collections], pta.oracle_terms()


@pytest.mark.parametrize("name", ["c5_small", "c5_mono", "c5_dipo", "c5_noauto"])
def test_helper_returns_the_stored_goldens_bit_for_bit(name):
    pta, z = load_golden(name, full=True)
    const, fixed, psrs, terms = _refs(pta)
    ent = TermOraclePTA(psrs, terms, fixed_params=fixed)
    ext = TermDeviceOrderPTA(psrs, terms, fixed, np.longdouble)
    for i in (0, 3, 8, 12):
        d = dict(const)
        d.update(pta.map_params(z["theta"][i]))
        assert ent.lnlikelihood(d) == z["lnl"][i], i
        assert ext.lnlikelihood(d) == z["lnl_exact"][i], i


def test_helper_equals_the_unmodified_oracle_for_hd_plus_monopole():
    from oracle.enterprise_ref import OraclePTA
    pta, z = load_golden("mc_hd_mono", full=True)
    const, fixed, psrs, terms = _refs(pta)
    a = TermOraclePTA(psrs, terms, fixed_params=fixed)
    b = OraclePTA(psrs, terms, fixed_params=fixed)
    for x in z["theta"]:
        d = dict(const)
        d.update(pta.map_params(x))
        assert a.lnlikelihood(d) == b.lnlikelihood(d)


def test_binned_orf_dense_against_woodbury():
    """3 pulsars x 60 TOAs with a binned ORF: the dense covariance
    C = N + T Phi T^T against the Woodbury route, both on the helper's
    phi_global, at the tolerance of test_corr_wide_host.py (1e-9 relative)."""
    from oracle.dense_ref import dense_lnl_pta, woodbury_lnl_pta
    pta, _, _, wn = _pta("varorf_vary_gamma_5_nfreqs", n_psr=3, n_toa=60, seed=710)
    truth = synth.truth_values(pta, 712, white=wn)
    truth.update(gw_log10_A_orf=-14.3, gw_orf_gamma=13.0 / 3.0,
                 gw_orf_bin=np.array([0.30, 0.05, -0.11, -0.15, -0.11, 0.02, 0.20]))
    synth.simulate_residuals(pta, truth, 713)
    o = TermOraclePTA([c.psr for c in pta.signal_collections], pta.oracle_terms())
    x = pta._theta({p.name: truth[p.name] for p in pta.params})[0]
    d = dict(pta.constant_values())
    d.update(pta.map_params(x))
    a = dense_lnl_pta(o, d, 1e-12)
    b = woodbury_lnl_pta(o, d, 1e-12)
    print(f"dense {a!r} woodbury {b!r} rel {abs(a - b) / abs(a):.3e}")
    assert np.isfinite(a) and abs(a - b) <= 1e-9 * abs(a)


# --------------------------------------------------------------------------
# fixtures
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", MULTI_NAMES)
def test_fixture_regenerates(name):
    """The stored theta is the generator's; the references agree on -inf;
    near-truth draws are finite; lnl regenerates on two samples (bit for bit
    for the near-exact value); mc_binorf holds both finite and -inf prior
    draws and every sampled-ORF draw meets the conditioning bound."""
    pta, z = load_golden(name, full=True)
    _, _, X = build(name)
    np.testing.assert_array_equal(z["theta"], X)
    near = z["near"]
    assert near.sum() == 8 and (~near).sum() == 8
    assert np.array_equal(np.isfinite(z["lnl"]), np.isfinite(z["lnl_exact"]))
    assert np.all(np.isfinite(z["lnl"][near]))
    const, mdl = references(pta)
    for i in (0, 8):
        d = dict(const)
        d.update(pta.map_params(z["theta"][i]))
        got = mdl[0].lnlikelihood(d)
        assert got == z["lnl"][i] or abs(got - z["lnl"][i]) <= 1e-9 * abs(z["lnl"][i])
        assert mdl[-1].lnlikelihood(d) == z["lnl_exact"][i]
    if name == "mc_binorf":
        fin = np.isfinite(z["lnl"][~near])
        assert fin.sum() >= 2 and (~fin).sum() >= 2
    if "orf" in name:
        assert np.all(mg_condition(pta, mdl[2], const, z["theta"]) >= MG_COND_MIN)
