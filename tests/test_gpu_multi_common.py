"""Several correlated common processes and sampled-parameter ORFs on the GPU
(the term form of include/ewarp_hip.h: M_g = sum_t coef_t phi_t(g) B_t +
diag(own), common_minv_kernel<true> / common_minv_reg_kernel<true>), on the
fixtures of tests/golden/make_multi_common.py and on small synthetic models."""
import functools

import numpy as np
import pytest

from conftest import check_accuracy, check_parity, load_golden, oracle_lnl, strict_tolerance
from enterprise_warp_amd import models, synth

pytestmark = pytest.mark.gpu

MULTI = ["mc_hd_mono", "mc_three", "mc_f31", "mc_varwn", "mc_binorf", "mc_legendre"]


@functools.lru_cache(maxsize=None)
def golden(name):
    return load_golden(name, full=True)


@functools.lru_cache(maxsize=None)
def default_lnl(name):
    pta, z = golden(name)
    return pta.get_lnlikelihood_batch(z["theta"])


@pytest.mark.parametrize("name", MULTI)
def test_parity(require_gpu, name):
    """Near-truth draws at strict against the enterprise-order and the
    near-exact values, prior draws no less accurate than enterprise's order,
    the -inf pattern (indefinite sampled ORFs) equal."""
    pta, z = golden(name)
    got = default_lnl(name)
    fin = np.isfinite(got) & np.isfinite(z["lnl_dev"])
    print(f"{name}: |gpu - lnl_dev| / strict {np.abs(got[fin] - z['lnl_dev'][fin]) / strict_tolerance(z['lnl_dev'][fin])}")
    check_accuracy(got, z["lnl"], z["lnl_exact"], name, near=z["near"])


@pytest.mark.parametrize("mode", [7, 27])
@pytest.mark.parametrize("name", ["mc_hd_mono", "mc_f31", "mc_binorf"])
def test_kernel_modes_match_default(require_gpu, name, mode):
    """Mode 7 (the LDS M_g kernel, common_minv_kernel<true>) and mode 27
    (chol_wide everywhere) against the default route, within strict."""
    pta, z = golden(name)
    a = default_lnl(name)
    eng = pta.engine()
    eng.set_kernel_mode(mode)
    try:
        b = pta.get_lnlikelihood_batch(z["theta"])
    finally:
        eng.set_kernel_mode(0)
    check_parity(b, a, f"{name}: mode {mode} vs default")


class SplitHD:
    """Test-only ORF: Hellings-Downs as two terms (0.5, Gamma_HD) + (0.5,
    Gamma_HD) -- the same model as the name "hd", on the general kernels."""

    def terms(self, positions, pref):
        G = models.orf_matrix("hd", positions)
        return [((-1, 0.5), G), ((-1, 0.5), G.copy())]


@pytest.mark.parametrize("name", ["c5_small", "c5_f31"])
def test_general_kernel_against_established_results(require_gpu, name):
    """The established HD fixtures through the general kernels: the stored
    references by the accuracy criterion, the legacy route at strict (not
    bitwise: the legacy element orf * phi + own may be one contracted fma)."""
    pta, z = load_golden(name, full=True)
    legacy = pta.get_lnlikelihood_batch(z["theta"])
    split, orf = load_golden(name, full=True)[0], SplitHD()
    for c in split.signal_collections:
        c.commons[0]["orf"] = orf
    cl = split.common_layout()
    assert cl["orf"] is None and len(cl["terms"]) == 2
    got = split.get_lnlikelihood_batch(z["theta"])
    check_accuracy(got, z["lnl"], z["lnl_exact"], f"{name} as two terms", near=z["near"])
    check_parity(got, legacy, f"{name}: two terms vs the legacy route")


@functools.lru_cache(maxsize=None)
def many_pulsars(P):
    """P pulsars x 40 TOAs, HD 2 freqs + monopole 2 freqs, red and DM noise 2
    freqs (the red noise merges onto the common columns, the DM columns are
    the pulsar's own block): (pta, 4 near-truth draws, enterprise-order lnL)."""
    seed = 900 + P
    rng = np.random.default_rng(seed)
    psrs = []
    for i in range(P):
        v = rng.standard_normal(3)
        psrs.append(synth.make_pulsar(f"J{i:04d}+{seed:04d}", 40, seed=seed * 1000 + i, pos=v / np.linalg.norm(v),
                                      epoch_size=4))
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    ns = synth.params_namespace(Tspan, True)
    wn = synth.white_noisedict(psrs, seed + 1)
    terms = {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend", "spin_noise": "powerlaw_2_nfreqs",
             "dm_noise": "powerlaw_2_nfreqs"}
    pta = synth.build_pta(psrs, terms, {"gwb_multi": "hd_vary_gamma_2_nfreqs+mono_vary_gamma_2_nfreqs"}, ns, wn)
    truth = synth.truth_values(pta, seed + 2, white=wn)
    truth.update(gw_log10_A_hd=-14.3, gw_hd_gamma=13.0 / 3.0, gw_log10_A_mono=-14.8, gw_mono_gamma=13.0 / 3.0)
    synth.simulate_residuals(pta, truth, seed + 3)
    X = synth.near_draws(pta, truth, 4, seed + 4)
    return pta, X, oracle_lnl(pta, X)


@pytest.mark.parametrize("mode", [0, 7])
@pytest.mark.parametrize("P", [20, 70])
def test_register_kernel_beyond_one_row_group(require_gpu, P, mode):
    """P = 20 gives each wave more than one live row register, P = 70 reaches
    the second column half (cc = 1) of common_minv_reg_kernel<true>; mode 7
    runs the same models on the LDS kernel."""
    pta, X, want = many_pulsars(P)
    eng = pta.engine()
    eng.set_kernel_mode(mode)
    try:
        got = pta.get_lnlikelihood_batch(X)
    finally:
        eng.set_kernel_mode(0)
    check_parity(got, want, f"P = {P}, mode {mode} vs the enterprise-order oracle")


@pytest.mark.parametrize("name", ["mc_three", "mc_binorf"])
def test_batch_sizes_bit_identical(require_gpu, name):
    pta, z = golden(name)
    X = z["theta"]
    left = pta.get_lnlikelihood_batch(np.vstack([X] * 8))[:len(X)]
    for B in (1, 12, 13):
        got = np.concatenate([pta.get_lnlikelihood_batch(X[i:i + B]) for i in range(0, len(X), B)])
        np.testing.assert_array_equal(got, left)


@pytest.mark.parametrize("name", ["mc_three", "mc_binorf"])
def test_device_list_bit_identical(require_gpu, name):
    pta, z = golden(name)
    X = z["theta"]
    one = pta.get_lnlikelihood_batch(X)
    try:
        eng = pta.engine(devices=[0, 0])
        assert eng.num_devices() == 2
        np.testing.assert_array_equal(pta.get_lnlikelihood_batch(X), one)
        np.testing.assert_array_equal(pta.get_lnlikelihood_batch(X[:1]), one[:1])   # (B < contexts: pulsars split)
    finally:
        pta.engine(devices=[0])


def test_exchange_protocol(require_gpu):
    """ewh_corr_partial_device on two pulsar ranges, then
    ewh_corr_finish_device: the single-handle lnL bit for bit."""
    import torch
    pta, z = golden("mc_three")
    X = np.ascontiguousarray(z["theta"])
    one = pta.get_lnlikelihood_batch(X)
    eng = pta.engine(devices=[0])
    kd = eng.keep_dim()
    assert kd == 16
    P, B = len(pta.signal_collections), len(X)
    th = torch.from_numpy(X).cuda()
    keep = torch.zeros((P, B, kd, kd), dtype=torch.float64, device="cuda")
    local = torch.zeros((P, B), dtype=torch.float64, device="cuda")
    out = torch.zeros(B, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for p0, p1 in ((0, 1), (1, P)):
        eng.corr_partial_device(th.data_ptr(), B, p0, p1, keep.data_ptr(), local.data_ptr(), s)
    eng.corr_finish_device(th.data_ptr(), B, keep.data_ptr(), local.data_ptr(), out.data_ptr(), s)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), one)


def test_nan_row(require_gpu):
    """A NaN ORF value (row 5) or amplitude (row 9) gives -inf on that row and
    leaves every other row as it was."""
    pta, z = golden("mc_binorf")
    X = z["theta"].copy()
    clean = pta.get_lnlikelihood_batch(X)
    assert np.isfinite(clean[5]) and np.isfinite(clean[9])
    X[5, pta.param_names.index("gw_orf_bin_2")] = np.nan
    X[9, pta.param_names.index("gw_log10_A_orf")] = np.nan
    got = pta.get_lnlikelihood_batch(X)
    assert got[5] == -np.inf and got[9] == -np.inf
    rest = ~np.isin(np.arange(len(X)), (5, 9))
    np.testing.assert_array_equal(got[rest], clean[rest])


def test_more_than_sixteen_terms_is_refused(require_gpu):
    pta, _, _ = many_pulsars(20)
    psrs = [c.psr for c in pta.signal_collections][:3]
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    wide = synth.build_pta(psrs, {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend"},
                           {"gwb_multi": "legendreorf_16_vary_gamma_2_nfreqs"}, synth.params_namespace(Tspan, True),
                           {k: v for k, v in pta.constant_values().items() if v is not None})
    with pytest.raises(NotImplementedError, match="at most 16"):
        wide.engine()
