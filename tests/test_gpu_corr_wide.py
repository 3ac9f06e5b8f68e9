"""The correlated common process past 31 common columns (15 frequencies) and
the optimal statistic up to 63 columns on the GPU, on the fixtures of
tests/golden/make_corr_wide.py (kept block KD = 48 with pad columns, 47 of
48, 63 of 64, the varying-white-noise layout at KD = 64, and 180 columns at
KD = 192) and on small synthetic models that reach each register
instantiation chol_mfma_kernel<NB, KEEP = 3 / 4>."""
import functools

import numpy as np
import pytest

from conftest import check_accuracy, check_parity, load_golden, oracle_lnl, strict_tolerance
from enterprise_warp_amd import _lib, synth
from oracle import enterprise_ref as ref

pytestmark = pytest.mark.gpu

C5_WIDE = ["c5_f16", "c5_f23", "c5_f31", "c5_f24v", "c5_f90"]
OS_RTOL = 1e-7            # tests/test_optstat.py


@functools.lru_cache(maxsize=None)
def golden(name):
    return load_golden(name, full=True)


def reduced_blocks(pta):
    """(nb, keep) of each pulsar's fixed-white-noise reduced matrix: own
    columns in whole 16-column blocks, then the kept common columns + r."""
    out = []
    for L in pta.layout():
        nloc = L["T"].shape[1] - L["n_lead"] - L["n_common"]
        keep = (L["n_common"] + 1 + 15) // 16
        out.append(((nloc + 15) // 16 + keep, keep))
    return out


@pytest.mark.parametrize("name", C5_WIDE)
def test_parity(require_gpu, name):
    """The criterion of test_gpu_parity.py on c5_small: near-truth draws at
    strict against the enterprise-order and the near-exact values, prior
    draws no less accurate than enterprise's order, the -inf pattern equal."""
    pta, z = golden(name)
    got = pta.get_lnlikelihood_batch(z["theta"])
    fin = np.isfinite(got) & np.isfinite(z["lnl_dev"])
    print(f"{name}: |gpu - lnl_dev| / strict {np.abs(got[fin] - z['lnl_dev'][fin]) / strict_tolerance(z['lnl_dev'][fin])}")
    check_accuracy(got, z["lnl"], z["lnl_exact"], name, near=z["near"])


@pytest.mark.parametrize("name", ["c5_f16", "c5_f31", "c5_f24v"])
def test_wide_route_matches_default(require_gpu, name):
    """Kernel mode 27 (every factorisation by chol_wide_kernel) against the
    default route, within strict."""
    pta, z = golden(name)
    X = z["theta"]
    a = pta.get_lnlikelihood_batch(X)
    eng = pta.engine()
    eng.set_kernel_mode(27)
    try:
        b = pta.get_lnlikelihood_batch(X)
    finally:
        eng.set_kernel_mode(0)
    check_parity(b, a, f"{name}: mode 27 vs default")


# common frequencies, own red / DM frequencies -> (nb, keep) of every pulsar:
# each register instantiation with KEEP = 3 / 4 that is built, the two that
# spill (<7, 3>, <7, 4>: chol_wide's) and a kept size with no phase-3 room
REGISTER_CASES = [(16, 10, (5, 3)), (23, 23, (6, 3)), (23, 27, (7, 3)), (23, 31, (8, 3)), (23, 34, (9, 3)),
                  (31, 10, (6, 4)), (31, 20, (7, 4)), (31, 31, (8, 4)), (31, 35, (9, 4))]


@pytest.mark.parametrize("ncommon, nown, blocks", REGISTER_CASES)
def test_partial_routes_against_wide_and_oracle(require_gpu, ncommon, nown, blocks):
    """3 pulsars x 300 TOAs whose reduced matrices have exactly `blocks` =
    (nb, keep): near-truth draws at strict against the enterprise-order
    oracle on the default route (chol_mfma_kernel<nb, keep> where it is
    built) and on chol_wide_kernel (mode 27), and the two within strict of
    each other."""
    c5 = synth.config_c5(n_psr=3, n_toa=300, seed=1000 + 40 * ncommon + nown, epoch_size=4,
                         gwb=f"hd_vary_gamma_{ncommon}_nfreqs", nfreqs=nown)
    pta = c5.pta
    assert reduced_blocks(pta) == [blocks] * 3
    X = synth.near_draws(pta, c5.truth, 4, 5)
    want = oracle_lnl(pta, X)
    a = pta.get_lnlikelihood_batch(X)
    eng = pta.engine()
    assert eng.keep_dim() == 16 * blocks[1]
    eng.set_kernel_mode(27)
    try:
        b = pta.get_lnlikelihood_batch(X)
    finally:
        eng.set_kernel_mode(0)
    check_parity(a, want, f"{blocks} default vs oracle")
    check_parity(b, want, f"{blocks} wide vs oracle")
    check_parity(b, a, f"{blocks} wide vs default")


@pytest.mark.parametrize("name", ["c5_f31", "c5_f90"])
def test_batch_sizes_bit_identical(require_gpu, name):
    """Chunks of up to 12 samples factor Sigma_c right-looking, larger ones
    left-looking (fused with the panel from 64 on): the same lnL bit for bit."""
    pta, z = golden(name)
    X = z["theta"]
    left = pta.get_lnlikelihood_batch(np.vstack([X] * 8))[:len(X)]
    for B in (1, 12, 13):
        got = np.concatenate([pta.get_lnlikelihood_batch(X[i:i + B]) for i in range(0, len(X), B)])
        np.testing.assert_array_equal(got, left)


def test_device_list_bit_identical(require_gpu):
    pta, z = golden("c5_f31")
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
    """ewh_corr_partial_device on the pulsar ranges [0, 1) and [1, 3) into
    pulsar-major buffers of ewh_keep_dim()^2 doubles per unit, then
    ewh_corr_finish_device: the single-handle lnL bit for bit."""
    import torch
    pta, z = golden("c5_f31")
    X = np.ascontiguousarray(z["theta"])
    one = pta.get_lnlikelihood_batch(X)
    eng = pta.engine(devices=[0])
    kd = eng.keep_dim()
    assert kd == 64
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
    pta, z = golden("c5_f16")
    X = z["theta"].copy()
    clean = pta.get_lnlikelihood_batch(X)
    X[5, 3] = np.nan
    got = pta.get_lnlikelihood_batch(X)
    assert got[5] == -np.inf
    rest = np.arange(len(X)) != 5
    check_parity(got[rest], clean[rest], "c5_f16 rows beside a NaN row")


# --------------------------------------------------------------------------
# optimal statistic
# --------------------------------------------------------------------------
@pytest.mark.parametrize("orf", ["hd", "monopole"])
def test_os_at_62_columns(require_gpu, orf):
    """c3_f31 (CURN at 31 frequencies): os_xz_wide_kernel against the oracle
    on the near-truth draws, with the assertions of test_optstat.py."""
    from enterprise_warp_amd.optstat import OptimalStatistic
    pta, z = golden("c3_f31")
    const_ = pta.constant_values()
    o = ref.OraclePTA([c.psr for c in pta.signal_collections], pta.oracle_terms(), fixed_params=const_)
    ost = OptimalStatistic(pta, orf=orf)
    draws = z["theta"][z["near"]]
    OS, OS_sig, rho, sig = ost.compute_noise_marginalised_os(draws, want_pairs=True)
    iu = np.triu_indices(len(pta.signal_collections), 1)
    for i, x in enumerate(draws):
        d = dict(const_)
        d.update(pta.map_params(x))
        xi, r_w, s_w, os_w, oss_w = ref.optimal_statistic(o, d, orf=orf)
        r_g, s_g = rho[i][iu], sig[i][iu]
        print(f"{orf} draw {i}: rho {np.max(np.abs(r_g - r_w)) / np.max(np.abs(r_w)):.2e} "
              f"sig {np.max(np.abs(s_g - s_w) / s_w):.2e} OS {abs(OS[i] - os_w) / max(abs(os_w), oss_w):.2e} "
              f"OS_sig {abs(OS_sig[i] - oss_w) / oss_w:.2e} (bound {OS_RTOL:.0e})")
        assert np.max(np.abs(r_g - r_w)) <= OS_RTOL * np.max(np.abs(r_w)), (i, r_g, r_w)
        assert np.max(np.abs(s_g - s_w) / s_w) <= OS_RTOL
        assert abs(OS[i] - os_w) <= OS_RTOL * max(abs(os_w), oss_w)
        assert abs(OS_sig[i] - oss_w) <= OS_RTOL * oss_w


def test_os_above_the_cap_is_refused(require_gpu):
    """32 CURN frequencies are 64 common columns, one frequency past
    EWH_OS_MAX_COMMON_COLS = 63: ewh_create's EWH_E_UNSUPPORTED reaches the
    caller as _lib.EngineError naming the cap."""
    from enterprise_warp_amd.optstat import OptimalStatistic
    psrs = synth.c3_pulsars(n_psr=2, n_min=300, n_max=320, seed=332, epoch_size=4)
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    wn = synth.white_noisedict(psrs, 333)
    terms = {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend", "spin_noise": "powerlaw_10_nfreqs"}
    pta = synth.build_pta(psrs, terms, {"gwb": "vary_gamma_32_nfreqs"}, synth.params_namespace(Tspan, True), wn)
    with pytest.raises(_lib.EngineError, match="EWH_OS_MAX_COMMON_COLS = 63"):
        OptimalStatistic(pta, orf="hd")
