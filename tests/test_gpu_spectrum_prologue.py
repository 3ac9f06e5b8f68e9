"""The fixed-form spectrum prologue of the product register kernel
(csrc/ewarp_dev.h chol_mfma_kernel<..., PL>; csrc/ewarp_spec.h): a launch whose
jobs all carry compact power-law records evaluates them straight-line, every
other launch keeps the interpreted staged prologue -- and both give the same
bits.

chol_lat_kernel keeps the interpreted prologue, so "latency B = 8 == batched
B = 32, bit for bit" compares the two prologues in the product library (frames
of up to eight blocks; a nine-block frame has no latency kernel: it is held to
the enterprise-order oracle and the double-double reference, and its unit
terms to those of the same pulsar in a launch that falls back).  On the
dev library (EWARP_HIP_LIB; tests/test_gpu_ab_spectrum_prologue.py runs this
file there) every case is also compared with kernel mode 14, which forces the
interpreted prologue, over all 32 rows, and the launch counters
(ewh_dev_prologue_launches) tell which prologue the batched launch took.

~300 TOAs per pulsar (the fixtures of test_gpu_front_pads.py); half prior and
half near-truth draws; the B = 8 rows are four of each."""
import ctypes as C

import numpy as np
import pytest

from enterprise_warp_amd import parameter, signals, synth
from enterprise_warp_amd.models import StandardModels
from enterprise_warp_amd.pta import PTA
from enterprise_warp_amd.signals import TimingModel

from test_gpu_front_pads import N_TOA, _c3_width, _pta

pytestmark = pytest.mark.gpu

B = 32
LAT_ROWS = np.r_[0:4, B // 2:B // 2 + 4]     # four prior and four near-truth rows


def _rows(pta, truth):
    return np.vstack([synth.prior_draws(pta, B // 2, 5), synth.near_draws(pta, truth, B // 2, 6)])


def _model(seed, per_psr, common=(), n_toa=N_TOA):
    """One pulsar per dict of per-pulsar terms; common: functions of Tspan
    returning a signal that every pulsar takes (uncorrelated: merged onto the
    red-noise columns of the same frequencies)."""
    psrs = [synth.make_pulsar(f"J{i:04d}+{seed:04d}", n_toa, seed=seed * 100 + i, epoch_size=8)
            for i in range(len(per_psr))]
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    ns = synth.params_namespace(Tspan, True)
    wn = synth.white_noisedict(psrs, seed + 1)
    models = []
    for psr, terms in zip(psrs, per_psr):
        sm = StandardModels(psr=psr, params=ns)
        m = TimingModel()
        for mk in common:
            m = m + mk(Tspan)
        for term, opt in dict({"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend"}, **terms).items():
            m = m + getattr(sm, term)(option=opt)
        models.append(m(psr))
    pta = PTA(models)
    pta.set_default_params(wn)
    truth = synth.truth_values(pta, seed + 2, white=wn)
    synth.simulate_residuals(pta, truth, seed + 3)
    return pta, truth


def _common(name, nfreqs, lgA=None, gamma=None):
    """An uncorrelated common power law `name` on nfreqs frequencies; lgA /
    gamma: a constant value, or None for a sampled parameter."""
    def make(Tspan):
        a = parameter.Uniform(-18, -12) if lgA is None else parameter.Constant(lgA)
        g = parameter.Uniform(0, 7) if gamma is None else parameter.Constant(gamma)
        spec = signals.powerlaw(log10_A=a(f"{name}_log10_A"), gamma=g(f"{name}_gamma"))
        return signals.FourierBasisGP(spec, components=nfreqs, name=name, Tspan=Tspan)
    return make


def _freespec(name, nfreqs):
    def make(Tspan):
        rho = parameter.Uniform(-9, -5, size=nfreqs)(f"{name}_log10_rho")
        return signals.FourierBasisGP(signals.free_spectrum(log10_rho=rho), components=nfreqs, name=name, Tspan=Tspan)
    return make


RN_DM = {"spin_noise": "powerlaw_6_nfreqs", "dm_noise": "powerlaw_6_nfreqs"}     # width 25: two blocks, 7 pads

# name -> (builder, the batched launch takes the fixed-form prologue)
CASES = {
    "pads7_image": (lambda: _pta([25], 12), True),                  # front order, operand image
    "pads3_stored": (lambda: _pta([29], 11), True),                 # stored order
    "c3_width_curn": (_c3_width, True),                             # eight blocks, CURN merged: two entries
    "two_common": (lambda: _model(31, [RN_DM], [_common("gw", 4), _common("gwb2", 3)]), True),    # three entries
    "const_gamma": (lambda: _model(32, [RN_DM], [_common("gw", 4, gamma=4.33)]), True),
    "const_amplitude": (lambda: _model(33, [RN_DM], [_common("gw", 4, lgA=-14.4)]), True),
    # one launch holding a power-law and a turnover pulsar of equal width: falls back
    "powerlaw_and_turnover": (lambda: _model(34, [RN_DM, {"spin_noise": "turnover_6_nfreqs",
                                                          "dm_noise": "powerlaw_6_nfreqs"}]), False),
    "free_spectrum": (lambda: _model(35, [RN_DM], [_freespec("gw", 4)]), False),
}


def _dev(eng):
    return hasattr(eng.lib, "ewh_dev_prologue_launches")


def _launches(eng):
    out = (C.c_int64 * 2)()
    assert eng.lib.ewh_dev_prologue_launches(out) == 0
    return np.array(out[:])


def _batched(pta, X, fixed_form):
    """The B = 32 result; on the dev library also: which prologue the launch
    took, and equality with the forced interpreted prologue (mode 14)."""
    eng = pta.engine()
    before = _launches(eng) if _dev(eng) else None
    got = pta.get_lnlikelihood_batch(X)
    if _dev(eng):
        took = _launches(eng) - before
        assert took[1 if fixed_form else 0] >= 1 and took[0 if fixed_form else 1] == 0, f"launches {took}"
        eng.set_kernel_mode(14)
        try:
            interp = pta.get_lnlikelihood_batch(X)
        finally:
            eng.set_kernel_mode(0)
        assert (_launches(eng) - before)[1] == took[1]            # mode 14 took the interpreted prologue
        np.testing.assert_array_equal(got, interp)
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_fixed_form_equals_interpreted(require_gpu, name):
    make, fixed_form = CASES[name]
    pta, truth = make()
    X = _rows(pta, truth)
    got = _batched(pta, X, fixed_form)
    assert np.isfinite(got[B // 2:]).all()
    assert pta.engine().lat_b_max() >= 8
    lat = pta.get_lnlikelihood_batch(X[LAT_ROWS])                  # B = 8: chol_lat_kernel, interpreted
    print(f"{name}: latency vs batched max |diff| {np.nanmax(np.abs(lat - got[LAT_ROWS])):.3e}")
    np.testing.assert_array_equal(lat, got[LAT_ROWS])


def test_nine_blocks_second_record_trip(require_gpu):
    """67 distinct spectra (34 red + 33 DM frequencies, width 135, nine
    blocks): lanes 0..2 evaluate a second record."""
    from conftest import check_accuracy, reference_lnl
    pta, truth = _pta([135], 21, 3 * N_TOA)
    sc = pta.signal_collections[0]
    width = sc.T.shape[1] - sc.n_lead_const + 1
    assert width == 135 and -(-width // 16) == 9 and (width - 1) // 2 > 64
    X = _rows(pta, truth)
    got = _batched(pta, X, True)
    ent, ext = reference_lnl(pta, X, exact="dd")
    check_accuracy(got, ent, ext, "nine blocks, 67 spectra", near=np.arange(B) >= B // 2, per_sample=True)


def _nine_block_pair():
    """The nine-block pulsar alone (fixed form), and in one launch with a
    turnover pulsar of the same width (that launch falls back): the same
    pulsar, data, Tspan and white noise in both handles."""
    n = 3 * N_TOA
    psrs = [synth.make_pulsar(f"J{i:04d}+0041", n, seed=4100 + i, epoch_size=8) for i in range(2)]
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    ns = synth.params_namespace(Tspan, True)
    wn = synth.white_noisedict(psrs, 42)

    def model(psr, spin):
        sm = StandardModels(psr=psr, params=ns)
        m = TimingModel()
        for term, opt in {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend",
                          "spin_noise": f"{spin}_34_nfreqs", "dm_noise": "powerlaw_33_nfreqs"}.items():
            m = m + getattr(sm, term)(option=opt)
        return m(psr)
    both = PTA([model(psrs[0], "powerlaw"), model(psrs[1], "turnover")])
    alone = PTA([model(psrs[0], "powerlaw")])
    for pta in (both, alone):
        pta.set_default_params(wn)
    truth = synth.truth_values(both, 43, white=wn)
    synth.simulate_residuals(both, truth, 44)
    alone._drop_engine()
    return alone, both, truth


def test_second_record_trip_bit_for_bit_on_any_library(require_gpu):
    """Bit identity of the second record trip without the dev library: the
    unit terms of the nine-block pulsar from its own launch (fixed form)
    against those from a launch it shares with a turnover pulsar
    (interpreted)."""
    alone, both, truth = _nine_block_pair()
    XB = _rows(both, truth)
    cols = [list(both.param_names).index(n) for n in alone.param_names]
    XA = np.ascontiguousarray(XB[:, cols])
    _batched(both, XB, False)
    want = both.engine().unit_terms(B)[0]
    _batched(alone, XA, True)
    got = alone.engine().unit_terms(B)[0]
    assert np.isfinite(want[B // 2:]).all()
    print(f"nine blocks, unit terms alone vs in a mixed launch: max |diff| {np.nanmax(np.abs(got - want)):.3e}")
    np.testing.assert_array_equal(got, want)


def test_nan_and_inf_parameters_stay_in_their_sample(require_gpu):
    pta, truth = _pta([25], 12)
    X = _rows(pta, truth)
    clean = _batched(pta, X, True)
    names = list(pta.param_names)
    ia = next(i for i, n in enumerate(names) if n.endswith("red_noise_log10_A"))
    ig = next(i for i, n in enumerate(names) if n.endswith("dm_gp_gamma") or n.endswith("dm_noise_gamma")
              or (n.endswith("gamma") and "red_noise" not in n))
    bad = X.copy()
    bad[1, ia] = np.nan
    bad[B // 2 + 2, ig] = np.inf
    bad[B // 2 + 3, ia] = -np.inf
    hit = np.zeros(B, dtype=bool)
    hit[[1, B // 2 + 2, B // 2 + 3]] = True
    got = _batched(pta, bad, True)
    lat = pta.get_lnlikelihood_batch(bad[LAT_ROWS])                # rows 1, 18 and 19 are among them
    print("bad rows:", got[hit], "latency:", lat[hit[LAT_ROWS]])
    assert not np.isfinite(got[hit]).any()
    np.testing.assert_array_equal(got[~hit], clean[~hit])
    np.testing.assert_array_equal(lat, got[LAT_ROWS])


def test_unit_range_starting_inside_a_pulsar(require_gpu):
    """ewh_lnl_units_device over [0, cut) and [cut, P B) with u0 % B != 0 (as
    a sharded run splits the units): the two partial sums add up to the
    full-range result.  Two pulsars, so each sample's sum has two terms and is
    the same in either order: equal bits."""
    import torch
    pta, truth = _pta([25, 25], 15)
    X = _rows(pta, truth)
    full = pta.get_lnlikelihood_batch(X)
    eng = pta.engine()
    th = torch.from_numpy(X).cuda()
    s = torch.cuda.current_stream().cuda_stream
    for cut in (11, B + 21, 2 * B - 1):
        parts = []
        for u0, u1 in ((0, cut), (cut, 2 * B)):
            part = torch.zeros(B, dtype=torch.float64, device="cuda")
            eng.lnl_units_device(th.data_ptr(), B, u0, u1, part.data_ptr(), s)
            torch.cuda.synchronize()
            parts.append(part.cpu().numpy())
        print(f"cut {cut}: max |sum of parts - full| {np.nanmax(np.abs(parts[0] + parts[1] - full)):.3e}")
        np.testing.assert_array_equal(parts[0] + parts[1], full)
