"""The operand images of the fixed-white-noise reduced matrix (csrc/ewarp_dev.h
img_index): chol_mfma_kernel reads S_p from a copy laid out as its registers,
built once at create and again at every ewh_set_fixed_white
(white.hip operand_image_kernel).  chol_lat_kernel keeps reading the stored
S_p, so "latency == batched, bit for bit" compares a stored-fed kernel with an
image-fed one, and "in-place == fresh handle" compares an image that was
rebuilt with one that was built once: a stale or misplaced image fails both.

~300 TOAs per pulsar, B = 32 (chol_mfma_kernel) and B = 8 (chol_lat_kernel);
the frames are those of test_gpu_front_pads.py (7 pads: the front-order image;
3 pads: the stored-order image only), and one eight-block frame at C3's width
(608 TOAs, as there).

White noise is fixed per handle (ewh_pta_desc.white_fixed), not per pulsar: a
PTA with one constant-noise and one sampled-noise pulsar is a varying-noise
handle whose two launches both read the per-sample slots (no image).  The
image launch beside a stored launch in one call is the fixed handle with a
delay pulsar, test_gpu_delay.py::test_fixed_white_mixed_handle."""
import numpy as np
import pytest

from enterprise_warp_amd import synth
from enterprise_warp_amd.models import StandardModels
from enterprise_warp_amd.pta import PTA
from enterprise_warp_amd.signals import TimingModel

from test_gpu_front_pads import N_TOA, _c3_width, _pta

pytestmark = pytest.mark.gpu

B = 32


def _new_white(pta, seed):
    rng = np.random.default_rng(seed)
    return {k: (v * rng.uniform(0.95, 1.05) if k.endswith("_efac") else v + rng.uniform(-0.2, 0.2))
            for k, v in pta.constant_values().items() if k.endswith(("_efac", "_log10_tnequad", "_log10_ecorr"))}


def _rows(pta, truth):
    return np.vstack([synth.prior_draws(pta, B // 2, 5), synth.near_draws(pta, truth, B // 2, 6)])


@pytest.mark.parametrize("width,pads,seed", [(25, 7, 12), (29, 3, 11)])
def test_white_noise_reset_rebuilds_image(require_gpu, width, pads, seed):
    pta, truth = _pta([width], seed)
    sc = pta.signal_collections[0]
    assert 32 - (sc.T.shape[1] - sc.n_lead_const + 1) == pads
    X = _rows(pta, truth)
    eng = pta.engine()
    before = pta.get_lnlikelihood_batch(X)
    new = _new_white(pta, 7)
    pta.set_default_params(new)
    assert pta.engine() is eng                               # in place (ewh_set_fixed_white)
    got = pta.get_lnlikelihood_batch(X)                      # B = 32: chol_mfma_kernel, from the image
    assert eng.lat_b_max() >= 8
    lat = pta.get_lnlikelihood_batch(X[:8])                  # B = 8: chol_lat_kernel, from S
    assert np.isfinite(got).any() and not np.array_equal(got, before)
    fresh, _ = _pta([width], seed)
    fresh.set_default_params(new)
    want = fresh.get_lnlikelihood_batch(X)
    print(f"pads {pads}: in place vs fresh max |diff| {np.nanmax(np.abs(got - want)):.3e}, "
          f"latency vs batched {np.nanmax(np.abs(lat - got[:8])):.3e}")
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(lat, got[:8])


def test_fixed_and_varying_noise_pulsars(require_gpu):
    """One pulsar with constant and one with sampled white noise in one
    handle, against the enterprise-order oracle and the double-double
    reference per sample, as test_gpu_front_pads.py."""
    from conftest import check_accuracy, reference_lnl
    psrs = [synth.make_pulsar(f"J{i:04d}+0031", N_TOA, seed=3100 + i, epoch_size=8) for i in range(2)]
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    wn = synth.white_noisedict(psrs[:1], 32)
    models = []
    for psr, fixed in zip(psrs, (True, False)):
        sm = StandardModels(psr=psr, params=synth.params_namespace(Tspan, fixed))
        m = TimingModel()
        for term, opt in {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend",
                          "spin_noise": "powerlaw_6_nfreqs", "dm_noise": "powerlaw_6_nfreqs"}.items():
            m = m + getattr(sm, term)(option=opt)
        models.append(m(psr))
    pta = PTA(models)
    pta.set_default_params(wn)
    assert not pta.white_fixed() and pta.constant_values()
    truth = synth.truth_values(pta, 33, white=wn)
    synth.simulate_residuals(pta, truth, 34)
    X = _rows(pta, truth)
    got = pta.get_lnlikelihood_batch(X)
    ent, ext = reference_lnl(pta, X, exact="dd")
    check_accuracy(got, ent, ext, "fixed + varying noise", near=np.arange(B) >= B // 2, per_sample=True)


def test_c3_width_latency_equals_batched_after_reset(require_gpu):
    pta, truth = _c3_width()
    X = _rows(pta, truth)
    eng = pta.engine()
    before = pta.get_lnlikelihood_batch(X)
    pta.set_default_params(_new_white(pta, 8))
    assert pta.engine() is eng
    got = pta.get_lnlikelihood_batch(X)
    assert eng.lat_b_max() >= 8
    lat = pta.get_lnlikelihood_batch(X[:8])
    assert np.isfinite(got).any() and not np.array_equal(got, before)
    print(f"c3 width: latency vs batched max |diff| {np.nanmax(np.abs(lat - got[:8])):.3e}")
    np.testing.assert_array_equal(lat, got[:8])
