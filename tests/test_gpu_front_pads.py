"""The front-pad working order of the register Cholesky kernels
(csrc/ewarp_dev.h front_src): the pads of the reduced frame are factored
first, and the k-slices of block row 0 that hold only pads (DEAD = pads / 4)
are not issued.

Fixed white noise, ~300 TOAs, through the public batch entry.  Two-block
frames (32 wide) at every pad count class, one eight-block frame at C3's
width, six-block frames (where the one-dead-slice instantiation is not built
and both kernels must fall back to the stored order together), and handles
whose pulsars differ in their pad counts (the launch then takes the smallest
DEAD and the wider-padded pulsar pivots its further pads as the identity rows
they are).  A launch without a dead slice (under 4 pads) runs the stored
order.  Reduced width = 2 (red + DM frequencies) + 1 (the residual column).

  pads  width  case
     3     29  no dead slice, the guard case (the stored order)
     7     25  C3's case: one dead slice plus three pad rows in the next
    11     21  DEAD 2
    15     17  DEAD 3
     7    121  C3's own width (eight blocks)
     7     89  six blocks, one dead slice: stored order in both kernels
    11     85  six blocks, DEAD 2

Per case: prior and near-truth draws at B = 32 (chol_mfma_kernel) against the
enterprise-order oracle and the double-double reference by check_accuracy per
sample, and B = 8 (chol_lat_kernel) against rows 0..7 of the B = 32 result bit
for bit.
"""
import numpy as np
import pytest

from enterprise_warp_amd import synth
from enterprise_warp_amd.models import StandardModels
from enterprise_warp_amd.pta import PTA
from enterprise_warp_amd.signals import TimingModel

pytestmark = pytest.mark.gpu

N_TOA = 304
B = 32


def _pta(widths, seed, n_toa=N_TOA):
    """One pulsar per reduced width (odd, 2 (n_red + n_dm) + 1); red and DM
    noise share the frequencies as evenly as the width allows."""
    psrs = [synth.make_pulsar(f"J{i:04d}+{seed:04d}", n_toa, seed=seed * 100 + i, epoch_size=8)
            for i in range(len(widths))]
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    ns = synth.params_namespace(Tspan, True)
    wn = synth.white_noisedict(psrs, seed + 1)
    models = []
    for psr, w in zip(psrs, widths):
        nf = (w - 1) // 2
        n_red = (nf + 1) // 2
        terms = {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend",
                 "spin_noise": f"powerlaw_{n_red}_nfreqs", "dm_noise": f"powerlaw_{nf - n_red}_nfreqs"}
        sm = StandardModels(psr=psr, params=ns)
        m = TimingModel()
        for term, opt in terms.items():
            m = m + getattr(sm, term)(option=opt)
        models.append(m(psr))
    pta = PTA(models)
    pta.set_default_params(wn)
    truth = synth.truth_values(pta, seed + 2, white=wn)
    synth.simulate_residuals(pta, truth, seed + 3)
    return pta, truth


def _c3_width():
    # (608 TOAs: at ~300 the 120-column model is so ill-conditioned on prior
    # draws that the enterprise-order oracle itself returns -inf where the
    # double-double reference is finite, and cannot serve as a reference)
    cfg = synth.config_c3(n_psr=1, n_min=2 * N_TOA, n_max=2 * N_TOA, seed=71, epoch_size=8)
    return cfg.pta, cfg.truth


CASES = {
    "pads3": lambda: _pta([29], 11),
    "pads7": lambda: _pta([25], 12),
    "pads11": lambda: _pta([21], 13),
    "pads15": lambda: _pta([17], 14),
    "pads7x2": lambda: _pta([25, 25], 15),
    "pads11x2": lambda: _pta([21, 21], 16),
    "mixed_7_15": lambda: _pta([25, 17], 17),        # launch DEAD 1; the second pulsar has 15 pads
    "mixed_11_3": lambda: _pta([21, 29], 18),        # no common dead slice: stored order; the first pulsar has 11 pads
    "c3_width": _c3_width,
    # (608 TOAs, as c3_width: ~100 columns on ~300 TOAs leave the oracle at -inf on prior draws)
    "nb6_pads7": lambda: _pta([89], 19, 2 * N_TOA),
    "nb6_pads11": lambda: _pta([85], 20, 2 * N_TOA),
}
# (pads, blocks) of each pulsar's reduced frame, as the case intends it
FRAMES = {"pads3": [(3, 2)], "pads7": [(7, 2)], "pads11": [(11, 2)], "pads15": [(15, 2)],
          "pads7x2": [(7, 2)] * 2, "pads11x2": [(11, 2)] * 2, "mixed_7_15": [(7, 2), (15, 2)],
          "mixed_11_3": [(11, 2), (3, 2)], "c3_width": [(7, 8)], "nb6_pads7": [(7, 6)], "nb6_pads11": [(11, 6)]}


@pytest.mark.parametrize("name", list(CASES))
def test_front_pads(require_gpu, name):
    from conftest import check_accuracy, reference_lnl
    pta, truth = CASES[name]()
    # the frames are the ones the case is about: reduced width = columns past
    # the timing model + r, in 16-wide blocks
    for sc, (pads, nb) in zip(pta.signal_collections, FRAMES[name]):
        width = sc.T.shape[1] - sc.n_lead_const + 1
        assert (16 * nb - width, -(-width // 16)) == (pads, nb), f"{name}: reduced width {width}"
    X = np.vstack([synth.prior_draws(pta, B // 2, 5), synth.near_draws(pta, truth, B // 2, 6)])
    near = np.arange(B) >= B // 2
    got = pta.get_lnlikelihood_batch(X)                      # B = 32: chol_mfma_kernel
    assert pta.engine().lat_b_max() >= 8
    lat = pta.get_lnlikelihood_batch(X[:8])                  # B = 8: chol_lat_kernel
    ent, ext = reference_lnl(pta, X, exact="dd")
    check_accuracy(got, ent, ext, f"front pads {name}", near=near, per_sample=True)
    print(f"{name}: latency vs batched max |diff| {np.nanmax(np.abs(lat - got[:8])):.3e}")
    np.testing.assert_array_equal(lat, got[:8])
