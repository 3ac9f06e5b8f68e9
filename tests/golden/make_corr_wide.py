"""Generate the golden vectors of the correlated common process past 15
frequencies (more than 31 common columns per pulsar) and of the optimal
statistic at 31 frequencies (CPU only; seconds per fixture).

    python tests/golden/make_corr_wide.py [name prefix ...]

Same .npz format and the same five orderings as make_golden.py (its dump /
oracle_lnl are used as they are): 8 prior draws + 8 near-truth draws each.
The shapes are the smallest that reach each boundary of the kept common block
(KD = 16 ceil((2 nfreq + 1) / 16) columns: the common columns, pads, r):

  c5_f16   3 psr x 300 TOAs, HD 16 freqs: 32 columns, KD = 48 with pad columns
  c5_f23   23 freqs: 47 of KD = 48, the kept block full but for one pad
  c5_f31   31 freqs: 63 of KD = 64, the last width of the register kernel
  c5_f24v  3 psr x 400 TOAs, 24 freqs, red / DM 30 freqs, VARYING white noise:
           the per-sample contraction into the kept layout
  c5_f90   2 psr x 600 TOAs, 90 freqs: 180 columns, KD = 192 (the reference's
           default count for a ~15 yr span with red_general_freqs tobs_60days)
  c3_f31   CURN 31 freqs, 3 psr x 300-400 TOAs: the optimal statistic at 62
           columns (residuals simulated at the truth)

The seeds below were fixed on the CPU, before any device run.  One was moved
there: c5_f31's first prior seed (311, and 313 after it) drew points on which
enterprise's order returns -inf while the extended-precision value is finite
-- the two references disagree on the -inf pattern, so the accuracy criterion
of the device tests (conftest.check_accuracy) is not defined on them -- and
the next seed on which the references agree (314) was taken.  main() refuses to write
a fixture on which they disagree.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from enterprise_warp_amd import synth  # noqa: E402
from make_golden import dump, recipe_of  # noqa: E402

# name -> config_c5 arguments, (prior seed, near seed)
C5_WIDE = {
    "c5_f16": (dict(n_psr=3, n_toa=300, seed=160, gwb="hd_vary_gamma_16_nfreqs", nfreqs=10), (161, 162)),
    "c5_f23": (dict(n_psr=3, n_toa=300, seed=230, gwb="hd_vary_gamma_23_nfreqs", nfreqs=10), (231, 232)),
    "c5_f31": (dict(n_psr=3, n_toa=300, seed=310, gwb="hd_vary_gamma_31_nfreqs", nfreqs=10), (314, 312)),
    "c5_f24v": (dict(n_psr=3, n_toa=400, seed=240, gwb="hd_vary_gamma_24_nfreqs", nfreqs=30, fixed_white=False),
                (241, 242)),
    "c5_f90": (dict(n_psr=2, n_toa=600, seed=900, gwb="hd_vary_gamma_90_nfreqs", nfreqs=10), (901, 902)),
}
CORR_WIDE_NAMES = list(C5_WIDE) + ["c3_f31"]


def build_c5(name):
    """(pta, recipe, theta) of one c5_* fixture."""
    kw, (s_prior, s_near) = C5_WIDE[name]
    c5 = synth.config_c5(epoch_size=4, **kw)
    X = np.vstack([synth.prior_draws(c5.pta, 8, s_prior), synth.near_draws(c5.pta, c5.truth, 8, s_near)])
    return c5.pta, recipe_of(c5, c5.terms, c5.common, kw.get("fixed_white", True)), X


def build_c3_f31():
    """(pta, recipe, theta): CURN at 31 frequencies merged with 10-frequency
    red noise, fixed white noise, residuals simulated at the truth."""
    seed = 331
    psrs = synth.c3_pulsars(n_psr=3, n_min=300, n_max=400, seed=seed, epoch_size=4)
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    ns = synth.params_namespace(Tspan, True)
    wn = synth.white_noisedict(psrs, seed + 1)
    terms = {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend",
             "spin_noise": "powerlaw_10_nfreqs", "dm_noise": "powerlaw_10_nfreqs"}
    common = {"gwb": "vary_gamma_31_nfreqs"}
    pta = synth.build_pta(psrs, terms, common, ns, wn)
    truth = synth.truth_values(pta, seed + 2, white=wn)
    synth.simulate_residuals(pta, truth, seed + 3)
    X = np.vstack([synth.prior_draws(pta, 8, seed + 4), synth.near_draws(pta, truth, 8, seed + 5)])
    recipe = {"per_psr_terms": terms, "common_terms": common, "Tspan": float(Tspan), "fixed_white": True,
              "noisedict": wn}
    return pta, recipe, X


def build(name):
    return build_c3_f31() if name == "c3_f31" else build_c5(name)


def main():
    only = sys.argv[1:]
    for name in CORR_WIDE_NAMES:
        if only and not any(name.startswith(o) for o in only):
            continue
        pta, recipe, X = build(name)
        dump(name, pta, recipe, X)
        z = np.load(os.path.join(HERE, name + ".npz"))
        if not np.array_equal(np.isfinite(z["lnl"]), np.isfinite(z["lnl_exact"])):
            os.remove(os.path.join(HERE, name + ".npz"))
            raise SystemExit(f"{name}: the enterprise-order and near-exact references disagree on -inf")


if __name__ == "__main__":
    main()
