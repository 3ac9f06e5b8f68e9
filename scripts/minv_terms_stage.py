"""Whole-call time of a C5-shaped correlated model (P = 100 pulsars, 14 common
frequencies, red / DM noise 30 frequencies, fixed white noise, B = 512) whose
cross-pulsar prior has T terms, with the register (mode 0) and the LDS (mode 7)
M_g kernels.  Run under `rocprofv3 --kernel-trace --stats` for the M_g stage
itself: it is one launch of common_minv_reg_kernel / common_minv_kernel per
call (<false>: the legacy pair, T = 1; <true>: the term form).

    python scripts/minv_terms_stage.py T        (T in 1, 2, 4, 9)

T = 1: gwb hd (the legacy kernels); 2: gwb_multi hd + monopole; 4 / 9:
gwb_multi legendreorf_2 / legendreorf_7 (the identity term + 3 / 8 orders).
The per-sample cost does not depend on the TOA count with fixed white noise
(the Gram is cached), so 300 TOAs per pulsar stand for C5's 20000.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {1: {"gwb": "hd_vary_gamma_14_nfreqs"},
          2: {"gwb_multi": "hd_vary_gamma_14_nfreqs+mono_vary_gamma_14_nfreqs"},
          4: {"gwb_multi": "legendreorf_2_vary_gamma_14_nfreqs"},
          9: {"gwb_multi": "legendreorf_7_vary_gamma_14_nfreqs"}}


def main():
    from enterprise_warp_amd import synth
    T = int(sys.argv[1])
    P, B, seed = 100, 512, 100
    rng = np.random.default_rng(seed)
    psrs = []
    for i in range(P):
        v = rng.standard_normal(3)
        psrs.append(synth.make_pulsar(f"J{i:04d}+{seed:04d}", 300, seed=seed * 1000 + i, pos=v / np.linalg.norm(v),
                                      epoch_size=4))
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    terms = {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend",
             "spin_noise": "powerlaw_30_nfreqs", "dm_noise": "powerlaw_30_nfreqs"}
    wn = synth.white_noisedict(psrs, seed + 1)
    pta = synth.build_pta(psrs, terms, MODELS[T], synth.params_namespace(Tspan, True), wn)
    truth = synth.truth_values(pta, seed + 2, white=wn)
    for p in pta.params:
        if p.name.startswith("gw") and p.name.endswith("gamma"):
            truth[p.name] = 13.0 / 3.0
        elif p.name.startswith("gw_log10_A"):
            truth[p.name] = -14.3
        elif p.name == "gw_orf_legendre":
            truth[p.name] = np.zeros(p.size)
    synth.simulate_residuals(pta, truth, seed + 3)
    X = synth.near_draws(pta, truth, B, seed + 4, scale=0.05)
    n_term = len(pta.common_layout()["terms"])
    eng = pta.engine()
    for mode in (0, 7):
        eng.set_kernel_mode(mode)
        out = pta.get_lnlikelihood_batch(X)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            pta.get_lnlikelihood_batch(X)
            t.append((time.perf_counter() - t0) * 1e3)
        print(f"T = {n_term} mode {mode}: whole call B = {B} ms {np.round(t, 2)} finite {int(np.isfinite(out).sum())} of {B}",
              flush=True)
    eng.set_kernel_mode(0)


if __name__ == "__main__":
    main()
