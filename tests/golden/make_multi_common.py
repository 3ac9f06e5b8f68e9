"""Generate the golden vectors of several correlated common processes and of
sampled-parameter ORFs (StandardModels.gwb_multi; CPU only, seconds to a
minute per fixture).

    python tests/golden/make_multi_common.py [name prefix ...]

Same .npz keys as make_golden.py (8 prior draws + 8 near-truth draws, the
five orderings), loadable by conftest.load_golden through
common_terms = {"gwb_multi": ...}.  make_golden.dump is NOT used: its
near-exact reference (oracle/device_order_ref.py finish) reads one ORF and
would silently drop the others; the references here are the subclasses of
tests/_common_ref.py.

  mc_hd_mono   3 psr x 300 TOAs, HD 5 freqs + monopole 3 freqs, red / DM 10
               freqs, fixed white noise: the union of the columns (10), the
               monopole's spectrum zero on the last four; KD = 16
  mc_three     4 x 300, CURN 6 + HD 6 + monopole 6 + dipole 4
  mc_f31       3 x 300, HD 31 + monopole 31: 63 of KD = 64 (the register
               partial kernel's last width)
  mc_varwn     3 x 400, HD 8 + dipole 8, VARYING white noise
  mc_binorf    4 x 300, binned ORF (varorf), 5 freqs: six pairs over several
               of the seven bins
  mc_legendre  4 x 300, Legendre ORF up to l = 3, 5 freqs

A sampled ORF can make M_g indefinite (lnL = -inf).  So that the -inf pattern
does not depend on rounding in the pivots, main() refuses a sampled-ORF draw
on which any M_g, scaled to a unit diagonal, has |lambda_min| / lambda_max
< 1e-6 (a condition on the inputs), and it refuses any fixture on which the enterprise-order and
near-exact references disagree on -inf.  The prior seed of a sampled-ORF
fixture is searched upward from its starting value until every draw passes
the conditioning bound and, for mc_binorf, at least two prior draws are
finite and at least two are -inf; the seeds below are the ones found, on the
CPU, before any device run.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from enterprise_warp_amd import synth  # noqa: E402
from _common_ref import TermDeviceOrderPTA, TermOraclePTA  # noqa: E402

ORDERINGS = ("enterprise", "device", "device_blas", "reverse_chol", "extended")
MG_COND_MIN = 1e-6

# name -> (n_psr, n_toa, pulsar seed, gwb_multi option, fixed white noise, (prior seed, near seed))
MULTI = {
    "mc_hd_mono": (3, 300, 610, "hd_vary_gamma_5_nfreqs+mono_vary_gamma_3_nfreqs", True, (611, 612)),
    "mc_three": (4, 300, 620, "vary_gamma_6_nfreqs+hd_vary_gamma_6_nfreqs+mono_vary_gamma_6_nfreqs"
                              "+dipo_vary_gamma_4_nfreqs", True, (621, 622)),
    "mc_f31": (3, 300, 630, "hd_vary_gamma_31_nfreqs+mono_vary_gamma_31_nfreqs", True, (631, 632)),
    "mc_varwn": (3, 400, 640, "hd_vary_gamma_8_nfreqs+dipo_vary_gamma_8_nfreqs", False, (641, 642)),
    "mc_binorf": (4, 300, 650, "varorf_vary_gamma_5_nfreqs", True, (654, 652)),
    "mc_legendre": (4, 300, 660, "legendreorf_3_vary_gamma_5_nfreqs", True, (661, 662)),
}
MULTI_NAMES = list(MULTI)
# binned-ORF truth: Hellings-Downs at the bin centres; Legendre truth: its leading coefficients
TRUTH_ORF = {"gw_orf_bin": [0.30, 0.05, -0.11, -0.15, -0.11, 0.02, 0.20],
             "gw_orf_legendre": [0.0, 0.0, 0.3125, 0.0875]}


def references(pta):
    const = pta.constant_values()
    fixed = const if pta.white_fixed() else None
    psrs = [c.psr for c in pta.signal_collections]
    terms = pta.oracle_terms()
    return const, [TermOraclePTA(psrs, terms, fixed_params=fixed),
                   TermDeviceOrderPTA(psrs, terms, fixed, np.float64, gram_mode="device"),
                   TermDeviceOrderPTA(psrs, terms, fixed, np.float64, gram_mode="blas"),
                   TermDeviceOrderPTA(psrs, terms, fixed, np.float64, gram_mode="reverse", factor="chol"),
                   TermDeviceOrderPTA(psrs, terms, fixed, np.longdouble)]


def mg_condition(pta, model, const, X):
    """Per row of X: min over the M_g of |lambda_min| / lambda_max, of M_g
    scaled to a unit diagonal (D^-1/2 M_g D^-1/2, D = diag M_g > 0).  The
    pulsars' own red-noise variances on the diagonal span up to 28 decades
    over the prior, so the raw eigenvalue ratio measures that scale (1e-18 on
    every draw), not the distance to a singular matrix; the elimination's
    pivot signs are invariant under the diagonal scaling."""
    out = []
    for x in X:
        d = dict(const)
        d.update(pta.map_params(x))
        worst = np.inf
        for M in model.common_mg(d):
            M = np.asarray(M, dtype=float)
            sc = 1.0 / np.sqrt(np.diag(M))
            w = np.linalg.eigvalsh(M * sc[:, None] * sc[None, :])
            worst = min(worst, np.min(np.abs(w)) / np.max(np.abs(w)))
        out.append(worst)
    return np.array(out)


def build(name, s_prior=None):
    """(pta, recipe, theta) of one fixture."""
    n_psr, n_toa, seed, opt, fixed_white, (sp, s_near) = MULTI[name]
    s_prior = sp if s_prior is None else s_prior
    rng = np.random.default_rng(seed)
    psrs = []
    for i in range(n_psr):
        v = rng.standard_normal(3)
        psrs.append(synth.make_pulsar(f"J{i:04d}+{seed:04d}", n_toa, seed=seed * 1000 + i, pos=v / np.linalg.norm(v),
                                      epoch_size=4))
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    ns = synth.params_namespace(Tspan, fixed_white)
    wn = synth.white_noisedict(psrs, seed + 1)
    terms = {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend",
             "spin_noise": "powerlaw_10_nfreqs", "dm_noise": "powerlaw_10_nfreqs"}
    common = {"gwb_multi": opt}
    pta = synth.build_pta(psrs, terms, common, ns, wn if fixed_white else None)
    truth = synth.truth_values(pta, seed + 2, white=wn)
    for p in pta.params:                      # the common processes at realistic values
        if p.name.startswith("gw") and p.name.endswith("gamma"):
            truth[p.name] = 13.0 / 3.0
        elif p.name.startswith("gw_log10_A"):
            truth[p.name] = -14.3 if p.name in ("gw_log10_A", "gw_log10_A_hd", "gw_log10_A_orf") else -14.8
        elif p.name in TRUTH_ORF:
            truth[p.name] = np.array(TRUTH_ORF[p.name])
    synth.simulate_residuals(pta, truth, seed + 3)
    near = synth.near_draws(pta, truth, 8, s_near)
    for p in pta.params:                      # ORF values: a tighter cloud (Gamma stays positive definite)
        if p.name in TRUTH_ORF:
            i = pta.param_names.index(p.name + "_0")
            r = np.random.default_rng(s_near + 1000)
            near[:, i:i + p.size] = np.clip(truth[p.name][None, :] + 0.05 * r.standard_normal((8, p.size)), -1, 1)
    X = np.vstack([synth.prior_draws(pta, 8, s_prior), near])
    recipe = {"per_psr_terms": terms, "common_terms": common, "Tspan": float(Tspan), "fixed_white": fixed_white,
              "noisedict": wn if fixed_white else {}}
    return pta, recipe, X


def evaluate(pta, X):
    const, models = references(pta)
    vals = np.zeros((len(models), len(X)))
    for j, x in enumerate(X):
        d = dict(const)
        d.update(pta.map_params(x))
        for i, mdl in enumerate(models):
            vals[i, j] = mdl.lnlikelihood(d)
    return vals


def dump(name, pta, recipe, X, vals, n_prior=8):
    psrs = [c.psr for c in pta.signal_collections]
    arrays = {}
    for i, p in enumerate(psrs):
        arrays[f"p{i}_toas"] = p.toas
        arrays[f"p{i}_residuals"] = p.residuals
        arrays[f"p{i}_toaerrs"] = p.toaerrs
        arrays[f"p{i}_freqs"] = p.freqs
        arrays[f"p{i}_Mmat"] = p.Mmat
        arrays[f"p{i}_pos"] = p.pos
        for k, v in p.flags.items():
            arrays[f"p{i}_flag_{k}"] = v.astype(str)
    recipe = dict(recipe, names=[p.name for p in psrs], flag_names=[sorted(p.flags) for p in psrs],
                  param_names=pta.param_names)
    fin = np.isfinite(vals).all(axis=0)
    spread = np.zeros(len(X))
    spread[fin] = vals[:, fin].max(axis=0) - vals[:, fin].min(axis=0)
    spread[~fin & np.isfinite(vals).any(axis=0)] = np.inf
    near = np.arange(len(X)) >= n_prior
    np.savez_compressed(os.path.join(HERE, name + ".npz"), recipe=np.array(json.dumps(recipe)), theta=X, lnl=vals[0],
                        lnl_dev=vals[1], lnl_exact=vals[-1], lnl_orderings=vals, orderings=np.array(ORDERINGS),
                        spread=spread, near=near, min_eig=np.full(len(X), np.nan), **arrays)
    strict = 1e-6 + 1e-10 * np.abs(vals[-1])
    with np.errstate(invalid="ignore", divide="ignore"):
        print(name, "n_psr", len(psrs), "nparam", X.shape[1], "n_inf", int(np.sum(~np.isfinite(vals[0]))),
              "spread/strict", np.array2string(spread / strict, precision=1, max_line_width=200))


def make(name):
    sampled = "orf" in MULTI[name][3]
    s_prior = MULTI[name][5][0]
    for attempt in range(200):
        pta, recipe, X = build(name, s_prior + attempt)
        if sampled:
            const, models = references(pta)
            cond = mg_condition(pta, models[2], const, X)
            if np.any(cond < MG_COND_MIN):
                print(f"{name}: prior seed {s_prior + attempt} refused: an M_g with |lambda_min| / lambda_max = "
                      f"{cond.min():.1e}")
                continue
        vals = evaluate(pta, X)
        fin_ent, fin_ext = np.isfinite(vals[0]), np.isfinite(vals[-1])
        if not np.array_equal(fin_ent, fin_ext):
            if sampled:
                print(f"{name}: prior seed {s_prior + attempt} refused: the references disagree on -inf")
                continue
            raise SystemExit(f"{name}: the enterprise-order and near-exact references disagree on -inf")
        if name == "mc_binorf" and (np.sum(fin_ent[:8]) < 2 or np.sum(~fin_ent[:8]) < 2):
            print(f"{name}: prior seed {s_prior + attempt} refused: {np.sum(fin_ent[:8])} finite prior draws")
            continue
        if attempt:
            raise SystemExit(f"{name}: prior seed {s_prior} does not hold; {s_prior + attempt} does -- fix it in MULTI")
        dump(name, pta, recipe, X, vals)
        return
    raise SystemExit(f"{name}: no prior seed found")


def main():
    only = sys.argv[1:]
    for name in MULTI_NAMES:
        if only and not any(name.startswith(o) for o in only):
            continue
        make(name)


if __name__ == "__main__":
    main()
