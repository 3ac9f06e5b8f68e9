"""Shared by tests/test_delay_host.py, tests/_delay_worker.py and
tests/test_gpu_delay.py: golden fixtures with a chromatic exponential dip and
an annual DM sinusoid added to chosen pulsars, and references that do not
depend on the code under test -- the two waveforms restated in numpy, and the
enterprise-order / double-double oracles evaluated on r - delta (the oracle
itself is untouched: it sees the stochastic and white terms only)."""
import functools
import json
import os

import numpy as np

from conftest import GOLDEN, check_accuracy, check_parity

DAY = 86400.0
FYR = 1.0 / (365.25 * DAY)
TRUTH = {"dmexp_log10_Amp": -6.0, "dmexp_log10_tau": 1.7, "dm_s1yr_log10_Amp": -6.5, "dm_s1yr_phase": 1.0}


# --- the two waveforms, restated (enterprise_extensions chromatic.py) ---------
def ref_dip(toas, freqs, log10_Amp, log10_tau, t0, sign_param, idx=2.0):
    t0s, tau = t0 * DAY, 10.0 ** log10_tau * DAY
    wf = np.where(toas >= t0s, 10.0 ** log10_Amp, 0.0)
    after = toas > t0s
    wf[after] *= np.exp(-(toas[after] - t0s) / tau)
    return np.sign(sign_param) * wf * (1400.0 / freqs) ** idx


def ref_annual(toas, freqs, log10_Amp, phase, idx=2.0):
    return 10.0 ** log10_Amp * np.sin(2.0 * np.pi * FYR * toas + phase) * (1400.0 / freqs) ** idx


def ref_delay(psr, vals, sign=-1.0):
    """delta of one pulsar from {local name: value} (dmexp_*, dm_s1yr_*)."""
    t, f = np.asarray(psr.toas, float), np.asarray(psr.freqs, float)
    sp = vals.get("dmexp_sign_param", sign)
    return (ref_dip(t, f, vals["dmexp_log10_Amp"], vals["dmexp_log10_tau"], vals["dmexp_t0"], sp)
            + ref_annual(t, f, vals["dm_s1yr_log10_Amp"], vals["dm_s1yr_phase"]))


def span_mjd(psr):
    t = np.asarray(psr.toas, float)
    return t.min() / DAY, t.max() / DAY


def truth_for(psr):
    lo, hi = span_mjd(psr)
    return dict(TRUTH, dmexp_t0=lo + 0.4 * (hi - lo))


# --- fixtures with delays -------------------------------------------------------
def load_recipe(name):
    from enterprise_warp_amd.pulsar import Pulsar
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    rec = json.loads(str(z["recipe"]))
    psrs = []
    for i, nm in enumerate(rec["names"]):
        flags = {k: z[f"p{i}_flag_{k}"] for k in rec["flag_names"][i]}
        psrs.append(Pulsar(nm, z[f"p{i}_toas"], z[f"p{i}_residuals"], z[f"p{i}_toaerrs"], z[f"p{i}_freqs"],
                           flags=flags, Mmat=z[f"p{i}_Mmat"], pos=z[f"p{i}_pos"], sort=False))
    return rec, psrs, {k: z[k] for k in ("theta", "near")}


def build(rec, psrs, delay_psrs=(), sign="negative"):
    """The fixture's PTA (synth.build_pta's assembly) with dm_exponential_dip +
    dm_annual_signal added to the pulsars whose index is in delay_psrs."""
    from enterprise_warp_amd import synth
    from enterprise_warp_amd.deterministic import dm_annual_signal, dm_exponential_dip
    from enterprise_warp_amd.models import StandardModels
    from enterprise_warp_amd.pta import PTA
    from enterprise_warp_amd.signals import TimingModel
    ns = synth.params_namespace(rec["Tspan"], rec["fixed_white"])
    allm = StandardModels(psr=psrs, params=ns)
    m_all = TimingModel()
    for term, opt in rec["common_terms"].items():
        m_all = m_all + getattr(allm, term)(option=opt)
    models = []
    for i, psr in enumerate(psrs):
        sm = StandardModels(psr=psr, params=ns)
        m = m_all
        for term, opt in rec["per_psr_terms"].items():
            m = m + getattr(sm, term)(option=opt)
        if i in delay_psrs:
            lo, hi = span_mjd(psr)
            m = m + dm_exponential_dip(lo, hi, sign=sign) + dm_annual_signal()
        models.append(m(psr))
    pta = PTA(models)
    if rec["noisedict"]:
        pta.set_default_params(rec["noisedict"])
    return pta


def inject(psrs, delay_psrs):
    """New Pulsar objects whose residuals carry the truth dip + annual term."""
    from enterprise_warp_amd.pulsar import Pulsar
    out = []
    for i, p in enumerate(psrs):
        if i not in delay_psrs:
            out.append(p)
            continue
        r = np.asarray(p.residuals, float) + ref_delay(p, truth_for(p))
        out.append(Pulsar(p.name, p.toas, r, p.toaerrs, p.freqs, flags=p.flags, Mmat=p.Mmat, pos=p.pos, sort=False))
    return out


def delay_thetas(pta, psrs, delay_psrs, theta0, names0, seed):
    """Rows of the delay PTA: the fixture's noise rows, with the delay
    parameters (a) near truth (sigma 0.05 in the logs and the phase, 3 d in
    t0) and (b) drawn from their priors."""
    rng = np.random.default_rng(seed)
    names = pta.param_names
    col0 = {n: j for j, n in enumerate(names0)}
    prior = {p.name: p for p in pta.params}
    Xa = np.empty((len(theta0), len(names)))
    Xb = np.empty_like(Xa)
    for j, n in enumerate(names):
        if n in col0:
            Xa[:, j] = Xb[:, j] = theta0[:, col0[n]]
            continue
        i = next(i for i in delay_psrs if n.startswith(psrs[i].name + "_"))
        loc = n[len(psrs[i].name) + 1:]
        tv = truth_for(psrs[i])[loc]
        Xa[:, j] = tv + rng.normal(0.0, 3.0 if loc.endswith("_t0") else 0.05, len(theta0))
        Xb[:, j] = [prior[n].sample(rng) for _ in range(len(theta0))]
    return Xa, Xb


def local_values(pta, psr, x):
    d = pta.map_params(x)
    pre = psr.name + "_"
    return {k[len(pre):]: v for k, v in d.items() if k.startswith(pre + "dmexp_") or k.startswith(pre + "dm_s1yr_")}


class DelayCase:
    """One fixture with delays on delay_psrs: pta (with delays), the plain PTA
    of the same (injected) data, thetas and the references."""

    def __init__(self, name, delay_psrs=(0,), seed=11):
        rec, psrs0, z = load_recipe(name)
        self.name, self.rec = name, rec
        self.delay_psrs = tuple(i if i >= 0 else len(psrs0) + i for i in delay_psrs)
        self.psrs = inject(psrs0, self.delay_psrs)
        self.pta = build(rec, self.psrs, self.delay_psrs)
        self.plain = build(rec, self.psrs)
        self.near = np.asarray(z["near"], bool)
        self.Xa, self.Xb = delay_thetas(self.pta, self.psrs, self.delay_psrs, z["theta"], self.plain.param_names, seed)
        self._ref = {}

    def deltas(self, x):
        return {i: ref_delay(self.psrs[i], local_values(self.pta, self.psrs[i], x)) for i in self.delay_psrs}

    def plain_theta(self, X):
        col = {n: j for j, n in enumerate(self.pta.param_names)}
        return np.ascontiguousarray(X[:, [col[n] for n in self.plain.param_names]])

    def references(self, which):
        """(enterprise-order, double-double) lnL of Xa / Xb: the oracles of the
        stochastic model on r - delta, sample by sample."""
        if which in self._ref:
            return self._ref[which]
        from oracle.ddref import DDReferencePTA
        from oracle.enterprise_ref import OraclePTA
        pta = self.pta
        const = pta.constant_values()
        fixed = const if pta.white_fixed() else None
        terms = pta.oracle_terms()
        ent = OraclePTA(self.psrs, terms, fixed_params=fixed)
        dd = DDReferencePTA(self.psrs, terms)
        r0 = {i: np.asarray(self.psrs[i].residuals, float) for i in self.delay_psrs}
        a, b = [], []
        for x in (self.Xa if which == "a" else self.Xb):
            d = dict(const)
            d.update(pta.map_params(x))
            for i, dl in self.deltas(x).items():
                ent.pulsars[i].r = r0[i] - dl
                dd.pulsars[i].r = r0[i] - dl
                if ent.fixed is not None:
                    ent.fixed[i] = ent.pulsars[i].white_terms(fixed)
            dd._gram_cache.clear()
            a.append(ent.lnlikelihood(d))
            b.append(dd.lnlikelihood(d))
        self._ref[which] = (np.array(a), np.array(b))
        return self._ref[which]

    def check(self, got_a, got_b, label):
        """The issue's criteria; no row is left out.  Returns the printed ratios."""
        ea, xa = self.references("a")
        eb, xb = self.references("b")
        nr = self.near
        out = {}
        if nr.any():
            out["near_a_parity"] = check_parity(got_a[nr], ea[nr], f"{label} near x (a) vs enterprise order")
            out["near_b_accuracy"] = check_accuracy(got_b[nr], eb[nr], xb[nr], f"{label} near x (b)", per_sample=True)
        if (~nr).any():
            got = np.concatenate([got_a[~nr], got_b[~nr]])
            ent = np.concatenate([ea[~nr], eb[~nr]])
            ext = np.concatenate([xa[~nr], xb[~nr]])
            out["prior_accuracy"] = check_accuracy(got, ent, ext, f"{label} prior rows")
        return out


@functools.lru_cache(maxsize=None)
def case(name, delay_psrs=(0,)):
    return DelayCase(name, delay_psrs)
