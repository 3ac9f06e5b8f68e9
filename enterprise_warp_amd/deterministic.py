"""Deterministic delay signals: a parameter-dependent waveform subtracted from
the residuals before the likelihood is taken ([ent] deterministic_signals.
Deterministic; the reference's examples/custom_models.py returns
`enterprise_extensions.models.dm_exponential_dip(tmin, tmax)` for J1713+0747).

The waveforms and factories restate enterprise_extensions ([ent-ext]
chromatic.chrom_exp_decay / chrom_yearly_sinusoid / dm_exponential_dip /
dm_annual_signal) from its public source, as the [ent] restatements of
SURVEY.md do; the package itself is not a dependency.

    delta_dip(t, nu)  = sign(sign_param) 10^log10_Amp H(t - t0 day)
                        exp(-(t - t0 day) / (10^log10_tau day)) (1400 / nu)^idx
    delta_yr(t, nu)   = 10^log10_Amp sin(2 pi fyr t + phase) (1400 / nu)^idx

(t in seconds, t0 in MJD, H(0) = 1, the exponential applied only where
t > t0 day.)  A bound term contributes its parameters `{psr}_{name}_{par}` to
the model and one `ewh_delay_entry` to the pulsar's descriptor
(include/ewarp_hip.h): the device forms r - sum delta per sample
(csrc/delay.hip).  `get_delay` evaluates the same waveforms in numpy
(`SignalCollection.get_delay`, `PTA.get_delay`: enterprise's pta.get_delay).
"""
import numpy as np

from . import constants as const
from . import parameter
from .signals import Signal, _pname

DAY = 86400.0
DELAY_EXP_DIP, DELAY_YEARLY_SIN = 1, 2      # ewh_delay_kind


class Waveform:
    """An unbound waveform: kind, its parameters (prior specs, named
    Parameters or numbers) and the chromatic index."""

    def __init__(self, kind, params, idx):
        self.kind = kind
        self.params = dict(params)
        self.idx = float(idx)

    def evaluate(self, toas, freqs, **vals):
        return _WAVEFORMS[self.kind](np.asarray(toas, float), np.asarray(freqs, float), idx=self.idx, **vals)


def _exp_decay(toas, freqs, log10_Amp=-7.0, sign_param=-1.0, t0=54000.0, log10_tau=1.7, idx=2.0):
    """[ent-ext] chromatic.chrom_exp_decay."""
    t0 = t0 * DAY
    tau = 10 ** log10_tau * DAY
    ind = np.where(toas > t0)[0]
    wf = 10 ** log10_Amp * np.heaviside(toas - t0, 1)
    wf[ind] *= np.exp(-(toas[ind] - t0) / tau)
    return np.sign(sign_param) * wf * (1400.0 / freqs) ** idx


def _yearly_sinusoid(toas, freqs, log10_Amp=-7.0, phase=0.0, idx=2.0):
    """[ent-ext] chromatic.chrom_yearly_sinusoid."""
    wf = 10 ** log10_Amp * np.sin(2 * np.pi * const.fyr * toas + phase)
    return wf * (1400.0 / freqs) ** idx


_WAVEFORMS = {"exp_dip": _exp_decay, "yearly_sin": _yearly_sinusoid}
_KIND = {"exp_dip": DELAY_EXP_DIP, "yearly_sin": DELAY_YEARLY_SIN}
# descriptor slots p0..p3 per kind (include/ewarp_hip.h, ewh_delay_kind)
_SLOTS = {"exp_dip": ("log10_Amp", "log10_tau", "t0", "sign_param"), "yearly_sin": ("log10_Amp", "phase")}


def chrom_exp_decay(log10_Amp=-7.0, sign_param=-1.0, t0=54000.0, log10_tau=1.7, idx=2):
    """[ent-ext] chromatic.chrom_exp_decay as a waveform for `Deterministic`."""
    return Waveform("exp_dip", {"log10_Amp": log10_Amp, "sign_param": sign_param, "t0": t0,
                                "log10_tau": log10_tau}, idx)


def chrom_yearly_sinusoid(log10_Amp=-7.0, phase=0.0, idx=2):
    """[ent-ext] chromatic.chrom_yearly_sinusoid as a waveform for `Deterministic`."""
    return Waveform("yearly_sin", {"log10_Amp": log10_Amp, "phase": phase}, idx)


class Deterministic(Signal):
    """[ent] deterministic_signals.Deterministic(waveform, name): bound per
    pulsar; parameters `{psr}_{name}_{par}`."""

    signal_type = "deterministic"

    def __init__(self, waveform, name=""):
        if not isinstance(waveform, Waveform):
            raise TypeError("Deterministic needs a waveform from chrom_exp_decay / chrom_yearly_sinusoid")
        self.waveform, self.name = waveform, name

    def __call__(self, psr):
        return _BoundDeterministic(self, psr)


class _BoundDeterministic:
    kind = "deterministic"

    def __init__(self, sig, psr):
        self.name = sig.name
        self.waveform = sig.waveform
        self.toas = np.asarray(psr.toas, float)
        self.freqs = np.asarray(psr.freqs, float)
        self.pars = {loc: parameter.resolve(val, _pname(psr.name, sig.name, loc))
                     for loc, val in sig.waveform.params.items()}
        self.params = list(self.pars.values())

    def _value(self, p, params):
        if isinstance(p, parameter.ConstantParameter):
            if p.value is None:
                raise ValueError(f"Constant parameter {p.name} has no value")
            return float(p.value)
        return float(params[p.name])

    def get_delay(self, params):
        vals = {loc: self._value(p, params) for loc, p in self.pars.items()}
        return self.waveform.evaluate(self.toas, self.freqs, **vals)

    def entry(self, pref):
        """(kind, p0, p1, p2, p3, idx) for the descriptor; pref: Parameter -> (theta column or -1, constant)."""
        refs = [pref(self.pars[loc]) for loc in _SLOTS[self.waveform.kind]]
        refs += [(-1, 0.0)] * (4 - len(refs))
        return (_KIND[self.waveform.kind], *refs, self.waveform.idx)


def dm_exponential_dip(tmin, tmax, idx=2, sign="negative", name="dmexp"):
    """[ent-ext] models.dm_exponential_dip: a chromatic exponential dip with
    t0 ~ U(tmin, tmax) (MJD), log10_Amp ~ U(-10, -2), log10_tau ~ U(0, 2.5);
    sign='vary' samples sign_param ~ U(-1, 1), else it is the constant +-1."""
    t0 = parameter.Uniform(tmin, tmax)
    log10_Amp = parameter.Uniform(-10, -2)
    log10_tau = parameter.Uniform(0, 2.5)
    if sign == "vary":
        sign_param = parameter.Uniform(-1.0, 1.0)
    elif sign == "positive":
        sign_param = 1.0
    else:
        sign_param = -1.0
    wf = chrom_exp_decay(log10_Amp=log10_Amp, t0=t0, log10_tau=log10_tau, sign_param=sign_param, idx=idx)
    return Deterministic(wf, name=name)


def dm_annual_signal(idx=2, name="dm_s1yr"):
    """[ent-ext] models.dm_annual_signal: log10_Amp ~ U(-10, -2), phase ~ U(0, 2 pi)."""
    wf = chrom_yearly_sinusoid(log10_Amp=parameter.Uniform(-10, -2), phase=parameter.Uniform(0, 2 * np.pi), idx=idx)
    return Deterministic(wf, name=name)
