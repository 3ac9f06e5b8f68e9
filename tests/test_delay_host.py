"""CPU tests of the deterministic delay signals (enterprise_warp_amd/
deterministic.py, ABI 8): the numpy waveforms against an independent
restatement, parameter naming, the descriptor tables, the custom-model
extension point (a StandardModels subclass through a paramfile, as the
reference's examples/custom_models.py), descriptor validation on the host
twin, and the twin's likelihood under the criteria of _delay_common.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _delay_common as dc
from conftest import REF_EXAMPLES
from enterprise_warp_amd import _lib, parameter, warp
from enterprise_warp_amd.bilby_bridge import get_bilby_prior_dict
from enterprise_warp_amd.deterministic import (Deterministic, chrom_exp_decay, chrom_yearly_sinusoid,
                                               dm_annual_signal, dm_exponential_dip)
from enterprise_warp_amd.models import StandardModels
from enterprise_warp_amd.pta import PTA
from enterprise_warp_amd.pulsar import Pulsar
from enterprise_warp_amd.signals import MeasurementNoise, TimingModel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPU_LIB = os.path.join(ROOT, "enterprise_warp_amd", "libewarp_cpu.so")


def small_pulsar(n=40, name="J0000+0000"):
    rng = np.random.default_rng(3)
    toas = np.sort(rng.uniform(53000.0, 55000.0, n)) * dc.DAY
    toas[17] = 54000.0 * dc.DAY                       # a TOA exactly at t0 = 54000
    freqs = rng.choice([700.0, 1400.0, 3100.0], n)
    return Pulsar(name, toas, rng.normal(0, 1e-6, n), np.full(n, 1e-6), freqs,
                  flags={"group": np.array(["A"] * n)}, sort=False)


def model(psr, *delays):
    m = TimingModel() + MeasurementNoise(efac=parameter.Constant(1.0))
    for d in delays:
        m = m + d
    return PTA([m(psr)])


def test_get_delay_equals_restatement():
    psr = small_pulsar()
    pta = model(psr, dm_exponential_dip(53000, 55000, sign="vary"))
    names = pta.param_names
    assert names == [f"{psr.name}_dmexp_{p}" for p in ("log10_Amp", "log10_tau", "sign_param", "t0")]
    for sp in (0.7, -0.3, 0.0):
        vals = {"dmexp_log10_Amp": -6.2, "dmexp_log10_tau": 1.3, "dmexp_sign_param": sp, "dmexp_t0": 54000.0}
        x = [vals["dmexp_" + n.rsplit("dmexp_", 1)[1]] for n in names]
        got = pta.get_delay(x)[0]
        want = dc.ref_dip(psr.toas, psr.freqs, -6.2, 1.3, 54000.0, sp)
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
        k = 17                                                       # the TOA at t0: H(0) = 1, no decay yet
        assert got[k] == np.sign(sp) * 10 ** -6.2 * (1400.0 / psr.freqs[k]) ** 2
        assert np.all(got[psr.toas < 54000.0 * dc.DAY] == 0.0)
    # dict input, as pta.get_delay(params) in enterprise
    d = pta.map_params(x)
    np.testing.assert_array_equal(pta.get_delay(d)[0], got)


def test_parameter_names_priors_and_order():
    psr = small_pulsar()
    pta = model(psr, dm_exponential_dip(53005, 54995), dm_annual_signal())
    n = psr.name
    assert pta.param_names == [f"{n}_dm_s1yr_log10_Amp", f"{n}_dm_s1yr_phase", f"{n}_dmexp_log10_Amp",
                               f"{n}_dmexp_log10_tau", f"{n}_dmexp_t0"]
    pr = {p.name: p.prior._defaults for p in pta.params}
    assert pr[f"{n}_dmexp_t0"] == {"pmin": 53005.0, "pmax": 54995.0}
    assert pr[f"{n}_dmexp_log10_Amp"] == {"pmin": -10.0, "pmax": -2.0}
    assert pr[f"{n}_dmexp_log10_tau"] == {"pmin": 0.0, "pmax": 2.5}
    assert pr[f"{n}_dm_s1yr_log10_Amp"] == {"pmin": -10.0, "pmax": -2.0}
    assert pr[f"{n}_dm_s1yr_phase"] == {"pmin": 0.0, "pmax": 2 * np.pi}
    assert pta.constant_values()[f"{n}_dmexp_sign_param"] == -1.0
    # the oracle's view is unchanged: stochastic and white terms only
    assert [t["kind"] for t in pta.oracle_terms()[0]] == ["timing_model", "efac"]
    # a custom name / index through Deterministic itself
    wf = chrom_exp_decay(log10_Amp=parameter.Uniform(-9, -5), t0=54321.0, log10_tau=1.0, sign_param=1.0, idx=4)
    p2 = model(psr, Deterministic(wf, name="scat"))
    assert p2.param_names == [f"{n}_scat_log10_Amp"]
    np.testing.assert_allclose(p2.get_delay([-6.0])[0], dc.ref_dip(psr.toas, psr.freqs, -6.0, 1.0, 54321.0, 1.0, 4.0),
                               rtol=1e-14)


def test_dip_and_annual_add():
    psr = small_pulsar()
    pta = model(psr, dm_exponential_dip(53000, 55000), dm_annual_signal())
    x = np.array([-6.5, 1.0, -6.0, 1.7, 53800.0])
    want = dc.ref_dip(psr.toas, psr.freqs, -6.0, 1.7, 53800.0, -1.0) + dc.ref_annual(psr.toas, psr.freqs, -6.5, 1.0)
    np.testing.assert_allclose(pta.get_delay(x)[0], want, rtol=1e-13, atol=1e-22)
    only = model(psr, Deterministic(chrom_yearly_sinusoid(log10_Amp=-6.5, phase=1.0), name="yr"))
    np.testing.assert_allclose(only.get_delay([])[0], dc.ref_annual(psr.toas, psr.freqs, -6.5, 1.0), rtol=1e-13,
                               atol=1e-22)


def test_descriptor_prefs():
    psr = small_pulsar()
    for sign, sp_ref in (("negative", (-1, -1.0)), ("positive", (-1, 1.0)), ("vary", None)):
        pta = model(psr, dm_exponential_dip(53000, 55000, sign=sign), dm_annual_signal(idx=4))
        col = {n: j for j, n in enumerate(pta.param_names)}
        n = psr.name
        lay = pta.layout()[0]
        np.testing.assert_array_equal(lay["toas"], psr.toas)
        np.testing.assert_allclose(lay["ln_chrom"], np.log(1400.0 / psr.freqs))
        dip, yr = lay["delays"]
        if sp_ref is None:
            sp_ref = (col[f"{n}_dmexp_sign_param"], 0.0)
        assert dip == (_lib.DELAY_EXP_DIP, (col[f"{n}_dmexp_log10_Amp"], 0.0), (col[f"{n}_dmexp_log10_tau"], 0.0),
                       (col[f"{n}_dmexp_t0"], 0.0), sp_ref, 2.0)
        assert yr == (_lib.DELAY_YEARLY_SIN, (col[f"{n}_dm_s1yr_log10_Amp"], 0.0), (col[f"{n}_dm_s1yr_phase"], 0.0),
                      (-1, 0.0), (-1, 0.0), 4.0)


class CustomModels(StandardModels):
    """The reference's examples/custom_models.py event_j1713, on the example pulsar."""

    def __init__(self, psr=None, params=None):
        super().__init__(psr=psr, params=params)
        self.priors.update({"event_t0": [54500.0, 54900.0]})

    def event_dip(self, option="default"):
        if self.psr.name == "J1832-0836":
            from enterprise_warp_amd import models
            return models.dm_exponential_dip(tmin=self.params.event_t0[0], tmax=self.params.event_t0[1])

    def annual_dm(self, option="default"):
        from enterprise_warp_amd import models
        return models.dm_annual_signal()


def test_custom_models_through_paramfile(monkeypatch, tmp_path):
    monkeypatch.chdir(REF_EXAMPLES)
    nm = tmp_path / "noise_with_delays.json"
    base = json.load(open(os.path.join(REF_EXAMPLES, "example_noisemodels", "default_noise_example_1.json")))
    base["J1832-0836"].update({"event_dip": "default", "annual_dm": "default"})
    nm.write_text(json.dumps(base))
    src = open(os.path.join(REF_EXAMPLES, "example_params", "default_model_dynesty.dat")).read().splitlines()
    lines = [f"noise_model_file: {nm}" if ln.startswith("noise_model_file") else ln for ln in src]
    assert lines != src
    prfile = tmp_path / "with_delays.dat"
    prfile.write_text("\n".join(lines) + "\n")
    P = warp.Params(str(prfile), opts=None, custom_models_obj=CustomModels)
    pta = warp.init_pta(P)[0]
    new = ["J1832-0836_dm_s1yr_log10_Amp", "J1832-0836_dm_s1yr_phase", "J1832-0836_dmexp_log10_Amp",
           "J1832-0836_dmexp_log10_tau", "J1832-0836_dmexp_t0"]
    assert [n for n in pta.param_names if "dmexp" in n or "dm_s1yr" in n] == new
    assert pta.param_names == sorted(pta.param_names)
    pri = get_bilby_prior_dict(pta)
    for n in new:
        assert n in pri
    assert pri["J1832-0836_dmexp_t0"].minimum == 54500.0 and pri["J1832-0836_dmexp_t0"].maximum == 54900.0
    assert len(pta.layout()[0]["delays"]) == 2
    x = np.array([p.sample() for p in pta.params], dtype=float)
    assert pta.get_delay(x)[0].shape == (len(P.psrs[0].toas),)
    # the HyperModel sees them as any other Uniform parameter
    from enterprise_warp_amd.hypermodel import HyperModel
    hm = HyperModel({0: pta})
    assert set(new) <= set(hm.param_names)


def test_bayes_ephem_still_raises():
    from enterprise_warp_amd.signals import PhysicalEphemerisSignal
    with pytest.raises(NotImplementedError, match="ephemeris"):
        PhysicalEphemerisSignal()(small_pulsar())


# --- descriptor validation on the host twin (same ewarp_desc.h as the device library) ---
@pytest.fixture(scope="module")
def twin():
    if not os.path.exists(CPU_LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "enterprise_warp_amd", "csrc"), "cpu"], check=True,
                       capture_output=True)
    lib = C.CDLL(CPU_LIB)
    lib.ewh_create.argtypes = [C.POINTER(_lib.PtaDesc), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p)]
    lib.ewh_create.restype = C.c_int
    lib.ewh_last_error.restype = C.c_char_p
    lib.ewh_destroy.argtypes = [C.c_void_p]
    lib.ewh_destroy.restype = None
    return lib


def tiny_desc(n_param=5, common_kind=None, **over):
    n = 8
    keep = {}
    dbl = lambda v: (C.c_double * len(v))(*v)              # noqa: E731
    i32 = lambda v: (C.c_int32 * len(v))(*v)               # noqa: E731
    keep["basis"] = dbl([1.0] * n)
    keep["resid"] = dbl([1e-6 * (-1) ** t for t in range(n)])
    keep["err"] = dbl([1e-6] * n)
    keep["slots"] = (_lib.Pref * 1)(_lib.Pref(-1, 0, 1.0))
    keep["ef"] = i32([0] * n)
    keep["eq"] = i32([-1] * n)
    keep["spec"] = (_lib.SpecEntry * 1)(_lib.SpecEntry(_lib.SPEC_CONST, 0, _lib.Pref(-1, 0, 1e40), _lib.Pref(-1, 0, 0),
                                                       _lib.Pref(-1, 0, 0), 0.0, 0.0, 0.0))
    keep["lnc"] = dbl([0.1] * n)
    keep["toas"] = dbl([54000.0 * dc.DAY + 10 * dc.DAY * t for t in range(n)])
    keep["delays"] = (_lib.DelayEntry * 2)(
        _lib.DelayEntry(_lib.DELAY_EXP_DIP, 0, _lib.Pref(0, 0, 0), _lib.Pref(1, 0, 0), _lib.Pref(2, 0, 0),
                        _lib.Pref(-1, 0, -1.0), 2.0),
        _lib.DelayEntry(_lib.DELAY_YEARLY_SIN, 0, _lib.Pref(3, 0, 0), _lib.Pref(4, 0, 0), _lib.Pref(-1, 0, 0),
                        _lib.Pref(-1, 0, 0), 2.0))
    f = dict(n_toa=n, n_col=1, n_lead_const=1, n_spec=1, basis=keep["basis"], resid=keep["resid"], toaerr=keep["err"],
             n_slot=1, slots=keep["slots"], efac_slot=keep["ef"], equad_slot=keep["eq"], spec=keep["spec"],
             ln_chrom=keep["lnc"], n_delay=2, delays=keep["delays"], toas=keep["toas"])
    f.update(over)
    keep["psr"] = (_lib.PulsarDesc * 1)(_lib.PulsarDesc(**f))
    common = None
    if common_kind is not None:
        keep["orf"] = dbl([1.0])
        keep["cspec"] = (_lib.SpecEntry * 1)(_lib.SpecEntry(_lib.SPEC_CONST, 0, _lib.Pref(-1, 0, 1.0),
                                                           _lib.Pref(-1, 0, 0), _lib.Pref(-1, 0, 0), 0.0, 0.0, 0.0))
        keep["common"] = _lib.CommonDesc(1, keep["orf"], keep["cspec"], common_kind)
        common = C.pointer(keep["common"])
    keep["desc"] = _lib.PtaDesc(_lib.EWH_ABI_VERSION, 1, n_param, 1, keep["psr"], common)
    return keep


def create(lib, keep):
    h = C.c_void_p()
    rc = lib.ewh_create(C.byref(keep["desc"]), None, 0, C.byref(h))
    msg = lib.ewh_last_error().decode()
    if h:
        lib.ewh_destroy(h)
    return rc, msg


def test_descriptor_validation(twin):
    assert create(twin, tiny_desc())[0] == 0
    bad_kind = tiny_desc()
    bad_kind["delays"][1].kind = 3
    rc, msg = create(twin, bad_kind)
    assert rc == -1 and "delay kind" in msg
    rc, msg = create(twin, tiny_desc(n_param=4))
    assert rc == -1 and "delay theta index" in msg
    rc, msg = create(twin, tiny_desc(toas=None))
    assert rc == -1 and "toas and ln_chrom" in msg
    rc, msg = create(twin, tiny_desc(ln_chrom=None))
    assert rc == -1 and "toas and ln_chrom" in msg
    rc, msg = create(twin, tiny_desc(delays=None))
    assert rc == -1 and "delay table" in msg
    rc, msg = create(twin, tiny_desc(n_delay=9))
    assert rc == -4 and "more than 8 delay entries" in msg
    # without delays, toas and ln_chrom may be NULL (a value-initialised ABI-7-style descriptor)
    assert create(twin, tiny_desc(n_delay=0, delays=None, toas=None, ln_chrom=None))[0] == 0
    # the two unsupported combinations: EWH_E_UNSUPPORTED with a message
    rc, msg = create(twin, tiny_desc(common_kind=_lib.COMMON_CORRELATED, n_col=2, n_common=1))
    assert rc == -4 and "correlated common process" in msg
    rc, msg = create(twin, tiny_desc(common_kind=_lib.COMMON_OPTSTAT, n_col=2, n_common=1))
    assert rc == -4 and "optimal statistic" in msg


def test_twin_delay_models():
    """c1_j1832, c2_small (ECORR), c3_small (fixed white noise, delays on the
    first and last pulsar) on the host twin, in a subprocess (EWARP_BACKEND=cpu)."""
    env = dict(os.environ, EWARP_BACKEND="cpu", OMP_NUM_THREADS="4")
    env.pop("EWARP_HIP_LIB", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "_delay_worker.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    print(p.stdout)
    line = next(ln for ln in p.stdout.splitlines() if ln.startswith("DELAY_JSON "))
    res = json.loads(line[len("DELAY_JSON "):])
    assert res["lib"] == "libewarp_cpu.so"
    assert set(res["cases"]) == {"c1_j1832", "c2_small", "c3_small"}
    for r in res["cases"].values():
        assert set(r) == {"near_a_parity", "near_b_accuracy", "prior_accuracy"}
    assert res["others_bit_identical"] and res["delay_terms_differ"]
    assert res["nan_is_minus_inf"]
    assert res["c5_refused"]
