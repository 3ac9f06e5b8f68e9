"""Interleaved A/B timing of deterministic delay pulsars on the C3 synthetic
PTA (45 pulsars, white noise fixed, B = 4096 prior draws; the bench's
headline workload):

  base        the PTA as is
  delay1/3    dm_exponential_dip + dm_annual_signal on 1 / 3 pulsars of
              ~11k TOAs (the per-sample residual column, csrc/delay.hip;
              T^T N^-1 T still from the fixed-white-noise cache)
  efac1/3     the same pulsars with a sampled EFAC instead -- what a user
              had to do before to make a pulsar's N^-1 r terms per-sample;
              one theta-dependent white-noise slot puts the whole handle on
              the varying-white-noise contraction

Every form is warmed up, then the forms are timed in alternation (device
events around ewh_lnl_units_device), `--rounds` times; per form the median
and the spread go to profiles/<tag>/delay_ab.json together with the extra
time per delay pulsar, (form - base) / n, and the delay GEMM's share of the
fp64 MFMA peak computed from 2 n_toa ld B flops over that extra time (an
upper bound on the kernel's time: it includes the Gram broadcast and the
wider factorisation).

    python scripts/delay_ab.py --tag r07 [--rounds 7] [--batch 4096] [--skip-efac]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK = 78.6e12     # MI355X fp64 matrix peak, FLOP/s


def build(psrs, ns_fixed, ns_efac, wn, terms, delay=(), efac=()):
    from enterprise_warp_amd.deterministic import dm_annual_signal, dm_exponential_dip
    from enterprise_warp_amd.models import StandardModels
    from enterprise_warp_amd.pta import PTA
    from enterprise_warp_amd.signals import TimingModel
    m_all = TimingModel() + StandardModels(psr=psrs, params=ns_fixed).gwb(option="vary_gamma_14_nfreqs")
    models = []
    for i, psr in enumerate(psrs):
        sm = StandardModels(psr=psr, params=ns_efac if i in efac else ns_fixed)
        m = m_all
        for term, opt in terms.items():
            m = m + getattr(sm, term)(option=opt)
        if i in delay:
            lo, hi = psr.toas.min() / 86400.0, psr.toas.max() / 86400.0
            m = m + dm_exponential_dip(lo, hi) + dm_annual_signal()
        models.append(m(psr))
    pta = PTA(models)
    pta.set_default_params(wn)
    return pta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="delay_ab")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--skip-efac", action="store_true")
    args = ap.parse_args()
    import torch
    from enterprise_warp_amd import synth
    from enterprise_warp_amd.models import StandardModels
    assert torch.cuda.is_available(), "delay_ab.py measures on the GPU"
    cfg = synth.config_c3()
    psrs = [c.psr for c in cfg.pta.signal_collections]
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    ns_fixed = synth.params_namespace(Tspan, True)
    ns_efac = synth.params_namespace(Tspan, True, efac=StandardModels().priors["efac"])
    wn = synth.white_noisedict(psrs, 45 + 1)
    terms = {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend",
             "spin_noise": "powerlaw_30_nfreqs", "dm_noise": "powerlaw_30_nfreqs"}
    mid = len(psrs) // 2
    sel = {1: (mid,), 3: (mid - 1, mid, mid + 1)}
    forms = {"base": cfg.pta}
    for n, idx in sel.items():
        forms[f"delay{n}"] = build(psrs, ns_fixed, ns_efac, wn, terms, delay=idx)
    if not args.skip_efac:
        for n, idx in sel.items():
            forms[f"efac{n}"] = build(psrs, ns_fixed, ns_efac, wn, terms, efac=idx)
    B = args.batch
    run = {}
    for name, pta in forms.items():
        X = synth.prior_draws(pta, B, cfg.theta_seed)
        eng = pta.engine(0)
        th = torch.from_numpy(X).cuda()
        out = torch.zeros(B, dtype=torch.float64, device="cuda")
        U = len(psrs) * B
        s = torch.cuda.current_stream()

        def call(eng=eng, th=th, out=out, U=U, s=s):
            eng.lnl_units_device(th.data_ptr(), B, 0, U, out.data_ptr(), s.cuda_stream)

        for _ in range(3):
            call()
        torch.cuda.synchronize()
        run[name] = (call, out, pta)
    times = {k: [] for k in run}
    for _ in range(args.rounds):
        for name, (call, _, _) in run.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(3):
                call()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / 3.0)
    res = {"batch": B, "rounds": args.rounds, "forms": {}}
    for name, t in times.items():
        t = np.array(t)
        fin = int(np.isfinite(run[name][1].cpu().numpy()).sum())
        res["forms"][name] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max()),
                              "finite_lnl": fin, "n_param": len(run[name][2].param_names)}
    base = res["forms"]["base"]["ms_median"]
    for n, idx in sel.items():
        flops = sum(2.0 * len(psrs[i].toas) * 16 * ((forms["base"].signal_collections[i].T.shape[1] + 16) // 16) * B
                    for i in idx)
        extra = (res["forms"][f"delay{n}"]["ms_median"] - base) / n
        row = {"pulsars": list(idx), "n_toa": [len(psrs[i].toas) for i in idx],
               "delay_extra_ms_per_pulsar": extra, "gemm_gflop": flops / 1e9,
               "gemm_share_of_fp64_mfma_peak_lower_bound":
                   (flops / n) / (extra * 1e-3) / FP64_MFMA_PEAK if extra > 0 else None}
        if not args.skip_efac:
            row["efac_extra_ms_per_pulsar"] = (res["forms"][f"efac{n}"]["ms_median"] - base) / n
        res[f"per_pulsar_{n}"] = row
    outdir = os.path.join(ROOT, "profiles", args.tag)
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "delay_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
