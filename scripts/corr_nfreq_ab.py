"""The C5 workload (100 psr x 20k TOAs, fixed white noise) with the correlated
process on N common frequencies (default hd_vary_gamma_30_nfreqs: 60 common
columns, kept block KD = 64): the per-pulsar partial step (ewh_corr_partial_
device) and the dense stage (ewh_corr_finish_device) timed apart with device
events, the default route (chol_mfma_kernel<NB, KEEP = 4> where it is built)
alternated with kernel mode 27 (chol_wide_kernel for every factorisation), one
process.  Prints ms per batch per form, the spread over the alternations, the
dense stage's fraction of the fp64 MFMA peak and whether the two routes' lnL
agree.  python scripts/corr_nfreq_ab.py [--nfreq 30] [--B 64] [--rounds 7]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nfreq", type=int, default=30)
    ap.add_argument("--own-nfreq", type=int, default=30)
    ap.add_argument("--modes", default="0,27")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--n-psr", type=int, default=100)
    ap.add_argument("--n-toa", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from bench import FP64_MFMA_PEAK_TFLOPS
    from enterprise_warp_amd import synth
    cfg = synth.config_c5(n_psr=args.n_psr, n_toa=args.n_toa, gwb=f"hd_vary_gamma_{args.nfreq}_nfreqs",
                          nfreqs=args.own_nfreq)
    pta = cfg.pta
    eng = pta.engine(0)
    P, B = len(pta.signal_collections), args.B
    kd = eng.keep_dim()
    nc = pta.common_layout()["n_col"]
    blocks = sorted({((L["T"].shape[1] - L["n_lead"] - L["n_common"] + 15) // 16 + kd // 16, kd // 16)
                     for L in pta.layout()})
    X = synth.prior_draws(pta, B, cfg.theta_seed)
    th = torch.from_numpy(X).cuda()
    keep = torch.zeros((P, B, kd, kd), dtype=torch.float64, device="cuda")
    local = torch.zeros((P, B), dtype=torch.float64, device="cuda")
    out = torch.zeros(B, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream()
    s = st.cuda_stream

    def partial():
        eng.corr_partial_device(th.data_ptr(), B, 0, P, keep.data_ptr(), local.data_ptr(), s)

    def finish():
        eng.corr_finish_device(th.data_ptr(), B, keep.data_ptr(), local.data_ptr(), out.data_ptr(), s)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    modes = [int(v) for v in args.modes.split(",")]
    t_part = {md: [] for md in modes}
    t_dense = {md: [] for md in modes}
    vals = {}
    for r in range(args.rounds + 1):            # (round 0 warms every form up and is dropped)
        for md in modes:
            eng.set_kernel_mode(md)
            tp = timed(partial)
            td = timed(finish)
            if r > 0:
                t_part[md].append(tp)
                t_dense[md].append(td)
            vals[md] = out.cpu().numpy().copy()
    eng.set_kernel_mode(0)
    dense_flops = (P * nc + 1) ** 3 / 3.0 * B
    res = {"workload": {"n_psr": P, "n_toa": args.n_toa, "B": B, "common_freqs": args.nfreq, "common_cols": nc,
                        "KD": kd, "reduced_blocks_nb_keep": blocks, "rounds": args.rounds}}
    for md in modes:
        pm, dm = float(np.median(t_part[md])), float(np.median(t_dense[md]))
        res[f"mode{md}"] = {"partial_ms_median": pm, "partial_ms_min": min(t_part[md]), "partial_ms_max": max(t_part[md]),
                            "partial_ms_all": t_part[md], "dense_ms_median": dm, "dense_ms_min": min(t_dense[md]),
                            "dense_ms_max": max(t_dense[md]),
                            "dense_fp64_mfma_frac": dense_flops / (dm * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS}
    first = vals[modes[0]]
    fin = np.isfinite(first)
    for md in modes[1:]:
        same_inf = bool(np.array_equal(np.isfinite(vals[md]), fin))
        err = np.abs(vals[md][fin] - first[fin]) / (1e-6 + 1e-10 * np.abs(first[fin])) if fin.any() else np.zeros(1)
        res[f"mode{md}"]["vs_first"] = {"same_inf_pattern": same_inf, "max_err_over_strict": float(err.max()),
                                        "bit_identical": bool(np.array_equal(vals[md], first))}
    res["finite_fraction"] = float(fin.mean())
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
