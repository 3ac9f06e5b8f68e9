"""First timings of the joint conditional GP (JointConditionalGP ->
ewh_cond_joint, csrc/cond_joint.hip) at B = 16 with two groups (the common
process, everything else), on
  synth7   the 7-pulsar test case of tests/_cond_joint_ref.py (N_c = 126)
  c5r16    the 16-pulsar reduced C5 shape: synth.config_c5(n_psr=16,
           n_toa=2000), Hellings-Downs on 14 frequencies (N_c = 448)
with the wall time of a numpy fp64 reference (one scipy cho_factor of the
joint Sigma per sample, both solves, T b per group) beside it for scale only.
Nobody has measured this route before: there is no parent timing and no target.

The library has no per-stage timers.  Wall times come from this script; the
per-stage split comes from a kernel trace of the same calls:

    rocprofv3 --kernel-trace --stats -d DIR -o joint --output-format csv -- \\
        python scripts/cond_joint_time.py --case c5r16 --calls 3 --no-host
    python scripts/cond_joint_time.py --fold DIR --calls 3

--fold sums the kernels' TotalDurationNs by stage -- partial (the broadcast of
the cached Gram, cond_joint_partial), assemble + dense
(the M_g inverses, cond_joint_assemble, cond_joint_dense), back + process
(cond_joint_back, cond_pack, cond_process) -- and divides by the calls; the
first call's one-off kernels (the kept Grams of setup_fixed) and the copies
are "other".
"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = (("partial", ("cond_joint_partial", "gram_broadcast")),
          ("assemble + dense", ("common_minv", "cond_joint_assemble", "cond_joint_dense")),
          ("back + process", ("cond_joint_back", "cond_pack", "cond_process")))


def fold(directory, calls):
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_stats.csv under {directory}")
    tot = {s: 0.0 for s, _ in STAGES}
    other = 0.0
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            for s, keys in STAGES:
                if any(k in row["Name"] for k in keys):
                    tot[s] += ns
                    break
            else:
                other += ns
    print(f"  kernel time per call by stage ({calls} calls traced, {os.path.relpath(files[0], directory)}):")
    for s, _ in STAGES:
        print(f"    {s:<20s}{tot[s] / calls * 1e-6:10.3f} ms")
    print(f"    {'other kernels':<20s}{other / calls * 1e-6:10.3f} ms")


def build(case):
    from enterprise_warp_amd import synth
    if case == "synth7":
        import _cond_joint_ref as jr
        pta, theta, near = jr.synth_case_pta()
        return pta, theta[near], "7 pulsars x 250 TOAs, hd_vary_gamma_9_nfreqs"
    cfg = synth.config_c5(n_psr=16, n_toa=2000)
    return cfg.pta, synth.near_draws(cfg.pta, cfg.truth, 16, 3), "16 pulsars x 2000 TOAs, hd_vary_gamma_14_nfreqs"


def host_reference(pta, X, z, perm, groups):
    """One joint cho_factor per sample in fp64 (enterprise order), seconds per sample."""
    import scipy.linalg as sl
    from oracle.enterprise_ref import OraclePTA
    const = pta.constant_values()
    o = OraclePTA([c.psr for c in pta.signal_collections], pta.oracle_terms(), fixed_params=const)
    t0 = time.perf_counter()
    for b in range(len(X)):
        d = dict(const)
        d.update(pta.map_params(X[b]))
        Phi, off = o.phi_global(d)
        Sg, _ = o.phiinv_cliques(Phi)
        dv = np.zeros(len(perm))
        for p, (TNT, TNr, _, _) in enumerate(o.fixed):
            Sg[off[p]:off[p + 1], off[p]:off[p + 1]] += TNT
            dv[off[p]:off[p + 1]] = TNr
        cf = sl.cho_factor(Sg[np.ix_(perm, perm)], lower=True)
        coef = np.zeros(len(perm))
        coef[perm] = sl.cho_solve(cf, dv[perm]) + sl.solve_triangular(cf[0], z[b][perm], lower=True, trans="T")
        for p, pp in enumerate(o.pulsars):
            for cc in groups[p]:
                pp.T[:, cc] @ coef[off[p] + cc]
    return (time.perf_counter() - t0) / len(X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["synth7", "c5r16"], default="synth7")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--host-samples", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--fold", metavar="DIR")
    a = ap.parse_args()
    if a.fold:
        return fold(a.fold, a.calls)
    from enterprise_warp_amd import JointConditionalGP
    pta, X, what = build(a.case)
    B = 16
    X = np.ascontiguousarray(X[np.arange(B) % len(X)])
    jg = JointConditionalGP(pta)
    eng = jg._engine()
    z = jg.draw_normals(B, 11)
    col_group = np.ones(jg.n_coef, np.int32)
    groups, own, com = [], [], []
    for p, c in enumerate(pta.signal_collections):
        cc = np.asarray(c.common_cols, int)
        rest = np.setdiff1d(np.arange(c.T.shape[1]), cc)
        col_group[jg.col_off[p] + cc] = 0
        groups.append([cc, rest])
        own += list(jg.col_off[p] + rest)
        com += list(jg.col_off[p] + cc)
    perm = np.array(own + com, int)
    n_common = len(pta.signal_collections[0].common_cols)
    print(f"joint conditional GP timing, {a.case}: {what}; n_coef {jg.n_coef}, N_c {len(com)} "
          f"({len(pta.pulsars)} x {n_common}), n_toa_total {jg.n_toa_total}, fixed white noise, B = {B}, two groups")
    ts = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        _, _, st = eng.cond_joint(X, z=z, col_group=col_group, n_group=2, want_coef=False)
        ts.append(time.perf_counter() - t0)
    assert not st.any(), st
    print(f"  ewh_cond_joint, wall, per call: first {ts[0] * 1e3:.2f} ms (allocations, the kept Grams), "
          f"then median {np.median(ts[1:]) * 1e3:.2f} ms ({np.median(ts[1:]) / B * 1e3:.3f} ms per sample)")
    if not a.no_host:
        th = host_reference(pta, X[:a.host_samples], z, perm, groups)
        print(f"  numpy reference, enterprise order (measured on {a.host_samples} samples; scale only): "
              f"{th * B * 1e3:.2f} ms for B = {B} ({th * 1e3:.3f} ms per sample)")


if __name__ == "__main__":
    main()
