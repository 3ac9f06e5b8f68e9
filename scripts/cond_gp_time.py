"""Timing of the conditional GP (ConditionalGP.processes_batch -> ewh_cond_gp)
on synth's C3 shape (45 pulsars, fixed white noise) at B = 64 and 256 with
three groups (timing model, red noise + gw, DM), against the same work in
enterprise's order on the host (fp64 scipy cho_factor / cho_solve /
solve_triangular per pulsar per sample on the cached TNT, then T b per group).

The library has no per-stage timers; the stages are separated by calls that
stop earlier: coefficients only without output copy (matrix route + solve +
pack), coefficients with their copy, and the full call (+ the process GEMM and
its copy).  Differences of medians, so a stage can read slightly negative.

    python scripts/cond_gp_time.py [--psr 45] [--reps 5] > profiles/r11/cond_gp_time.txt
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def host_enterprise_order(pta, X, z, groups, n_host):
    import scipy.linalg as sl
    from oracle.enterprise_ref import OraclePTA
    const = pta.constant_values()
    o = OraclePTA([c.psr for c in pta.signal_collections], pta.oracle_terms(), fixed_params=const)
    t0 = time.perf_counter()
    for b in range(n_host):
        d = dict(const)
        d.update(pta.map_params(X[b]))
        off = 0
        for pp, (TNT, TNr, _, _), cols in zip(o.pulsars, o.fixed, groups):
            m = TNT.shape[0]
            cf = sl.cho_factor(TNT + np.diag(1.0 / pp.phi(d)), lower=True)
            coef = sl.cho_solve(cf, TNr) + sl.solve_triangular(cf[0], z[b, off:off + m], lower=True, trans="T")
            for cc in cols:
                pp.T[:, cc] @ coef[cc]
            off += m
    return (time.perf_counter() - t0) / n_host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--psr", type=int, default=45)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-samples", type=int, default=4)
    a = ap.parse_args()
    from enterprise_warp_amd import ConditionalGP, synth
    cfg = synth.config_c3(n_psr=a.psr)
    pta = cfg.pta
    cg = ConditionalGP(pta)
    eng = cg._engine()
    names = ["timing_model", "red_noise", "dm_gp"]
    col_group = np.full(cg.n_coef, -1, np.int32)
    groups = []
    for p, sc in enumerate(cg.signal_cols):
        groups.append([sc[n] for n in names])
        for g, n in enumerate(names):
            col_group[cg.col_off[p] + sc[n]] = g
    print(f"conditional GP timing: C3 shape, {len(pta.pulsars)} pulsars, n_coef {cg.n_coef}, "
          f"n_toa_total {cg.n_toa_total}, fixed white noise, groups {names}")
    print("(first numbers for this path: the parent commit has no conditional GP)")
    for B in (64, 256):
        X = synth.near_draws(pta, cfg.truth, B, 3)
        z = cg.draw_normals(B, 11)
        t_solve = median_time(lambda: eng.cond_gp(X, z=z, want_coef=False), a.reps)
        t_coef = median_time(lambda: eng.cond_gp(X, z=z), a.reps)
        t_full = median_time(lambda: eng.cond_gp(X, z=z, col_group=col_group, n_group=3, want_coef=False), a.reps)
        t_api = median_time(lambda: cg.processes_batch(X, z=z, signals=names), a.reps)
        host = host_enterprise_order(pta, X, z, groups, min(a.host_samples, B))
        print(f"B = {B}")
        print(f"  matrix route + solve + pack            {1e3 * t_solve:10.2f} ms")
        print(f"  + coefficient copy to the host         {1e3 * (t_coef - t_solve):10.2f} ms")
        print(f"  process GEMM + realisation copy        {1e3 * (t_full - t_solve):10.2f} ms")
        print(f"  ewh_cond_gp, three groups              {1e3 * t_full:10.2f} ms  ({1e3 * t_full / B:.3f} ms per sample)")
        print(f"  ConditionalGP.processes_batch          {1e3 * t_api:10.2f} ms")
        print(f"  host, enterprise order (1 core, measured on {min(a.host_samples, B)} samples) "
              f"{1e3 * host * B:10.2f} ms  ({1e3 * host:.3f} ms per sample)")
        print(f"  ratio host / device                    {host * B / t_full:10.1f} x")


if __name__ == "__main__":
    main()
