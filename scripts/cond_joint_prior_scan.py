"""How the prior rows of the synthetic joint-GP cases (tests/_cond_joint_ref.py,
SYNTH) were picked: with the two references alone, no device.  For every draw
synth.prior_draws(pta, 8, seed)[index] of the seeds asked for, fp64 enterprise
order (scipy cho_factor on the joint-ordered Sigma) either raises or stands;
on the standing draws both references are built and the draw's enterprise-order
coefficient error -- worst over pulsars, mean and draw, in posterior standard
deviations -- is printed.  The recipe keeps the four smallest.

  python scripts/cond_joint_prior_scan.py synth7_nc40 [--seeds 20 60]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _cond_joint_ref as jr  # noqa: E402
from enterprise_warp_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("case", choices=sorted(jr.SYNTH))
    ap.add_argument("--seeds", type=int, nargs=2, default=(20, 60), metavar=("FIRST", "END"))
    a = ap.parse_args()
    cs = jr.JointCase(a.case)
    pairs = [(s, i) for s in range(*a.seeds) for i in range(8)]
    X = np.array([synth.prior_draws(cs.pta, 8, s) for s in range(*a.seeds)]).reshape(len(pairs), -1)
    # a candidate batch in place of the case's rows: all prior rows, their own normals
    cs.X, cs.near, cs._ref = X, np.zeros(len(X), bool), None
    cs.z = np.random.default_rng(jr.Z_SEED).standard_normal((len(X), cs.n_coef))
    stands = []
    for b in range(len(X)):
        try:
            jr.joint_dense(cs, b)
            stands.append(b)
        except np.linalg.LinAlgError:
            pass
    print(f"{a.case}: enterprise order stands on {len(stands)} of {len(X)} draws")
    cs.X, cs.z, cs.near = X[stands], cs.z[stands], cs.near[stands]
    ok = cs.references()["ok"]
    ce, _ = cs.ent_errors()
    worst = {}
    for (p, b, kind), v in ce.items():
        worst[b] = max(worst.get(b, 0.0), v)
    rows = sorted((worst[b], pairs[stands[b]]) for b in worst)
    for e, pr in rows:
        print(f"  {pr}: {e:.1e} sigma")
    print("long-double reference fails on:", [pairs[stands[b]] for b in np.flatnonzero(~ok)])
    print("the four smallest:", tuple(sorted(pr for _, pr in rows[:4])), [f"{e:.1e}" for e, _ in rows[:4]])


if __name__ == "__main__":
    main()
