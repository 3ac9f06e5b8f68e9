"""Bit-identity of the legacy correlated models (one process, one fixed ORF)
across two builds of the library: the lnL of every correlated golden fixture
under the library EWARP_HIP_LIB names, saved to (or compared with) an .npz.

    EWARP_HIP_LIB=.../libewarp_hip_prev.so python scripts/corr_legacy_bitid.py save bench_out/corr.npz
    python scripts/corr_legacy_bitid.py compare bench_out/corr.npz

The saving side may be an older checkout (its own package and library): only
the fixture files and the .npz are shared.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ["c5_small", "c5_mono", "c5_dipo", "c5_noauto", "c5_varwn", "c5_f16", "c5_f23", "c5_f24v", "c5_f31", "c5_f90"]


def main():
    from conftest import load_golden
    from enterprise_warp_amd import _lib
    what, path = sys.argv[1], sys.argv[2]
    got = {}
    for name in NAMES:
        pta, X, _, _ = load_golden(name)
        got[name] = pta.get_lnlikelihood_batch(X)
        got[name + "_b1"] = np.concatenate([pta.get_lnlikelihood_batch(X[i:i + 1]) for i in range(len(X))])
        pta._drop_engine()
    print("library:", _lib.LIB_PATH, "ABI", _lib.EWH_ABI_VERSION)
    if what == "save":
        np.savez(path, **got)
        print(f"saved {len(got)} arrays")
        return
    ref = np.load(path)
    same = True
    for k, v in got.items():
        eq = np.array_equal(ref[k], v, equal_nan=True)
        same = same and eq
        print(f"{k}: bit-identical={eq} ({len(v)} draws, {int(np.sum(~np.isfinite(v)))} -inf)")
    print(f"legacy correlated fixtures, batch and one-by-one: bit-identical={same}")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
