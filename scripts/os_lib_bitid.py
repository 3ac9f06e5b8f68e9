"""Bit-identity of the optimal statistic across two builds of the library: the
OS, OS_sig, rho and sig of the c3_small fixture (CURN, 14 frequencies: 28
common columns, os_xz_kernel's range) for HD, monopole and dipole under the
library EWARP_HIP_LIB names, saved to (or compared with) an .npz.

    EWARP_HIP_LIB=.../libewarp_hip_prev.so python scripts/os_lib_bitid.py save bench_out/os.npz
    python scripts/os_lib_bitid.py compare bench_out/os.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from conftest import load_golden
    from enterprise_warp_amd import _lib
    from enterprise_warp_amd.optstat import OptimalStatistic
    what, path = sys.argv[1], sys.argv[2]
    pta, X, _, _ = load_golden("c3_small")
    got = {}
    for orf in ("hd", "monopole", "dipole"):
        ost = OptimalStatistic(pta, orf=orf)
        os_, os_sig, rho, sig = ost.compute_noise_marginalised_os(X, want_pairs=True)
        got.update({f"{orf}_os": os_, f"{orf}_os_sig": os_sig, f"{orf}_rho": rho, f"{orf}_sig": sig})
    print("library:", _lib.LIB_PATH)
    if what == "save":
        np.savez(path, **got)
        print(f"saved {len(got)} arrays of {len(X)} draws")
        return
    ref = np.load(path)
    same = all(np.array_equal(ref[k], v, equal_nan=True) for k, v in got.items())
    for k, v in got.items():
        print(f"{k}: bit-identical={np.array_equal(ref[k], v, equal_nan=True)}")
    print(f"optimal statistic on c3_small, 16 draws x 3 ORFs: bit-identical={same}")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
