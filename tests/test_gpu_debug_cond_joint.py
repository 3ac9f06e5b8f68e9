"""The joint conditional-GP kernels (csrc/cond_joint.hip) in the device-side
debug build (build/libewarp_hip_debug.so, -DEWH_DEBUG: `make -C
enterprise_warp_amd/csrc debug`): their EWH_DCHECK bound checks -- panel and
Schur tile indices, panel rows, the S slot, the status slot, the assemble and
dense shapes, the z index -- hold on synth7 (one trailing tile, masked
k-slices), synth7_nc40_varwn (off-diagonal Schur tiles, 0 / 1 / 15 inner pads,
n = 96, a dense stage of 288 rows), synth7_nc48_lead (a single pivot panel,
N_c = 336 with no pad rows) and on c5_noauto's failed rows.  The tests run in a
child process on the debug library (EWARP_HIP_LIB).  Marker gpu_debug: outside
the -m gpu suite."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "build", "libewarp_hip_debug.so")
CASES = ("(test_criterion and (synth7] or synth7_nc40_varwn or synth7_nc48_lead)) "
         "or test_indefinite_orf_rows_are_status_3")

pytestmark = pytest.mark.gpu_debug


def test_debug_build_cond_joint_kernels(require_gpu):
    if not os.path.exists(DEBUG_LIB):
        pytest.fail(f"{DEBUG_LIB} not built: make -C enterprise_warp_amd/csrc debug")
    env = dict(os.environ, EWARP_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_cond_joint.py"), "-m", "gpu", "-k", CASES],
                       env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert "EWH_DCHECK failed" not in out, "a device invariant failed in the debug build"
    assert "4 passed" in out and r.returncode == 0, f"joint conditional-GP tests on the debug library: rc {r.returncode}"
