"""The conditional-GP kernels (csrc/cond.hip) in the device-side debug build
(build/libewarp_hip_debug.so, -DEWH_DEBUG: `make -C enterprise_warp_amd/csrc
debug`): their EWH_DCHECK bound checks -- panel and trailing-tile indices, the
V / Y indices against the padded chunk, the status slot -- hold on c1_j1832
(326 TOAs, the TOA tail) and c2_small (ECORR epochs).  The criterion tests run
in a child process on the debug library (EWARP_HIP_LIB).  Marker gpu_debug:
outside the -m gpu suite."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "build", "libewarp_hip_debug.so")
CASES = "test_criterion and (c1_j1832 or c2_small)"

pytestmark = pytest.mark.gpu_debug


def test_debug_build_cond_kernels(require_gpu):
    if not os.path.exists(DEBUG_LIB):
        pytest.fail(f"{DEBUG_LIB} not built: make -C enterprise_warp_amd/csrc debug")
    env = dict(os.environ, EWARP_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_cond_gp.py"), "-m", "gpu", "-k", CASES],
                       env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert "EWH_DCHECK failed" not in out, "a device invariant failed in the debug build"
    assert "2 passed" in out and r.returncode == 0, f"conditional-GP tests on the debug library: rc {r.returncode}"
