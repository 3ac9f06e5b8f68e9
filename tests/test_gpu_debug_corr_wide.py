"""The correlated common process past 31 columns in the device-side debug
build (build/libewarp_hip_debug.so, -DEWH_DEBUG: `make -C enterprise_warp_amd/
csrc debug`): the EWH_DCHECK bound checks -- chol_wide_kernel's scratch slot,
its kept-block writes against KD x KD and the pulsar's slice of the kept
buffer, the register kernel's kept slice, os_xz_wide_kernel's LDS extents --
hold on c5_f16 (chol_mfma_kernel<5, 3>, KD = 48), c5_f24v (varying white
noise, chol_wide at keep = 4) and c5_f90 (keep = 12), and on the optimal
statistic at 62 columns.  The tests run in a child process on the debug
library (EWARP_HIP_LIB).  Marker gpu_debug: outside the -m gpu suite."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "build", "libewarp_hip_debug.so")
CASES = "(test_parity and (c5_f16 or c5_f24v or c5_f90)) or (test_os_at_62_columns and hd)"

pytestmark = pytest.mark.gpu_debug


def test_debug_build_corr_wide_kernels(require_gpu):
    if not os.path.exists(DEBUG_LIB):
        pytest.fail(f"{DEBUG_LIB} not built: make -C enterprise_warp_amd/csrc debug")
    env = dict(os.environ, EWARP_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_corr_wide.py"), "-m", "gpu", "-k", CASES],
                       env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert "EWH_DCHECK failed" not in out, "a device invariant failed in the debug build"
    assert "4 passed" in out and r.returncode == 0, f"corr-wide tests on the debug library: rc {r.returncode}"
