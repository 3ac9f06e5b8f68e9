"""Several correlated common processes and sampled-parameter ORFs in the
device-side debug build (build/libewarp_hip_debug.so, -DEWH_DEBUG: `make -C
enterprise_warp_amd/csrc debug`): the EWH_DCHECKs of the term-form M_g kernels
(the term count against the LDS weights, their extent inside the dynamic LDS)
and those of the kernels around them hold on mc_three (four sub-terms),
mc_binorf (eight terms, indefinite draws; also in modes 7, the LDS M_g kernel,
and 27) and mc_varwn (varying white noise).
The tests run in a child process on the debug library (EWARP_HIP_LIB).  Marker
gpu_debug: outside the -m gpu suite."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "build", "libewarp_hip_debug.so")
CASES = "(test_parity and (mc_three or mc_binorf or mc_varwn)) or (test_kernel_modes_match_default and mc_binorf)"

pytestmark = pytest.mark.gpu_debug


def test_debug_build_multi_common_kernels(require_gpu):
    if not os.path.exists(DEBUG_LIB):
        pytest.fail(f"{DEBUG_LIB} not built: make -C enterprise_warp_amd/csrc debug")
    env = dict(os.environ, EWARP_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_multi_common.py"), "-m", "gpu", "-k", CASES],
                       env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    print(out[-4000:])
    assert "EWH_DCHECK failed" not in out, "a device invariant failed in the debug build"
    assert "5 passed" in out and r.returncode == 0, f"multi-common tests on the debug library: rc {r.returncode}"
