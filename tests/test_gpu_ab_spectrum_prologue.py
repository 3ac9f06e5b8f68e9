"""tests/test_gpu_spectrum_prologue.py on the dev library (libewarp_hip_dev.so;
marker gpu_ab, in a separate process as test_gpu_ab.py): there every case is
also compared with kernel mode 14 -- the interpreted staged prologue forced
where the launch would take the fixed-form one -- over all its rows, and the
launch counters (ewh_dev_prologue_launches) show which prologue each batched
launch took, the fall-back cases included."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu_ab


def test_spectrum_prologue_on_dev_library():
    lib = os.path.join(ROOT, "enterprise_warp_amd", "libewarp_hip_dev.so")
    if not os.path.exists(lib):
        pytest.skip("dev library not built (make -C enterprise_warp_amd/csrc dev)")
    env = dict(os.environ, EWARP_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu",
                        os.path.join(ROOT, "tests", "test_gpu_spectrum_prologue.py")],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0
