"""The operand images against the reduced matrix they are built from (dev
library libewarp_hip_dev.so; marker gpu_ab, in a separate process as
test_gpu_ab.py): two-block frames with 3 / 7 / 11 / 15 pads and one
eight-block frame with 7 pads; S_p and both images are read back and every
image element is compared with S under the index map of csrc/ewarp_dev.h
recomputed in numpy (tests/_operand_image_worker.py)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu_ab


def test_images_equal_reduced_matrix_under_index_map():
    lib = os.path.join(ROOT, "enterprise_warp_amd", "libewarp_hip_dev.so")
    if not os.path.exists(lib):
        pytest.skip("dev library not built (make -C enterprise_warp_amd/csrc dev)")
    env = dict(os.environ, EWARP_HIP_LIB=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_operand_image_worker.py")],
                       capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0
