"""Buffer growth on one handle (csrc/ewarp_mem.h: every growable device and
pinned buffer is a Buf, the two chunk scratches are groups of them): batch
sizes that grow, shrink and grow again must give the bits of a fresh handle.
One golden per scratch family, at the golden shapes -- the smallest at which
a stale pointer or a wrong capacity can still show."""
import numpy as np
import pytest

import _delay_common as dc
from conftest import load_golden

pytestmark = pytest.mark.gpu

# (fixture, device list): what the handle allocates
CASES = [
    ("c2_small", [0]),         # the varying-WN chunk
    ("c5_small", [0]),         # kept blocks + the correlated chunk
    ("c5_varwn", [0]),         # both chunks
    ("c1_widefix", [0]),       # dd / wide scratch, d_units2, d_ddlist
    ("c1_system", [0]),        # big scratch
    ("delay:c1_j1832", [0]),   # the delay buffers (the smallest fixture of test_gpu_delay.py: one pulsar, 326 TOAs)
    ("c3_small", [0, 0]),      # two contexts: d_stage, d_seg, d_part
]


def _model(name):
    if name.startswith("delay:"):
        c = dc.case(name[len("delay:"):], (0,))
        return c.pta, c.Xa
    pta, X, _, _ = load_golden(name)
    return pta, X


@pytest.mark.parametrize("name,devices", CASES, ids=[f"{n}-{len(d)}ctx" for n, d in CASES])
def test_growth_cycles_bit_identical(require_gpu, name, devices):
    """The golden's 16 samples at B = 16 on a fresh handle are the reference;
    a second handle then runs B = 1, 16, 2, 48 (the rows three times), 16, 1:
    every value equals the reference row bit for bit."""
    pta, X = _model(name)
    X = np.ascontiguousarray(X)
    assert len(X) == 16
    try:
        pta._drop_engine()
        assert pta.engine(devices=devices).num_devices() == len(devices)
        ref = pta.get_lnlikelihood_batch(X)
        assert not np.any(np.isnan(ref)) and np.any(np.isfinite(ref))
        pta._drop_engine()
        eng = pta.engine(devices=devices)
        for rows, want in ((X[:1], ref[:1]), (X, ref), (X[:2], ref[:2]), (np.vstack([X] * 3), np.tile(ref, 3)),
                           (X, ref), (X[:1], ref[:1])):
            assert pta.engine() is eng                 # one handle throughout
            got = pta.get_lnlikelihood_batch(rows)
            print(f"{name} on {devices}: B = {len(rows)}, max |got - ref| = "
                  f"{np.nanmax(np.abs(np.where(got == want, 0.0, got - want))):.3e}")
            np.testing.assert_array_equal(got, want)
    finally:
        pta._drop_engine()
        pta._engine_devices = None
