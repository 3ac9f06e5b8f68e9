"""Subprocess body of tests/test_gpu_ab_operand_image.py: runs on the dev
library (EWARP_HIP_LIB; the ctypes binding is process-global), reads back the
cached reduced matrix S_p and its operand images (ewh_dev_reduced,
ewh_dev_images) and compares every image element with S under the index map
of csrc/ewarp_dev.h (img_index, front_src), restated here in numpy."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def expected_image(S, s):
    """The image of S (ld x ld, ld = 16 nb) in the working order with s
    leading pads (0: the stored order): block t = (bi, bj >= bi) in row-major
    order, then half h = r // 2, lane (q, c), register parity r % 2; the
    element is (16 bi + q + 4 r, 16 bj + c) of the working order."""
    ld = S.shape[0]
    nb = ld // 16
    w = np.arange(ld)
    src = np.where(w < s, ld - 1 - s + w, np.where(w == ld - 1, w, w - s))     # front_src
    img = np.full(256 * (nb * (nb + 1) // 2), np.nan)
    lane = np.arange(64)
    q, c = lane >> 4, lane & 15
    t = 0
    for bi in range(nb):
        for bj in range(bi, nb):
            for r in range(4):
                off = 256 * t + 128 * (r >> 1) + 2 * lane + (r & 1)
                img[off] = S[src[16 * bi + q + 4 * r], src[16 * bj + c]]
            t += 1
    assert not np.isnan(img).any()              # every offset written (S itself has no NaN)
    return img


def main():
    from enterprise_warp_amd import _lib
    from test_gpu_front_pads import _c3_width, _pta
    assert _lib.LIB_PATH.endswith("libewarp_hip_dev.so"), _lib.LIB_PATH
    cases = [("pads3", lambda: _pta([29], 11), 3, 2), ("pads7", lambda: _pta([25], 12), 7, 2),
             ("pads11", lambda: _pta([21], 13), 11, 2), ("pads15", lambda: _pta([17], 14), 15, 2),
             ("c3_width", _c3_width, 7, 8)]
    for name, make, pads, nb in cases:
        pta, _ = make()
        sc = pta.signal_collections[0]
        width = sc.T.shape[1] - sc.n_lead_const + 1
        assert (16 * nb - width, -(-width // 16)) == (pads, nb), f"{name}: reduced width {width}"
        eng = pta.engine()
        S, _ = eng.dev_reduced(0, 16 * nb)
        assert np.isfinite(S).all()
        got_nb, img, front = eng.dev_images(0)
        assert got_nb == nb, f"{name}: image of {got_nb} blocks"
        np.testing.assert_array_equal(img, expected_image(S, 0), err_msg=f"{name}: stored-order image")
        if pads >= 4:
            assert front is not None, f"{name}: no front-order image"
            np.testing.assert_array_equal(front, expected_image(S, pads), err_msg=f"{name}: front-order image")
            assert not np.array_equal(front, img)
        else:
            assert front is None, f"{name}: a front-order image without a dead slice"
        print(f"{name}: {nb} blocks, {pads} pads, {img.size} doubles per image: equal")
        pta._drop_engine()


if __name__ == "__main__":
    main()
