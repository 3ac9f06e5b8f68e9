"""Joint conditional GP (ABI 11: ewh_cond_joint_dims / ewh_cond_joint,
enterprise_warp_amd.JointConditionalGP) on the CPU: construction and the
column permutation without a device, the refusals on both sides, the exports
of both libraries, and the ordering and z convention pinned in numpy -- the
four stages of include/ewarp_hip.h against one dense Cholesky of the joint
Sigma (tests/_cond_joint_ref.py)."""
import ctypes
import os

import numpy as np
import pytest

import _cond_joint_ref as jr
from conftest import load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "enterprise_warp_amd", "libewarp_cpu.so")


def test_constructs_on_a_correlated_model_without_a_device():
    from enterprise_warp_amd import JointConditionalGP
    pta, _, _, _ = load_golden("c5_small")
    jg = JointConditionalGP(pta)
    cols = pta.signal_collections
    assert jg.n_coef == sum(c.T.shape[1] for c in cols) == 4 * 52
    assert jg.n_toa_total == sum(len(c.psr.toas) for c in cols)
    assert jg.names == pta.pulsars and pta._engine is None          # no engine, no device
    for p, c in enumerate(cols):
        assert list(jg.signal_cols[p]) == ["timing_model", "gw", "red_noise", "dm_gp"]
        assert np.array_equal(jg.signal_cols[p]["gw"], c.common_cols)
    for meth in ("coefficients_batch", "processes_batch", "get_mean_coefficients", "sample_coefficients",
                 "get_mean_processes", "sample_processes", "draw_normals"):
        assert callable(getattr(jg, meth))
    assert jg.draw_normals(3, rng=1).shape == (3, jg.n_coef)


def test_layout_order_round_trip():
    pta, _, _, _ = load_golden("c5_small")
    for L, c in zip(pta.layout(), pta.signal_collections):
        order, m = L["order"], c.T.shape[1]
        assert sorted(order) == list(range(m))
        assert np.array_equal(L["T"], c.T[:, order])                   # descriptor column k = T column order[k]
        assert list(order[m - L["n_common"]:]) == list(c.common_cols)   # [lead | own | common]
        assert list(order[:c.n_lead_const]) == list(range(c.n_lead_const))
        back = np.empty(m, int)
        back[order] = np.arange(m)
        assert np.array_equal(L["T"][:, back], c.T)
    pta3, _, _, _ = load_golden("c3_small")
    for L, c in zip(pta3.layout(), pta3.signal_collections):
        assert np.array_equal(L["order"], np.arange(c.T.shape[1]))      # uncorrelated: the identity


def test_refusals():
    from enterprise_warp_amd import ConditionalGP, JointConditionalGP
    c3, _, _, _ = load_golden("c3_small")
    with pytest.raises(ValueError):
        JointConditionalGP(c3)
    c5, _, _, _ = load_golden("c5_small")
    with pytest.raises(NotImplementedError):
        ConditionalGP(c5)
    with pytest.raises(TypeError):
        JointConditionalGP(object())


def test_exports_and_abi_version():
    from enterprise_warp_amd import _lib
    assert {"ewh_cond_joint_dims", "ewh_cond_joint"} <= set(_lib.EXPORTS) and _lib.EWH_ABI_VERSION >= 11
    with open(os.path.join(ROOT, "include", "ewarp_hip.h")) as f:
        assert f"#define EWH_ABI_VERSION {_lib.EWH_ABI_VERSION}\n" in f.read()


def test_twin_has_the_symbols_and_refuses():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "enterprise_warp_amd", "csrc"), "cpu"], check=True,
                       capture_output=True)
    from enterprise_warp_amd import _lib
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "ewh_cond_joint_dims") and hasattr(lib, "ewh_cond_joint")
    lib.ewh_version.restype = ctypes.c_int
    assert lib.ewh_version() == _lib.EWH_ABI_VERSION
    lib.ewh_cond_joint_dims.restype = ctypes.c_int
    assert lib.ewh_cond_joint_dims(None, None, None) == -4             # EWH_E_UNSUPPORTED


@pytest.mark.parametrize("name", ["c5_small", "c5_varwn"])
def test_four_stages_equal_the_joint_dense_solve(name):
    """The staged solve (own blocks, Sigma_c over (pulsar, column), back-
    substitution) and one Cholesky of the joint-ordered Sigma give the same
    mean and the same draw from the same z indexed by coefficient: worst
    |L^T (a - b)| <= 1e-9 sigma over the 4 prior and 4 near rows."""
    cs = jr.case(name)
    ref = cs.references()
    worst = {True: 0.0, False: 0.0}
    for b in range(len(cs.X)):
        for z in (None, cs.z[b]):
            a, d = jr.four_stages(cs, b, z), jr.joint_dense(cs, b, z)
            err = float(np.max(np.abs(ref["L"][b].T @ (a - d).astype(jr.LD)[cs.perm])))
            worst[bool(cs.near[b])] = max(worst[bool(cs.near[b])], err)
    print(f"{name}: four stages vs joint dense, worst {worst[True]:.3e} sigma (near rows), "
          f"{worst[False]:.3e} sigma (prior rows)")
    assert max(worst.values()) <= 1e-9
    # and the convention is the reference's: the dense solve is enterprise order's
    for b in np.flatnonzero(cs.near):
        assert np.array_equal(jr.joint_dense(cs, b, cs.z[b]), ref["ent"][b][1])
        assert np.array_equal(jr.joint_dense(cs, b), ref["ent"][b][0])


@pytest.mark.parametrize("name", ["c5_small", "c5_mono", "c5_dipo", "c5_varwn", "mc_hd_mono", "synth7", "c5_noauto"])
def test_reference_stands_on_every_row_but_the_goldens_inf_rows(name):
    """Both references succeed on every row of every case the device test
    uses, except exactly the -inf rows of c5_noauto's golden."""
    cs = jr.case(name)
    ref = cs.references()
    ok = ref["ok"]
    assert np.array_equal(~ok, cs.inf_rows) and ok[cs.near].all()
    assert cs.inf_rows.any() == (name == "c5_noauto")
    assert sorted(ref["ent"]) == sorted(ref["exact"]) == list(np.flatnonzero(ok))
