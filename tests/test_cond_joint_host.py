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


OLDER = ["c5_small", "c5_mono", "c5_dipo", "c5_varwn", "mc_hd_mono", "synth7", "c5_noauto"]
WIDE = ["synth7_nc40", "synth7_nc40_varwn", "synth7_nc48_lead"]


def _shape(cs):
    """The loop structure a case gives the kernels of csrc/cond_joint.hip:
    nc, and per pulsar the own block's width in its slot (varying white noise:
    up to the 16-aligned common block, inner pads included), the padded order n
    of the slot's matrix, the pivot panels nbo and the trailing tiles nt per
    side of cj_eliminate; N_c and Npad of the dense stage."""
    cols = cs.pta.signal_collections
    nc, P = len(cols[0].common_cols), len(cols)
    assert all(len(c.common_cols) == nc for c in cols) and all(cs.mo[p] + nc == cs.m[p] for p in range(P))
    mo = list(cs.mo) if cs.pta.white_fixed() else [16 * -(-nlo // 16) for nlo in cs.mo]
    n = [16 * -(-(w + nc) // 16) for w in mo]
    nbo = [-(-w // 16) for w in mo]
    nt = [a // 16 - b for a, b in zip(n, nbo)]
    return dict(nc=nc, mo=mo, n=n, nbo=nbo, nt=nt, N_c=P * nc, Npad=16 * -(-P * nc // 16))


def test_new_cases_hit_the_shapes_they_are_for():
    """The wide synthetic cases pin the loop structure they were added for
    (7 pulsars, n_tm = 11 / 12 / 13 in turn), so that an edit to synth cannot
    move one silently back to a single trailing tile; every older case has one
    trailing tile per side and a dense stage of at most 128 rows."""
    i3 = [i % 3 for i in range(7)]
    want = {
        # off-diagonal Schur tiles, waves 1-2; mo = 32 (a full last panel) beside 31 and 33; Npad > 256
        "synth7_nc40": dict(nc=40, mo=[31 + i for i in i3], n=[80] * 7, nbo=[(2, 2, 3)[i] for i in i3],
                            nt=[(3, 3, 2)[i] for i in i3], N_c=280, Npad=288),
        # nlo = 31 / 32 / 33: 1, 0 and 15 inner pads; n = 96
        "synth7_nc40_varwn": dict(nc=40, mo=[(32, 32, 48)[i] for i in i3], n=[(80, 80, 96)[i] for i in i3],
                                  nbo=[(2, 2, 3)[i] for i in i3], nt=[3] * 7, N_c=280, Npad=288),
        # a single (masked) pivot panel; N_c a multiple of 16: no identity pad rows
        "synth7_nc48_lead": dict(nc=48, mo=[11 + i for i in i3], n=[64] * 7, nbo=[1] * 7, nt=[3] * 7, N_c=336,
                                 Npad=336),
    }
    assert sorted(want) == sorted(WIDE)
    for name in WIDE:
        cs = jr.case(name)
        assert _shape(cs) == want[name], name
        assert cs.m == [a + want[name]["nc"] for a in cs.mo] and len(cs.psrs) == 7
    assert jr.case("synth7_nc40_varwn").mo == [31 + i for i in i3]
    assert len(jr.case("synth7_nc40_varwn").pta.param_names) == 114
    for name in OLDER:
        s = _shape(jr.case(name))
        assert set(s["nt"]) == {1} and s["Npad"] <= 128, (name, s)


@pytest.mark.parametrize("name", WIDE)
def test_four_stages_meet_the_cases_own_floor(name):
    """The fp64 staged restatement on the wide cases, against the long-double
    reference: mean and draw within the case's own coefficient floor (4 x
    enterprise order's worst near-row error) on every near row.  (Not the 1e-9
    of test_four_stages_equal_the_joint_dense_solve: that compares two fp64
    orders, whose own errors here reach 2e-9 sigma.)"""
    cs = jr.case(name)
    ce, _ = cs.ent_errors()
    floor = 4.0 * max(v for (p, b, kind), v in ce.items() if cs.near[b])
    worst = [0.0, 0.0]
    for b in np.flatnonzero(cs.near):
        for kind, z in enumerate((None, cs.z[b])):
            worst[kind] = max(worst[kind], max(cs.coef_err(b, jr.four_stages(cs, b, z), kind)))
    print(f"{name}: four stages vs long double, near rows: mean {worst[0]:.3e}, draw {worst[1]:.3e} sigma; "
          f"floor {floor:.3e}")
    assert max(worst) <= floor


@pytest.mark.parametrize("name", OLDER + WIDE)
def test_reference_stands_on_every_row_but_the_goldens_inf_rows(name):
    """Both references succeed on every row of every case the device test
    uses, except exactly the -inf rows of c5_noauto's golden."""
    cs = jr.case(name)
    ref = cs.references()
    ok = ref["ok"]
    assert np.array_equal(~ok, cs.inf_rows) and ok[cs.near].all()
    assert cs.inf_rows.any() == (name == "c5_noauto")
    assert sorted(ref["ent"]) == sorted(ref["exact"]) == list(np.flatnonzero(ok))
