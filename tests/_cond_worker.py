"""Subprocess body of tests/test_cond_gp_host.py: runs with EWARP_BACKEND=cpu,
so enterprise_warp_amd binds the host twin libewarp_cpu.so (the ctypes binding
is process-global), evaluates ewh_cond_gp on the cases of tests/_cond_ref.py
and writes the raw outputs to the .npz named on the command line.  The parent
computes the references and checks them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

CASES = [("c1_j1832", ()), ("c3_small", ()), ("c2_chromvary", ()), ("c3_small", (0,))]


def main(path):
    import _cond_ref as cr
    from enterprise_warp_amd import _lib
    assert _lib.LIB_PATH.endswith("libewarp_cpu.so"), _lib.LIB_PATH
    out = {}
    for i, (name, dl) in enumerate(CASES):
        cs = cr.case(name, dl)
        eng = cs.pta.engine()
        assert eng.cond_dims() == (cs.n_coef, int(cs.toa_off[-1]))
        coef, proc, status = cr.run_case(cs, lambda th, z, cg, ng: eng.cond_gp(th, z=z, col_group=cg, n_group=ng))
        for kind in (0, 1):
            out[f"c{i}_coef{kind}"] = coef[kind]
            for gi, y in proc[kind].items():
                out[f"c{i}_proc{kind}_{gi}"] = y
        out[f"c{i}_status"] = np.stack(status)
        if dl:
            # a NaN delay amplitude in row 2: status 2 and NaN there, the other rows unchanged
            X = cs.X.copy()
            j = next(k for k, n in enumerate(cs.pta.param_names) if n.endswith("dmexp_log10_Amp"))
            X[2, j] = np.nan
            grp = np.zeros(cs.n_coef, np.int32)
            c_bad, y_bad, s_bad = eng.cond_gp(X, z=cs.z, col_group=grp, n_group=1)
            c_ok, y_ok, _ = eng.cond_gp(cs.X, z=cs.z, col_group=grp, n_group=1)
            out["nan_status"] = s_bad
            out["nan_coef_bad"], out["nan_coef_ok"] = c_bad, c_ok
            out["nan_proc_bad"], out["nan_proc_ok"] = y_bad, y_ok
    np.savez(path, **out)
    print("COND_WORKER_OK")


if __name__ == "__main__":
    main(sys.argv[1])
