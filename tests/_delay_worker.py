"""Subprocess body of tests/test_delay_host.py::test_twin_delay_models: runs
with EWARP_BACKEND=cpu (the host twin libewarp_cpu.so; the ctypes binding is
process-global).  Delay models on c1_j1832, c2_small (ECORR) and c3_small
(fixed white noise, delays on the first and the last pulsar) under the
criteria of tests/_delay_common.py; prints one JSON object."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import _delay_common as dc
    from enterprise_warp_amd import _lib
    assert _lib.LIB_PATH.endswith("libewarp_cpu.so"), _lib.LIB_PATH
    out = {"lib": os.path.basename(_lib.LIB_PATH), "cases": {}}
    for name, dp in (("c1_j1832", (0,)), ("c2_small", (0,)), ("c3_small", (0, -1))):
        c = dc.case(name, dp)
        ga = c.pta.get_lnlikelihood_batch(c.Xa)
        gb = c.pta.get_lnlikelihood_batch(c.Xb)
        out["cases"][name] = c.check(ga, gb, name + " (cpu twin)")
    # c3_small: the pulsars without delays keep their terms bit for bit
    c = dc.case("c3_small", (0, -1))
    X = np.vstack([c.Xa, c.Xb])
    c.pta.get_lnlikelihood_batch(X)
    terms = c.pta.engine().unit_terms(len(X))
    c.plain.get_lnlikelihood_batch(c.plain_theta(X))
    plain_terms = c.plain.engine().unit_terms(len(X))
    others = [p for p in range(len(c.psrs)) if p not in c.delay_psrs]
    out["others_bit_identical"] = bool(others and np.array_equal(terms[others], plain_terms[others]))
    out["delay_terms_differ"] = bool(not np.array_equal(terms[list(c.delay_psrs)], plain_terms[list(c.delay_psrs)]))
    # a non-finite delay parameter: -inf for that sample alone
    Y = np.array(c.Xa[c.near][:4])
    good = c.pta.get_lnlikelihood_batch(Y)
    Y[2, c.pta.param_names.index(f"{c.psrs[0].name}_dmexp_t0")] = np.nan
    got = c.pta.get_lnlikelihood_batch(Y)
    keep = np.arange(4) != 2
    out["nan_is_minus_inf"] = bool(got[2] == -np.inf and np.array_equal(got[keep], good[keep]))
    # delays under a correlated common process are refused from Python
    rec, psrs, _ = dc.load_recipe("c5_small")
    try:
        dc.build(rec, psrs, (0,)).engine()
        out["c5_refused"] = False
    except NotImplementedError:
        out["c5_refused"] = True
    print("DELAY_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
