"""Deterministic delay signals on the device (csrc/delay.hip, ABI 8): the
chromatic exponential dip + annual DM sinusoid on golden fixtures, against the
enterprise-order and double-double oracles evaluated on r - delta
(tests/_delay_common.py) and against identities that need no reference.

Shapes: c1_j1832 (326 TOAs: neither a multiple of 4 nor of 64 -- varying
white noise, register route, TOA tail), c2_small (ECORR epochs), c3_small
(fixed white noise, delay pulsars first and last in a mixed handle),
c4_small (13 blocks: chol_big), c1_widefix / c1_wide (the wide / double-
double route: G_lo), c2_chromvary (a theta-dependent basis)."""
import numpy as np
import pytest

import _delay_common as dc
from conftest import check_parity, strict_tolerance

pytestmark = pytest.mark.gpu

CASES = {"c1_j1832": (0,), "c2_small": (0,), "c3_small": (0, -1), "c4_small": (0,), "c1_widefix": (0,),
         "c1_wide": (0,), "c2_chromvary": (0,)}


@pytest.mark.parametrize("name", list(CASES))
def test_delay_against_oracles(require_gpu, name):
    """Near rows x near-truth delays: strict against the enterprise-order
    oracle; near rows x prior delays: per sample no less accurate than that
    oracle against double-double; prior rows: check_accuracy and the same
    -inf pattern.  Every fixture row is used."""
    c = dc.case(name, CASES[name])
    ga = c.pta.get_lnlikelihood_batch(c.Xa)
    gb = c.pta.get_lnlikelihood_batch(c.Xb)
    print(c.check(ga, gb, name + " (gpu)"))


@pytest.mark.parametrize("name", ["c3_small", "c2_small"])
def test_delay_equals_preshifted_residuals(require_gpu, name):
    """No reference: lnL of the delay model at theta equals that of the plain
    PTA whose residuals were shifted on the host by the restated delta(theta)."""
    c = dc.case(name, CASES[name])
    X = np.vstack([c.Xa[c.near][:3], c.Xb[c.near][:3]])
    got = c.pta.get_lnlikelihood_batch(X)
    from enterprise_warp_amd.pulsar import Pulsar
    want = []
    for x in X:
        dl = c.deltas(x)
        psrs = [p if i not in dl else Pulsar(p.name, p.toas, p.residuals - dl[i], p.toaerrs, p.freqs, flags=p.flags,
                                             Mmat=p.Mmat, pos=p.pos, sort=False) for i, p in enumerate(c.psrs)]
        plain = dc.build(c.rec, psrs)
        want.append(plain.get_lnlikelihood_batch(c.plain_theta(x[None, :]))[0])
        plain._drop_engine()
    check_parity(got, np.array(want), f"{name}: delay model vs pre-shifted residuals")


def _c3_rows(c, B=37):
    X = np.vstack([c.Xa[c.near], c.Xb[c.near]])
    return np.vstack([X] * (B // len(X) + 1))[:B]


def test_fixed_white_mixed_handle(require_gpu):
    """c3_small, delays on the first and the last pulsar: the other pulsars
    stay on the cached reduced path bit for bit; new white-noise constants in
    place (ewh_set_fixed_white) equal a fresh build."""
    c = dc.case("c3_small", CASES["c3_small"])
    X = _c3_rows(c)
    got = c.pta.get_lnlikelihood_batch(X)
    terms = c.pta.engine().unit_terms(len(X))
    plain_lnl = c.plain.get_lnlikelihood_batch(c.plain_theta(X))
    plain_terms = c.plain.engine().unit_terms(len(X))
    assert np.all(np.isfinite(plain_lnl))
    others = [p for p in range(len(c.psrs)) if p not in c.delay_psrs]
    assert others
    np.testing.assert_array_equal(terms[others], plain_terms[others])
    assert not np.array_equal(terms[list(c.delay_psrs)], plain_terms[list(c.delay_psrs)])
    np.testing.assert_allclose(terms.sum(axis=0), got, rtol=1e-12, atol=1e-6)
    # in-place white noise
    const = c.pta.constant_values()
    rng = np.random.default_rng(5)
    new = {k: (v * rng.uniform(0.95, 1.05) if k.endswith("_efac") else v + rng.uniform(-0.2, 0.2))
           for k, v in const.items() if k.endswith(("_efac", "_log10_tnequad", "_log10_ecorr"))}
    pta = dc.build(c.rec, c.psrs, c.delay_psrs)
    eng = pta.engine()
    before = pta.get_lnlikelihood_batch(X)
    np.testing.assert_array_equal(before, got)
    pta.set_default_params(new)
    assert pta.engine() is eng
    after = pta.get_lnlikelihood_batch(X)
    assert not np.array_equal(after, before)
    fresh = dc.build(c.rec, c.psrs, c.delay_psrs)
    fresh.set_default_params(new)
    np.testing.assert_array_equal(fresh.get_lnlikelihood_batch(X), after)


def test_batch_sizes_and_graph_replay(require_gpu):
    """B = 1, 5, 17 (batches the latency path would have taken) and 37 on
    c3_small: sample-group tails; each equals the rows of the 37-row call at
    strict tolerance; a second call of the same B (graph replay) repeats the
    bits."""
    c = dc.case("c3_small", CASES["c3_small"])
    X = _c3_rows(c, 37)
    full = c.pta.get_lnlikelihood_batch(X)
    assert np.all(np.isfinite(full))
    for B in (1, 5, 17, 37):
        one = c.pta.get_lnlikelihood_batch(X[:B])
        two = c.pta.get_lnlikelihood_batch(X[:B])
        np.testing.assert_array_equal(one, two)
        check_parity(one, full[:B], f"c3_small B={B} vs rows of B=37")


def test_units_device_split_inside_delay_pulsar(require_gpu):
    import torch
    c = dc.case("c3_small", CASES["c3_small"])
    X = _c3_rows(c, 37)
    B = len(X)
    full = c.pta.get_lnlikelihood_batch(X)
    eng = c.pta.engine()
    th = torch.from_numpy(X).cuda()
    P = len(c.psrs)
    s = torch.cuda.current_stream().cuda_stream
    for cut in (11, (P - 1) * B + 20):          # inside the first / the last (delay) pulsar's samples
        parts = []
        for u0, u1 in ((0, cut), (cut, P * B)):
            part = torch.zeros(B, dtype=torch.float64, device="cuda")
            eng.lnl_units_device(th.data_ptr(), B, u0, u1, part.data_ptr(), s)
            torch.cuda.synchronize()
            parts.append(part.cpu().numpy())
        check_parity(parts[0] + parts[1], full, f"c3_small unit ranges split at {cut}")


def test_two_contexts_on_one_device(require_gpu):
    """A handle over device ids [0, 0]: every delay pref is in the per-context
    theta gather (a missing column reads NaN there)."""
    c = dc.case("c3_small", CASES["c3_small"])
    X = _c3_rows(c, 37)
    one = c.pta.get_lnlikelihood_batch(X)
    try:
        eng = c.pta.engine(devices=[0, 0])
        assert eng.num_devices() == 2
        got = c.pta.get_lnlikelihood_batch(X)
    finally:
        c.pta.engine(devices=[0])
    check_parity(got, one, "c3_small on [0, 0]")


@pytest.mark.parametrize("name", ["c3_small", "c1_j1832"])
def test_non_finite_delay_parameter(require_gpu, name):
    c = dc.case(name, CASES[name])
    X = np.array(c.Xa[c.near][:5])
    good = c.pta.get_lnlikelihood_batch(X)
    assert np.all(np.isfinite(good))
    names = c.pta.param_names
    for k, bad in ((1, np.nan), (3, np.inf)):
        Y = X.copy()
        Y[k, names.index(f"{c.psrs[0].name}_dmexp_log10_Amp")] = bad
        got = c.pta.get_lnlikelihood_batch(Y)
        assert got[k] == -np.inf
        keep = np.arange(len(X)) != k
        assert np.all(np.abs(got[keep] - good[keep]) <= strict_tolerance(good[keep]))


def test_unsupported_combinations_raise(require_gpu):
    """Delays under a correlated common process / the optimal statistic."""
    rec, psrs, _ = dc.load_recipe("c5_small")
    pta = dc.build(rec, psrs, (0,))
    with pytest.raises(NotImplementedError):
        pta.engine()
