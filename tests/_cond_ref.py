"""References for the conditional GP (ewh_cond_gp) that do not depend on the
code under test, shared by tests/test_cond_gp_host.py, tests/_cond_worker.py
and tests/test_gpu_cond_gp.py.

Per (pulsar, row), from OraclePulsar.white_terms / .phi and
DDReferencePTA._gram / ._phi (for deterministic delays r is shifted by the
restated waveform, as tests/_delay_common.py does):
  enterprise order  fp64 scipy cho_factor(Sigma, lower=True), cho_solve,
                    solve_triangular(trans='T') on TNT + diag(1/phi)
  near-exact        the double-double Gram summed into np.longdouble, then
                    Cholesky and both solves in np.longdouble
Errors: of a coefficient vector max |L_exact^T (coef - coef_exact)| (posterior
standard deviations); of a realisation max_t |y - y_exact| (seconds).

Criterion (per fixture; the first 4 prior and first 4 near rows):
  floor       4 x the largest enterprise-order error over the near rows, over
              mean and draw, for each error kind (computed here from the two
              references alone, printed)
  near rows   every unit within the floor
  prior rows  the fixture's worst error <= max(enterprise order's worst, floor)
  status      0 on every row
"""
import functools

import numpy as np
import scipy.linalg as sl

from conftest import load_golden

LD = np.longdouble
ROWS = np.r_[0:4, 8:12]        # the fixtures hold 8 prior rows, then 8 near rows
Z_SEED = 20240611


def chol_ld(A):
    """Lower Cholesky of a symmetric matrix in np.longdouble (by columns)."""
    A = np.array(A, dtype=LD)
    m = A.shape[0]
    L = np.zeros((m, m), LD)
    for k in range(m):
        d = A[k, k] - np.dot(L[k, :k], L[k, :k])
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {k}: {d}")
        L[k, k] = np.sqrt(d)
        if k + 1 < m:
            L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return L


def solve_lower(L, b):
    x = np.zeros(len(b), LD)
    for i in range(len(b)):
        x[i] = (b[i] - np.dot(L[i, :i], x[:i])) / L[i, i]
    return x


def solve_lower_t(L, b):
    x = np.zeros(len(b), LD)
    for i in range(len(b) - 1, -1, -1):
        x[i] = (b[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


class CondCase:
    """One fixture (optionally with delays on some pulsars): the PTA, the rows
    and normals the tests use, the groups, and both references."""

    def __init__(self, name, delay_psrs=()):
        self.name = name
        self.delay_psrs = tuple(delay_psrs)
        if delay_psrs:
            import _delay_common as dc
            self.dcase = dc.case(name, tuple(delay_psrs))
            self.pta = self.dcase.pta
            self.psrs = self.dcase.psrs
            theta, near = self.dcase.Xa, self.dcase.near
        else:
            self.dcase = None
            self.pta, z = load_golden(name, full=True)
            self.psrs = [c.psr for c in self.pta.signal_collections]
            theta, near = z["theta"], np.asarray(z["near"], bool)
        assert not near[:8].any() and near[8:].all(), "fixture layout: 8 prior rows, then 8 near rows"
        self.X = np.ascontiguousarray(theta[ROWS])
        self.near = near[ROWS]
        cols = self.pta.signal_collections
        self.m = [c.T.shape[1] for c in cols]
        self.n_toa = [len(c.psr.toas) for c in cols]
        self.col_off = np.concatenate([[0], np.cumsum(self.m)])
        self.toa_off = np.concatenate([[0], np.cumsum(self.n_toa)])
        self.n_coef = int(self.col_off[-1])
        self.z = np.random.default_rng(Z_SEED).standard_normal((len(self.X), self.n_coef))
        # groups: every signal of every pulsar (the timing model included) and
        # one holding every column
        self.groups = []
        for p, c in enumerate(cols):
            for sig, cc in c.signal_cols.items():
                self.groups.append((p, sig, np.asarray(cc, int)))
            self.groups.append((p, "*", np.arange(self.m[p])))
        self._ref = None

    # ---------------------------------------------------------------- references
    def references(self):
        if self._ref is not None:
            return self._ref
        from oracle.ddref import DDReferencePTA
        from oracle.enterprise_ref import OraclePTA
        pta = self.pta
        const = pta.constant_values()
        terms = pta.oracle_terms()
        ent = OraclePTA(self.psrs, terms, fixed_params=None)
        dd = DDReferencePTA(self.psrs, terms)
        for p, (pp, c) in enumerate(zip(ent.pulsars, pta.signal_collections)):
            fixed = np.flatnonzero(np.asarray(c.col_bgroup) < 0)
            assert pp.T.shape == c.T.shape and np.array_equal(pp.T[:, fixed], c.T[:, fixed]), \
                "the oracle's column order differs from SignalCollection.T"
        r0 = [np.asarray(ps.residuals, float) for ps in self.psrs]
        B, P = len(self.X), len(self.psrs)
        out = {"ent": {}, "exact": {}, "L": {}, "T": {}}
        gram_cache = {}
        for b, x in enumerate(self.X):
            d = dict(const)
            d.update(pta.map_params(x))
            deltas = self.dcase.deltas(x) if self.dcase else {}
            for p in range(P):
                pe, pd = ent.pulsars[p], dd.pulsars[p]
                r = r0[p] - deltas[p] if p in deltas else r0[p]
                pe.r = r
                pd.r = r
                zz = self.z[b, self.col_off[p]:self.col_off[p + 1]]
                # enterprise order
                TNT, TNr, _, _ = pe.white_terms(d)
                Sigma = TNT + np.diag(1.0 / pe.phi(d))
                cf = sl.cho_factor(Sigma, lower=True)
                mean = sl.cho_solve(cf, TNr)
                draw = mean + sl.solve_triangular(cf[0], zz, lower=True, trans="T")
                T = np.asarray(pe.basis(d), float)
                out["ent"][(p, b)] = (mean, draw)
                # near-exact (the Gram depends on theta through white noise, a
                # sampled chromatic index and the delays only: cached on those)
                key = (p, tuple(float(d[nm]) for _, _, names in pd.white for nm in sorted(names.values())),
                       tuple(float(d[pn]) for _, _, pn in pd.basis_params), b if p in deltas else -1)
                if key not in gram_cache:
                    Xa = np.concatenate([T, r[:, None]], axis=1)
                    G, _ = dd._gram(pd, d, Xa)
                    gram_cache[key] = np.asarray(G[0], LD) + np.asarray(G[1], LD)
                G = gram_cache[key]
                phiinv, _ = dd._phi(pd, d)
                m = self.m[p]
                S = G[:m, :m].copy()
                S[np.arange(m), np.arange(m)] += np.asarray(phiinv[0], LD) + np.asarray(phiinv[1], LD)
                L = chol_ld(S)
                y = solve_lower(L, G[:m, m])
                out["exact"][(p, b)] = (solve_lower_t(L, y), solve_lower_t(L, y + zz.astype(LD)))
                out["L"][(p, b)] = L
                out["T"][(p, b)] = T
        self._ref = out
        return out

    def coef_err(self, p, b, coef, kind):
        ref = self.references()
        ex = ref["exact"][(p, b)][kind]
        return float(np.max(np.abs(ref["L"][(p, b)].T @ (np.asarray(coef, LD) - ex))))

    def proc_exact(self, p, b, cols, kind):
        ref = self.references()
        return ref["T"][(p, b)][:, cols].astype(LD) @ ref["exact"][(p, b)][kind][cols]

    def ent_errors(self):
        """Enterprise order's own errors: {(p, b, kind): coef error}, {(gi, b, kind): realisation error}."""
        ref = self.references()
        ce, ye = {}, {}
        for (p, b), pair in ref["ent"].items():
            for kind in (0, 1):
                ce[(p, b, kind)] = self.coef_err(p, b, pair[kind], kind)
        for gi, (p, _, cols) in enumerate(self.groups):
            for b in range(len(self.X)):
                for kind in (0, 1):
                    y = ref["T"][(p, b)][:, cols] @ ref["ent"][(p, b)][kind][cols]
                    ye[(gi, b, kind)] = float(np.max(np.abs(y.astype(LD) - self.proc_exact(p, b, cols, kind))))
        return ce, ye

    # ------------------------------------------------------------------ criterion
    def check(self, coef, proc, status, label):
        """coef: (mean, draw) each [B, n_coef]; proc: (mean, draw) each a dict
        {group index: [B, n_toa_p]}; status: [P, B] (or a pair of them).
        Asserts the criterion; returns the printed figures."""
        for st in (status if isinstance(status, (tuple, list)) else [status]):
            assert not np.asarray(st).any(), f"{label}: non-zero status {np.argwhere(np.asarray(st))}"
        ce, ye = self.ent_errors()
        B, P = len(self.X), len(self.psrs)
        gc, gy = {}, {}
        for p in range(P):
            for b in range(B):
                for kind in (0, 1):
                    gc[(p, b, kind)] = self.coef_err(p, b, coef[kind][b, self.col_off[p]:self.col_off[p + 1]], kind)
        for gi, (p, _, cols) in enumerate(self.groups):
            for b in range(B):
                for kind in (0, 1):
                    y = np.asarray(proc[kind][gi][b], LD)
                    gy[(gi, b, kind)] = float(np.max(np.abs(y - self.proc_exact(p, b, cols, kind))))
        res = {}
        for what, got, ent, unit in (("coef", gc, ce, "sigma"), ("proc", gy, ye, "s")):
            nr = [k for k in ent if self.near[k[1]]]
            pr = [k for k in ent if not self.near[k[1]]]
            floor = 4.0 * max(ent[k] for k in nr)
            g_near, e_near = max(got[k] for k in nr), max(ent[k] for k in nr)
            g_prior, e_prior = max(got[k] for k in pr), max(ent[k] for k in pr)
            print(f"{label} {what}: floor {floor:.3e} {unit}; near worst {g_near:.3e} (enterprise order {e_near:.3e}, "
                  f"ratio {g_near / e_near:.3f}); prior worst {g_prior:.3e} (enterprise order {e_prior:.3e}, "
                  f"ratio {g_prior / e_prior:.3e})")
            res[what] = dict(floor=floor, near=g_near, near_ent=e_near, prior=g_prior, prior_ent=e_prior)
            bad = [(k, got[k]) for k in nr if not got[k] <= floor]
            assert not bad, f"{label} {what}: near units outside the floor {floor:.3e}: {bad[:4]}"
            assert g_prior <= max(e_prior, floor), \
                f"{label} {what}: prior rows' worst error {g_prior:.3e} exceeds max(enterprise order {e_prior:.3e}, " \
                f"floor {floor:.3e})"
        return res


@functools.lru_cache(maxsize=None)
def case(name, delay_psrs=()):
    return CondCase(name, tuple(delay_psrs))


def run_case(cs, cond_gp):
    """Evaluate a case through `cond_gp(theta, z, col_group, n_group) -> (coef,
    proc, status)` (Engine.cond_gp's signature): the mean and the draw with
    the case's z, per-signal groups in one call and the all-columns group in a
    second.  Returns (coef pair, proc pair, status list) for CondCase.check."""
    P = len(cs.psrs)
    # call 1: each pulsar's signals as disjoint column sets (merged columns:
    # the columns two signals share form their own set, summed below)
    col_group = np.full(cs.n_coef, -1, np.int32)
    parts, n_group = {}, 0
    for p, c in enumerate(cs.pta.signal_collections):
        owner = [[] for _ in range(cs.m[p])]
        for sig, cc in c.signal_cols.items():
            for j in cc:
                owner[j].append(sig)
        atoms = {}
        for j, own in enumerate(owner):
            col_group[cs.col_off[p] + j] = atoms.setdefault(tuple(own), len(atoms))
        for sig in c.signal_cols:
            parts[(p, sig)] = [g for own, g in atoms.items() if sig in own]
        n_group = max(n_group, len(atoms))
    all_group = np.zeros(cs.n_coef, np.int32)
    coef, proc, status = [], [], []
    for z in (None, cs.z):
        c1, y1, s1 = cond_gp(cs.X, z, col_group, n_group)
        c2, y2, s2 = cond_gp(cs.X, z, all_group, 1)
        assert np.array_equal(c1, c2), "coefficients depend on the grouping"
        out = {}
        for gi, (p, sig, _) in enumerate(cs.groups):
            sl_ = slice(cs.toa_off[p], cs.toa_off[p + 1])
            if sig == "*":
                out[gi] = y2[:, 0, sl_]
            else:
                out[gi] = sum(y1[:, g, sl_] for g in parts[(p, sig)])
        coef.append(c1)
        proc.append(out)
        status += [s1, s2]
    return coef, proc, status
