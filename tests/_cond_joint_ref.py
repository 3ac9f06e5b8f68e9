"""References for the joint conditional GP (ewh_cond_joint,
enterprise_warp_amd.JointConditionalGP) that do not depend on the code under
test, shared by tests/test_cond_joint_host.py and tests/test_gpu_cond_joint.py,
in the pattern of tests/_cond_ref.py.

Ordering (include/ewarp_hip.h): every pulsar's own block -- the columns that
are not the common process's, timing model included, in SignalCollection.T
order -- pulsar-major, then the common columns in (pulsar a, column g) order.
Per row, in that order:
  Sigma = blockdiag_p(T_p^T N_p^-1 T_p) + Phi^-1,  d = concat_p T_p^T N_p^-1 r_p
  Sigma = L L^T,  mean = Sigma^-1 d,  draw = mean + L^-T z
with z indexed by coefficient (its [B, n_coef] position in T order).
  near-exact        Grams from DDReferencePTA._gram summed into np.longdouble,
                    Phi from OraclePTA.phi_global, Phi^-1 by connected
                    components (as OraclePTA.phiinv_cliques does) in long
                    double, chol_ld and both solves in long double
  enterprise order  fp64: OraclePulsar.white_terms, phiinv_cliques, scipy
                    cho_factor(lower=True) on the same (joint-ordered) matrix
Errors: of the coefficients of pulsar p, max over p's entries of
|L_exact^T (coef - exact)| with the joint L (posterior standard deviations);
of a realisation max_t |y - y_exact| (seconds).

Criterion: the project's own, unchanged from _cond_ref.py -- floor = 4 x
enterprise order's worst near-row error per error kind; near rows: every unit
within the floor; prior rows: worst <= max(enterprise order's worst, floor);
status 0.  A row on which the long-double reference itself fails (Phi not
positive definite: c5_noauto's prior rows) is left out of the criterion and
must have a non-zero device status.

The synthetic case follows synth.config_c5's recipe (7 pulsars, 250 TOAs,
hd_vary_gamma_9_nfreqs: N_c = 126 crosses 16- and 64-column panels, n_col = 18
is no multiple of 16) with 11 / 12 / 13 timing-model columns per pulsar:
config_c5 gives every pulsar 12, which makes every own block even, and the
masked k-slice of the Schur update needs mo = 33 (1 mod 4) and 35 (3 mod 4).
"""
import functools

import numpy as np
import scipy.linalg as sl

import _cond_ref as cr
from conftest import load_golden

LD = np.longdouble
ROWS = cr.ROWS
Z_SEED = cr.Z_SEED


# The synthetic cases: synth7's recipe (seed 7, 7 pulsars, 250 TOAs, epoch_size 16, n_tm = 11 + i % 3) with
# gwb: frequencies of hd_vary_gamma_*_nfreqs; spin / dm: frequencies of the powerlaw (None: no such term);
# fixed_white; prior: the (seed, index) pairs of the prior rows, synth.prior_draws(pta, 8, seed)[index].
# At these sizes fp64 enterprise order fails on most prior draws (a pivot of the common block), and the
# criterion needs its error: the draws are ones it stands on, picked with the references alone.  The wide
# cases': of the standing draws of seeds 20 .. 59 (scripts/cond_joint_prior_scan.py) the four with the
# smallest enterprise-order coefficient error (worst over pulsars, mean and draw; sigma), listed beside them.
# (scan: the error with the scan's normals; case: with the normals the draw gets as a row of the case)
PRIOR_NC40 = ((36, 3), (46, 1), (55, 4), (51, 5))       # 27 of 320 stand; scan 3.1e-7, 1.0e-6, 5.6e-6, 1.3e-5;
#                                                         case 2.6e-7, 9.3e-7, 7.9e-7, 2.6e-5
PRIOR_VARWN = ((22, 5), (27, 1), (55, 7), (51, 3))      # 66 of 320; scan 2.3e-6, 3.5e-6, 6.4e-6, 1.6e-5;
#                                                         case 2.6e-6, 2.9e-6, 6.4e-5, 2.3e-5
PRIOR_LEAD = ((36, 1), (40, 6), (34, 5), (20, 5))       # 113 of 320; scan 1.8e-12, 5.2e-12, 5.8e-11, 8.2e-10;
#                                                         case 1.8e-12, 5.2e-12, 7.4e-11, 5.5e-9
SYNTH = {
    "synth7": dict(gwb=9, spin=10, dm=10, fixed_white=True, prior=((22, 0), (22, 3), (37, 0), (37, 1))),
    "synth7_nc40": dict(gwb=20, spin=10, dm=10, fixed_white=True, prior=PRIOR_NC40),
    "synth7_nc40_varwn": dict(gwb=20, spin=10, dm=10, fixed_white=False, prior=PRIOR_VARWN),
    "synth7_nc48_lead": dict(gwb=24, spin=4, dm=None, fixed_white=True, prior=PRIOR_LEAD),
}


def synth_case_pta(variant="synth7"):
    """(pta, theta [16 x n_param], near [16]): 8 prior rows, then 8 near rows."""
    from enterprise_warp_amd import synth
    v = SYNTH[variant]
    seed, n_psr, n_toa = 7, 7, 250
    rng = np.random.default_rng(seed)
    psrs = []
    for i in range(n_psr):
        u = rng.standard_normal(3)
        psrs.append(synth.make_pulsar(f"J{i:04d}+{seed:04d}", n_toa, seed=seed * 1000 + i, pos=u / np.linalg.norm(u),
                                      epoch_size=16, n_tm=11 + i % 3))
    Tspan = max(p.toas.max() for p in psrs) - min(p.toas.min() for p in psrs)
    ns = synth.params_namespace(Tspan, v["fixed_white"])
    wn = synth.white_noisedict(psrs, seed + 1)
    terms = {"efac": "by_backend", "equad": "by_backend", "ecorr": "by_backend",
             "spin_noise": f"powerlaw_{v['spin']}_nfreqs"}
    if v["dm"] is not None:
        terms["dm_noise"] = f"powerlaw_{v['dm']}_nfreqs"
    pta = synth.build_pta(psrs, terms, {"gwb": f"hd_vary_gamma_{v['gwb']}_nfreqs"}, ns, wn)
    truth = synth.truth_values(pta, seed + 2, white=wn)
    synth.simulate_residuals(pta, truth, seed + 3)
    prior = np.array([synth.prior_draws(pta, 8, s)[i] for s, i in v["prior"]])
    theta = np.vstack([prior, prior, synth.near_draws(pta, truth, 8, seed + 5)])
    return pta, theta, np.r_[np.zeros(8, bool), np.ones(8, bool)]


def phiinv_components_ld(Phi):
    """Phi^-1 in np.longdouble, block by connected component (a column alone:
    1 / phi; a common column across the pulsars: the P x P block by chol_ld)."""
    from scipy.sparse.csgraph import connected_components
    ncomp, lab = connected_components(Phi != 0, directed=False)
    inv = np.zeros(Phi.shape, LD)
    single = np.flatnonzero(np.bincount(lab, minlength=ncomp)[lab] == 1)
    inv[single, single] = LD(1.0) / Phi[single, single].astype(LD)
    for c in np.unique(lab[np.bincount(lab, minlength=ncomp)[lab] > 1]):
        ix = np.flatnonzero(lab == c)
        L = cr.chol_ld(Phi[np.ix_(ix, ix)])
        eye = np.eye(len(ix), dtype=LD)
        inv[np.ix_(ix, ix)] = np.stack([cr.solve_lower_t(L, cr.solve_lower(L, eye[:, k])) for k in range(len(ix))],
                                       axis=1)
    return inv


class JointCase:
    """One correlated fixture: the PTA, the rows and normals the tests use,
    the groups, the joint permutation and both references."""

    def __init__(self, name):
        self.name = name
        if name in SYNTH:
            self.pta, theta, near = synth_case_pta(name)
            self.inf_rows = np.zeros(len(theta), bool)[ROWS]
        else:
            self.pta, z = load_golden(name, full=True)
            theta, near = z["theta"], np.asarray(z["near"], bool)
            self.inf_rows = ~np.isfinite(z["lnl"])[ROWS]          # the golden's -inf rows (c5_noauto)
        assert not near[:8].any() and near[8:].all(), "fixture layout: 8 prior rows, then 8 near rows"
        self.psrs = [c.psr for c in self.pta.signal_collections]
        self.X = np.ascontiguousarray(theta[ROWS])
        self.near = near[ROWS]
        cols = self.pta.signal_collections
        self.m = [c.T.shape[1] for c in cols]
        self.n_toa = [len(c.psr.toas) for c in cols]
        self.col_off = np.concatenate([[0], np.cumsum(self.m)])
        self.toa_off = np.concatenate([[0], np.cumsum(self.n_toa)])
        self.n_coef = int(self.col_off[-1])
        self.z = np.random.default_rng(Z_SEED).standard_normal((len(self.X), self.n_coef))
        self.groups = []
        for p, c in enumerate(cols):
            for sig, cc in c.signal_cols.items():
                self.groups.append((p, sig, np.asarray(cc, int)))
            self.groups.append((p, "*", np.arange(self.m[p])))
        # the joint order as indices into the pulsar-major T order, and the pulsar of each joint position
        own, com = [], []
        for p, c in enumerate(cols):
            cc = list(c.common_cols)
            own += [self.col_off[p] + j for j in range(self.m[p]) if j not in set(cc)]
            com += [self.col_off[p] + j for j in cc]
        self.perm = np.array(own + com, int)
        self.owner = np.searchsorted(self.col_off, self.perm, side="right") - 1
        self.mo = [self.m[p] - len(c.common_cols) for p, c in enumerate(cols)]
        self._ref = None

    # ---------------------------------------------------------------- references
    def references(self):
        """{"exact" / "ent": {b: (mean, draw)} in T order, "L": {b: joint L},
        "T": {p: basis}, "ok": rows on which the long-double reference stands}."""
        if self._ref is not None:
            return self._ref
        from oracle.ddref import DDReferencePTA
        from oracle.enterprise_ref import OraclePTA
        pta = self.pta
        const = pta.constant_values()
        terms = pta.oracle_terms()
        ent = OraclePTA(self.psrs, terms, fixed_params=None)
        # (its constructor takes uncorrelated models only; the Gram needs no state of it)
        dd = DDReferencePTA.__new__(DDReferencePTA)
        for pp, c in zip(ent.pulsars, pta.signal_collections):
            assert pp.T.shape == c.T.shape and np.array_equal(pp.T, c.T), \
                "the oracle's column order differs from SignalCollection.T"
        P, n, perm = len(self.psrs), self.n_coef, self.perm
        out = {"ent": {}, "exact": {}, "L": {}, "T": {p: np.asarray(ent.pulsars[p].T, float) for p in range(P)},
               "ok": np.zeros(len(self.X), bool)}
        gram_cache = {}
        for b, x in enumerate(self.X):
            d = dict(const)
            d.update(pta.map_params(x))
            Phi, off = ent.phi_global(d)
            assert np.array_equal(off, self.col_off)
            zj = self.z[b][perm]
            # near-exact
            try:
                Sig = phiinv_components_ld(Phi)
            except np.linalg.LinAlgError:
                continue
            dvec = np.zeros(n, LD)
            for p in range(P):
                pd = ent.pulsars[p]
                key = (p, tuple(float(d[nm]) for _, _, names in pd.white for nm in sorted(names.values())))
                if key not in gram_cache:
                    Xa = np.concatenate([out["T"][p], np.asarray(pd.r, float)[:, None]], axis=1)
                    G, _ = dd._gram(pd, d, Xa)
                    gram_cache[key] = np.asarray(G[0], LD) + np.asarray(G[1], LD)
                G, m, s = gram_cache[key], self.m[p], slice(off[p], off[p + 1])
                Sig[s, s] += G[:m, :m]
                dvec[s] = G[:m, m]
            try:
                L = cr.chol_ld(Sig[np.ix_(perm, perm)])
            except np.linalg.LinAlgError:
                continue
            y = cr.solve_lower(L, dvec[perm])
            mean, draw = np.zeros(n, LD), np.zeros(n, LD)
            mean[perm] = cr.solve_lower_t(L, y)
            draw[perm] = cr.solve_lower_t(L, y + zj.astype(LD))
            out["exact"][b], out["L"][b] = (mean, draw), L
            out["ok"][b] = True
            # enterprise order
            Sg, _ = ent.phiinv_cliques(Phi)
            dv = np.zeros(n)
            for p in range(P):
                TNT, TNr, _, _ = ent.pulsars[p].white_terms(d)
                Sg[off[p]:off[p + 1], off[p]:off[p + 1]] += TNT
                dv[off[p]:off[p + 1]] = TNr
            cf = sl.cho_factor(Sg[np.ix_(perm, perm)], lower=True)
            me, de = np.zeros(n), np.zeros(n)
            me[perm] = sl.cho_solve(cf, dv[perm])
            de[perm] = me[perm] + sl.solve_triangular(cf[0], zj, lower=True, trans="T")
            out["ent"][b] = (me, de)
        self._ref = out
        return out

    def coef_err(self, b, coef, kind):
        """Per pulsar: max over its joint positions of |L^T (coef - exact)|."""
        ref = self.references()
        e = np.abs(ref["L"][b].T @ (np.asarray(coef, LD) - ref["exact"][b][kind])[self.perm])
        return [float(e[self.owner == p].max()) for p in range(len(self.psrs))]

    def proc_exact(self, p, b, cols, kind):
        ref = self.references()
        return ref["T"][p][:, cols].astype(LD) @ ref["exact"][b][kind][self.col_off[p] + cols]

    def ent_errors(self):
        ref = self.references()
        ce, ye = {}, {}
        for b, pair in ref["ent"].items():
            for kind in (0, 1):
                for p, v in enumerate(self.coef_err(b, pair[kind], kind)):
                    ce[(p, b, kind)] = v
                for gi, (p, _, cols) in enumerate(self.groups):
                    y = ref["T"][p][:, cols] @ pair[kind][self.col_off[p] + cols]
                    ye[(gi, b, kind)] = float(np.max(np.abs(y.astype(LD) - self.proc_exact(p, b, cols, kind))))
        return ce, ye

    # ------------------------------------------------------------------ criterion
    def check(self, coef, proc, status, label):
        """coef: (mean, draw) each [B, n_coef]; proc: (mean, draw) each a dict
        {group index: [B, n_toa_p]}; status: a list of [P, B].  Asserts the
        criterion on the rows the long-double reference stands on, a non-zero
        status on the others; returns the printed figures."""
        ok = self.references()["ok"]
        for st in status:
            st = np.asarray(st)
            assert not st[:, ok].any(), f"{label}: non-zero status {np.argwhere(st)}"
            assert st[:, ~ok].all(), f"{label}: status 0 on a row whose reference fails: {st}"
        ce, ye = self.ent_errors()
        gc, gy = {}, {}
        for b in np.flatnonzero(ok):
            for kind in (0, 1):
                for p, v in enumerate(self.coef_err(b, coef[kind][b], kind)):
                    gc[(p, b, kind)] = v
                for gi, (p, _, cols) in enumerate(self.groups):
                    y = np.asarray(proc[kind][gi][b], LD)
                    gy[(gi, b, kind)] = float(np.max(np.abs(y - self.proc_exact(p, b, cols, kind))))
        res = {}
        for what, got, ent, unit in (("coef", gc, ce, "sigma"), ("proc", gy, ye, "s")):
            nr = [k for k in ent if self.near[k[1]]]
            pr = [k for k in ent if not self.near[k[1]]]
            floor = 4.0 * max(ent[k] for k in nr)
            g_near, e_near = max(got[k] for k in nr), max(ent[k] for k in nr)
            g_prior = max((got[k] for k in pr), default=0.0)
            e_prior = max((ent[k] for k in pr), default=0.0)
            print(f"{label} {what}: floor {floor:.3e} {unit}; near worst {g_near:.3e} (enterprise order {e_near:.3e}, "
                  f"ratio {g_near / e_near:.3f}); prior worst {g_prior:.3e} (enterprise order {e_prior:.3e}, "
                  f"ratio {g_prior / e_prior if pr else float('nan'):.3e})")
            res[what] = dict(floor=floor, near=g_near, near_ent=e_near, prior=g_prior, prior_ent=e_prior)
            bad = [(k, got[k]) for k in nr if not got[k] <= floor]
            assert not bad, f"{label} {what}: near units outside the floor {floor:.3e}: {bad[:4]}"
            assert g_prior <= max(e_prior, floor), \
                f"{label} {what}: prior rows' worst error {g_prior:.3e} exceeds max(enterprise order {e_prior:.3e}, " \
                f"floor {floor:.3e})"
        return res


@functools.lru_cache(maxsize=None)
def case(name):
    return JointCase(name)


def run_case(cs, cond_joint):
    """Evaluate a case through `cond_joint(theta, z, col_group, n_group) ->
    (coef, proc, status)`: the mean and the draw with the case's z, per-signal
    groups in one call and the all-columns group in a second, as
    _cond_ref.run_case does (NaN rows of a failed sample compare equal).
    Returns (coef pair, proc pair, status list) for JointCase.check."""
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
        c1, y1, s1 = cond_joint(cs.X, z, col_group, n_group)
        c2, y2, s2 = cond_joint(cs.X, z, all_group, 1)
        assert np.array_equal(c1, c2, equal_nan=True), "coefficients depend on the grouping"
        out = {}
        for gi, (p, sig, _) in enumerate(cs.groups):
            sl_ = slice(cs.toa_off[p], cs.toa_off[p + 1])
            out[gi] = y2[:, 0, sl_] if sig == "*" else sum(y1[:, g, sl_] for g in parts[(p, sig)])
        coef.append(c1)
        proc.append(out)
        status += [s1, s2]
    return coef, proc, status


# ---------------------------------------------------------- the four stages
def four_stages(cs, b, z=None):
    """A numpy fp64 restatement of the staged solve (include/ewarp_hip.h): per
    pulsar L_A, W, y_a, S, e; Sigma_c over the (pulsar, column) pairs with
    M_g^-1 from the P x P blocks of Phi; L_c, y_c, x_c; the per-pulsar
    back-substitution.  z: [n_coef] in T order or None.  Returns the
    coefficients in T order."""
    from oracle.enterprise_ref import OraclePTA
    pta = cs.pta
    d = dict(pta.constant_values())
    d.update(pta.map_params(cs.X[b]))
    ent = OraclePTA(cs.psrs, pta.oracle_terms(), fixed_params=None)
    Phi, off = ent.phi_global(d)
    P = len(cs.psrs)
    cols = pta.signal_collections
    nc = len(cols[0].common_cols)
    z = np.zeros(cs.n_coef) if z is None else np.asarray(z, float)
    LA, W, ya, own_idx, com_idx = [], [], [], [], []
    Sc = np.zeros((P * nc, P * nc))
    e = np.zeros(P * nc)
    for p, c in enumerate(cols):
        TNT, TNr, _, _ = ent.pulsars[p].white_terms(d)
        com = np.asarray(c.common_cols, int)
        own = np.array([j for j in range(cs.m[p]) if j not in set(com)], int)
        phi_own = Phi[off[p] + own, off[p] + own]
        A = TNT[np.ix_(own, own)] + np.diag(1.0 / phi_own)
        L = np.linalg.cholesky(A)
        Wp = sl.solve_triangular(L, TNT[np.ix_(own, com)], lower=True).T          # C^T L^-T
        y = sl.solve_triangular(L, TNr[own], lower=True)
        s = slice(p * nc, (p + 1) * nc)
        Sc[s, s] = TNT[np.ix_(com, com)] - Wp @ Wp.T
        e[s] = TNr[com] - Wp @ y
        LA.append(L), W.append(Wp), ya.append(y), own_idx.append(off[p] + own), com_idx.append(off[p] + com)
    for g in range(nc):
        ix = np.array([com_idx[a][g] for a in range(P)])
        Minv = np.linalg.inv(Phi[np.ix_(ix, ix)])
        Sc[np.ix_(g + nc * np.arange(P), g + nc * np.arange(P))] += Minv
    Lc = np.linalg.cholesky(Sc)
    zc = np.concatenate([z[com_idx[a]] for a in range(P)])
    xc = sl.solve_triangular(Lc, sl.solve_triangular(Lc, e, lower=True) + zc, lower=True, trans="T")
    out = np.zeros(cs.n_coef)
    for p in range(P):
        xp = xc[p * nc:(p + 1) * nc]
        out[com_idx[p]] = xp
        out[own_idx[p]] = sl.solve_triangular(LA[p], ya[p] + z[own_idx[p]] - W[p].T @ xp, lower=True, trans="T")
    return out


def joint_dense(cs, b, z=None):
    """The joint dense solve in fp64 numpy: one Cholesky of Sigma in the joint
    order; coefficients in T order."""
    from oracle.enterprise_ref import OraclePTA
    pta = cs.pta
    d = dict(pta.constant_values())
    d.update(pta.map_params(cs.X[b]))
    ent = OraclePTA(cs.psrs, pta.oracle_terms(), fixed_params=None)
    Phi, off = ent.phi_global(d)
    Sg, _ = ent.phiinv_cliques(Phi)
    dv = np.zeros(cs.n_coef)
    for p in range(len(cs.psrs)):
        TNT, TNr, _, _ = ent.pulsars[p].white_terms(d)
        Sg[off[p]:off[p + 1], off[p]:off[p + 1]] += TNT
        dv[off[p]:off[p + 1]] = TNr
    perm = cs.perm
    cf = sl.cho_factor(Sg[np.ix_(perm, perm)], lower=True)
    out = np.zeros(cs.n_coef)
    out[perm] = sl.cho_solve(cf, dv[perm])
    if z is not None:
        out[perm] += sl.solve_triangular(cf[0], np.asarray(z, float)[perm], lower=True, trans="T")
    return out
