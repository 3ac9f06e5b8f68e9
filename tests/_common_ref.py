"""TEST INFRASTRUCTURE ONLY -- the CPU references for several correlated common
processes and for ORFs whose values are sampled (the term form of
include/ewarp_hip.h, ewh_common_term).

oracle/enterprise_ref.py already sums `get_phicross` per signal name, so it
serves several fixed-ORF processes as it is; oracle/device_order_ref.py
assumes one process in `finish`.  Both take the ORF as a name.  The
subclasses here extend them without editing oracle/:

* `TermOraclePTA(OraclePTA)`: enterprise's order.  `phi_global` and the ORF
  diagonal of the per-pulsar phi evaluate the ORF through `orf_of`, which
  also restates the sampled ORFs of enterprise_extensions.model_orfs
  (`bin_orf`: Gamma_ab = params[bin of the angular separation]; `legendre_orf`:
  Gamma_ab = legval(cos xi, params); Gamma_aa = 1).  An indefinite Phi fails
  `cho_factor` -> -inf, as in enterprise.
* `TermDeviceOrderPTA(DeviceOrderPTA)`: the device's order, or with
  np.longdouble the near-exact value.  `_common_cols` is the union of the
  processes' columns (the widest one's) and `finish` builds
  M_g = sum_k Gamma_k(theta) phi_k(g) + diag(own).

For one fixed-ORF process both restate the base classes operation for
operation (tests/test_multi_common_host.py holds them to the stored goldens
bit for bit).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle.device_order_ref import DeviceOrderPTA, _cast, _gauss_jordan, _spectrum, phi_columns  # noqa: E402
from oracle.enterprise_ref import OraclePTA, OraclePulsar, orf_value  # noqa: E402


def orf_of(orf, params, pos1, pos2, dt=float):
    """Gamma(pos1, pos2) of an ORF given by name (oracle.enterprise_ref.orf_value)
    or by a sampled-ORF description {"kind", "edges_deg", "param"}."""
    if isinstance(orf, str):
        return orf_value(orf, pos1, pos2)
    if np.all(pos1 == pos2):
        return dt(1)
    theta = np.atleast_1d(params[orf["param"]])
    if orf["kind"] == "bin":
        bins = np.array(orf["edges_deg"]) * np.pi / 180.0
        angsep = np.arccos(np.clip(np.dot(pos1, pos2), -1.0, 1.0))
        return theta[min(max(np.digitize(angsep, bins), 1), len(theta)) - 1]
    if orf["kind"] == "legendre":
        return np.polynomial.legendre.legval(dt(np.clip(np.dot(pos1, pos2), -1.0, 1.0)), theta)
    raise ValueError(orf["kind"])


class TermOraclePulsar(OraclePulsar):
    def phi(self, params):
        """OraclePulsar.phi with the ORF diagonal through orf_of."""
        phi = np.zeros(self.T.shape[1])
        pos = np.asarray(self.psr.pos, float)
        for g in self.gps:
            if g["kind"] == "tm":
                phi[g["idx"]] += 1e40
            elif g.get("orf"):
                phi[g["idx"]] += orf_of(g["orf"], params, pos, pos) * self.gp_values(g, params)
            else:
                phi[g["idx"]] += self.gp_values(g, params)
        return phi


class TermOraclePTA(OraclePTA):
    def __init__(self, psrs, terms_per_psr, fixed_params=None):
        self.pulsars = [TermOraclePulsar(p, t) for p, t in zip(psrs, terms_per_psr)]
        self.fixed = None
        if fixed_params is not None and not any(pp.basis_params for pp in self.pulsars):
            self.fixed = [pp.white_terms(fixed_params) for pp in self.pulsars]

    def phi_global(self, params):
        """OraclePTA.phi_global with the cross terms through orf_of."""
        sizes = [pp.T.shape[1] for pp in self.pulsars]
        off = np.concatenate(([0], np.cumsum(sizes)))
        Phi = np.zeros((off[-1], off[-1]))
        for a, pp in enumerate(self.pulsars):
            Phi[np.arange(off[a], off[a + 1]), np.arange(off[a], off[a + 1])] = pp.phi(params)
        commons = {}
        for a, pp in enumerate(self.pulsars):
            for g in pp.gps:
                if g.get("orf"):
                    commons.setdefault(g["name"], []).append((a, g))
        for name, lst in commons.items():
            for a, ga in lst:
                va = self.pulsars[a].gp_values(ga, params)
                for b, gb in lst:
                    if b == a:
                        continue
                    gam = orf_of(ga["orf"], params, np.asarray(self.pulsars[a].psr.pos, float),
                                 np.asarray(self.pulsars[b].psr.pos, float))
                    ia = off[a] + np.asarray(ga["idx"])
                    ib = off[b] + np.asarray(gb["idx"])
                    Phi[ia, ib] += gam * va
        return Phi, off


class TermDeviceOrderPTA(DeviceOrderPTA):
    def _common_cols(self, pp):
        """The pulsar's common columns: the widest process's (every other
        one's are a prefix of them)."""
        lists = [list(g["idx"]) for g in pp.gps if g.get("orf")]
        com = max(lists, key=len, default=[])
        for li in lists:
            if li != com[:len(li)]:
                raise ValueError("the common processes' columns are not prefixes of the widest one's")
        return com

    def common_mg(self, params):
        """[M_g] for every common column g: sum over the processes of
        Gamma_k(theta) phi_k(g) (zero past the process's columns) + diag(own)."""
        dt = self.dt
        p = _cast(params, dt)
        P = len(self.pulsars)
        pp0 = self.pulsars[0]
        nc = len(self._common_cols(pp0))
        own = [phi_columns(pp, p, dt, with_common=False)[self._common_cols(pp)] for pp in self.pulsars]
        pos = [np.asarray(pp.psr.pos, float) for pp in self.pulsars]
        procs = []
        for gc in (g for g in pp0.gps if g.get("orf")):
            Gam = np.array([[orf_of(gc["orf"], p, pos[a], pos[b], dt) for b in range(P)] for a in range(P)], dtype=dt)
            procs.append((Gam, _spectrum(gc, p, dt)))
        out = []
        for g in range(nc):
            M = None
            for Gam, phic in procs:
                if g < len(phic):
                    M = Gam * phic[g] if M is None else M + Gam * phic[g]
            out.append(M + np.diag(np.array([own[a][g] for a in range(P)], dtype=dt)))
        return out

    def finish(self, params, locals_, keeps):
        """DeviceOrderPTA.finish with M_g from common_mg."""
        dt = self.dt
        P = len(self.pulsars)
        if not np.all(np.isfinite(np.asarray(locals_, dtype=float))):
            return dt(-np.inf)
        nc = keeps[0].shape[0] - 1
        N = P * nc
        Sc = np.zeros((N + 1, N + 1), dtype=dt)
        mlog = dt(0)
        for g, M in enumerate(self.common_mg(params)):
            Minv, ld, ok = _gauss_jordan(M)
            if not ok:
                return dt(-np.inf)
            mlog += ld
            ix = np.arange(P) * nc + g
            Sc[np.ix_(ix, ix)] += Minv
        for a, kp in enumerate(keeps):
            s = slice(a * nc, (a + 1) * nc)
            Sc[s, s] += kp[:nc, :nc]
            Sc[s, N] = kp[:nc, nc]
            Sc[N, s] = kp[nc, :nc]
            Sc[N, N] += kp[nc, nc]
        d, A = self.factor(Sc, N)
        if not np.all(d > 0):
            return dt(-np.inf)
        return sum(locals_) - (np.sum(np.log(d)) + A[N, N] + mlog) / 2


def _models(pta):
    const = pta.constant_values()
    fixed = const if pta.white_fixed() else None
    return const, fixed, [c.psr for c in pta.signal_collections], pta.oracle_terms()


def reference_lnl(pta, X):
    """(enterprise-order lnL, near-exact lnL) of every row of X, as
    conftest.reference_lnl for the term form."""
    const, fixed, psrs, terms = _models(pta)
    ent = TermOraclePTA(psrs, terms, fixed_params=fixed)
    ext = TermDeviceOrderPTA(psrs, terms, fixed, np.longdouble)
    a, b = [], []
    for x in X:
        d = dict(const)
        d.update(pta.map_params(x))
        a.append(ent.lnlikelihood(d))
        b.append(ext.lnlikelihood(d))
    return np.array(a), np.array(b)
