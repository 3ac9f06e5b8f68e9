"""`ConditionalGP`: posterior means, draws and time-domain realisations of the
Gaussian-process coefficients at chain samples (noise reconstruction).

Reference boundary: the reference reaches noise realisations only by shelling
out to tempo2 (enterprise_warp/tempo2_warp.py); with enterprise the same thing
is `enterprise.signals.utils.ConditionalGP(pta)` or la_forge's
`Signal_Reconstruction`, one `cho_factor` per pulsar per chain sample on the
host.  Here one device call (ewh_cond_gp, csrc/cond.hip) serves a batch of
chain samples: per (pulsar, sample)

    Sigma = T^T N^-1 T + diag(1/phi),  d = T^T N^-1 (r - delay)
    Sigma = L L^T,  mean = Sigma^-1 d,  draw = mean + L^-T z

with z standard normals drawn on the HOST (`rng.standard_normal`), so one seed
gives the same draws on the device, the host twin and a numpy reference.

Scope of `ConditionalGP`: uncorrelated / CURN models, the engine's first
device; a correlated (ORF) common process raises NotImplementedError there and
is served by `JointConditionalGP` (ewh_cond_joint, csrc/cond_joint.hip), the
same surface over the joint solve that couples the pulsars' common columns.

Merged columns.  Signals whose basis columns were merged (CURN `gw` on the
red-noise Fourier columns, [ent] SignalCollection._combine_basis_columns)
share those coefficients: every such name reports the shared values, and its
realisation is that of the SUM of the merged processes on those columns.
This convention has not been checked against enterprise (absent here).
"""
import numpy as np

from .pta import PTA


class _ConditionalBase:
    """The surface both classes share: the column map, the column groups, the
    batched calls and the enterprise-style methods.  A subclass checks the
    model in `_accept` and names its engine entries in `_dims` / `_solve`."""

    def __init__(self, pta, device=0):
        if not isinstance(pta, PTA):
            raise TypeError(f"{type(self).__name__} needs an enterprise_warp_amd.PTA")
        self._accept(pta)
        self.pta = pta
        self._device = device
        self.names = pta.pulsars
        # per pulsar: column / TOA offsets into ewh_cond_gp's arrays and the
        # per-signal column map (SignalCollection.signal_cols)
        self.col_off, self.toa_off, self.signal_cols = [], [], []
        c0 = t0 = 0
        for c in pta.signal_collections:
            self.col_off.append(c0)
            self.toa_off.append(t0)
            self.signal_cols.append({k: np.asarray(v, int) for k, v in c.signal_cols.items()})
            c0 += c.T.shape[1]
            t0 += len(c.psr.toas)
        self.n_coef, self.n_toa_total = c0, t0
        self.n_toa = [len(c.psr.toas) for c in pta.signal_collections]

    def _engine(self):
        eng = self.pta.engine(device=self._device) if self.pta._engine is None else self.pta.engine()
        got = self._dims(eng)
        if got != (self.n_coef, self.n_toa_total):
            raise RuntimeError(f"engine layout {got} differs from the model's {(self.n_coef, self.n_toa_total)}")
        return eng

    def draw_normals(self, B, rng=None):
        """z [B, n_coef] for B draws (host side: reproducible from the seed)."""
        rng = np.random.default_rng(rng) if not isinstance(rng, np.random.Generator) else rng
        return rng.standard_normal((B, self.n_coef))

    # ------------------------------------------------------------------ batched
    def coefficients_batch(self, X, z=None):
        """Coefficients [B, n_coef] (pulsar-major, each pulsar's columns in
        SignalCollection.T order, timing model first) of every row of X:
        the posterior mean (z None) or mean + L^-T z.  Rows of a unit whose
        factorisation failed are NaN."""
        coef, _, _ = self._solve(self._engine(), self.pta._theta(X), z=z)
        return coef

    def _atoms(self, signals):
        """Disjoint column groups: per pulsar, columns with the same set of
        owning signals form one group (merged or overlapping signals share
        columns); a signal's realisation is the sum of its groups."""
        col_group = np.full(self.n_coef, -1, np.int32)
        members, n_group = [], 0
        for p, sc in enumerate(self.signal_cols):
            m = (self.col_off[p + 1] if p + 1 < len(self.col_off) else self.n_coef) - self.col_off[p]
            owner = [[] for _ in range(m)]
            for name in sc:
                if signals is None or name in signals:
                    for j in sc[name]:
                        owner[j].append(name)
            atoms = {}
            for j, own in enumerate(owner):
                if own:
                    g = atoms.setdefault(tuple(own), len(atoms))
                    col_group[self.col_off[p] + j] = g
            members.append({name: [g for own, g in atoms.items() if name in own] for name in sc
                            if signals is None or name in signals})
            n_group = max(n_group, len(atoms))
        return col_group, members, n_group

    def processes_batch(self, X, z=None, signals=None):
        """({(psr, signal): realisations [B, n_toa]}, status [n_pulsar, B]) of
        every row of X; signals: names to reconstruct (default: all, the
        timing model as "timing_model").  status: 0 ok, 1 a failed pivot,
        2 a non-finite delay parameter (those rows are NaN)."""
        col_group, members, n_group = self._atoms(None if signals is None else set(signals))
        if n_group == 0:
            raise ValueError(f"no signal of {signals} in the model")
        _, proc, status = self._solve(self._engine(), self.pta._theta(X), z=z, col_group=col_group, n_group=n_group,
                                      want_coef=False)
        out = {}
        for p, mem in enumerate(members):
            sl = slice(self.toa_off[p], self.toa_off[p] + self.n_toa[p])
            for name, gs in mem.items():
                y = proc[:, gs[0], sl].copy()
                for g in gs[1:]:
                    y += proc[:, g, sl]
                out[(self.names[p], name)] = y
        return out, status

    # --------------------------------------------------------- enterprise names
    def _coef_dict(self, row):
        out = {}
        for p, sc in enumerate(self.signal_cols):
            for name, cols in sc.items():
                out[f"{self.names[p]}_{name}_coefficients"] = row[self.col_off[p] + cols].copy()
        return out

    @staticmethod
    def _check(arr, what):
        if np.isnan(arr).any():
            raise np.linalg.LinAlgError(f"ConditionalGP: Sigma is not positive definite at these parameters ({what})")

    def get_mean_coefficients(self, params):
        """[ent] ConditionalGP.get_mean_coefficients: {f"{psr}_{signal}_coefficients": array}
        (the timing model as {psr}_timing_model_coefficients, normed columns)."""
        coef = self.coefficients_batch(self.pta._theta(params))
        self._check(coef, "mean coefficients")
        return self._coef_dict(coef[0])

    def sample_coefficients(self, params, n=1, rng=None):
        """[ent] ConditionalGP.sample_coefficients: one dict, or a list of n."""
        th = np.repeat(self.pta._theta(params)[:1], n, axis=0)
        coef = self.coefficients_batch(th, z=self.draw_normals(n, rng))
        self._check(coef, "coefficient draws")
        out = [self._coef_dict(r) for r in coef]
        return out[0] if n == 1 else out

    def _proc_dicts(self, th, z):
        procs, status = self.processes_batch(th, z=z)
        if status.any():
            raise np.linalg.LinAlgError("ConditionalGP: Sigma is not positive definite at these parameters")
        return [{f"{psr}_{name}": y[b] for (psr, name), y in procs.items()} for b in range(len(th))]

    def get_mean_processes(self, params):
        """[ent] ConditionalGP.get_mean_processes: {f"{psr}_{signal}": array[n_toa]}."""
        return self._proc_dicts(self.pta._theta(params)[:1], None)[0]

    def sample_processes(self, params, n=1, rng=None):
        """[ent] ConditionalGP.sample_processes: one dict, or a list of n."""
        th = np.repeat(self.pta._theta(params)[:1], n, axis=0)
        out = self._proc_dicts(th, self.draw_normals(n, rng))
        return out[0] if n == 1 else out


class ConditionalGP(_ConditionalBase):
    """Per-pulsar conditional GP of an uncorrelated / CURN model (ewh_cond_gp)."""

    @staticmethod
    def _accept(pta):
        if pta.correlated():
            raise NotImplementedError("ConditionalGP: a correlated (ORF) common process needs the dense "
                                      "cross-pulsar solve; only uncorrelated / CURN models are supported")

    @staticmethod
    def _dims(eng):
        return eng.cond_dims()

    @staticmethod
    def _solve(eng, theta, **kw):
        return eng.cond_gp(theta, **kw)


class JointConditionalGP(_ConditionalBase):
    """Conditional GP under a correlated (ORF) common process -- Hellings-Downs,
    monopole, dipole, several processes, sampled ORFs: the joint solve over
    all pulsars (ewh_cond_joint, csrc/cond_joint.hip), with the surface of
    `ConditionalGP`.  The common process's coefficients appear under each
    pulsar's `{psr}_{name}_coefficients`, its realisation in that pulsar's
    TOAs under `{psr}_{name}`.  A PTA that is not correlated raises ValueError.

    The ordering of the draw.  Per pulsar the columns split into the own
    block (every column that is not the common process's, timing model
    included) and the common columns.  The joint elimination order is every
    pulsar's own block, pulsar-major, then the common columns in (pulsar,
    common column) order, pulsar-major:

        Sigma = blockdiag_p(T_p^T N_p^-1 T_p) + Phi^-1,  d = concat_p T_p^T N_p^-1 r_p
        Sigma = L L^T in that order (L lower, positive diagonal)
        mean = Sigma^-1 d,  draw = mean + L^-T z

    z [B, n_coef] is indexed by coefficient (pulsar-major, SignalCollection.T
    column order): the normal of a coefficient is the one at its position,
    whatever its place in the elimination order.  enterprise's own draw goes
    through a permuted sparse factor of the same Sigma (a fill-reducing
    ordering chosen by CHOLMOD): a different convention with the same
    distribution -- mean + L^-T z has covariance Sigma^-1 for every
    ordering -- so draws agree in law, not value by value; the means agree.

    status [n_pulsar, B]: 0 ok; 1 this pulsar's own block had a failed pivot;
    3 the sample failed elsewhere (the ORF matrix M_g not positive definite, a
    pivot of the dense common block, another pulsar's own block).  Any
    failure puts NaN in that sample's rows of every pulsar.
    max_chunk: 0, or an upper bound on the samples per device chunk."""

    def __init__(self, pta, device=0, max_chunk=0):
        super().__init__(pta, device=device)
        self.max_chunk = int(max_chunk)

    @staticmethod
    def _accept(pta):
        if not pta.correlated():
            raise ValueError("JointConditionalGP: the PTA has no correlated (ORF) common process; "
                             "use ConditionalGP")

    @staticmethod
    def _dims(eng):
        return eng.cond_joint_dims()

    def _solve(self, eng, theta, **kw):
        return eng.cond_joint(theta, max_chunk=self.max_chunk, **kw)
