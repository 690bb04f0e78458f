"""The executable specification of ``alignn_amd.relax`` (csrc/relax.hip): float64 numpy / scipy restatements of ASE 3.22.1's
FIRE, ``Optimizer.run``, ``ExpCellFilter`` and ``FixAtoms`` as the reference's ``ForceField.optimize_atoms`` drives them
(alignn/ff/ff.py:373-415: ``FIRE(atoms).run(fmax, steps)``, ``downhill_check=False``, with or without ``optimize_lattice``).
ASE is not a dependency of this project.

- ``FireRef`` and ``run_ref`` follow ASE's published ``ase/optimize/fire.py`` (``FIRE.step``) and ``ase/optimize/optimize.py``
  (``Optimizer.run`` / ``Dynamics.irun`` / ``Optimizer.converged``) line by line; tests/test_relax_fire.py pins them to steps
  computed by hand on a 1-D harmonic well.
- ``ExpCellFilterRef`` and ``run_cell_ref`` restate ``ExpCellFilter`` (ase/constraints.py, default arguments) and the run loop
  of ``Optimizer.run`` over its n + 3 generalised rows; tests/test_relax_cell.py pins them by gradient checks against the
  analytic periodic potential of tests/springs_ref.py.
- ``ConstrainedFilterRef``, ``run_constrained_ref`` and ``run_fixed_ref`` restate ``FixAtoms`` and the arguments ``mask``,
  ``hydrostatic_strain``, ``constant_volume`` and ``scalar_pressure`` of ``ExpCellFilter``; tests/test_relax_constraints.py
  pins them by a case worked out by hand, by gradient checks of the enthalpy and by the physics of converged runs.

``ExpCellFilter.get_forces`` with its arguments, in ASE's order (V = |det C|, S the symmetrised stress, L = X_c / c):
  1. FixAtoms: the fixed atoms' rows of the forces are zero (``atoms.get_forces(apply_constraint=True)``); atom rows f F
  2. virial W = -V (S + scalar_pressure I)
  3. hydrostatic_strain: W <- (tr W / 3) I
  4. W <- W * mask
  5. naive force W, exact force -expm([[L, -W expm(-L)], [0, L]])[0:3, 3:6] symmetrised, ASE's switch between them
  6. constant_volume: tr / 3 off the diagonal of the chosen one
  7. / c

The GPU tests (test_gpu_relax.py, test_gpu_relax_cell.py, test_gpu_relax_constraints.py) hold the kernel and the batched relaxer
to this file."""

import numpy as np
from scipy.linalg import expm, logm

from tests.springs_ref import spring_list, springs_efs

# --- FIRE and Optimizer.run ---------------------------------------------------------------------------------------------------


# ASE's FIRE defaults
DEFAULTS = dict(dt=0.1, maxstep=0.2, dtmax=1.0, Nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, a=0.1)


class FireRef:
    """ase/optimize/fire.py FIRE.step, downhill_check=False, one structure; ``r`` [n, 3] Cartesian positions."""

    def __init__(self, r, dt=0.1, maxstep=0.2, dtmax=1.0, Nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, a=0.1):
        self.r = np.array(r, dtype=np.float64)
        self.v = None  # FIRE.initialize
        self.dt, self.maxstep, self.dtmax, self.Nmin = dt, maxstep, dtmax, Nmin
        self.finc, self.fdec, self.astart, self.fa, self.a = finc, fdec, astart, fa, a
        self.Nsteps = 0

    def step(self, f):
        f = np.asarray(f, dtype=np.float64)
        if self.v is None:
            self.v = np.zeros((len(self.r), 3))
        else:
            vf = np.vdot(f, self.v)
            if vf > 0.0:
                self.v = (1.0 - self.a) * self.v + self.a * f / np.sqrt(np.vdot(f, f)) * np.sqrt(np.vdot(self.v, self.v))
                if self.Nsteps > self.Nmin:
                    self.dt = min(self.dt * self.finc, self.dtmax)
                    self.a *= self.fa
                self.Nsteps += 1
            else:
                self.v[:] *= 0.0
                self.a = self.astart
                self.dt *= self.fdec
                self.Nsteps = 0
        self.v += self.dt * f
        dr = self.dt * self.v
        normdr = np.sqrt(np.vdot(dr, dr))
        if normdr > self.maxstep:
            dr = self.maxstep * dr / normdr
        self.r = self.r + dr


def converged(f, fmax):
    """Optimizer.converged: max over atoms of |F_i|^2 below fmax^2."""
    return bool((np.asarray(f) ** 2).sum(axis=1).max() < fmax ** 2)


def run_ref(r0, energy_forces, fmax=0.1, steps=100, **fire):
    """Optimizer.run(fmax, steps): evaluate, then step while not converged and fewer than ``steps`` steps were taken.
    ``energy_forces(r) -> (e, f)``.  -> dict(r, e, f, n_steps, converged, n_evals, traj: positions after each step)."""
    opt = FireRef(r0, **{**DEFAULTS, **fire})
    e, f = energy_forces(opt.r)
    n_evals, n_steps, traj = 1, 0, [opt.r.copy()]
    conv = converged(f, fmax)
    while not conv and n_steps < steps:
        opt.step(f)
        n_steps += 1
        traj.append(opt.r.copy())
        e, f = energy_forces(opt.r)
        n_evals += 1
        conv = converged(f, fmax)
    return dict(r=opt.r, e=e, f=np.asarray(f, dtype=np.float64), n_steps=n_steps, converged=conv, n_evals=n_evals, traj=traj,
                opt=opt)


def well(k, x0=0.0):
    """1-D harmonic well along x for one atom: E = k (x - x0)^2 / 2, F = -k (x - x0)."""

    def ef(r):
        d = r[:, 0] - x0
        f = np.zeros_like(r)
        f[:, 0] = -k * d
        return 0.5 * k * float(d @ d), f

    return ef


# --- ExpCellFilter -----------------------------------------------------------------------------------------------------------
def sym3(s):
    """full_3x3_to_voigt_6_stress followed by voigt_6_to_full_3x3_stress: the off-diagonal pairs averaged."""
    s = np.asarray(s, dtype=np.float64)
    out = s.copy()
    for i, j in ((0, 1), (0, 2), (1, 2)):
        out[i, j] = out[j, i] = (s[i, j] + s[j, i]) / 2
    return out


class ExpCellFilterRef:
    """ExpCellFilter(atoms) of one structure with original cell ``C0`` (rows a, b, c): generalised positions X [n + 3, 3]."""

    def __init__(self, C0, n):
        self.C0 = np.array(C0, dtype=np.float64)
        self.n = n
        self.c = float(n)  # cell_factor = exp_cell_factor = len(atoms)
        self.branch = None  # "naive" / "exact": which cell force the last forces() call used

    def initial(self, pos):
        return np.vstack([np.asarray(pos, dtype=np.float64), np.zeros((3, 3))])  # F = I: X_c = c logm(I) = 0

    def atoms(self, X):
        """set_positions: -> (cell C, Cartesian positions, deformation gradient F)."""
        F = expm(X[self.n:] / self.c)
        return self.C0 @ F.T, X[:self.n] @ F.T, F

    def from_atoms(self, C, pos):
        """get_positions: X from the cell and the Cartesian positions (ASE recomputes this every step)."""
        F = np.linalg.solve(self.C0, C).T
        return np.vstack([pos @ np.linalg.inv(F).T, self.c * np.real(logm(F))])

    def cell_forces(self, X, stress):
        """-> (naive, exact) cell forces before the division by c."""
        C, _, _ = self.atoms(X)
        W = -abs(np.linalg.det(C)) * sym3(stress)
        L = X[self.n:] / self.c
        Y = np.zeros((6, 6))
        Y[0:3, 0:3] = L
        Y[3:6, 3:6] = L
        Y[0:3, 3:6] = -W @ expm(-L)
        E = -expm(Y)[0:3, 3:6]
        for i, j in ((0, 1), (0, 2), (1, 2)):
            E[i, j] = E[j, i] = 0.5 * (E[i, j] + E[j, i])
        return W.copy(), E

    def forces(self, X, f, stress):
        """get_forces from the atoms' Cartesian forces f [n, 3] and the calculator's stress (eV/A^3, ASE's sign)."""
        _, _, F = self.atoms(X)
        N, E = self.cell_forces(X, stress)
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = np.sum(E * N) / np.sqrt(np.sum(E ** 2) * np.sum(N ** 2))
        naive = bool(np.all(np.isclose(E, N))) or bool(cos > 0.8)
        self.branch = "naive" if naive else "exact"
        return np.vstack([np.asarray(f, dtype=np.float64) @ F, (N if naive else E) / self.c])


def run_cell_ref(C0, pos0, efs, fmax=0.1, steps=100, **fire):
    """Optimizer.run(fmax, steps) of FIRE(ExpCellFilter(atoms)); ``efs(C, pos) -> (e, f [n, 3], stress [3, 3])``.
    -> dict(X, C, pos, e, f, s, g (the n + 3 rows), n_steps, converged, n_evals, traj (C, pos after each step), branches)."""
    filt = ExpCellFilterRef(C0, len(pos0))
    opt = FireRef(filt.initial(pos0), **{**DEFAULTS, **fire})

    def evaluate():
        C, pos, _ = filt.atoms(opt.r)
        e, f, s = efs(C, pos)
        return e, f, s, filt.forces(opt.r, f, s)

    e, f, s, g = evaluate()
    n_evals, n_steps, branches = 1, 0, [filt.branch]
    traj = [filt.atoms(opt.r)[:2]]
    conv = converged(g, fmax)
    while not conv and n_steps < steps:
        opt.step(g)
        n_steps += 1
        traj.append(filt.atoms(opt.r)[:2])
        e, f, s, g = evaluate()
        branches.append(filt.branch)
        n_evals += 1
        conv = converged(g, fmax)
    C, pos, _ = filt.atoms(opt.r)
    return dict(X=opt.r, C=C, pos=pos, e=e, f=f, s=s, g=g, n_steps=n_steps, converged=conv, n_evals=n_evals, traj=traj,
                branches=branches, opt=opt)


# --- cases on the spring crystals of springs_ref ------------------------------------------------------------------------------
def sym_strain(rng, eps):
    A = rng.normal(0.0, eps, (3, 3))
    return np.eye(3) + (A + A.T) / 2


def _case(seed, n, eps=0.05):
    """target (lat*, frac*), a start cell lat* S (S symmetric, ~eps) and start positions near the strained target."""
    from alignn_amd.synthetic import make_crystal

    lat_t, frac_t, _ = make_crystal(max(n, 2), 700 + seed)
    frac_t = frac_t[:n]
    rng = np.random.default_rng(seed)
    C0 = lat_t @ sym_strain(rng, eps)
    pos0 = frac_t @ C0 + rng.normal(0.0, 0.05, (n, 3))
    return lat_t, frac_t, C0, pos0


def _strained_state(seed, n, eps):
    lat_t, frac_t, C0, pos0 = _case(seed, n)
    filt = ExpCellFilterRef(C0, n)
    rng = np.random.default_rng(100 + seed)
    F = sym_strain(rng, eps)  # ~eps strain / shear on top of C0
    X = np.vstack([pos0 + rng.normal(0.0, 0.05, (n, 3)), n * np.real(logm(F))])
    return filt, X, springs_efs(*spring_list(lat_t, frac_t))


def exact_branch_state(seed):
    """A large symmetric log-strain L and a skewed virial for which cos(exact, naive) < 0.8: (L, stress) with the stress
    in eV/A^3 for a cell of volume ``V``."""
    rng = np.random.default_rng(seed)
    while True:
        A = rng.normal(size=(3, 3))
        L = 0.6 * (A + A.T)
        B = rng.normal(size=(3, 3))
        W = 50.0 * (B + B.T)
        Y = np.zeros((6, 6))
        Y[:3, :3] = Y[3:, 3:] = L
        Y[:3, 3:] = -W @ expm(-L)
        E = -expm(Y)[:3, 3:]
        E = (E + E.T) / 2
        if np.sum(E * W) / np.sqrt(np.sum(E * E) * np.sum(W * W)) < 0.6:
            return L, W


# --- FixAtoms and the arguments of ExpCellFilter ------------------------------------------------------------------------------
def voigt_mask(m):
    """A mask of six Voigt flags (xx, yy, zz, yz, xz, xy) as the full 3 x 3 (voigt_6_to_full_3x3_stress); a [3, 3] as it is."""
    m = np.asarray(m, dtype=np.float64)
    if m.shape == (3, 3):
        return m.copy()
    xx, yy, zz, yz, xz, xy = m
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


class ConstrainedFilterRef(ExpCellFilterRef):
    """ExpCellFilter(atoms, mask, hydrostatic_strain, constant_volume, scalar_pressure) around atoms with FixAtoms(fixed)."""

    def __init__(self, C0, n, mask=None, hydrostatic_strain=False, constant_volume=False, scalar_pressure=0.0, fixed=None):
        super().__init__(C0, n)
        self.mask = np.ones((3, 3)) if mask is None else voigt_mask(mask)
        self.hydrostatic_strain, self.constant_volume = hydrostatic_strain, constant_volume
        self.pressure = float(scalar_pressure)
        self.fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)

    def virial(self, X, stress):
        C, _, _ = self.atoms(X)
        W = -abs(np.linalg.det(C)) * (sym3(stress) + np.diag([self.pressure] * 3))
        if self.hydrostatic_strain:
            vtr = W.trace()
            W = np.diag([vtr / 3.0, vtr / 3.0, vtr / 3.0])
        if (self.mask != 1.0).any():
            W = W * self.mask
        return W

    def cell_forces(self, X, stress):
        W = self.virial(X, stress)
        L = X[self.n:] / self.c
        Y = np.zeros((6, 6))
        Y[0:3, 0:3] = L
        Y[3:6, 3:6] = L
        Y[0:3, 3:6] = -W @ expm(-L)
        E = -expm(Y)[0:3, 3:6]
        for i, j in ((0, 1), (0, 2), (1, 2)):
            E[i, j] = E[j, i] = 0.5 * (E[i, j] + E[j, i])
        return W.copy(), E

    def constrain(self, G):
        """The constant-volume step on a cell force (after the choice between naive and exact)."""
        G = G.copy()
        if self.constant_volume:
            np.fill_diagonal(G, np.diag(G) - G.trace() / 3.0)
        return G

    def forces(self, X, f, stress):
        f = np.array(f, dtype=np.float64)
        f[self.fixed] = 0.0
        _, _, F = self.atoms(X)
        N, E = self.cell_forces(X, stress)
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = np.sum(E * N) / np.sqrt(np.sum(E ** 2) * np.sum(N ** 2))
        naive = bool(np.all(np.isclose(E, N))) or bool(cos > 0.8)
        self.branch = "naive" if naive else "exact"
        return np.vstack([f @ F, self.constrain(N if naive else E) / self.c])

    def enthalpy(self, X, e):
        return e + self.pressure * abs(np.linalg.det(self.atoms(X)[0]))


def run_constrained_ref(C0, pos0, efs, fmax=0.1, steps=100, fire=None, **options):
    """run_cell_ref with the constrained filter: Optimizer.run(fmax, steps) of FIRE(ExpCellFilter(atoms, **options)).
    Beside run_cell_ref's fields: h (the enthalpy), h0 (that of the start), Xs (X at the start and after each step)."""
    filt = ConstrainedFilterRef(C0, len(pos0), **options)
    opt = FireRef(filt.initial(pos0), **{**DEFAULTS, **(fire or {})})

    def evaluate():
        C, pos, _ = filt.atoms(opt.r)
        e, f, s = efs(C, pos)
        return e, f, s, filt.forces(opt.r, f, s)

    e, f, s, g = evaluate()
    h0 = filt.enthalpy(opt.r, e)
    n_evals, n_steps, branches, Xs = 1, 0, [filt.branch], [opt.r.copy()]
    traj = [filt.atoms(opt.r)[:2]]
    conv = converged(g, fmax)
    while not conv and n_steps < steps:
        opt.step(g)
        n_steps += 1
        Xs.append(opt.r.copy())
        traj.append(filt.atoms(opt.r)[:2])
        e, f, s, g = evaluate()
        branches.append(filt.branch)
        n_evals += 1
        conv = converged(g, fmax)
    C, pos, _ = filt.atoms(opt.r)
    return dict(X=opt.r, C=C, pos=pos, e=e, f=f, s=s, g=g, n_steps=n_steps, converged=conv, n_evals=n_evals, traj=traj,
                branches=branches, opt=opt, h=filt.enthalpy(opt.r, e), h0=h0, Xs=Xs, filt=filt)


def run_fixed_ref(pos0, ef, fixed, fmax=0.1, steps=100, fire=None):
    """Optimizer.run(fmax, steps) of FIRE(atoms) at fixed cell with FixAtoms(fixed); ``ef(pos) -> (e, f)``.  ``f`` of the result
    is the force as evaluated, ``g`` the constrained one."""
    fixed = np.asarray(fixed, dtype=bool)
    opt = FireRef(pos0, **{**DEFAULTS, **(fire or {})})

    def evaluate():
        e, f = ef(opt.r)
        g = np.array(f, dtype=np.float64)
        g[fixed] = 0.0
        return e, np.asarray(f, dtype=np.float64), g

    e, f, g = evaluate()
    n_steps, Xs = 0, [opt.r.copy()]
    conv = converged(g, fmax)
    while not conv and n_steps < steps:
        opt.step(g)
        n_steps += 1
        Xs.append(opt.r.copy())
        e, f, g = evaluate()
        conv = converged(g, fmax)
    return dict(r=opt.r, e=e, f=f, g=g, n_steps=n_steps, converged=conv, n_evals=n_steps + 1, Xs=Xs)


SLAB = [1, 1, 0, 0, 0, 1]  # the in-plane cell free, the vacuum axis frozen
