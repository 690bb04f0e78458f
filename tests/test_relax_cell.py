"""The executable specification of ``alignn_amd.relax(..., optimize_lattice=True)`` (csrc/relax.hip, ``alignn_fire_step`` with the filter's state):
a float64 numpy / scipy restatement of ASE's ``ExpCellFilter`` (ase/constraints.py, 3.22.1, default arguments) as the
reference's ``ForceField.optimize_atoms`` applies it (alignn/ff/ff.py:373-415, ``optimize_lattice=True``), and the run loop of
``Optimizer.run`` over its n + 3 generalised rows with ``FireRef`` / ``converged`` of test_relax_fire.py.  ASE is not a
dependency: the restatement is pinned by gradient checks against an analytic periodic potential (harmonic springs over a
fixed list of periodic images) instead.  The GPU tests (test_gpu_relax_cell.py) hold the kernel and the relaxer to it."""

import inspect
import itertools

import numpy as np
import pytest
from scipy.linalg import expm, logm

from alignn_amd.relax import RelaxResult, relax
from tests.test_relax_fire import DEFAULTS, FireRef, converged


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


# --- an analytic periodic potential: harmonic springs over a fixed image list, at rest in a target structure ----------------
def spring_list(lat, frac, nnb=8):
    """Each atom tied to its ``nnb`` nearest neighbours (images within one cell) of the target (lat, frac), rest length the
    target distance.  -> (i, j, image [m, 3], d0, k)."""
    lat, frac = np.asarray(lat, dtype=np.float64), np.asarray(frac, dtype=np.float64)
    pos = frac @ lat
    n = len(pos)
    rows = []
    for i in range(n):
        cand = []
        for j in range(n):
            for img in itertools.product((-1, 0, 1), repeat=3):
                if i == j and img == (0, 0, 0):
                    continue
                d = pos[j] + np.array(img) @ lat - pos[i]
                cand.append((float(np.linalg.norm(d)), j, img))
        cand.sort(key=lambda t: t[0])
        rows += [(i, j, img, d0) for d0, j, img in cand[:nnb]]
    I = np.array([r[0] for r in rows])
    J = np.array([r[1] for r in rows])
    img = np.array([r[2] for r in rows], dtype=np.float64)
    d0 = np.array([r[3] for r in rows])
    k = 1.0 + 0.5 * (np.arange(len(rows)) % 3)
    return I, J, img, d0, k


def springs_efs(I, J, img, d0, k):
    """-> efs(C, pos) = (E, forces, stress = (1/V) dE/d strain): ASE's sign (positive under tension)."""

    def efs(C, pos):
        d = pos[J] - pos[I] + img @ C
        r = np.sqrt((d * d).sum(1))
        dphi = k * (r - d0)
        fv = (dphi / r)[:, None] * d  # dE / dd
        f = np.zeros_like(pos)
        np.add.at(f, I, fv)
        np.add.at(f, J, -fv)
        s = fv.T @ d / abs(np.linalg.det(C))
        return 0.5 * float((k * (r - d0) ** 2).sum()), f, s

    return efs


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


def _energy_of_X(filt, efs):
    def E(X):
        C, pos, _ = filt.atoms(X)
        return efs(C, pos)[0]

    return E


def test_cell_rows_at_identity_are_the_virial_over_n():
    lat_t, frac_t, C0, pos0 = _case(1, 5)
    efs = springs_efs(*spring_list(lat_t, frac_t))
    filt = ExpCellFilterRef(C0, 5)
    X = filt.initial(pos0)
    C, pos, F = filt.atoms(X)
    assert np.array_equal(F, np.eye(3)) and np.array_equal(C, C0) and np.array_equal(pos, pos0)
    e, f, s = efs(C, pos)
    g = filt.forces(X, f, s)
    W = -abs(np.linalg.det(C0)) * sym3(s)
    assert filt.branch == "naive" and np.abs(W).max() > 1e-2
    assert np.array_equal(g[5:], W / 5) and np.array_equal(g[:5], f @ np.eye(3))


def _strained_state(seed, n, eps):
    lat_t, frac_t, C0, pos0 = _case(seed, n)
    filt = ExpCellFilterRef(C0, n)
    rng = np.random.default_rng(100 + seed)
    F = sym_strain(rng, eps)  # ~eps strain / shear on top of C0
    X = np.vstack([pos0 + rng.normal(0.0, 0.05, (n, 3)), n * np.real(logm(F))])
    return filt, X, springs_efs(*spring_list(lat_t, frac_t))


@pytest.mark.parametrize("seed,n,eps", [(2, 3, 0.05), (3, 6, 0.08), (4, 1, 0.05)])
def test_exact_cell_rows_and_atom_rows_are_minus_the_gradient(seed, n, eps):
    filt, X, efs = _strained_state(seed, n, eps)
    C, pos, F = filt.atoms(X)
    e, f, s = efs(C, pos)
    N, E = filt.cell_forces(X, s)
    g_atoms = f @ F
    Efn = _energy_of_X(filt, efs)
    h = 1e-5
    for a in range(n):
        for b in range(3):
            Xp, Xm = X.copy(), X.copy()
            Xp[a, b] += h
            Xm[a, b] -= h
            fd = -(Efn(Xp) - Efn(Xm)) / (2 * h)
            assert fd == pytest.approx(g_atoms[a, b], rel=1e-6, abs=1e-9 + 1e-6 * np.abs(g_atoms).max())
    cell = E / filt.c
    scale = np.abs(cell).max()
    assert scale > 1e-3
    for i in range(3):
        for j in range(i, 3):  # X_c stays symmetric: move (i, j) and (j, i) together
            Xp, Xm = X.copy(), X.copy()
            for (p, q) in {(i, j), (j, i)}:
                Xp[n + p, q] += h
                Xm[n + p, q] -= h
            fd = -(Efn(Xp) - Efn(Xm)) / (2 * h)
            want = cell[i, j] + (cell[j, i] if i != j else 0.0)
            assert fd == pytest.approx(want, rel=1e-6, abs=1e-6 * scale), (i, j)
    # (the naive force is not the gradient away from F = I, but at ~5 % strain it is close: the filter uses it)
    assert np.abs(N / filt.c - cell).max() > 1e-9 * scale
    filt.forces(X, f, s)
    assert filt.branch == "naive"


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


def test_switch_takes_the_exact_force_when_the_two_point_apart():
    from alignn_amd.synthetic import make_crystal

    n = 4
    C0 = make_crystal(n, 11)[0]
    filt = ExpCellFilterRef(C0, n)
    L, W = exact_branch_state(5)
    X = np.vstack([np.zeros((n, 3)), n * L])
    C = filt.atoms(X)[0]
    s = -W / abs(np.linalg.det(C))
    N, E = filt.cell_forces(X, s)
    np.testing.assert_allclose(N, W, rtol=1e-13)
    g = filt.forces(X, np.zeros((n, 3)), s)
    assert filt.branch == "exact" and np.array_equal(g[n:], E / n)
    # the upper-right block of expm(Y) is the Frechet derivative of expm at L in the direction -W expm(-L)
    h = 1e-6
    D = -W @ expm(-L)
    fd = (expm(L + h * D) - expm(L - h * D)) / (2 * h)
    Y = np.zeros((6, 6))
    Y[:3, :3] = Y[3:, 3:] = L
    Y[:3, 3:] = D
    np.testing.assert_allclose(expm(Y)[:3, 3:], fd, rtol=1e-6, atol=1e-6 * np.abs(fd).max())


def test_expm_logm_round_trip():
    """The kernel keeps X_c instead of recomputing c logm(F) from the cell every step, as ASE does: the round trip changes
    nothing beyond 1e-12 on the tests' cells."""
    for seed, n, eps in [(2, 3, 0.05), (3, 6, 0.08), (4, 1, 0.05), (6, 17, 0.1)]:
        filt, X, _ = _strained_state(seed, n, eps)
        C, pos, _ = filt.atoms(X)
        X2 = filt.from_atoms(C, pos)
        assert np.abs(X2 - X).max() <= 1e-12 * max(1.0, np.abs(X).max()), seed
    L, _ = exact_branch_state(5)
    filt = ExpCellFilterRef(np.eye(3) * 4.0, 4)
    X = np.vstack([np.ones((4, 3)), 4 * L])
    assert np.abs(filt.from_atoms(*filt.atoms(X)[:2]) - X).max() <= 1e-12 * np.abs(X).max()


def simple_cubic(a0, k=2.0):
    """One atom, springs of rest length a0 (faces) and a0 sqrt(2) (edges) to its periodic images."""
    imgs = [v for v in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(x) for x in v) <= 2]
    img = np.array(imgs, dtype=np.float64)
    d0 = a0 * np.sqrt((img ** 2).sum(1))
    z = np.zeros(len(imgs), dtype=int)
    return springs_efs(z, z, img, d0, np.full(len(imgs), k))


def test_one_atom_cubic_crystal_relaxes_to_its_lattice_constant():
    a0 = 3.0
    res = run_cell_ref(1.05 * a0 * np.eye(3), np.zeros((1, 3)), simple_cubic(a0), fmax=1e-6, steps=1000)
    assert res["converged"] and res["n_steps"] > 5
    np.testing.assert_allclose(res["C"], a0 * np.eye(3), atol=1e-6)


def test_spring_crystal_relaxes_to_its_target_cell():
    lat_t, frac_t, C0, pos0 = _case(7, 5, 0.05)
    res = run_cell_ref(C0, pos0, springs_efs(*spring_list(lat_t, frac_t)), fmax=1e-6, steps=3000)
    assert res["converged"]
    np.testing.assert_allclose(res["C"], lat_t, atol=1e-4)
    rel = res["pos"] - res["pos"][0]
    want = frac_t @ lat_t - frac_t[0] @ lat_t
    np.testing.assert_allclose(rel, want, atol=1e-4)


def test_relax_accepts_optimize_lattice():
    sig = inspect.signature(relax).parameters
    assert sig["optimize_lattice"].default is False and sig["stress_weight"].default == 1.0
    assert RelaxResult.__dataclass_fields__["lattices"].default is None
    assert RelaxResult.__dataclass_fields__["stresses"].default is None
    with pytest.raises(ValueError):
        relax(None, [np.eye(3)], [np.zeros((1, 3)), np.zeros((1, 3))], forces_fn=lambda lat, pos: None, optimize_lattice=True)


def test_relax_cell_needs_a_stress_model():
    import torch

    from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig

    for kw in (dict(stresswise_weight=0.0), dict(stresswise_weight=0.05, batch_stress=False)):
        cfg = ALIGNNAtomWiseConfig(name="alignn_atomwise", alignn_layers=1, gcn_layers=1, hidden_features=16,
                                   embedding_features=16, atom_input_features=4, calculate_gradient=True, **kw)
        model = ALIGNNAtomWise(cfg).eval()
        with pytest.raises(ValueError, match="stress"):
            relax(model, [np.eye(3) * 4.0], [np.zeros((1, 3))], [torch.zeros(1, 4)], optimize_lattice=True)
