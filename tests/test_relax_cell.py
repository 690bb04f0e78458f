"""Checks of ``ExpCellFilterRef`` and ``run_cell_ref`` of tests/relax_ref.py, the float64 numpy / scipy restatement of ASE's
``ExpCellFilter`` that specifies ``alignn_amd.relax(..., optimize_lattice=True)`` (csrc/relax.hip, ``alignn_fire_step`` with the
filter's state).  ASE is not a dependency: the restatement is pinned by gradient checks against an analytic periodic potential
(the harmonic springs of tests/springs_ref.py) instead.  The GPU tests (test_gpu_relax_cell.py) hold the kernel and the relaxer
to it."""

import inspect

import numpy as np
import pytest
from scipy.linalg import expm

from alignn_amd.relax import RelaxResult, relax
from tests.relax_ref import ExpCellFilterRef, _case, _strained_state, exact_branch_state, run_cell_ref, sym3
from tests.springs_ref import simple_cubic, spring_list, springs_efs


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
