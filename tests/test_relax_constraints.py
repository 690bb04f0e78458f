"""Checks of ``ConstrainedFilterRef``, ``run_constrained_ref`` and ``run_fixed_ref`` of tests/relax_ref.py, the restatement of
ASE 3.22.1's ``FixAtoms`` and of the arguments ``mask``, ``hydrostatic_strain``, ``constant_volume`` and ``scalar_pressure`` of
``ExpCellFilter`` that specifies the constraints of ``alignn_amd.relax`` (csrc/relax.hip, the last fields of
``alignn_fire_args``); the order of ``ExpCellFilter.get_forces`` is written out there.  ASE is not a dependency: the restatement
is pinned by a case worked out by hand, by gradient checks of the enthalpy of the analytic spring potential of
tests/springs_ref.py, and by the physics of converged runs.  The GPU tests (test_gpu_relax_constraints.py) hold the kernel and
the relaxer to it."""

import inspect

import numpy as np
import pytest

from alignn_amd import _lib
from alignn_amd.relax import RelaxResult, relax
from tests.relax_ref import (SLAB, ConstrainedFilterRef, _case, _strained_state, run_cell_ref, run_constrained_ref, run_fixed_ref,
                             sym3, voigt_mask)
from tests.springs_ref import simple_cubic, spring_list, springs_efs


# --- the restatement with everything off is ExpCellFilterRef ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 40])
def test_all_options_off_is_the_plain_filter_bit_for_bit(n):
    rng = np.random.default_rng(n)
    for seed in range(4):
        filt0, X, _ = _strained_state(10 + seed, n, 0.08)
        filt = ConstrainedFilterRef(filt0.C0, n)
        f, s = rng.normal(0.0, 1.0, (n, 3)), rng.normal(0.0, 0.02, (3, 3))
        want, got = filt0.forces(X, f, s), filt.forces(X, f, s)
        assert got.tobytes() == want.tobytes() and filt.branch == filt0.branch
        N0, E0 = filt0.cell_forces(X, s)
        N, E = filt.cell_forces(X, s)
        assert N.tobytes() == N0.tobytes() and E.tobytes() == E0.tobytes()
    lat_t, frac_t, C0, pos0 = _case(7, 5, 0.05)
    efs = springs_efs(*spring_list(lat_t, frac_t))
    a, b = run_cell_ref(C0, pos0, efs, fmax=1e-3, steps=300), run_constrained_ref(C0, pos0, efs, fmax=1e-3, steps=300)
    assert a["n_steps"] == b["n_steps"] > 5 and a["X"].tobytes() == b["X"].tobytes() and b["h"] == b["e"]


# --- by hand ----------------------------------------------------------------------------------------------------------------
def test_cell_rows_by_hand():
    """One atom in a cube of edge 2 (V = 8) at F = I, stress diag(0.01, 0.02, 0.03) eV/A^3, scalar_pressure 0.005:
    W = -8 diag(0.015, 0.025, 0.035) = diag(-0.12, -0.20, -0.28).  At L = 0 the block matrix Y is nilpotent, expm(Y) = I + Y:
    the exact force is W itself, the switch takes the naive one, c = n = 1."""
    C0, X = 2.0 * np.eye(3), np.zeros((4, 3))
    s = np.diag([0.01, 0.02, 0.03])
    f = np.array([[0.3, -0.2, 0.1]])

    def rows(**kw):
        filt = ConstrainedFilterRef(C0, 1, scalar_pressure=0.005, **kw)
        g = filt.forces(X, f, s)
        assert filt.branch == "naive"
        return g

    g = rows()
    assert np.array_equal(g[0], f[0])
    assert g[1:] == pytest.approx(np.diag([-0.12, -0.20, -0.28]), abs=1e-15)
    # without the pressure: -8 diag(0.01, 0.02, 0.03)
    assert ConstrainedFilterRef(C0, 1).forces(X, f, s)[1:] == pytest.approx(np.diag([-0.08, -0.16, -0.24]), abs=1e-15)
    # the slab mask keeps xx, yy (and xy, zero here): the zz row is exactly zero
    g = rows(mask=SLAB)
    assert g[1:] == pytest.approx(np.diag([-0.12, -0.20, 0.0]), abs=1e-15) and np.array_equal(g[3], np.zeros(3))
    # hydrostatic: tr W / 3 = -0.60 / 3 = -0.20 on the diagonal
    assert rows(hydrostatic_strain=True)[1:] == pytest.approx(-0.20 * np.eye(3), abs=1e-15)
    # hydrostatic first, then the mask: diag(-0.20, -0.20, 0)
    assert rows(hydrostatic_strain=True, mask=SLAB)[1:] == pytest.approx(np.diag([-0.20, -0.20, 0.0]), abs=1e-15)
    # constant volume: tr / 3 = -0.20 off the diagonal of diag(-0.12, -0.20, -0.28)
    g = rows(constant_volume=True)
    assert g[1:] == pytest.approx(np.diag([0.08, 0.0, -0.08]), abs=1e-15) and abs(np.trace(g[1:])) < 1e-16
    # the mask, then constant volume: diag(-0.12, -0.20, 0) - (-0.32 / 3)
    g = rows(mask=SLAB, constant_volume=True)
    assert g[1:] == pytest.approx(np.diag([-0.12 + 0.32 / 3, -0.20 + 0.32 / 3, 0.32 / 3]), abs=1e-15)
    # a fixed atom: its row is zero, the cell rows are not touched
    g = rows(fixed=[True])
    assert np.array_equal(g[0], np.zeros(3)) and g[1:] == pytest.approx(np.diag([-0.12, -0.20, -0.28]), abs=1e-15)
    # off-diagonal: a Voigt mask frees (i, j) and (j, i) together; two atoms: c = 2 halves the rows
    filt = ConstrainedFilterRef(C0, 2, mask=[0, 0, 0, 0, 0, 1])
    g = filt.forces(np.zeros((5, 3)), np.zeros((2, 3)), np.array([[0.01, 0.04, 0.05], [0.02, 0.02, 0.06], [0.05, 0.06, 0.03]]))
    want = np.zeros((3, 3))
    want[0, 1] = want[1, 0] = -8 * 0.03 / 2  # sym: (0.04 + 0.02) / 2
    assert g[2:] == pytest.approx(want, abs=1e-15) and np.count_nonzero(g[2:]) == 2
    assert np.array_equal(voigt_mask([1, 2, 3, 4, 5, 6]), [[1, 6, 5], [6, 2, 4], [5, 4, 3]])


# --- the cell rows are minus the gradient of the enthalpy over the free components -------------------------------------------
def _state_in(seed, n, eps, basis):
    """A strained state (relax_ref._strained_state) whose log-strain L lies in the span of ``basis`` (symmetric 3 x 3
    matrices, orthogonal to each other): its projection onto it."""
    filt, X, efs = _strained_state(seed, n, eps)
    L = X[n:] / n
    X[n:] = n * sum(np.sum(L * b) / np.sum(b * b) * b for b in basis)
    return filt.C0, X, efs


def _sym_basis(mask):
    out = []
    for i in range(3):
        for j in range(i, 3):
            if mask[i, j]:
                b = np.zeros((3, 3))
                b[i, j] = b[j, i] = 1.0
                out.append(b)
    return out


def _check_gradient(filt, X, efs, directions, tol_scale=None):
    """-d (E + p V) / d X_c along each of ``directions`` (symmetric 3 x 3) by central differences against the exact cell rows of
    ``filt`` (after its constant-volume step): the step and tolerance of
    test_relax_cell.test_exact_cell_rows_and_atom_rows_are_minus_the_gradient."""
    n = filt.n

    def H(Xq):
        C, pos, _ = filt.atoms(Xq)
        return efs(C, pos)[0] + filt.pressure * abs(np.linalg.det(C))

    C, pos, _ = filt.atoms(X)
    _, E = filt.cell_forces(X, efs(C, pos)[2])
    cell = filt.constrain(E) / filt.c
    scale = np.abs(cell).max()
    assert scale > 1e-3
    h = 1e-5
    for D in directions:
        Xp, Xm = X.copy(), X.copy()
        Xp[n:] += h * D
        Xm[n:] -= h * D
        fd = -(H(Xp) - H(Xm)) / (2 * h)
        assert fd == pytest.approx(np.sum(cell * D), rel=1e-6, abs=1e-6 * scale), D
    return cell


@pytest.mark.parametrize("seed,n,eps", [(2, 3, 0.05), (3, 6, 0.08), (4, 1, 0.05)])
def test_cell_rows_are_minus_the_enthalpy_gradient_over_the_free_components(seed, n, eps):
    """Each option alone, then mask + pressure.  The pressure term: d (p V) / d F = p V F^-T is what the virial -p V I carries
    through the same Frechet derivative, so it holds at any L.  A mask acts on the virial BEFORE the exact transform (ASE's
    order), so the masked rows are the gradient over the free components where the free components are closed under matrix
    products and L lies in them - the block masks of everyday use (the slab mask: the xy block; the diagonal; and the run
    keeps L there, its masked rows being exactly zero); these are checked.  hydrostatic_strain: L = l I, the one free direction
    I.  constant_volume: the traceless directions, and the rows' trace is zero."""
    full = _sym_basis(np.ones((3, 3)))
    p = 0.02
    C0, X, efs = _state_in(seed, n, eps, full)
    cell = _check_gradient(ConstrainedFilterRef(C0, n, scalar_pressure=p), X, efs, full)
    assert np.abs(cell - _check_gradient(ConstrainedFilterRef(C0, n), X, efs, full)).max() > 1e-3  # (the pressure matters)
    for mask in (SLAB, [1, 1, 1, 0, 0, 0]):
        basis = _sym_basis(voigt_mask(mask))
        C0, X, efs = _state_in(seed, n, eps, basis)
        for pp in (0.0, p):
            filt = ConstrainedFilterRef(C0, n, mask=mask, scalar_pressure=pp)
            cell = _check_gradient(filt, X, efs, basis)
            assert np.array_equal(cell[voigt_mask(mask) == 0], np.zeros(int((voigt_mask(mask) == 0).sum())))
    C0, X, efs = _state_in(seed, n, eps, [np.eye(3)])
    X[n:] += n * 0.03 * np.eye(3)
    cell = _check_gradient(ConstrainedFilterRef(C0, n, hydrostatic_strain=True), X, efs, [np.eye(3)])
    assert np.abs(cell - cell[0, 0] * np.eye(3)).max() <= 1e-12 * abs(cell[0, 0])
    traceless = [b for b in full if b[0, 1] or b[0, 2] or b[1, 2]] + [np.diag([1.0, -1.0, 0.0]), np.diag([1.0, 1.0, -2.0])]
    C0, X, efs = _state_in(seed, n, eps, full)
    cell = _check_gradient(ConstrainedFilterRef(C0, n, constant_volume=True), X, efs, traceless)
    assert abs(np.trace(cell)) <= 1e-15 * np.abs(cell).max()


# --- converged runs on the spring crystal -----------------------------------------------------------------------------------
FMAX, STEPS = 1e-6, 3000


def _spring_case(seed=1, n=5, eps=0.05):
    """(the seed: one whose float64 restatement converges well inside the cap under every option; each run asserts it)"""
    lat_t, frac_t, C0, pos0 = _case(seed, n, eps)
    return C0, pos0, springs_efs(*spring_list(lat_t, frac_t))


def test_pressure_run_ends_at_the_target_pressure():
    C0, pos0, efs = _spring_case()
    p = 0.01
    res = run_constrained_ref(C0, pos0, efs, fmax=FMAX, steps=STEPS, scalar_pressure=p)
    assert res["converged"] and 5 < res["n_steps"] < STEPS
    V = abs(np.linalg.det(res["C"]))
    assert abs(-np.trace(sym3(res["s"])) / 3 - p) <= FMAX * len(pos0) / V  # every cell row V |S + p I|_ij / c < fmax
    assert res["h"] <= res["h0"] and res["h"] == pytest.approx(res["e"] + p * V, rel=1e-15)
    free = run_constrained_ref(C0, pos0, efs, fmax=FMAX, steps=STEPS)
    assert V < abs(np.linalg.det(free["C"])) * (1 - 1e-4)  # compressed against the free cell


def test_hydrostatic_run_scales_the_cell():
    C0, pos0, efs = _spring_case()
    res = run_constrained_ref(C0, pos0, efs, fmax=FMAX, steps=STEPS, hydrostatic_strain=True)
    assert res["converged"] and 5 < res["n_steps"] < STEPS
    lam = (abs(np.linalg.det(res["C"])) / abs(np.linalg.det(C0))) ** (1.0 / 3.0)
    assert abs(lam - 1.0) > 1e-4
    assert np.abs(res["C"] - lam * C0).max() <= 1e-12 * np.abs(C0).max()


def test_constant_volume_run_keeps_the_volume():
    C0, pos0, efs = _spring_case()
    res = run_constrained_ref(C0, pos0, efs, fmax=FMAX, steps=STEPS, constant_volume=True)
    assert res["converged"] and 5 < res["n_steps"] < STEPS
    assert np.abs(res["C"] - C0).max() > 1e-3  # the shape relaxed
    V0 = abs(np.linalg.det(C0))
    for C, _ in res["traj"]:
        assert abs(abs(np.linalg.det(C)) - V0) <= 1e-12 * V0


def test_masked_components_and_fixed_rows_never_move():
    C0, pos0, efs = _spring_case()
    n = len(pos0)
    fixed = np.array([True, False, False, True, False])
    res = run_constrained_ref(C0, pos0, efs, fmax=FMAX, steps=STEPS, mask=SLAB, fixed=fixed)
    assert res["converged"] and 5 < res["n_steps"] < STEPS and set(res["branches"]) == {"naive"}
    m = voigt_mask(SLAB)
    for X in res["Xs"]:
        assert np.array_equal(X[n:][m == 0], np.zeros(5)) and np.array_equal(X[n:], X[n:].T)
        assert X[:n][fixed].tobytes() == pos0[fixed].tobytes()
    assert np.abs(res["X"][n:][m == 1]).max() > 1e-3 and np.abs(res["X"][:n][~fixed] - pos0[~fixed]).max() > 1e-3
    # F = expm(L) is the identity along the frozen axis: no cell vector changes its z component
    assert np.abs(res["C"][:, 2] - C0[:, 2]).max() <= 1e-14 * np.abs(C0).max() and np.abs(res["C"] - C0).max() > 1e-3
    assert np.abs(res["f"][fixed]).max() > 1e-3  # held against a force that the convergence test does not see
    assert np.array_equal(res["g"][:n][fixed], np.zeros((2, 3)))


def test_all_atoms_fixed_at_fixed_cell_is_converged_at_step_zero():
    C0, pos0, efs = _spring_case()
    res = run_fixed_ref(pos0, lambda r: efs(C0, r)[:2], np.ones(len(pos0), dtype=bool), fmax=FMAX, steps=STEPS)
    assert res["converged"] and res["n_steps"] == 0 and res["n_evals"] == 1 and np.abs(res["f"]).max() > 1e-3
    part = run_fixed_ref(pos0, lambda r: efs(C0, r)[:2], [True, False, False, True, False], fmax=FMAX, steps=STEPS)
    assert part["converged"] and part["n_steps"] > 5
    for X in part["Xs"]:
        assert X[[0, 3]].tobytes() == pos0[[0, 3]].tobytes()
    # one atom in the cube of test_relax_cell under pressure: V k ... the cell ends where the springs' pressure is p
    one = run_constrained_ref(3.15 * np.eye(3), np.zeros((1, 3)), simple_cubic(3.0), fmax=FMAX, steps=STEPS,
                              scalar_pressure=0.05, fixed=[True])
    assert one["converged"] and one["C"][0, 0] < 3.0 and np.array_equal(one["X"][0], np.zeros(3))


# --- the public interface ---------------------------------------------------------------------------------------------------
def test_relax_signature_and_result_fields():
    sig = inspect.signature(relax).parameters
    assert sig["fixed"].default is None and sig["cell_mask"].default is None
    assert sig["hydrostatic_strain"].default is False and sig["constant_volume"].default is False
    assert sig["scalar_pressure"].default == 0.0
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("fixed", "cell_mask", "hydrostatic_strain",
                                                                       "constant_volume", "scalar_pressure"))
    assert RelaxResult.__dataclass_fields__["enthalpies"].default is None


def test_fire_args_carry_the_constraints():
    names = [f[0] for f in _lib.FireArgs._fields_]
    new = ["fixed", "cell_mask", "scalar_pressure", "hydrostatic_strain", "constant_volume", "enthalpy_out"]
    assert names[-6:] == new and names[-7] == "fa"  # appended: the block before them is the old one
    blank = _lib.FireArgs()
    assert all(not getattr(blank, k) for k in new)  # a field left out is NULL / 0: off
    lib = _lib.load()  # (after build(); load() itself refuses a block of another size)
    import ctypes

    assert lib.alignn_fire_args_sizeof() == ctypes.sizeof(_lib.FireArgs)


def _call(**kw):
    lat, pos = [np.eye(3) * 5, np.eye(3) * 6], [np.zeros((2, 3)), np.ones((3, 3))]
    ff = lambda lat, pos: None  # noqa: E731
    return relax(None, lat, pos, forces_fn=ff, device="cpu", **kw)


def test_relax_validates_the_constraints_before_touching_a_device():
    ok_fixed = [np.array([True, False]), None]
    bad = [
        dict(cell_mask=SLAB),  # the filter's arguments without the filter
        dict(hydrostatic_strain=True),
        dict(constant_volume=True),
        dict(scalar_pressure=0.01),
        dict(scalar_pressure=[0.0, 0.01]),
        dict(optimize_lattice=True, cell_mask=[1, 1, 0.5, 0, 0, 1]),  # neither 0 nor 1
        dict(optimize_lattice=True, cell_mask=[1, 1, 2, 0, 0, 1]),
        dict(optimize_lattice=True, cell_mask=np.full((3, 3), -1.0)),
        dict(optimize_lattice=True, cell_mask=[1, 1, float("nan"), 0, 0, 1]),
        dict(optimize_lattice=True, cell_mask=[1, 1, 0, 0, 1]),  # shapes and counts
        dict(optimize_lattice=True, cell_mask=np.ones((2, 3))),
        dict(optimize_lattice=True, cell_mask=[SLAB] * 3),
        dict(optimize_lattice=True, cell_mask=[SLAB, np.ones((3, 2))]),
        dict(optimize_lattice=True, cell_mask=1),
        dict(optimize_lattice=True, scalar_pressure=[0.01, 0.02, 0.03]),
        dict(optimize_lattice=True, scalar_pressure=np.zeros((2, 1))),
        dict(optimize_lattice=True, scalar_pressure="high"),
        dict(optimize_lattice=True, scalar_pressure=float("inf")),  # not finite
        dict(optimize_lattice=True, scalar_pressure=[0.0, float("nan")]),
        dict(optimize_lattice=True, hydrostatic_strain=[True, False]),  # one bool for the call
        dict(optimize_lattice=True, constant_volume=1),
        dict(fixed=[np.array([True, False])]),  # counts
        dict(fixed=ok_fixed + [None]),
        dict(fixed=[np.array([True, False, False]), None]),  # shapes
        dict(fixed=[np.array([[True, False]]), None]),
        dict(fixed=np.array([True, False])),
        dict(fixed=[np.array([1, 0]), None]),  # not boolean
        dict(fixed=[np.array([0.0, 1.0]), None]),
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="relax"):
            _call(**kw)
    good = [
        dict(fixed=ok_fixed),
        dict(fixed=[[True, True], [True, True, True]]),  # everything held at fixed cell: legal
        dict(fixed=[None, None], scalar_pressure=0.0),
        dict(optimize_lattice=True, fixed=ok_fixed, cell_mask=SLAB, scalar_pressure=0.01),
        dict(optimize_lattice=True, cell_mask=np.ones((3, 3))),
        dict(optimize_lattice=True, cell_mask=[SLAB, np.eye(3)], scalar_pressure=[0.0, -0.01]),
        dict(optimize_lattice=True, cell_mask=np.ones((2, 6)), hydrostatic_strain=True, constant_volume=True),
        dict(optimize_lattice=True, cell_mask=np.ones((2, 3, 3), dtype=bool), scalar_pressure=np.float32(0.5)),
    ]
    for kw in good:
        with pytest.raises(TypeError, match="GPU"):  # a CPU device: every check of the arguments has passed
            _call(**kw)
