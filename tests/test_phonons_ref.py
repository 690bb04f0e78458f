"""Checks of tests/phonons_ref.py, the float64 numpy restatement of ASE 3.22.1's ``Phonons`` that specifies
``alignn_amd.phonons`` (csrc/phonon.hip): the order of the displaced supercells, the drift, symmetrize and acoustic passes, the
analytic dispersion of spring crystals, the DOS, and what the entry point refuses before it touches a device.  The GPU tests
(test_gpu_phonons.py) hold the kernels and ``phonons`` to the restatement."""

import numpy as np
import pytest

from alignn_amd.phonons import (EV_TO_CM1, EV_TO_THZ, FREQ_SCALE, MAX_DIM, PhononResult, lattice_points, monkhorst_pack,
                                phonons)
from tests.phonons_ref import (acoustic, displaced_supercells, dos, dq, inv_supercell, omega, phonons_ref, raw_force_constants,
                               sc_analytic, simple_cubic, spring_forces_of, supercell_images, symmetrize)

# ---- checks ---------------------------------------------------------------------------------------------------------------


def test_frequency_scale_and_units():
    assert FREQ_SCALE == pytest.approx(0.0646541, rel=1e-6)
    assert FREQ_SCALE == 1.054571800e-34 * 1e10 / np.sqrt(1.6021766208e-19 * 1.660539040e-27)
    assert EV_TO_THZ == pytest.approx(241.7989, rel=1e-6) and EV_TO_CM1 == pytest.approx(8065.544, rel=1e-6)
    assert omega(-4.0) == -2.0 * FREQ_SCALE and omega(0.0) == 0.0


@pytest.mark.parametrize("N,want", [(3, [0, 1, -1]), (4, [0, 1, -2, -1]), (1, [0]), (2, [0, -1]), (5, [0, 1, 2, -2, -1])])
def test_centred_lattice_points(N, want):
    R = lattice_points((N, 1, 2))
    assert R.shape == (2 * N, 3)
    assert list(R[::2, 0]) == want and list(R[:2, 2]) == [0, -1] and (R[:, 1] == 0).all()
    img = supercell_images((N, 1, 2))  # R is the image offset shifted into [-N // 2, ...)
    assert np.array_equal((R - img) % np.array([N, 1, 2]), np.zeros_like(R))


def test_monkhorst_pack():
    k = monkhorst_pack((2, 3, 1))
    assert k.shape == (6, 3)
    assert np.allclose(k[:, 0], [-0.25] * 3 + [0.25] * 3) and np.allclose(k[:3, 1], [-1 / 3, 0.0, 1 / 3]) and (k[:, 2] == 0).all()
    assert np.allclose(monkhorst_pack((20, 20, 20)).sum(0), 0.0)


def test_displaced_supercells_order():
    lat = np.array([[3.0, 0.1, 0.0], [0.2, 3.5, 0.0], [0.0, 0.3, 4.0]])
    pos = np.array([[0.1, 0.2, 0.3], [1.5, 1.7, 2.1]])
    N = (2, 3, 1)
    cells = displaced_supercells(lat, pos, N, 0.05, inv_supercell(lat, N))
    assert len(cells) == 12
    ideal = cells[0][1].copy()
    ideal[0, 0] += 0.05
    for d, (f, cart) in enumerate(cells):
        a, i, sg = d // 6, (d // 2) % 3, (-1.0, 1.0)[d % 2]
        diff = cart - ideal
        want = np.zeros_like(ideal)
        want[a, i] = sg * 0.05
        assert np.allclose(diff, want, atol=1e-14)
        assert (f >= 0).all() and (f < 1).all()
        assert np.allclose(np.exp(2j * np.pi * (f @ (lat * np.array(N, dtype=float)[:, None]) - cart) @ inv_supercell(lat, N)), 1.0)
    # image (m0 N1 + m1) N2 + m2 holds the atoms in input order, offset by m . lattice
    img = supercell_images(N)
    assert np.allclose(ideal.reshape(6, 2, 3), pos[None] + (img @ lat)[:, None, :])


@pytest.mark.parametrize("N", [(3, 3, 3), (4, 4, 4)])
def test_simple_cubic_springs_match_the_analytic_dispersion(N):
    lat, pos, shells = simple_cubic()
    m = 26.98
    qs = np.random.default_rng(1).uniform(-0.5, 0.5, (12, 3))
    qs[0] = 0.0
    _, _, _, w = phonons_ref(lat, pos, [m], N, 1e-3, spring_forces_of(shells), qs=qs)
    want = np.array([np.sort(sc_analytic(q, lat[0, 0], shells[0][1], shells[1][1], m)) for q in qs])
    assert np.abs(w - want).max() <= 1e-5 * np.abs(want).max(), np.abs(w - want).max()
    assert np.abs(w[0]).max() <= 1e-8  # acoustic rule: zero at Gamma


@pytest.mark.parametrize("N", [(3, 1, 1), (4, 1, 1)])
def test_two_mass_chain_branches(N):
    a, k, m1, m2 = 3.0, 2.0, 12.0, 40.0
    lat = np.diag([a, 12.0, 12.0])
    pos = np.array([[0.0, 0.0, 0.0], [a / 2, 0.0, 0.0]])
    _, D_N, R, _ = phonons_ref(lat, pos, [m1, m2], N, 1e-3, spring_forces_of([(a / 2, k)]))
    for qx in np.linspace(-0.5, 0.5, 11):
        D = dq(D_N, R, [qx, 0.3, -0.2])[np.ix_([0, 3], [0, 3])]
        got = omega(np.linalg.eigvalsh(D, UPLO="U"))
        s = 1 / m1 + 1 / m2
        root = np.sqrt(s * s - 4 * np.sin(np.pi * qx) ** 2 / (m1 * m2))
        want = omega(np.array([k * (s - root), k * (s + root)]))
        assert np.abs(got - want).max() <= 1e-5 * want.max(), (qx, got, want)


def test_drift_modes_and_raw_rows():
    rng = np.random.default_rng(5)
    n, N = 2, (2, 1, 1)
    forces = [rng.normal(size=(4, 3)) for _ in range(6 * n)]
    C0 = raw_force_constants(forces, n, N, 0.1, None)
    assert C0.shape == (2, 6, 6)
    assert C0[1, 3 * 1 + 2, 3 * 0 + 1] == (forces[6 + 4][2, 1] - forces[6 + 5][2, 1]) / 0.2  # cell 1 atom 0, row a=1 i=z
    Cf = raw_force_constants(forces, n, N, 0.1, "frederiksen")
    sm, sp = forces[0].sum(0), forces[1].sum(0)  # row 0: atom 0 along x
    assert np.allclose(Cf[0, 0, 0:3], ((forces[0][0] - sm) - (forces[1][0] - sp)) / 0.2)
    assert np.array_equal(Cf[1, 0], C0[1, 0]) and np.array_equal(Cf[0, 0, 3:], C0[0, 0, 3:])
    Cm = raw_force_constants(forces, n, N, 0.1, "mean")
    assert np.allclose(Cm[:, 0].reshape(-1, 3).sum(0), 0.0)


def test_symmetrize_is_idempotent_on_symmetric_input_and_acoustic_zeroes_gamma():
    rng = np.random.default_rng(2)
    for N in [(3, 3, 3), (2, 3, 4), (4, 1, 2)]:
        m = 6
        C_N = rng.normal(size=(int(np.prod(N)), m, m))
        S = symmetrize(C_N, N)
        assert np.allclose(symmetrize(S, N), S, rtol=0, atol=1e-15)
        A = C_N.copy()
        for _ in range(3):
            A = symmetrize(A, N)
            acoustic(A)
        R = lattice_points(N)
        D0 = dq(A, R, [0.0, 0.0, 0.0])
        # the acoustic sum rule: every block row of D(Gamma) sums to zero, so uniform translations are zero modes
        assert np.abs(D0.reshape(m, m // 3, 3).sum(1)).max() <= 1e-12 * np.abs(A).max()


def test_dq_uses_the_upper_triangle():
    rng = np.random.default_rng(3)
    D_N = rng.normal(size=(3, 5, 5))  # not symmetric: only the upper triangle of D(q) counts
    R = lattice_points((3, 1, 1))
    H = dq(D_N, R, [0.2, 0.0, 0.0])
    U = np.triu(H, 1)
    full = U + U.conj().T + np.diag(H.diagonal().real)
    assert np.allclose(np.linalg.eigvalsh(H, UPLO="U"), np.linalg.eigvalsh(full))


def test_dos_is_gaussian_sum_on_the_padded_grid():
    e = np.array([0.01, 0.012, 0.03])
    x, w = dos(e, 50, 1e-3)
    assert x[0] == 0.01 - 3e-3 and x[-1] == 0.03 + 3e-3 and len(x) == 50
    assert np.trapezoid(w, x) == pytest.approx(3.0, rel=2e-2)


def test_phonons_validates_before_touching_a_device():
    import alignn_amd

    assert alignn_amd.phonons is phonons and alignn_amd.PhononResult is PhononResult
    assert set(PhononResult.__dataclass_fields__) >= {"force_constants", "lattice_points", "frequencies", "modes",
                                                      "dos_energies", "dos_weights", "n_evals", "n_supercells"}
    lat, pos, m = [np.eye(3) * 5], [np.zeros((2, 3))], [np.ones(2)]
    ff = lambda lat, pos: None  # noqa: E731
    bad = [
        dict(lattices=lat, positions=pos + pos, masses=m),
        dict(masses=[np.ones(3)]),
        dict(masses=[np.array([1.0, 0.0])]),
        dict(positions=[np.zeros((2, 2))]),
        dict(positions=[np.zeros((MAX_DIM // 3 + 1, 3))], masses=[np.ones(MAX_DIM // 3 + 1)]),
        dict(supercell=(2, 2)),
        dict(supercell=(2, 0, 2)),
        dict(supercell=(2, 2.5, 2)),
        dict(supercell=[(2, 2, 2), (2, 2, 2)]),
        dict(delta=0.0),
        dict(delta=-0.01),
        dict(delta=float("nan")),
        dict(drift="standard"),
        dict(symmetrize=-1),
        dict(qpoints=np.zeros((4, 2))),
        dict(modes=True),
        dict(dos_kpts=(20, 20)),
        dict(dos_npts=1),
        dict(dos_width=0.0),
        dict(max_atoms_per_eval=0),
    ]
    for kw in bad:
        args = dict(lattices=lat, positions=pos, masses=m)
        args.update(kw)
        with pytest.raises(ValueError):
            phonons(None, args.pop("lattices"), args.pop("positions"), None, args.pop("masses"), forces_fn=ff, device="cpu",
                    **args)
    with pytest.raises(ValueError, match=str(MAX_DIM)):
        phonons(None, lat, [np.zeros((33, 3))], None, [np.ones(33)], forces_fn=ff, device="cpu")
    with pytest.raises(TypeError):  # a CPU device: the launches are HIP only
        phonons(None, lat, pos, None, m, forces_fn=ff, device="cpu")
    with pytest.raises(TypeError):
        phonons(object(), lat, pos, [np.zeros((2, 92))], m)


def test_phonons_validates_the_model():
    import torch

    from alignn_amd import ALIGNNAtomWise, ALIGNNAtomWiseConfig

    lat, pos, m, f = [np.eye(3) * 5], [np.zeros((2, 3))], [np.ones(2)], [np.zeros((2, 92))]
    torch.manual_seed(0)
    cfg = dict(name="alignn_atomwise", alignn_layers=1, gcn_layers=1, hidden_features=64, embedding_features=32,
               atom_input_features=92)
    model = ALIGNNAtomWise(ALIGNNAtomWiseConfig(calculate_gradient=True, **cfg))
    with pytest.raises(ValueError, match="training"):
        phonons(model.train(), lat, pos, f, m)
    no_forces = ALIGNNAtomWise(ALIGNNAtomWiseConfig(calculate_gradient=False, **cfg)).eval()
    with pytest.raises(ValueError, match="calculate_gradient"):
        phonons(no_forces, lat, pos, f, m)
    with pytest.raises(ValueError):
        phonons(model.eval(), lat, pos, None, m)
    with pytest.raises(TypeError):  # a model on the CPU
        phonons(model.eval(), lat, pos, f, m)
