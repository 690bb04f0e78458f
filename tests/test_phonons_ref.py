"""The executable specification of ``alignn_amd.phonons`` (csrc/phonon.hip): a float64 numpy restatement of ASE 3.22.1's
``Phonons`` (ase/phonons.py: the displaced supercells of ``run``, ``read`` with its ``symmetrize`` / ``acoustic`` passes,
``lattice_vectors``, ``band_structure``, ``get_dos`` + ``RawDOSData.sample_grid``) as the reference's ``ase_phonon`` drives it
(alignn/ff/ff.py:1337), and of the mean-drift correction of its phonopy path (ff.py:1175-1177).  ASE is not a dependency of
this project; the restatement follows the published ase/phonons.py, and the checks below pin it to physics: the analytic
dispersion of spring crystals.  Where a detail of ASE was not checked against its source, the project's statement rules:

- the DOS gives every one of the K * 3n mesh frequencies weight 1 (``RawDOSData(omega, ones)``);
- ``band_structure(modes=True)`` is not restated: ``PhononResult.modes`` holds the unit eigenvectors of D(q) as columns.

The GPU tests (test_gpu_phonons.py) hold the kernels and ``phonons`` to this file."""

import itertools

import numpy as np
import pytest

from alignn_amd.phonons import (EV_TO_CM1, EV_TO_THZ, FREQ_SCALE, MAX_DIM, PhononResult, lattice_points, monkhorst_pack,
                                phonons)

# ---- the restatement -----------------------------------------------------------------------------------------------------


def supercell_images(N):
    """(m0, m1, m2) of image (m0 N1 + m1) N2 + m2 -> [Ncell, 3] float64 (ASE's atoms * N order)."""
    return np.indices(N).reshape(3, -1).T.astype(np.float64)


def displaced_supercells(lat, pos, N, delta, inv_super):
    """The 6n displaced supercells of one structure in the order atom a, axis i, sign (-, +): [(frac, cart)], each [n Ncell,
    3].  cart = ((r_b + m0 L0) + m1 L1) + m2 L2 (+ the displacement of atom a of image 0), unwrapped; frac = (x S0 + y S1) +
    z S2 with S = inv_super, wrapped into [0, 1).  Operation for operation what the kernel computes."""
    lat, pos = np.asarray(lat, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    n = len(pos)
    img = supercell_images(N)
    cart0 = pos[None, :, :] + img[:, 0, None, None] * lat[0]
    cart0 = cart0 + img[:, 1, None, None] * lat[1]
    cart0 = (cart0 + img[:, 2, None, None] * lat[2]).reshape(-1, 3)
    out = []
    for a in range(n):
        for i in range(3):
            for sg in (-1.0, 1.0):
                cart = cart0.copy()
                cart[a, i] = cart[a, i] + sg * delta
                f = cart[:, 0:1] * inv_super[0] + cart[:, 1:2] * inv_super[1]
                f = f + cart[:, 2:3] * inv_super[2]
                f = f - np.floor(f)
                f = np.where(f < 1.0, f, 0.0)
                out.append((f, cart))
    return out


def raw_force_constants(forces, n, N, delta, drift="frederiksen"):
    """ASE's Phonons.read up to the reshape: forces = the 6n force arrays [n Ncell, 3] in displacement order ->
    C_N [Ncell, 3n, 3n].  drift: "frederiksen" (the force sum off the displaced atom's row), "mean" (sum / atoms off every
    row) or None."""
    ncell = int(np.prod(N))
    C_xNav = np.empty((3 * n, ncell, n, 3))
    for a in range(n):
        for i in range(3):
            fm, fp = (np.array(forces[6 * a + 2 * i + k], dtype=np.float64) for k in (0, 1))
            if drift == "frederiksen":
                fm[a] -= fm.sum(0)
                fp[a] -= fp.sum(0)
            elif drift == "mean":
                fm -= fm.sum(0) / len(fm)
                fp -= fp.sum(0) / len(fp)
            C_xNav[3 * a + i] = ((fm - fp) / (2 * delta)).reshape(ncell, n, 3)
    return C_xNav.swapaxes(0, 1).reshape((ncell, 3 * n, 3 * n))


def symmetrize(C_N, N):
    """One pass of ASE's Phonons.symmetrize (offset 0)."""
    m = C_N.shape[1]
    C = np.fft.fftshift(C_N.reshape(tuple(N) + (m, m)), axes=(0, 1, 2)).copy()
    i, j, k = 1 - np.asarray(N) % 2
    C[i:, j:, k:] *= 0.5
    C[i:, j:, k:] += C[i:, j:, k:][::-1, ::-1, ::-1].transpose(0, 1, 2, 4, 3).copy()
    return np.fft.ifftshift(C, axes=(0, 1, 2)).copy().reshape(C_N.shape)


def acoustic(C_N):
    """ASE's Phonons.acoustic (offset 0), in place: the block row sums of every cell off the diagonal blocks of cell 0."""
    n = C_N.shape[1] // 3
    tmp = C_N.copy()
    for C in tmp:
        for a in range(n):
            for a_ in range(n):
                C_N[0, 3 * a:3 * a + 3, 3 * a:3 * a + 3] -= C[3 * a:3 * a + 3, 3 * a_:3 * a_ + 3]


def force_constants(forces, n, N, delta, drift="frederiksen", n_sym=3, use_acoustic=True):
    C_N = raw_force_constants(forces, n, N, delta, drift)
    for _ in range(n_sym or 0):
        C_N = symmetrize(C_N, N)
        if not use_acoustic:
            break
        acoustic(C_N)
    return C_N


def dynamical_matrices(C_N, masses):
    m_inv_x = np.repeat(np.asarray(masses, dtype=np.float64) ** -0.5, 3)
    return C_N * np.outer(m_inv_x, m_inv_x)[None]


def dq(D_N, R, q):
    """sum_R D_R exp(-2 pi i q.R) (as ASE's band_structure: np.dot(q, R_cN))."""
    phase = np.exp(-2.0j * np.pi * np.dot(np.asarray(q, dtype=np.float64), R.T))
    return np.sum(phase[:, None, None] * D_N, axis=0)


def omega(l):
    """Eigenvalues (eV/A^2/amu) -> frequencies (eV), imaginary as negative."""
    return np.sign(l) * FREQ_SCALE * np.sqrt(np.abs(l))


def frequencies(D_N, R, qs):
    return np.array([omega(np.sort(np.linalg.eigvalsh(dq(D_N, R, q), UPLO="U"))) for q in np.asarray(qs).reshape(-1, 3)])


def dos(freqs, npts, width):
    """RawDOSData(freqs, ones).sample_grid(npts, width=width): (energies, weights)."""
    e = np.asarray(freqs, dtype=np.float64).reshape(-1)
    x = np.linspace(e.min() - 3 * width, e.max() + 3 * width, npts)
    w = np.zeros(npts)
    for e0 in e:
        w += np.exp(-0.5 * ((x - e0) / width) ** 2) / (np.sqrt(2 * np.pi) * width)
    return x, w


def inv_supercell(lat, N):
    return np.linalg.inv(np.asarray(lat, dtype=np.float64) * np.asarray(N, dtype=np.float64)[:, None])


def phonons_ref(lat, pos, masses, N, delta, forces_of, drift="frederiksen", n_sym=3, use_acoustic=True, qs=None):
    """The whole pipeline for one structure; forces_of(superlattice, cart) -> forces [n Ncell, 3]."""
    n = len(pos)
    sl = np.asarray(lat, dtype=np.float64) * np.asarray(N, dtype=np.float64)[:, None]
    cells = displaced_supercells(lat, pos, N, delta, inv_supercell(lat, N))
    C_N = force_constants([forces_of(sl, cart) for _, cart in cells], n, N, delta, drift, n_sym, use_acoustic)
    R = lattice_points(N)
    D_N = dynamical_matrices(C_N, masses)
    return C_N, D_N, R, (None if qs is None else frequencies(D_N, R, qs))


# ---- springs ---------------------------------------------------------------------------------------------------------------
def spring_table(sl, cart, shells, tol=1e-6):
    """Every (i, j, image shift) of the supercell (lattice sl, positions cart) whose distance is one of the shells' rest
    lengths d0 -> (I, J, shift [., 3] Cartesian, d0, k); both directions listed."""
    rows = []
    for i, j in itertools.product(range(len(cart)), repeat=2):
        for img in itertools.product((-1, 0, 1), repeat=3):
            sh = np.asarray(img, dtype=np.float64) @ sl
            d = np.linalg.norm(cart[j] + sh - cart[i])
            for d0, k in shells:
                if abs(d - d0) < tol:
                    rows.append((i, j, sh, d0, k))
    I, J = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    return I, J, np.array([r[2] for r in rows]), np.array([r[3] for r in rows]), np.array([r[4] for r in rows])


def spring_forces(table, cart):
    I, J, sh, d0, k = table
    d = cart[J] + sh - cart[I]
    r = np.sqrt((d * d).sum(1))
    fv = (k * (r - d0) / r)[:, None] * d
    F = np.zeros_like(cart)
    np.add.at(F, I, fv)
    return F


def simple_cubic(a=2.7, k1=1.3, k2=0.45):
    """Monatomic simple cubic, nearest (k1) and next-nearest (k2) central springs at rest length."""
    return np.eye(3) * a, np.zeros((1, 3)), [(a, k1), (a * np.sqrt(2.0), k2)]


def sc_analytic(q, a, k1, k2, m):
    """D(q) = (1/m) sum_{R != 0} k_R (1 - cos 2 pi q.R) e_R e_R^T over the 6 + 12 neighbours -> frequencies (eV)."""
    D = np.zeros((3, 3))
    for R in itertools.product((-1, 0, 1), repeat=3):
        R = np.array(R, dtype=np.float64)
        nr = int(np.abs(R).sum())
        if nr not in (1, 2):
            continue
        k = k1 if nr == 1 else k2
        e = R / np.linalg.norm(R)
        D += k * (1.0 - np.cos(2 * np.pi * q @ R)) * np.outer(e, e)
    return omega(np.linalg.eigvalsh(D / m))


def spring_forces_of(shells):
    cache = {}

    def forces_of(sl, cart):
        key = (sl.tobytes(), len(cart))
        if key not in cache:  # (the ideal supercell's table: the displacements are far below the shell spacing)
            cache[key] = spring_table(sl, cart, shells, tol=1e-2)
        return spring_forces(cache[key], cart)

    return forces_of


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
