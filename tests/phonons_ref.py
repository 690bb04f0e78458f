"""The executable specification of ``alignn_amd.phonons`` (csrc/phonon.hip): a float64 numpy restatement of ASE 3.22.1's
``Phonons`` (ase/phonons.py: the displaced supercells of ``run``, ``read`` with its ``symmetrize`` / ``acoustic`` passes,
``lattice_vectors``, ``band_structure``, ``get_dos`` + ``RawDOSData.sample_grid``) as the reference's ``ase_phonon`` drives it
(alignn/ff/ff.py:1337), and of the mean-drift correction of its phonopy path (ff.py:1175-1177).  ASE is not a dependency of
this project; the restatement follows the published ase/phonons.py, and tests/test_phonons_ref.py pins it to physics: the analytic
dispersion of spring crystals.  Where a detail of ASE was not checked against its source, the project's statement rules:

- the DOS gives every one of the K * 3n mesh frequencies weight 1 (``RawDOSData(omega, ones)``);
- ``band_structure(modes=True)`` is not restated: ``PhononResult.modes`` holds the unit eigenvectors of D(q) as columns.

The GPU tests (test_gpu_phonons.py) hold the kernels and ``phonons`` to this file."""

import itertools

import numpy as np

from alignn_amd.phonons import FREQ_SCALE, lattice_points


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
