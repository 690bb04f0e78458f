"""The executable specification of ``alignn_amd.defects`` (csrc/defects.hip): float64 numpy restatements of ``miller_basis``
(ASE's ``surface()`` of ase/build/general_surface.py), of the two device builders and of the two energy formulas of the
reference's ``vacancy_formation`` / ``surface_energy`` (alignn/ff/ff.py:808-981).  ASE and jarvis-tools are not dependencies of
this project.

The builders are written operation for operation as the kernels are - every three-term sum as ``(x + y) + z``, elementwise
numpy only (no ``@`` / ``dot``: a BLAS may fuse or reorder) - so the device results are expected to be the same bits.
tests/test_defects_ref.py pins this file by geometry and by bond counting; tests/test_gpu_defects.py holds the kernels to it."""

import math

import numpy as np

TOL = 1e-10  # general_surface's tolerance of the wrap
EV_A2_TO_J_M2 = 16.02176634


# --- miller_basis ----------------------------------------------------------------------------------------------------------------
def ext_gcd(a, b):
    if b == 0:
        return 1, 0
    if a % b == 0:
        return 0, 1
    x, y = ext_gcd(b, a % b)
    return y, x - y * (a // b)


def det3i(m):
    m = [[int(v) for v in row] for row in m]
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def ase_basis(lattice, hkl):
    """ASE's surface(): the basis before the flip (det +1 or -1); hkl reduced by its gcd first."""
    h, k, l = (int(v) for v in hkl)
    g = math.gcd(math.gcd(h, k), l)
    if g == 0:
        raise ValueError("hkl = 0")
    h, k, l = h // g, k // g, l // g
    h0, k0, l0 = h == 0, k == 0, l == 0
    if h0 and k0 or h0 and l0 or k0 and l0:
        if not h0:
            c1, c2, c3 = (0, 1, 0), (0, 0, 1), (1, 0, 0)
        if not k0:
            c1, c2, c3 = (0, 0, 1), (1, 0, 0), (0, 1, 0)
        if not l0:
            c1, c2, c3 = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    else:
        p, q = ext_gcd(k, l)
        a1, a2, a3 = np.asarray(lattice, dtype=np.float64)
        k1 = np.dot(p * (k * a1 - h * a2) + q * (l * a1 - h * a3), l * a2 - k * a3)
        k2 = np.dot(l * (k * a1 - h * a2) - k * (l * a1 - h * a3), l * a2 - k * a3)
        if abs(k2) > TOL:
            i = -int(round(k1 / k2))
            p, q = p + i * l, q - i * k
        a, b = ext_gcd(p * k + q * l, h)
        c1 = (p * k + q * l, -p * h, -q * h)
        c2 = tuple(int(v) for v in np.array((0, l, -k)) // abs(math.gcd(l, k)))
        c3 = (b, a * p, a * q)
    return np.array([c1, c2, c3], dtype=np.int64)


def miller_basis(lattice, hkl):
    b = ase_basis(lattice, hkl)
    if det3i(b) == -1:
        b[1] = -b[1]
    return b


# --- the builders ------------------------------------------------------------------------------------------------------------------
def inv3_cof(a):
    """Inverse of a [3, 3] by cofactors, every element its cofactor / det (csrc/cell3.h inv3_cof)."""
    a = [float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[3] * a[8] - a[5] * a[6], a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c00 - a[1] * c01) + a[2] * c02
    return np.array([c00 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                     -c01 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                     c02 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det]).reshape(3, 3)


def row_dot(x, m):
    """x [rows, 3] times m [3, 3]: (x0 m0k + x1 m1k) + x2 m2k."""
    return (x[:, 0:1] * m[0] + x[:, 1:2] * m[1]) + x[:, 2:3] * m[2]


def wrap01(f):
    f = f - np.floor(f)
    return np.where(f < 1.0, f, 0.0)


def supercell(lat, pos, dims, removed=-1, beg=0):
    """alignn_defect_supercells for one job: -> (cell, cart, frac, src); ``beg`` the parent's first row in the packed atoms."""
    lat, pos = np.asarray(lat, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    n = len(pos)
    n0, n1, n2 = (int(v) for v in dims)
    cell = np.array([float(n0), float(n1), float(n2)])[:, None] * lat
    j = np.arange(n * n0 * n1 * n2)
    img, b = j // n, j % n
    m2, m1, m0 = (img % n2).astype(np.float64), ((img // n2) % n1).astype(np.float64), (img // (n1 * n2)).astype(np.float64)
    r = pos[b] + m0[:, None] * lat[0]
    r = r + m1[:, None] * lat[1]
    r = r + m2[:, None] * lat[2]
    frac = wrap01(row_dot(r, inv3_cof(cell)))
    src = (beg + b).astype(np.int32)
    keep = j != removed
    return cell, r[keep], frac[keep], src[keep]


def slab(lat, pos, basis, layers, vacuum, beg=0):
    """alignn_slab_build for one job: -> (cell, cart, frac, src)."""
    lat, pos = np.asarray(lat, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    n = len(pos)
    Bm = [[int(v) for v in row] for row in basis]
    adj = [[Bm[1][1] * Bm[2][2] - Bm[1][2] * Bm[2][1], Bm[0][2] * Bm[2][1] - Bm[0][1] * Bm[2][2], Bm[0][1] * Bm[1][2] - Bm[0][2] * Bm[1][1]],
           [Bm[1][2] * Bm[2][0] - Bm[1][0] * Bm[2][2], Bm[0][0] * Bm[2][2] - Bm[0][2] * Bm[2][0], Bm[0][2] * Bm[1][0] - Bm[0][0] * Bm[1][2]],
           [Bm[1][0] * Bm[2][1] - Bm[1][1] * Bm[2][0], Bm[0][1] * Bm[2][0] - Bm[0][0] * Bm[2][1], Bm[0][0] * Bm[1][1] - Bm[0][1] * Bm[1][0]]]
    det = Bm[0][0] * adj[0][0] + Bm[0][1] * adj[1][0] + Bm[0][2] * adj[2][0]
    assert det in (1, -1), det
    Binv = np.array([[float(v * det) for v in row] for row in adj])
    Bf = np.array(Bm, dtype=np.float64)
    C = row_dot(Bf, lat)  # 1.
    f = row_dot(pos, inv3_cof(lat))  # 2.
    o = row_dot(f, Binv)
    o = o - np.floor(o + TOL)  # 3.
    nu = np.array([C[0, 1] * C[1, 2] - C[0, 2] * C[1, 1], C[0, 2] * C[1, 0] - C[0, 0] * C[1, 2], C[0, 0] * C[1, 1] - C[0, 1] * C[1, 0]])
    t = float(layers) * C[2]
    q = ((t[0] * nu[0] + t[1] * nu[1]) + t[2] * nu[2]) / ((nu[0] * nu[0] + nu[1] * nu[1]) + nu[2] * nu[2])
    S = np.array([C[0], C[1], nu * q])  # 5., 6.
    length = np.sqrt((S[2, 0] * S[2, 0] + S[2, 1] * S[2, 1]) + S[2, 2] * S[2, 2])
    final = np.array([S[0], S[1], S[2] + vacuum * (S[2] / length)])  # 8.
    j = np.arange(n * layers)
    m, b = j // n, j % n
    o2 = o[b, 2] + m.astype(np.float64)
    r = (o[b, 0:1] * C[0] + o[b, 1:2] * C[1]) + o2[:, None] * C[2]  # 4.
    f = row_dot(r, inv3_cof(S))
    f = f - np.floor(f + TOL)
    r = row_dot(f, S)  # 7.
    return final, r, wrap01(row_dot(r, inv3_cof(final))), (beg + b).astype(np.int32)  # 9., 10.


def layers_for(lat, basis, thickness):
    """max(1, int(thickness / h3)), h3 the height of the oriented cell over its in-plane face."""
    C = np.asarray(basis, dtype=np.float64) @ np.asarray(lat, dtype=np.float64)
    nu = np.cross(C[0], C[1])
    return max(1, int(thickness / (abs(np.dot(C[2], nu)) / np.sqrt(np.dot(nu, nu)))))


# --- the energies --------------------------------------------------------------------------------------------------------------
def formation_energy(e_defect, n_defect, e_bulk, n_bulk, mu=0.0):
    """ff.py:885: pred_def_energy - (defective_atoms.num_atoms + 1) * (energy / bulk_atoms.num_atoms) + chem_pot."""
    return e_defect - (n_defect + 1) * e_bulk / n_bulk + mu


def surface_energy(e_slab, n_slab, epa, cell):
    """ff.py:969-971 without its factor 16: (energy - epa * num_atoms) / (2 |a x b|), eV/A^2."""
    cell = np.asarray(cell, dtype=np.float64)
    nu = np.cross(cell[0], cell[1])
    return (e_slab - epa * n_slab) / (2 * np.sqrt((nu * nu).sum()))


# --- geometry helpers of the tests ---------------------------------------------------------------------------------------------
def fcc(a=4.0):
    """The conventional fcc cell: (lattice, Cartesian positions)."""
    frac = np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]])
    return a * np.eye(3), frac * a


def rock_salt(a=4.0):
    """The 8-atom cubic cell of two species (labels 0 / 1): a simple cubic lattice of spacing a / 2."""
    lat, p = fcc(a)
    return lat, np.vstack([p, p + np.array([a / 2, 0.0, 0.0])]), np.array([0, 0, 0, 0, 1, 1, 1, 1])


def shortest_pair(cell, pos, periodic=(1, 1, 1)):
    """The shortest distance between two atoms (or an atom and an image of itself) over the images -1 .. 1 of the periodic
    axes."""
    cell, pos = np.asarray(cell, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    best = np.inf
    rng = [range(-1, 2) if p else range(1) for p in periodic]
    for i0 in rng[0]:
        for i1 in rng[1]:
            for i2 in rng[2]:
                d = pos[None, :, :] + (i0 * cell[0] + i1 * cell[1] + i2 * cell[2]) - pos[:, None, :]
                r = np.sqrt((d * d).sum(-1))
                if (i0, i1, i2) == (0, 0, 0):
                    r = r + np.where(np.eye(len(pos)) > 0, np.inf, 0.0)
                best = min(best, r.min())
    return best
