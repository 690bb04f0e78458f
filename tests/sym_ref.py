"""The symmetry search and the symmetrisers of alignn_amd/symmetry.py (csrc/symmetry.hip) restated in numpy by brute force, with
the definitions of include/alignn_sym.h; and the small crystals the tests search.  A support module: no tests in it.

An operation {W | t} acts on fractional column coordinates as x' = W x + t; the cell's rows are the lattice vectors, so
r = x A for a row x.  ``find_symmetry`` makes every comparison the definitions ask for - rejected candidates and the atoms after
the first miss included - and returns, as ``margin``, the smallest |value - symprec| / symprec over all of them: a decision
taken at a margin of 0.05 or more does not depend on the last bits of the value."""

import itertools

import numpy as np

from tests.defects_ref import inv3_cof, row_dot

MAX_IMAGE_RANGE = 8
SYSTEMS = ("triclinic", "monoclinic", "orthorhombic", "tetragonal", "trigonal", "hexagonal", "cubic")
_ORDER_OF_TRACE = {3: 1, -1: 2, 0: 3, 1: 4, 2: 6}


def _norm(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def det3i(W):
    W = np.asarray(W)
    return int(W[0, 0] * (W[1, 1] * W[2, 2] - W[1, 2] * W[2, 1]) - W[0, 1] * (W[1, 0] * W[2, 2] - W[1, 2] * W[2, 0])
               + W[0, 2] * (W[1, 0] * W[2, 1] - W[1, 1] * W[2, 0]))


def inverse_int(W):
    """W^-1 of a unimodular integer W: the adjugate times det."""
    W = np.asarray(W, dtype=np.int64)
    adj = np.array([[W[1, 1] * W[2, 2] - W[1, 2] * W[2, 1], W[0, 2] * W[2, 1] - W[0, 1] * W[2, 2], W[0, 1] * W[1, 2] - W[0, 2] * W[1, 1]],
                    [W[1, 2] * W[2, 0] - W[1, 0] * W[2, 2], W[0, 0] * W[2, 2] - W[0, 2] * W[2, 0], W[0, 2] * W[1, 0] - W[0, 0] * W[1, 2]],
                    [W[1, 0] * W[2, 1] - W[1, 1] * W[2, 0], W[0, 1] * W[2, 0] - W[0, 0] * W[2, 1], W[0, 0] * W[1, 1] - W[0, 1] * W[1, 0]]])
    return adj * det3i(W)


def image_range(A, symprec):
    """floor((max_i |a_i| + symprec) / h_k) per axis, h_k the cell's heights."""
    A = np.asarray(A, dtype=np.float64)
    a = [float(v) for v in A.reshape(-1)]
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[3] * a[8] - a[5] * a[6], a[3] * a[7] - a[4] * a[6]
    vol = abs((a[0] * c00 - a[1] * c01) + a[2] * c02)
    longest = max(float(_norm(A[i])) for i in range(3))
    out = []
    for k in range(3):
        u, v = A[(k + 1) % 3], A[(k + 2) % 3]
        c = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
        out.append(int(np.floor((longest + symprec) / (vol / float(_norm(c))))))
    return out


def lattice_operations(A, symprec):
    """-> (W [L, 3, 3] int sorted by their entries row-major, margin).  ValueError past the image range."""
    A = np.asarray(A, dtype=np.float64)
    N = image_range(A, symprec)
    if max(N) > MAX_IMAGE_RANGE:
        raise ValueError(f"image range {N} above {MAX_IMAGE_RANGE}")
    n = np.array(list(itertools.product(*[range(-m, m + 1) for m in N])), dtype=np.int64)
    nf = n.astype(np.float64)
    v = (nf[:, 0:1] * A[0] + nf[:, 1:2] * A[1]) + nf[:, 2:3] * A[2]
    vl = _norm(v)
    margin, cand = np.inf, []
    for i in range(3):
        dev = np.abs(vl - float(_norm(A[i])))
        margin = min(margin, float(np.abs(dev - symprec).min()) / symprec)
        cand.append(np.nonzero(dev <= symprec)[0])
    want = [float(_norm(A[i] - A[j])) for i, j in ((0, 1), (0, 2), (1, 2))]
    ops = []
    for c0, c1, c2 in itertools.product(*cand):
        W = np.stack([n[c0], n[c1], n[c2]], axis=1)  # column i: the coefficients of the image of a_i
        if abs(det3i(W)) != 1:
            continue
        img, ok = (v[c0], v[c1], v[c2]), True
        for (i, j), w in zip(((0, 1), (0, 2), (1, 2)), want):
            dev = abs(float(_norm(img[i] - img[j])) - w)
            margin = min(margin, abs(dev - symprec) / symprec)
            ok = ok and dev <= symprec
        if ok:
            ops.append(W)
    ops.sort(key=lambda W: tuple(W.reshape(-1)))
    return np.array(ops, dtype=np.int64).reshape(-1, 3, 3), margin


def fractional(A, pos):
    return row_dot(np.asarray(pos, dtype=np.float64), inv3_cof(A))


def apply_w(W, x):
    """W x for the rows of x: (W_r0 x_0 + W_r1 x_1) + W_r2 x_2."""
    Wf = np.asarray(W, dtype=np.float64)
    return np.stack([(Wf[r, 0] * x[..., 0] + Wf[r, 1] * x[..., 1]) + Wf[r, 2] * x[..., 2] for r in range(3)], axis=-1)


def crystal_system(rotations):
    """From the distinct proper parts det(W) W of the distinct rotations, the rules of the header in their order."""
    proper = {tuple((det3i(W) * np.asarray(W)).reshape(-1)) for W in rotations}
    count = {1: 0, 2: 0, 3: 0, 4: 0, 6: 0}
    for p in proper:
        order = _ORDER_OF_TRACE.get(p[0] + p[4] + p[8])
        if order is not None:
            count[order] += 1
    if count[6] > 0:
        return "hexagonal"
    if count[3] == 8:
        return "cubic"
    if count[3] == 2:
        return "trigonal"
    if count[4] > 0:
        return "tetragonal"
    if count[2] == 3:
        return "orthorhombic"
    if count[2] == 1:
        return "monoclinic"
    return "triclinic"


def find_symmetry(A, pos, species=None, symprec=1e-3):
    """One structure -> dict(rotations [G, 3, 3], translations [G, 3], atom_map [G, n], shifts [G, n, 3], orbits [n], n_ops,
    n_translations, point_group_order, crystal_system, margin)."""
    A, pos = np.asarray(A, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    n = len(pos)
    z = np.zeros(n, dtype=np.int64) if species is None else np.asarray(species).astype(np.int64)
    lat_ops, margin = lattice_operations(A, symprec)
    x = fractional(A, pos)
    kinds, counts = np.unique(z, return_counts=True)
    pivot_kind = kinds[np.argmin(counts)]  # (the first minimum: the lowest species number among equals)
    pivots = np.nonzero(z == pivot_kind)[0]
    p = pivots[0]
    same = z[:, None] == z[None, :]
    rot, tr, amap, shifts = [], [], [], []
    for W in lat_ops:
        y = apply_w(W, x)  # [n, 3]
        d = x[pivots] - y[p]
        t = d - np.floor(d)
        t = np.where(t < 1.0, t, 0.0)  # [n_p, 3]
        delta = (y[None, :, None, :] + t[:, None, None, :]) - x[None, None, :, :]  # [j, i, k, 3]
        f = delta - np.rint(delta)
        dist = _norm(np.stack([(f[..., 0] * A[0, c] + f[..., 1] * A[1, c]) + f[..., 2] * A[2, c] for c in range(3)], axis=-1))
        margin = min(margin, float(np.abs(dist - symprec)[:, same].min()) / symprec)
        hit = (dist <= symprec) & same[None]
        for jj in np.nonzero(hit.any(axis=2).all(axis=1))[0]:
            k = np.argmin(np.where(hit[jj], dist[jj], np.inf), axis=1)  # (the first of equals: the lowest k)
            rot.append(W)
            tr.append(t[jj])
            amap.append(k)
            shifts.append(np.rint(delta[jj, np.arange(n), k]).astype(np.int64))
    G = len(rot)
    rot = np.array(rot, dtype=np.int64).reshape(G, 3, 3)
    amap = np.array(amap, dtype=np.int64).reshape(G, n)
    distinct = {tuple(W.reshape(-1)) for W in rot}
    return dict(rotations=rot, translations=np.array(tr, dtype=np.float64).reshape(G, 3), atom_map=amap,
                shifts=np.array(shifts, dtype=np.int64).reshape(G, n, 3), orbits=amap.min(axis=0) if G else np.arange(n), n_ops=G,
                n_translations=sum(1 for W in rot if np.array_equal(W, np.eye(3, dtype=np.int64))),
                point_group_order=len(distinct), crystal_system=crystal_system([np.array(w).reshape(3, 3) for w in distinct]),
                margin=margin)


# --- the symmetrisers: operation for operation what the kernels do ---------------------------------------------------------------
def cartesian_rotation(A, W):
    """Q = A^T W A^-T: M = A^T W first, then M A^-T, every element (m0 + m1) + m2."""
    A, Wf, Ai = np.asarray(A, dtype=np.float64), np.asarray(W, dtype=np.float64), inv3_cof(A)
    M = np.array([[(A[0, a] * Wf[0, c] + A[1, a] * Wf[1, c]) + A[2, a] * Wf[2, c] for c in range(3)] for a in range(3)])
    return np.array([[(M[a, 0] * Ai[d, 0] + M[a, 1] * Ai[d, 1]) + M[a, 2] * Ai[d, 2] for d in range(3)] for a in range(3)])


def symmetrize_forces(sym, A, forces):
    """-> (F' [n, 3], the sum of the magnitudes of the G terms of every element [n, 3])."""
    F = np.asarray(forces, dtype=np.float64)
    acc, mag = np.zeros_like(F), np.zeros_like(F)
    for W, m in zip(sym["rotations"], sym["atom_map"]):
        Q, Fm = cartesian_rotation(A, W), F[m]
        term = np.stack([(Q[0, d] * Fm[:, 0] + Q[1, d] * Fm[:, 1]) + Q[2, d] * Fm[:, 2] for d in range(3)], axis=-1)
        acc, mag = acc + term, mag + np.abs(term)
    return acc / float(sym["n_ops"]), mag


def symmetrize_stress(sym, A, stress):
    S = np.asarray(stress, dtype=np.float64)
    acc, mag = np.zeros((3, 3)), np.zeros((3, 3))
    for W in sym["rotations"]:
        Q = cartesian_rotation(A, W)
        for a in range(3):
            for c in range(3):
                tmp = [(S[p, 0] * Q[0, c] + S[p, 1] * Q[1, c]) + S[p, 2] * Q[2, c] for p in range(3)]
                term = (Q[0, a] * tmp[0] + Q[1, a] * tmp[1]) + Q[2, a] * tmp[2]
                acc[a, c], mag[a, c] = acc[a, c] + term, mag[a, c] + abs(term)
    return acc / float(sym["n_ops"]), mag


def symmetrize_positions(sym, A, pos):
    """-> (Cartesian r' [n, 3], the sum of the magnitudes of the G fractional terms [n, 3])."""
    A = np.asarray(A, dtype=np.float64)
    x = fractional(A, pos)
    acc, mag = np.zeros_like(x), np.zeros_like(x)
    for W, t, m, s in zip(sym["rotations"], sym["translations"], sym["atom_map"], sym["shifts"]):
        u = (x[m] + s.astype(np.float64)) - t
        term = apply_w(inverse_int(W), u)
        acc, mag = acc + term, mag + np.abs(term)
    return row_dot(acc / float(sym["n_ops"]), A), mag


def distinct_miller_indices(rotations, max_index, merge_opposite=True):
    """The representatives of the orbits of the primitive (h, k, l) under hkl -> hkl W, by brute force."""
    Ws = [np.array(w).reshape(3, 3) for w in {tuple(np.asarray(W).reshape(-1)) for W in rotations}]
    r = range(-max_index, max_index + 1)
    todo = {h for h in itertools.product(r, r, r) if any(h) and np.gcd.reduce(h) == 1}
    reps = []
    while todo:
        orbit, new = set(), {next(iter(todo))}
        while new:
            orbit |= new
            grown = {tuple(int(v) for v in np.array(h) @ W) for h in new for W in Ws}
            if merge_opposite:
                grown |= {tuple(-v for v in h) for h in grown | new}
            new = grown - orbit
        reps.append(max(orbit))
        todo -= orbit
    return sorted(reps, key=lambda h: (h[0] * h[0] + h[1] * h[1] + h[2] * h[2], tuple(-v for v in h)))


# --- crystals (cell [3, 3], Cartesian positions [n, 3], species [n]) -------------------------------------------------------------
FCC = 0.5 * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])


def _crystal(A, frac, species):
    A = np.asarray(A, dtype=np.float64)
    return A, np.asarray(frac, dtype=np.float64) @ A, np.asarray(species, dtype=np.int64)


def hexagonal_cell(a, c):
    return np.array([[a, 0.0, 0.0], [-0.5 * a, 0.5 * np.sqrt(3.0) * a, 0.0], [0.0, 0.0, c]])


def rhombohedral_cell(a, alpha_degrees):
    al = np.radians(alpha_degrees)
    cx = np.cos(al)
    cy = (np.cos(al) - cx * cx) / np.sin(al)
    return a * np.array([[1.0, 0.0, 0.0], [cx, np.sin(al), 0.0], [cx, cy, np.sqrt(1.0 - cx * cx - cy * cy)]])


def crystals(a=3.6):
    """name -> (cell, positions, species, operations, distinct rotations, system): the table of the feature's issue."""
    tri = np.array([[3.1, 0.0, 0.0], [0.4, 3.6, 0.0], [0.3, -0.5, 4.2]])
    rho = rhombohedral_cell(a, 70.0)
    be = np.radians(100.0)
    out = {
        "fcc": _crystal(a * FCC, [[0, 0, 0]], [29]) + (48, 48, "cubic"),
        "diamond": _crystal(a * FCC, [[0, 0, 0], [0.25, 0.25, 0.25]], [6, 6]) + (48, 48, "cubic"),
        "rocksalt": _crystal(a * FCC, [[0, 0, 0], [0.5, 0.5, 0.5]], [11, 17]) + (48, 48, "cubic"),
        "zincblende": _crystal(a * FCC, [[0, 0, 0], [0.25, 0.25, 0.25]], [30, 16]) + (24, 24, "cubic"),
        "simple_cubic": _crystal(a * np.eye(3), [[0, 0, 0]], [84]) + (48, 48, "cubic"),
        "cscl": _crystal(a * np.eye(3), [[0, 0, 0], [0.5, 0.5, 0.5]], [55, 17]) + (48, 48, "cubic"),
        "bcc_cube": _crystal(a * np.eye(3), [[0, 0, 0], [0.5, 0.5, 0.5]], [26, 26]) + (96, 48, "cubic"),
        "hcp": _crystal(hexagonal_cell(3.2, 3.2 * 1.633), [[1 / 3, 2 / 3, 0.25], [2 / 3, 1 / 3, 0.75]], [12, 12]) + (24, 24, "hexagonal"),
        "wurtzite": _crystal(hexagonal_cell(3.8, 6.2), [[1 / 3, 2 / 3, 0.0], [2 / 3, 1 / 3, 0.5], [1 / 3, 2 / 3, 0.375],
                                                         [2 / 3, 1 / 3, 0.875]], [30, 30, 16, 16]) + (12, 12, "hexagonal"),
        "tetragonal": _crystal(np.diag([3.0, 3.0, 4.1]), [[0, 0, 0]], [50]) + (16, 16, "tetragonal"),
        "orthorhombic": _crystal(np.diag([3.0, 3.5, 4.1]), [[0, 0, 0]], [50]) + (8, 8, "orthorhombic"),
        "monoclinic": _crystal([[3.0, 0.0, 0.0], [0.0, 3.5, 0.0], [4.1 * np.cos(be), 0.0, 4.1 * np.sin(be)]], [[0, 0, 0]], [50]) + (4, 4, "monoclinic"),
        "triclinic_two_species": _crystal(tri, [[0, 0, 0], [0.13, 0.27, 0.41]], [3, 8]) + (1, 1, "triclinic"),
        "triclinic_inversion_pair": _crystal(tri, [[0.13, 0.27, 0.41], [-0.13, -0.27, -0.41]], [8, 8]) + (2, 2, "triclinic"),
        "rhombohedral": _crystal(rho, [[0, 0, 0]], [83]) + (12, 12, "trigonal"),
    }
    A, pos, z = supercell(*out["fcc"][:3], (2, 2, 2))
    out["fcc_2x2x2"] = (A, pos, z, 384, 48, "cubic")
    return out


def supercell(A, pos, species, dims):
    shifts = np.array(list(itertools.product(*[range(d) for d in dims])), dtype=np.float64) @ A
    return np.diag(dims).astype(np.float64) @ A, (pos[None] + shifts[:, None]).reshape(-1, 3), np.tile(species, len(shifts))


def rebased(A, U):
    """The same lattice in the basis U A, U unimodular."""
    assert abs(det3i(np.asarray(U))) == 1
    return np.asarray(U, dtype=np.float64) @ A


def diamond_cube(a=3.57):
    frac = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]], dtype=np.float64)
    return _crystal(a * np.eye(3), np.vstack([frac, frac + 0.25]), [6] * 8)


# --- hard structures: every branch of the crystal-system rule, screws and glides, unequal species counts, odd cells -----------------
def _fluorite(a=5.46):
    fcc = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]], dtype=np.float64)
    return _crystal(a * np.eye(3), np.vstack([fcc, fcc + 0.25, fcc + 0.75]), [20] * 4 + [9] * 8)  # Ca first, sorted after F


def hard_crystals(a=3.6):
    """name -> (cell, positions, species, operations, pure translations, distinct rotations, system) at symprec = 1e-3: the
    entries of ``crystals()`` that no device test searches, and structures with a non-symmorphic group (quartz: a threefold
    screw with translations of thirds; rutile), centred monoclinic and orthorhombic cells, a pivot species chosen by count and
    sorted last (rhomb_obtuse, fluorite), a left-handed cell, an obtuse rhombohedral one and atoms far outside [0, 1)."""
    C = crystals(a)
    out = {k: C[k][:3] + (C[k][3], C[k][3] // C[k][4], C[k][4], C[k][5]) for k in
           ("zincblende", "rocksalt", "cscl", "bcc_cube", "tetragonal", "orthorhombic", "monoclinic", "triclinic_two_species",
            "rhombohedral")}
    out["hBN"] = _crystal(hexagonal_cell(2.5, 6.6), [[1 / 3, 2 / 3, 0], [2 / 3, 1 / 3, 0]], [5, 7]) + (12, 1, 12, "hexagonal")
    u, (x, y, z) = 0.4697, (0.4135, 0.2669, 0.1191)
    out["quartz"] = _crystal(hexagonal_cell(4.916, 5.405),
                             [[u, 0, 2 / 3], [0, u, 1 / 3], [-u, -u, 0], [x, y, z], [-y, x - y, z + 2 / 3], [-x + y, -x, z + 1 / 3],
                              [y, x, -z], [x - y, -y, -z + 1 / 3], [-x, -x + y, -z + 2 / 3]], [14] * 3 + [8] * 6) + (6, 1, 6, "trigonal")
    u = 0.305
    out["rutile"] = _crystal(np.diag([4.594, 4.594, 2.959]),
                             [[0, 0, 0], [0.5, 0.5, 0.5], [u, u, 0], [-u, -u, 0], [0.5 + u, 0.5 - u, 0.5], [0.5 - u, 0.5 + u, 0.5]],
                             [22] * 2 + [8] * 4) + (16, 1, 16, "tetragonal")
    out["ortho_C"] = _crystal(np.diag([3.0, 5.0, 4.1]),
                              [[0, 0, 0], [0.5, 0.5, 0], [0, 0.3, 0.5], [0, -0.3, 0.5], [0.5, 0.8, 0.5], [0.5, 0.2, 0.5]],
                              [50] * 2 + [8] * 4) + (16, 2, 8, "orthorhombic")
    be = np.radians(105.0)
    out["mono_C2m"] = _crystal([[5.0, 0.0, 0.0], [0.0, 3.2, 0.0], [4.1 * np.cos(be), 0.0, 4.1 * np.sin(be)]],
                               [[0, 0, 0], [0.5, 0.5, 0], [0.2, 0, 0.3], [-0.2, 0, -0.3], [0.7, 0.5, 0.3], [0.3, 0.5, -0.3]],
                               [50] * 2 + [8] * 4) + (8, 2, 4, "monoclinic")
    out["rhomb_obtuse"] = _crystal(rhombohedral_cell(a, 100.0), [[0, 0, 0], [0.27, 0.27, 0.27], [-0.27, -0.27, -0.27]],
                                   [83, 52, 52]) + (12, 1, 12, "trigonal")
    A, pos, z = C["diamond"][:3]
    out["diamond_left"] = (A[[1, 0, 2]], pos, z, 48, 1, 48, "cubic")  # det < 0
    A, pos, z = C["wurtzite"][:3]
    out["wurtzite_shifted"] = (A, pos + np.array([[3, -2, 1], [0, 0, 0], [-5, 4, -7], [1, 1, -1]], dtype=np.float64) @ A, z,
                               12, 1, 12, "hexagonal")
    out["fluorite_2x2x1"] = supercell(*_fluorite(), (2, 2, 1)) + (256, 16, 16, "tetragonal")
    out["fluorite_2x2x2"] = supercell(*_fluorite(), (2, 2, 2)) + (1536, 32, 48, "cubic")  # pivot_lo = 64, 32 pivots: two chunks
    return out


def rotation_about(axis, angle):
    """Rodrigues' formula."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.sqrt(k @ k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def moved(A, pos, z, U, R, origin, perm, cells):
    """The same crystal described differently: the basis U A (U unimodular), the whole rotated rigidly by R (r -> R r) and
    shifted by ``origin``; atom k of the copy is atom perm[k] of the original, displaced by the lattice vector cells[k] (integers
    in the new basis).  -> (cell, positions, species)."""
    R, perm = np.asarray(R, dtype=np.float64), np.asarray(perm)
    A2 = rebased(A, U) @ R.T
    return A2, (pos @ R.T + np.asarray(origin, dtype=np.float64))[perm] + np.asarray(cells, dtype=np.float64) @ A2, np.asarray(z)[perm]


MOVED_BASES = {  # name of the original -> U; the image ranges of the copies are asserted in tests/test_sym_ref.py
    "quartz": [[1, 1, 0], [0, 1, 0], [0, 1, 1]],
    "rutile": [[1, 2, 0], [0, 1, 1], [0, 0, 1]],
    "mono_C2m": [[1, 0, 0], [1, 1, 0], [0, 0, 1]],
    "fluorite_2x2x1": [[1, 0, 0], [0, 1, 0], [0, 1, 1]],
    "triclinic_inversion_pair": [[1, 0, 1], [0, 1, 0], [0, 0, -1]],
}


def moved_copies(a=3.6):
    """name -> (name of the original, cell, positions, species, U, perm): the crystals of ``MOVED_BASES`` in another basis,
    rotated about (1, 2, 3) by 0.7 rad, with another origin, a seeded atom order and atoms up to three cells away."""
    H, C = hard_crystals(a), crystals(a)
    R, out = rotation_about((1.0, 2.0, 3.0), 0.7), {}
    for seed, (name, U) in enumerate(MOVED_BASES.items()):
        A, pos, z = (H[name] if name in H else C[name])[:3]
        rng = np.random.default_rng(100 + seed)
        perm, cells = rng.permutation(len(pos)), rng.integers(-3, 4, size=(len(pos), 3))
        out[name + "_moved"] = (name,) + moved(A, pos, z, U, R, (0.31, -1.27, 2.6), perm, cells) + (np.array(U), perm)
    return out


def _rotation_keys(W):
    """One integer per rotation, for entries within +-17."""
    return ((np.asarray(W, dtype=np.int64).reshape(-1, 9) + 17) * (35 ** np.arange(8, -1, -1, dtype=np.int64))).sum(axis=1)


def orbits_of_maps(atom_map, n):
    """The classes the maps generate, every atom labelled by the lowest atom of its class."""
    label = np.arange(n)
    while True:
        low = label.copy()
        for m in atom_map:  # i and m[i] share a class: the lower label goes both ways
            there = low.copy()
            np.minimum.at(there, m, low)
            low = np.minimum(there, there[m])
        if np.array_equal(low, label):
            return label
        label = low


def check_space_group(A, pos, z, result, symprec, exact=None, sample=8, seed=0):
    """What a set of space-group operations must satisfy whatever found it; reads only ``result`` (the dict of ``find_symmetry``
    above, or the device's arrays as numpy under the same names) and the structure.  Raises AssertionError naming the operation.

    Every W is an integer matrix with |det| = 1; every map a permutation that keeps the species; the Cartesian length of
    (W x_i + t - x_map(i) - shift_i) A is at most symprec, and at most ``exact`` where that is given (an exact crystal: 1e-9 A
    lies three orders above the rounding of W x, |W x| < 200 cells of < 15 A, 200 x 15 x 2^-53 x a few = 1e-12 A); the identity
    with t = 0 modulo 1 is present; the product (W_g W_h, W_g t_h + t_g) of every pair - of every operation with a seeded sample
    of ``sample``, on either side, where G > 400 - is a member (equal rotation, translation within 2 symprec in Cartesian length
    modulo the lattice) whose map is the composition of the two; every inverse is a member, with the inverse map; the three
    counts are those of the set, n_ops = point_group_order x n_translations; the orbits are the classes the maps generate."""
    A, pos, z = np.asarray(A, dtype=np.float64), np.asarray(pos, dtype=np.float64), np.asarray(z)
    W, t = np.asarray(result["rotations"]), np.asarray(result["translations"], dtype=np.float64)
    amap, shifts, orbits = np.asarray(result["atom_map"]), np.asarray(result["shifts"]), np.asarray(result["orbits"])
    n, G = len(pos), int(result["n_ops"])
    assert G >= 1 and W.shape == (G, 3, 3) and t.shape == (G, 3) and amap.shape == (G, n) and shifts.shape == (G, n, 3), "shapes"
    assert orbits.shape == (n,) and W.dtype.kind == "i" and amap.dtype.kind == "i" and shifts.dtype.kind == "i", "shapes and types"
    W, amap = W.astype(np.int64), amap.astype(np.int64)
    x = fractional(A, pos)
    for g in range(G):
        assert abs(det3i(W[g])) == 1, f"operation {g}: det W = {det3i(W[g])}"
        assert np.array_equal(np.sort(amap[g]), np.arange(n)), f"operation {g}: its map is no permutation"
        assert np.array_equal(z[amap[g]], z), f"operation {g}: its map changes a species"
        miss = _norm(row_dot((apply_w(W[g], x) + t[g]) - (x[amap[g]] + shifts[g]), A)).max()
        assert miss <= symprec, f"operation {g}: an image {miss:.3e} from its atom, symprec {symprec}"
        assert exact is None or miss <= exact, f"operation {g}: an image {miss:.3e} from its atom of an exact crystal"
    keys = _rotation_keys(W)
    Wf = W.astype(np.float64)

    def member(g, Wp, tp, mp, what, which):  # the products [H, ...] of operation g with the operations ``which``
        hit = _rotation_keys(Wp)[:, None] == keys[None, :]  # [H, G]
        d = tp[:, None, :] - t[None, :, :]
        d = d - np.rint(d)
        hit &= _norm(np.stack([(d[..., 0] * A[0, c] + d[..., 1] * A[1, c]) + d[..., 2] * A[2, c] for c in range(3)], axis=-1)) <= 2.0 * symprec
        for h in np.nonzero(~hit.any(axis=1))[0]:
            raise AssertionError(f"operation {g}: {what} {which[h]} is no member")
        for h in np.nonzero((amap[hit.argmax(axis=1)] != mp).any(axis=1))[0]:  # (the first member that fits is not it: any other?)
            if not any(np.array_equal(amap[f], mp[h]) for f in np.nonzero(hit[h])[0]):
                raise AssertionError(f"operation {g}: the map of {what} {which[h]} is not the composition")

    one = np.eye(3, dtype=np.int64)
    member(-1, one[None], np.zeros((1, 3)), np.arange(n)[None], "the identity", [""])
    others = np.arange(G) if G <= 400 else np.sort(np.random.default_rng(seed).choice(G, size=sample, replace=False))
    for g in range(G):
        Wi = inverse_int(W[g])
        inv_map = np.empty(n, dtype=np.int64)
        inv_map[amap[g]] = np.arange(n)
        member(g, Wi[None], -(Wi.astype(np.float64) @ t[g])[None], inv_map[None], "its inverse", [""])
        member(g, W[g] @ W[others], t[others] @ Wf[g].T + t[g], amap[g][amap[others]], "its product with operation", others)
        if G > 400:
            member(g, W[others] @ W[g], np.einsum("hrc,c->hr", Wf[others], t[g]) + t[others], amap[others][:, amap[g]],
                   "its product from the left with operation", others)
    n_tr, pg = int((keys == _rotation_keys(one)[0]).sum()), len(np.unique(keys))
    assert int(result["n_translations"]) == n_tr, f"n_translations {result['n_translations']}, operations with W = 1: {n_tr}"
    assert int(result["point_group_order"]) == pg, f"point_group_order {result['point_group_order']}, distinct W: {pg}"
    assert G == pg * n_tr, f"{G} operations, {pg} rotations x {n_tr} translations"
    assert np.array_equal(orbits, orbits_of_maps(amap, n)), "the orbits are not the classes of the maps"


def same_group(result, result_moved, U, perm):
    """The group of a crystal and of ``moved(...)`` of it.  With A' = U A (a rigid rotation and another origin change no W) a
    point has the fractional row x' = x U^-1, the column x' = U^-T x, so x -> W x + t reads x' -> (U^-T W U^T) x' + U^-T t:
    the distinct rotations of the copy are the conjugates U^-T W U^T.  Atom k of the copy is atom perm[k]: its class, labelled
    by its lowest atom, is that of the original read through perm."""
    for f in ("n_ops", "n_translations", "point_group_order", "crystal_system"):
        assert result[f] == result_moved[f], (f, result[f], result_moved[f])
    through = np.asarray(result["orbits"])[np.asarray(perm)]
    lowest = np.array([np.nonzero(through == v)[0][0] for v in through])
    assert np.array_equal(lowest, np.asarray(result_moved["orbits"])), "the orbit partitions differ"
    Ut = np.asarray(U, dtype=np.int64).T
    Uit = inverse_int(U).T
    want = {tuple((Uit @ np.asarray(W, dtype=np.int64) @ Ut).reshape(-1)) for W in result["rotations"]}
    got = {tuple(np.asarray(W, dtype=np.int64).reshape(-1)) for W in result_moved["rotations"]}
    assert got == want, "the rotations of the copy are not the conjugates of the original's"


NOISE = 1e-5
NOISY = ("rutile", "mono_C2m", "fluorite_2x2x1")  # no polar axis: see noisy_copies


def noisy_copies(a=3.6):
    """name -> (cell, positions, species, exact positions): every atom displaced by a seeded vector of length at most NOISE.
    With n the noise, P its symmetrised part and p the pivot atom, whose own noise enters every translation t = x_j - W x_p,
    ``symmetrize_positions`` returns exact_i + P(n)_i + (n_p - P(n)_p).  The crystals here have no polar axis: along one, where
    every W acts as the identity, the noise of t is not averaged away and each further application shifts the whole crystal again
    (wurtzite: by 2e-6 A), so that the symmetrised positions of a polar crystal are no fixed point."""
    H, out = hard_crystals(a), {}
    for seed, name in enumerate(NOISY):
        A, pos, z = H[name][:3]
        rng = np.random.default_rng(200 + seed)
        v = rng.normal(size=pos.shape)
        out[name + "_noisy"] = (A, pos + v / _norm(v)[:, None] * rng.uniform(0.0, NOISE, size=(len(pos), 1)), z, pos)
    return out


def crystal_at_the_atom_limit():
    """1024 atoms: simple cubic a = 3.0 x (8, 8, 16), atom 0 of another species, which is the one pivot and is sorted last."""
    A, pos, z = supercell(3.0 * np.eye(3), np.zeros((1, 3)), np.array([7]), (8, 8, 16))
    z = z.copy()
    z[0] = 8
    return A, pos, z


# --- a device result (alignn_amd.symmetry.SymmetryResult) against the dict of find_symmetry above --------------------------------
MARGIN = 0.05
# translations modulo 1: the rounding of a three-term integer-weighted sum with |W_ij| <= 17 stays below 60 x 2^-53 = 7e-15; 1e-12
# leaves two orders above that and sits nine orders below the smallest symprec searched
T_ATOL = 1e-12


def same_as_restated(res, b, want, what):
    """Structure b of the device's result equals the restatement's: the integers bit for bit, the translations modulo 1 within
    T_ATOL.  -> the largest deviation of a translation."""
    import torch

    assert want["margin"] >= MARGIN, (what, want["margin"])  # the precondition: no decision near symprec
    assert res.n_ops[b] == want["n_ops"] and res.n_translations[b] == want["n_translations"], what
    assert res.point_group_order[b] == want["point_group_order"] and res.crystal_system[b] == want["crystal_system"], what
    for got, exp in ((res.rotations[b], want["rotations"]), (res.atom_map[b], want["atom_map"]), (res.shifts[b], want["shifts"]),
                     (res.orbits[b], want["orbits"])):
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), exp), what
    dt = res.translations[b].cpu().numpy() - want["translations"]
    dt = np.abs(dt - np.rint(dt))
    t = res.translations[b].cpu().numpy()
    assert ((t >= 0.0) & (t < 1.0)).all() and (dt.max() if dt.size else 0.0) <= T_ATOL, (what, dt.max())
    return float(dt.max()) if dt.size else 0.0


def same_bits(a, i, b, j):
    """Structure i of the device result a and structure j of b agree in every bit of every field."""
    import torch

    return all(torch.equal(getattr(a, f)[i], getattr(b, f)[j]) for f in ("rotations", "translations", "atom_map", "shifts", "orbits")) and \
        all(getattr(a, f)[i] == getattr(b, f)[j] for f in ("n_ops", "n_translations", "point_group_order", "crystal_system"))
