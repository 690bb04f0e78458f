"""The executable specification of ``phonons(displacements="symmetry")`` (csrc/phonon_sym.hip): rules 1-6 of
include/alignn_phsym.h restated in float64 numpy, on top of tests/phonons_ref.py (the displaced supercells, the drift corrections,
ASE's symmetrize / acoustic passes) and tests/sym_ref.py (the operations, ``cartesian_rotation``).  phonopy is not a dependency
of this project and its direction lists are not reproduced: the rules of the header are the definition, and
tests/test_phonons_sym_ref.py pins them to physics (an exactly linear force field gives the force constants of all 6n
displacements back, and they are covariant under every usable operation).  A support module: no tests in it.

A symmetry is the dict of ``sym_ref.find_symmetry`` (or anything with ``rotations`` [G, 3, 3], ``atom_map`` [G, n] and
``shifts`` [G, n, 3]).  Supercell atom (m, j) has the index ((m0 N1 + m1) N2 + m2) n + j."""

import itertools

import numpy as np

from tests import phonons_ref
from tests.defects_ref import inv3_cof as inv_cof
from tests.sym_ref import cartesian_rotation

TAU = 1e-4  # ALIGNN_PHSYM_TAU: det M >= TAU (trace M / 3)^3 is "the images span space"
_C = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, -1, 0], [1, 0, -1], [0, 1, -1],
               [1, 1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1]], dtype=np.float64)
CANDIDATES = _C / np.sqrt((_C[:, 0] * _C[:, 0] + _C[:, 1] * _C[:, 1]) + _C[:, 2] * _C[:, 2])[:, None]


def usable(W, N):
    """Rule 1: W maps the supercell's lattice onto itself."""
    return all((int(W[r][c]) * int(N[c])) % int(N[r]) == 0 for r in range(3) for c in range(3))


def rotation(A, W):
    """Q_g = A^T W A^-T with the arithmetic of sym_ref.cartesian_rotation; the identity exactly for W = I."""
    if np.array_equal(np.asarray(W), np.eye(3, dtype=np.int64)):
        return np.eye(3)
    return cartesian_rotation(A, W)


def images(sym, g, N, fixed=None):
    """The permutation B -> g~ B of the supercell atoms: (m, j) -> ((W m + shift[g][j] - shift[g][fixed]) mod N, map[g][j]);
    without ``fixed`` no translation follows g."""
    W, amap, sh = (np.asarray(sym[k][g], dtype=np.int64) for k in ("rotations", "atom_map", "shifts"))
    n, Nv = len(amap), np.asarray(N, dtype=np.int64)
    m = np.indices(tuple(int(v) for v in N)).reshape(3, -1).T.astype(np.int64)  # [Ncell, 3]
    back = np.zeros(3, dtype=np.int64) if fixed is None else sh[fixed]
    mm = (m @ W.T)[:, None, :] + sh[None, :, :] - back[None, None, :]  # [Ncell, n, 3]
    mm = np.mod(mm, Nv)
    cell = (mm[..., 0] * Nv[1] + mm[..., 1]) * Nv[2] + mm[..., 2]
    return (cell * n + amap[None, :]).reshape(-1)


def det_cof(M):
    a = [float(v) for v in np.asarray(M).reshape(-1)]
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[3] * a[8] - a[5] * a[6], a[3] * a[7] - a[4] * a[6]
    return (a[0] * c00 - a[1] * c01) + a[2] * c02


def images_of_direction(Q, d):
    """u = Q^T d: u_a = (Q_0a d_0 + Q_1a d_1) + Q_2a d_2."""
    return np.array([(Q[0, a] * d[0] + Q[1, a] * d[1]) + Q[2, a] * d[2] for a in range(3)])


def span_matrix(Qs, dirs):
    """M = sum over g (ascending), then d (ascending) of u u^T -> (M, [u_gm])."""
    M, us = np.zeros((3, 3)), []
    for Q in Qs:
        for d in dirs:
            u = images_of_direction(Q, d)
            us.append(u)
            for a in range(3):
                for b in range(3):
                    M[a, b] = M[a, b] + u[a] * u[b]
    return M, us


def span_ratio(M):
    t = ((M[0, 0] + M[1, 1]) + M[2, 2]) / 3.0
    return det_cof(M) / ((t * t) * t)


def choose_directions(Qs, tau=TAU, ratios=None):
    """Rule 4: the candidate indices chosen for a site group with rotations Qs; ``ratios`` collects (k, subset, ratio) of
    every subset tried."""
    for k in (1, 2):
        for subset in itertools.combinations(range(len(CANDIDATES)), k):
            M, _ = span_matrix(Qs, CANDIDATES[list(subset)])
            t = ((M[0, 0] + M[1, 1]) + M[2, 2]) / 3.0
            if ratios is not None:
                ratios.append((k, subset, span_ratio(M)))
            if det_cof(M) >= tau * ((t * t) * t):
                return list(subset)
    return [0, 1, 2]


def plan(sym, A, N, tau=TAU):
    """Rules 1-4 and the choice of rule 6 for one structure -> dict(usable [G] bool, Q [G, 3, 3], rep [n], reps, site {i: [g]},
    cand {i: [candidate index]}, dirs {i: [k, 3]}, Minv {i: [3, 3]}, dist [n] (the distributing operation, -1 for a
    representative), displaced_atoms [D], directions [D, 3], ratios)."""
    W, amap = np.asarray(sym["rotations"], dtype=np.int64), np.asarray(sym["atom_map"], dtype=np.int64)
    G, n = amap.shape
    use = np.array([usable(W[g], N) for g in range(G)], dtype=bool)
    Q = np.array([rotation(A, W[g]) for g in range(G)]).reshape(G, 3, 3)
    # rule 2: the classes of the atoms under the usable operations (connected through j -> map[g][j]), named by their lowest atom
    rep = np.arange(n)
    changed = True
    while changed:
        changed = False
        for g in np.nonzero(use)[0]:
            for j in range(n):
                lo = min(rep[j], rep[amap[g, j]])
                if rep[j] != lo or rep[amap[g, j]] != lo:
                    rep[j] = rep[amap[g, j]] = lo
                    changed = True
    reps = [i for i in range(n) if rep[i] == i]
    site, cand, dirs, Minv, ratios = {}, {}, {}, {}, []
    for i in reps:
        site[i] = [int(g) for g in np.nonzero(use)[0] if amap[g, i] == i]
        cand[i] = choose_directions(Q[site[i]], tau, ratios)
        dirs[i] = CANDIDATES[cand[i]]
        Minv[i] = inv_cof(span_matrix(Q[site[i]], dirs[i])[0])
    dist = np.full(n, -1, dtype=np.int64)
    for j in range(n):
        if rep[j] != j:
            dist[j] = min(int(g) for g in np.nonzero(use)[0] if amap[g, rep[j]] == j)
    return dict(usable=use, Q=Q, rep=rep, reps=reps, site=site, cand=cand, dirs=dirs, Minv=Minv, dist=dist,
                displaced_atoms=np.array([i for i in reps for _ in cand[i]], dtype=np.int32),
                directions=np.concatenate([dirs[i] for i in reps]), ratios=ratios, N=tuple(int(v) for v in N), n=n)


def displaced_supercells_sym(lat, pos, N, delta, inv_super, pl):
    """The 2 D displaced supercells in the order representative, direction, sign (-, +): [(frac, cart)].  The arithmetic of
    phonons_ref.displaced_supercells with a general direction: cart_a = cart_a + (sg delta) d."""
    lat, pos = np.asarray(lat, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    img = phonons_ref.supercell_images(N)
    cart0 = pos[None, :, :] + img[:, 0, None, None] * lat[0]
    cart0 = cart0 + img[:, 1, None, None] * lat[1]
    cart0 = (cart0 + img[:, 2, None, None] * lat[2]).reshape(-1, 3)
    out = []
    for a, d in zip(pl["displaced_atoms"], pl["directions"]):
        for sg in (-1.0, 1.0):
            cart = cart0.copy()
            cart[a] = cart[a] + (sg * delta) * d
            f = cart[:, 0:1] * inv_super[0] + cart[:, 1:2] * inv_super[1]
            f = f + cart[:, 2:3] * inv_super[2]
            f = f - np.floor(f)
            f = np.where(f < 1.0, f, 0.0)
            out.append((f, cart))
    return out


def difference_rows(forces, pl, delta, drift="frederiksen"):
    """G_m [n_sc, 3] of every direction from the 2 D force arrays, with the drift corrections of
    phonons_ref.raw_force_constants."""
    out = []
    for k, a in enumerate(pl["displaced_atoms"]):
        fm, fp = (np.array(forces[2 * k + s], dtype=np.float64) for s in (0, 1))
        if drift == "frederiksen":
            fm[a] -= fm.sum(0)
            fp[a] -= fp.sum(0)
        elif drift == "mean":
            fm -= fm.sum(0) / len(fm)
            fp -= fp.sum(0) / len(fp)
        out.append((fm - fp) / (2 * delta))
    return out


def raw_force_constants_sym(forces, pl, sym, delta, drift="frederiksen"):
    """Rules 5 and 6 -> C_N [Ncell, 3n, 3n]."""
    n, N = pl["n"], pl["N"]
    ncell = int(np.prod(N))
    G_rows = difference_rows(forces, pl, delta, drift)
    Phi = np.zeros((n, ncell * n, 3, 3))  # Phi[i][B] = Phi(i; B)
    k0 = 0
    for i in pl["reps"]:
        dirs = pl["dirs"][i]
        T = np.zeros((ncell * n, 3, 3))
        for g in pl["site"][i]:
            Q, perm = pl["Q"][g], images(sym, g, N, fixed=i)
            for m, d in enumerate(dirs):
                u = images_of_direction(Q, d)
                Gm = G_rows[k0 + m][perm]  # [n_sc, 3]
                row = np.stack([(Gm[:, 0] * Q[0, b] + Gm[:, 1] * Q[1, b]) + Gm[:, 2] * Q[2, b] for b in range(3)], axis=-1)
                for a in range(3):
                    T[:, a, :] = T[:, a, :] + u[a] * row
        Mi = pl["Minv"][i]
        for a in range(3):
            Phi[i][:, a, :] = (Mi[a, 0] * T[:, 0, :] + Mi[a, 1] * T[:, 1, :]) + Mi[a, 2] * T[:, 2, :]
        k0 += len(dirs)
    for j in range(n):
        if pl["rep"][j] == j:
            continue
        g, i = int(pl["dist"][j]), int(pl["rep"][j])
        Q, perm = pl["Q"][g], images(sym, g, N, fixed=i)
        P = Phi[i]
        PQ = np.stack([(P[:, :, 0] * Q[b, 0] + P[:, :, 1] * Q[b, 1]) + P[:, :, 2] * Q[b, 2] for b in range(3)], axis=-1)  # Phi Q^T
        out = np.stack([(Q[a, 0] * PQ[:, 0, :] + Q[a, 1] * PQ[:, 1, :]) + Q[a, 2] * PQ[:, 2, :] for a in range(3)], axis=1)
        Phi[j][perm] = out
    # C[cell][3i + a][3j + b] = Phi(i; (cell, j))[a][b]
    return Phi.reshape(n, ncell, n, 3, 3).transpose(1, 0, 3, 2, 4).reshape(ncell, 3 * n, 3 * n).copy()


def force_constants_sym(forces, pl, sym, delta, drift="frederiksen", n_sym=3, use_acoustic=True):
    """The force constants of phonons(displacements="symmetry") from the forces of the 2 D displaced supercells."""
    C_N = raw_force_constants_sym(forces, pl, sym, delta, drift)
    for _ in range(n_sym or 0):
        C_N = phonons_ref.symmetrize(C_N, pl["N"])
        if not use_acoustic:
            break
        phonons_ref.acoustic(C_N)
    return C_N


def covariance_error(C_N, sym, pl):
    """max over the usable g and all A = (0, i), B of |Phi(g A, g B) - Q Phi(A, B) Q^T|."""
    n, N = pl["n"], pl["N"]
    ncell = int(np.prod(N))
    Phi = C_N.reshape(ncell, n, 3, n, 3).transpose(1, 0, 3, 2, 4).reshape(n, ncell * n, 3, 3)
    worst = 0.0
    for g in np.nonzero(pl["usable"])[0]:
        Q = pl["Q"][g]
        for i in range(n):
            perm = images(sym, g, N, fixed=i)
            j = int(np.asarray(sym["atom_map"])[g, i])
            want = np.einsum("ac,Bcd,bd->Bab", Q, Phi[i], Q)
            worst = max(worst, float(np.abs(Phi[j][perm] - want).max()))
    return worst


# ---- an exactly linear force field ---------------------------------------------------------------------------------------------
def pair_spring_hessian(sl, cart, species, rc=4.2, reach=2):
    """The Hessian [3 n_sc, 3 n_sc] at rest of springs between every pair of atoms (all periodic images) closer than rc, each at
    its rest length, of stiffness k(d) = k_zz' (1 - d / rc)^2: a function of the distance and the two species alone, so the
    table has every symmetry of the structure, and continuous at rc, so no pair near the cutoff breaks one."""
    sl, cart, z = np.asarray(sl, dtype=np.float64), np.asarray(cart, dtype=np.float64), np.asarray(species)
    ns = len(cart)
    H = np.zeros((ns, 3, ns, 3))
    kz = 1.0 + 0.05 * ((z[:, None] * z[None, :]) % 7)
    idx = np.arange(ns)
    for img in itertools.product(range(-reach, reach + 1), repeat=3):
        d = cart[None, :, :] + (np.asarray(img, dtype=np.float64) @ sl) - cart[:, None, :]  # [i, j, 3]
        r = np.sqrt((d * d).sum(-1))
        on = (r > 1e-9) & (r < rc)
        k = np.where(on, kz * (1.0 - np.where(on, r, 0.0) / rc) ** 2, 0.0)
        e = d / np.where(on, r, 1.0)[..., None]
        blk = k[..., None, None] * e[..., :, None] * e[..., None, :]  # [i, j, 3, 3]
        H -= blk.transpose(0, 2, 1, 3)
        H[idx, :, idx, :] += blk.sum(1)
    return H.reshape(3 * ns, 3 * ns)


def harmonic_forces(Phi0, cart0):
    """forces_of(superlattice, cart) = -Phi0 (cart - cart0): exactly linear, so central differences are exact."""
    Phi0, flat0 = np.asarray(Phi0, dtype=np.float64), np.asarray(cart0, dtype=np.float64).reshape(-1)

    def forces_of(sl, cart):
        return -(Phi0 @ (np.asarray(cart, dtype=np.float64).reshape(-1) - flat0)).reshape(-1, 3)

    return forces_of


def ideal_supercell(lat, pos, N):
    """The undisplaced supercell's Cartesian positions, in the order of the displaced supercells' rows."""
    lat = np.asarray(lat, dtype=np.float64)
    img = phonons_ref.supercell_images(N)
    return (np.asarray(pos, dtype=np.float64)[None] + (img @ lat)[:, None, :]).reshape(-1, 3)
