"""The executable specification of ``alignn_amd.interface`` (csrc/interface.hip): float64 restatements of the lattice match
(``alignn_zsl_match``), of the interface builder (``alignn_interface_build``) and of the work of adhesion of the reference's
``get_interface_energy`` (alignn/ff/ff.py:984-1116).  The reference leaves the match and the stacking to jarvis-tools'
``make_interface``; jarvis-tools, pymatgen and ASE are not dependencies of this project, so the match is specified here
(INTEGRATION.md has the same text) and not as "whatever jarvis-tools returns".

Everything is written operation for operation as the kernels are - Python floats and elementwise numpy only, every sum in the
kernels' order, no ``@`` / ``dot`` - so the device results are expected to be the same bits.  tests/test_interface_ref.py pins
this file against a brute force over integer matrices and by geometry; tests/test_gpu_interface.py holds the kernels to it."""

import math

import numpy as np

from tests.defects_ref import EV_A2_TO_J_M2, inv3_cof, row_dot, wrap01  # noqa: F401

TOL = 1e-10
MAX_N = 256
ROUNDS = 64


# --- the match ---------------------------------------------------------------------------------------------------------------------
def hnf_list(n):
    """The Hermite normal forms [[a, b], [0, n / a]] of multiple n: (a, b), a ascending, then b ascending."""
    return [(a, b) for a in range(1, n + 1) if n % a == 0 for b in range(n // a)]


def hnf_tables(max_n=MAX_N):
    """-> (hnf int32 [E, 3] = (n, a, b), prefix int32 [max_n + 2]: the first entry of multiple n; prefix[0] = prefix[1] = 0)."""
    rows, prefix = [], [0, 0]
    for n in range(1, max_n + 1):
        rows += [(n, a, b) for a, b in hnf_list(n)]
        prefix.append(len(rows))
    return np.array(rows, dtype=np.int32), np.array(prefix, dtype=np.int32)


def cross2(cell):
    cell = np.asarray(cell, dtype=np.float64)
    return float(cell[0, 0]) * float(cell[1, 1]) - float(cell[0, 1]) * float(cell[1, 0])


def cell_valid(cell):
    cell = np.asarray(cell, dtype=np.float64)
    if not np.isfinite(cell).all():
        return False
    a = cross2(cell)
    return 0.0 < a < np.inf


def largest_multiple(area, max_area):
    """The largest n with n area <= max_area (0 if none)."""
    n = int(max_area / area)
    while (n + 1) * area <= max_area:
        n += 1
    while n > 0 and n * area > max_area:
        n -= 1
    return n


def _swap(u, w, m):
    return [w[0], w[1]], [-u[0], -u[1]], [m[2], m[3], -m[0], -m[1]]


def reduce_basis(cell, n, a, b):
    """The super-lattice u = a v1 + b v2, w = (n / a) v2 after the orientation-preserving Lagrange reduction
    -> (u, w, integer matrix [4] rows u, w)."""
    v = [[float(x) for x in row] for row in np.asarray(cell, dtype=np.float64)]
    d = n // a
    u = [float(a) * v[0][0] + float(b) * v[1][0], float(a) * v[0][1] + float(b) * v[1][1]]
    w = [float(d) * v[1][0], float(d) * v[1][1]]
    m = [a, b, 0, d]
    for _ in range(ROUNDS):
        if u[0] * u[0] + u[1] * u[1] > w[0] * w[0] + w[1] * w[1]:
            u, w, m = _swap(u, w, m)
        k = float(np.rint((u[0] * w[0] + u[1] * w[1]) / (u[0] * u[0] + u[1] * u[1])))
        if k == 0.0:
            break
        w = [w[0] - k * u[0], w[1] - k * u[1]]
        m = [m[0], m[1], m[2] - int(k) * m[0], m[3] - int(k) * m[1]]
    if u[0] * u[0] + u[1] * u[1] > w[0] * w[0] + w[1] * w[1]:
        u, w, m = _swap(u, w, m)
    return u, w, m


def variant(v, u, w):
    """Variant v of the rows (u, w): (u, w), (u, w + u), (u, w - u), (w, -u), (w, -u + w), (w, -u - w); floats or ints."""
    if v < 3:
        return list(u), [w[k] if v == 0 else (w[k] + u[k] if v == 1 else w[k] - u[k]) for k in range(2)]
    return list(w), [-u[k] if v == 3 else (-u[k] + w[k] if v == 4 else -u[k] - w[k]) for k in range(2)]


def basis_entry(u, w):
    """(|u|, |w|, u . w, u x w)."""
    return [math.sqrt(u[0] * u[0] + u[1] * u[1]), math.sqrt(w[0] * w[0] + w[1] * w[1]), u[0] * w[0] + u[1] * w[1],
            u[0] * w[1] - u[1] * w[0]]


def side_table(cell, nmax, variants):
    """Per multiple n = 1 .. nmax: (entries float64 [sigma(n) (x 6), 4], matrices int [sigma(n), 4])."""
    out = [None]
    for n in range(1, nmax + 1):
        ent, mats = [], []
        for a, b in hnf_list(n):
            u, w, m = reduce_basis(cell, n, a, b)
            mats.append(m)
            if variants:
                ent += [basis_entry(*variant(v, u, w)) for v in range(6)]
            else:
                ent.append(basis_entry(u, w))
        out.append((np.array(ent, dtype=np.float64), np.array(mats, dtype=np.int64)))
    return out


def mismatch(f, s, ltol, cos_atol):
    """Film entries f [nf, 4] against substrate entries s [ns, 4] -> (accepted, ru, rw, sin, score), each [nf, ns]."""
    f0, f1, f2, f3 = (f[:, k:k + 1] for k in range(4))
    s0, s1, s2, s3 = (s[None, :, k] for k in range(4))
    with np.errstate(all="ignore"):
        ru = np.abs(s0 / f0 - 1.0)
        rw = np.abs(s1 / f1 - 1.0)
        den = ((f0 * f1) * s0) * s1
        cs = (f2 * s2 + f3 * s3) / den
        sn = (f2 * s3 - f3 * s2) / den
        ok = (ru <= ltol) & (rw <= ltol) & (cs >= cos_atol)
        return ok, ru, rw, sn, np.maximum(np.maximum(ru, rw), np.abs(sn))


def cos_of_degrees(atol):
    return math.cos(math.radians(atol))


def match(film_cell, subs_cell, max_area=500.0, max_area_ratio_tol=1.0, ltol=0.05, atol=1.0):
    """alignn_zsl_match for one pair -> dict(status, i, j, film_matrix [2, 2], subs_matrix [2, 2], ru, rw, sin, score)."""
    if not (cell_valid(film_cell) and cell_valid(subs_cell)):
        return dict(status=2)
    af, as_ = cross2(film_cell), cross2(subs_cell)
    nf_max, ns_max = largest_multiple(af, max_area), largest_multiple(as_, max_area)
    if nf_max > MAX_N or ns_max > MAX_N:
        raise ValueError(f"multiples {nf_max}, {ns_max} > {MAX_N}")
    cos_atol = cos_of_degrees(atol)
    ft, st = side_table(film_cell, nf_max, False), side_table(subs_cell, ns_max, True)
    for i in range(1, nf_max + 1):
        best = None
        for j in range(1, ns_max + 1):
            ratio = (float(i) * af) / (float(j) * as_)
            if not abs(ratio - 1.0) <= max_area_ratio_tol:
                continue
            ok, ru, rw, sn, score = mismatch(ft[i][0], st[j][0], ltol, cos_atol)
            if not ok.any():
                continue
            flat = int(np.argmin(np.where(ok, score, np.inf)))  # the first of equal scores: (film entry, substrate entry, variant)
            fe, r = divmod(flat, score.shape[1])
            if best is None or score[fe, r] < best[0]:  # (equal scores: the smaller j stays)
                best = (score[fe, r], j, fe, r // 6, r % 6, ru[fe, r], rw[fe, r], sn[fe, r])
        if best is not None:
            score, j, fe, se, v, ru, rw, sn = best
            ms = st[j][1][se]
            mu, mw = variant(v, [int(ms[0]), int(ms[1])], [int(ms[2]), int(ms[3])])
            return dict(status=0, i=i, j=j, film_matrix=ft[i][1][fe].reshape(2, 2).copy(), subs_matrix=np.array([mu, mw], dtype=np.int64),
                        ru=float(ru), rw=float(rw), sin=float(sn), score=float(score))
    return dict(status=1)


# --- the builder -------------------------------------------------------------------------------------------------------------------
def plane_cell(C):
    """The 2 x 2 cell of the first two rows of a slab cell in their plane, x along row 0: [[l0, 0], [x1, y1]]."""
    C = [[float(x) for x in row] for row in np.asarray(C, dtype=np.float64)]
    l0 = math.sqrt((C[0][0] * C[0][0] + C[0][1] * C[0][1]) + C[0][2] * C[0][2])
    x1 = ((C[0][0] * C[1][0] + C[0][1] * C[1][1]) + C[0][2] * C[1][2]) / l0
    n0, n1, n2 = (C[0][1] * C[1][2] - C[0][2] * C[1][1], C[0][2] * C[1][0] - C[0][0] * C[1][2], C[0][0] * C[1][1] - C[0][1] * C[1][0])
    return np.array([[l0, 0.0], [x1, math.sqrt((n0 * n0 + n1 * n1) + n2 * n2) / l0]])


def _side(cell, cart, M):
    cell, cart = np.asarray(cell, dtype=np.float64), np.asarray(cart, dtype=np.float64)
    m = [int(v) for v in np.asarray(M).reshape(-1)]
    det = m[0] * m[3] - m[1] * m[2]
    assert det >= 1, det
    a = math.gcd(abs(m[0]), abs(m[2]))
    f = row_dot(cart, inv3_cof(cell))
    la3 = math.sqrt((cell[2, 0] * cell[2, 0] + cell[2, 1] * cell[2, 1]) + cell[2, 2] * cell[2, 2])
    return dict(f=f, h=f[:, 2] * la3, m=[float(v) for v in m], det=float(det), a=a, d=det // a, n=len(cart))


def _place(S, A, z_of_h):
    q = np.arange(S["a"] * S["d"] * S["n"])
    img, b = q // S["n"], q % S["n"]
    m0, m1 = img // S["d"], img % S["d"]
    f0, f1 = S["f"][b, 0] + m0.astype(np.float64), S["f"][b, 1] + m1.astype(np.float64)
    g0 = (f0 * S["m"][3] - f1 * S["m"][2]) / S["det"]
    g1 = (f1 * S["m"][0] - f0 * S["m"][1]) / S["det"]
    g0 = g0 - np.floor(g0 + TOL)
    g1 = g1 - np.floor(g1 + TOL)
    return np.stack([g0 * A[0, 0] + g1 * A[1, 0], g1 * A[1, 1], z_of_h(S["h"][b])], axis=1), b


def interface(film_slab, subs_slab, film_matrix, subs_matrix, separation, vacuum):
    """alignn_interface_build for one pair.  A slab is (cell, cart, src) of ``defects_ref.slab`` with vacuum 0.
    -> (cell, [cart] x 3, [frac] x 3, [src] x 3, [part] x 3, area): the substrate, the film, both."""
    F, S = _side(film_slab[0], film_slab[1], film_matrix), _side(subs_slab[0], subs_slab[1], subs_matrix)
    p = plane_cell(subs_slab[0])
    l0, x1, y1 = float(p[0, 0]), float(p[1, 0]), float(p[1, 1])
    ux, uy = S["m"][0] * l0 + S["m"][1] * x1, S["m"][1] * y1
    wx, wy = S["m"][2] * l0 + S["m"][3] * x1, S["m"][3] * y1
    nu = math.sqrt(ux * ux + uy * uy)
    min_s, max_s, min_f, max_f = float(S["h"].min()), float(S["h"].max()), float(F["h"].min()), float(F["h"].max())
    top_s = max_s - min_s
    lz = (((max_f - min_f) + top_s) + separation) + vacuum
    A = np.array([[nu, 0.0, 0.0], [(ux * wx + uy * wy) / nu, (ux * wy - uy * wx) / nu, 0.0], [0.0, 0.0, lz]])
    Ainv = inv3_cof(A)
    rs, bs = _place(S, A, lambda h: h - min_s)
    rf, bf = _place(F, A, lambda h: ((h - min_f) + top_s) + separation)
    src_s, src_f = np.asarray(subs_slab[2], dtype=np.int32)[bs], np.asarray(film_slab[2], dtype=np.int32)[bf]
    carts = [rs, rf, np.concatenate([rs, rf])]
    srcs = [src_s, src_f, np.concatenate([src_s, src_f])]
    parts = [np.zeros(len(rs), dtype=np.int32), np.ones(len(rf), dtype=np.int32)]
    parts.append(np.concatenate(parts))
    return A, carts, [wrap01(row_dot(r, Ainv)) for r in carts], srcs, parts, abs(A[0, 0] * A[1, 1])


# --- the energy ------------------------------------------------------------------------------------------------------------------
def work_of_adhesion(e_interface, e_subs, e_film, area):
    """ff.py:1107-1112 without its factor 16: -(E_int - E_sub - E_film) / area, eV/A^2."""
    return -(e_interface - e_subs - e_film) / area


# --- geometry helpers of the tests ---------------------------------------------------------------------------------------------
def rot(t):
    """Right-multiplying a cell (rows) by it turns the cell by t."""
    return np.array([[math.cos(t), math.sin(t)], [-math.sin(t), math.cos(t)]])


def hexagonal(a):
    return np.array([[a, 0.0], [-0.5 * a, 0.5 * math.sqrt(3.0) * a]])


def random_cell(rng):
    """Lengths 2.5 - 4.5 A, angle 60 - 120 degrees, any orientation, right-handed."""
    a, b = rng.uniform(2.5, 4.5, 2)
    g = math.radians(rng.uniform(60.0, 120.0))
    return np.array([[a, 0.0], [b * math.cos(g), b * math.sin(g)]]) @ rot(rng.uniform(0, 2 * math.pi))


def random_pairs(n=40, seed=2024):
    rng = np.random.default_rng(seed)
    return [(random_cell(rng), random_cell(rng)) for _ in range(n)]


def triclinic():
    """The triclinic 6-atom crystal of tests/test_gpu_defects.py: (lattice, Cartesian positions)."""
    from alignn_amd.synthetic import make_crystal

    lat, frac, _ = make_crystal(6, 77)
    lat = np.asarray(lat, dtype=np.float64)
    return lat, np.asarray(frac, dtype=np.float64) @ lat


def ref_slab(parent, hkl, layers, beg=0):
    """(cell, cart, src) of the vacuum-free slab of ``defects_ref.slab``."""
    from tests.defects_ref import miller_basis, slab

    cell, cart, _, src = slab(parent[0], parent[1], miller_basis(parent[0], hkl), layers, 0.0, beg=beg)
    return cell, cart, src


BUILDER_CASES = [  # (film parent, hkl, layers, substrate parent, hkl, layers, film matrix, substrate matrix)
    ("fcc", (1, 0, 0), 1, "fcc", (1, 0, 0), 3, [[1, 0], [0, 1]], [[1, 0], [0, 1]]),
    ("fcc", (1, 1, 1), 3, "tri", (1, 0, 0), 1, [[2, 1], [0, 3]], [[1, 1], [-2, 1]]),  # b != 0; a reduced matrix
    ("tri", (1, -1, 0), 1, "fcc", (1, 1, 0), 3, [[0, 2], [-2, -1]], [[0, 1], [-3, 2]]),  # variants that swap the vectors
]
