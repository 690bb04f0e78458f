"""tests/interface_ref.py, the executable specification of the interface task, pinned on the CPU: (a) the restated lattice match
against a brute force over integer matrices that shares none of its enumeration (no Hermite normal forms, no reduction, no
variants); (b) the restated builder by geometry; (c) the work of adhesion and its unit factor."""

import math

import numpy as np
import pytest

from tests import defects_ref as dref
from tests import interface_ref as ref

# Entries of the brute force's matrices run over [-R, R].  R = 6 is too small: the brute force (not the matcher) then misses
# the skinny substrate bases of multiples >= 7, whose shortest vectors need coefficients beyond 6 in the given basis.  With 12
# every basis of the multiples met below (<= 20) that can pass the acceptance rule is inside the box.
R = 12
_M = np.array(np.meshgrid(*[np.arange(-R, R + 1)] * 4, indexing="ij")).reshape(4, -1).T
_DET = _M[:, 0] * _M[:, 3] - _M[:, 1] * _M[:, 2]
_M, _DET = _M[_DET > 0], _DET[_DET > 0]
_BY_DET = {}


def _with_det(n):
    if n not in _BY_DET:
        _BY_DET[n] = _M[_DET == n].astype(np.float64)
    return _BY_DET[n]


def _bases(cell, n):
    m = _with_det(n)
    return m[:, 0:1] * cell[0] + m[:, 1:2] * cell[1], m[:, 2:3] * cell[0] + m[:, 3:4] * cell[1]


def brute_force(film, subs, max_area, ratio_tol, ltol, atol):
    """(i, j, score) of the best match, or None: every integer film basis that is reduced (within 1e-9) against every integer
    substrate basis; the smallest i, then the smallest score, then the smallest j."""
    film, subs = np.asarray(film, dtype=np.float64), np.asarray(subs, dtype=np.float64)
    af, as_ = abs(np.linalg.det(film)), abs(np.linalg.det(subs))
    cos_atol = math.cos(math.radians(atol))
    for i in range(1, int(max_area / af) + 1):
        uf, wf = _bases(film, i)
        uu, ww, d = (uf * uf).sum(1), (wf * wf).sum(1), (uf * wf).sum(1)
        keep = (uu <= ww * (1 + 1e-9)) & (np.abs(d) <= 0.5 * uu * (1 + 1e-9))
        uf, wf = uf[keep], wf[keep]
        best = None
        for j in range(1, int(max_area / as_) + 1):
            if abs(i * af / (j * as_) - 1.0) > ratio_tol:
                continue
            us, ws = _bases(subs, j)
            nuf, nwf = np.linalg.norm(uf, axis=1)[:, None], np.linalg.norm(wf, axis=1)[:, None]
            nus, nws = np.linalg.norm(us, axis=1)[None, :], np.linalg.norm(ws, axis=1)[None, :]
            ru, rw = np.abs(nus / nuf - 1.0), np.abs(nws / nwf - 1.0)
            df, cf = (uf * wf).sum(1)[:, None], (uf[:, 0] * wf[:, 1] - uf[:, 1] * wf[:, 0])[:, None]
            ds, cs = (us * ws).sum(1)[None, :], (us[:, 0] * ws[:, 1] - us[:, 1] * ws[:, 0])[None, :]
            den = nuf * nwf * nus * nws
            ok = (ru <= ltol) & (rw <= ltol) & ((df * ds + cf * cs) / den >= cos_atol)
            if ok.any():
                score = np.where(ok, np.maximum(np.maximum(ru, rw), np.abs((df * cs - cf * ds) / den)), np.inf).min()
                if best is None or score < best[1] - 1e-13:
                    best = (j, score)
        if best is not None:
            return i, best[0], best[1]
    return None


_rot, _hex = ref.rot, ref.hexagonal


def _agree(film, subs, **kw):
    got = ref.match(film, subs, **kw)
    want = brute_force(film, subs, kw.get("max_area", 500.0), kw.get("max_area_ratio_tol", 1.0), kw.get("ltol", 0.05),
                       kw.get("atol", 1.0))
    if want is None:
        assert got["status"] == 1, (got, want)
        return None
    assert got["status"] == 0 and (got["i"], got["j"]) == want[:2], (got, want)
    assert abs(got["score"] - want[2]) <= 1e-12, (got, want)
    # the integer matrices give the reported mismatches back
    uf, wf = got["film_matrix"].astype(np.float64) @ np.asarray(film)
    us, ws = got["subs_matrix"].astype(np.float64) @ np.asarray(subs)
    assert round(np.linalg.det(got["film_matrix"])) == got["i"] and round(np.linalg.det(got["subs_matrix"])) == got["j"]
    assert abs(np.linalg.norm(us) / np.linalg.norm(uf) - 1.0) == pytest.approx(got["ru"], abs=1e-12)
    assert abs(np.linalg.norm(ws) / np.linalg.norm(wf) - 1.0) == pytest.approx(got["rw"], abs=1e-12)
    return got


# --- (a) the match -----------------------------------------------------------------------------------------------------------------
def test_hermite_normal_forms_and_tables():
    assert ref.hnf_list(6) == [(1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (6, 0)]
    hnf, prefix = ref.hnf_tables()
    assert len(hnf) == prefix[-1] == 54077 and prefix[1] == 0 and prefix[2] == 1 and len(prefix) == 258
    assert max(np.diff(prefix)) == 744 and prefix[61] - prefix[60] == 168 and prefix[121] - prefix[120] == 360
    assert (hnf[prefix[6]:prefix[7], 0] == 6).all() and [tuple(r[1:]) for r in hnf[prefix[6]:prefix[7]]] == ref.hnf_list(6)


def test_reduction_keeps_lattice_and_orientation():
    rng = np.random.default_rng(5)
    for _ in range(50):
        cell = rng.normal(size=(2, 2)) * 3
        if ref.cross2(cell) < 0:
            cell = cell[::-1].copy()
        n = int(rng.integers(1, 40))
        a, b = ref.hnf_list(n)[int(rng.integers(0, len(ref.hnf_list(n))))]
        u, w, m = ref.reduce_basis(cell, n, a, b)
        assert m[0] * m[3] - m[1] * m[2] == n
        assert np.allclose(np.array(m, dtype=np.float64).reshape(2, 2) @ cell, [u, w], rtol=0, atol=1e-9)
        uu, ww, d = u[0] ** 2 + u[1] ** 2, w[0] ** 2 + w[1] ** 2, u[0] * w[0] + u[1] * w[1]
        assert uu <= ww and abs(d) <= 0.5 * uu * (1 + 1e-12)


def test_identical_oblique_cells_rotated():
    cell = np.array([[3.1, 0.0], [1.2, 2.7]])
    got = _agree(cell, cell @ _rot(0.7))
    assert (got["i"], got["j"]) == (1, 1) and got["score"] < 1e-14


def test_hexagonal_root3_on_hexagonal():
    got = _agree(_hex(3.0 * math.sqrt(3.0)), _hex(3.0) @ _rot(0.3))
    assert (got["i"], got["j"]) == (1, 3) and got["score"] < 1e-14  # (sqrt 3 x sqrt 3) R 30


def test_square_3_on_square_4():
    got = _agree(3.0 * np.eye(2), 4.0 * np.eye(2))
    assert (got["i"], got["j"]) == (9, 5)  # 3 x 3 on the sqrt 5 cell (9 against 4 sqrt 5 = 8.944), not the exact 16 : 9
    assert got["score"] == pytest.approx(6.19e-3, abs=5e-6)


def test_a_cell_does_not_match_its_mirror_image():
    """An implementation that compares |theta|, or negates one vector during the reduction, returns (1, 1) here.

    The issue that asked for this case expected no match at all up to max_area = 150.  That does not hold for this cell under
    the specified rule: 0.9 / 3 is rational, so the lattice and its mirror image share super-lattices.  The restatement and the
    brute force both find (4, 4) with score 0.0403 at ltol = 0.05 (a nearly rhombic super-cell, |u| = 5.50, |w| = 5.72, which
    its mirror image matches with the two vectors exchanged) and an exact (5, 5) coincidence at any tighter ltol.  What the case
    is there for holds: no multiple below 4 matches, and (1, 1) is never returned."""
    cell = np.array([[3.0, 0.0], [0.9, 2.6]])
    mirror = np.array([[3.0, 0.0], [-0.9, 2.6]])
    assert _agree(cell, mirror, max_area=30.0) is None  # multiples 1 .. 3
    got = _agree(cell, mirror, max_area=150.0)
    assert (got["i"], got["j"]) == (4, 4) and got["score"] == pytest.approx(0.0403040405, abs=1e-9)
    got = _agree(cell, mirror, max_area=150.0, ltol=0.01, atol=0.2)
    assert (got["i"], got["j"]) == (5, 5) and got["score"] < 1e-14
    got = _agree(cell, cell, max_area=150.0)
    assert (got["i"], got["j"]) == (1, 1) and got["score"] == 0.0


def test_hexagonal_on_square():
    got = _agree(_hex(2.9), 3.6 * np.eye(2), ltol=0.05, atol=1.0)
    assert (got["i"], got["j"]) == (5, 3)
    # at the tight tolerances none within the multiples the brute force covers; the first one lies beyond (area 364)
    assert _agree(_hex(2.9), 3.6 * np.eye(2), max_area=150.0, ltol=0.01, atol=0.2) is None
    far = ref.match(_hex(2.9), 3.6 * np.eye(2), ltol=0.01, atol=0.2)
    assert (far["i"], far["j"]) == (50, 28) and far["film_matrix"].tolist() == [[5, 5], [-5, 5]]


def test_forty_random_pairs():
    matched = 0
    for film, subs in ref.random_pairs(40, 2024):
        got = _agree(film, subs, max_area=110.0, max_area_ratio_tol=0.1, ltol=0.05, atol=1.0)
        matched += got is not None
    print("matched", matched, "of 40")
    assert matched >= 10  # both outcomes are met


def test_degenerate_cells_and_large_multiples():
    assert ref.match(np.array([[1.0, 0.0], [2.0, 0.0]]), np.eye(2))["status"] == 2
    assert ref.match(np.eye(2), np.array([[1.0, np.nan], [0.0, 1.0]]))["status"] == 2
    assert ref.match(np.eye(2)[::-1], np.eye(2))["status"] == 2  # left-handed
    with pytest.raises(ValueError):
        ref.match(np.eye(2), np.eye(2), max_area=300.0)
    assert ref.largest_multiple(2.0, 10.0) == 5 and ref.largest_multiple(3.0, 10.0) == 3 and ref.largest_multiple(11.0, 10.0) == 0


# --- (b) the builder ---------------------------------------------------------------------------------------------------------------
_slab = ref.ref_slab
CASES = ref.BUILDER_CASES


def _parents():
    return {"fcc": dref.fcc(4.0), "tri": ref.triclinic()}


@pytest.mark.parametrize("case", CASES)
def test_builder_geometry(case):
    P = _parents()
    fp, fh, fl, sp, sh, sl, Mf, Ms = case
    film, subs = _slab(P[fp], fh, fl, beg=100), _slab(P[sp], sh, sl, beg=7)
    sep, vac = 2.5, 9.0
    A, carts, fracs, srcs, parts, area = ref.interface(film, subs, Mf, Ms, sep, vac)
    Mf, Ms = np.array(Mf), np.array(Ms)
    i, j = round(np.linalg.det(Mf)), round(np.linalg.det(Ms))
    nf, ns = len(film[1]), len(subs[1])
    assert [len(c) for c in carts] == [j * ns, i * nf, j * ns + i * nf]
    assert np.linalg.det(A) > 0 and A[0, 1] == A[0, 2] == A[1, 2] == A[2, 0] == A[2, 1] == 0.0
    assert area == pytest.approx(np.linalg.norm(np.cross(A[0], A[1])), rel=1e-14)
    assert area == pytest.approx(j * np.linalg.norm(np.cross(subs[0][0], subs[0][1])), rel=1e-12)
    for f, c in zip(fracs, carts):
        assert (f >= 0.0).all() and (f < 1.0).all()
        d = f @ A - c  # the same point up to a cell vector in the plane
        assert np.abs(d @ np.linalg.inv(A) - np.round(d @ np.linalg.inv(A))).max() < 1e-9 and np.abs(d[:, 2]).max() < 1e-9
    assert np.array_equal(carts[2], np.concatenate(carts[:2])) and np.array_equal(srcs[2], np.concatenate(srcs[:2]))
    assert (parts[0] == 0).all() and (parts[1] == 1).all() and np.array_equal(parts[2], np.concatenate(parts[:2]))
    # every parent atom of a side as often as its multiple times its layers
    assert (np.bincount(srcs[0] - 7, minlength=len(P[sp][1])) == j * sl).all()
    assert (np.bincount(srcs[1] - 100, minlength=len(P[fp][1])) == i * fl).all()
    # the film above the substrate by the separation, the vacuum above the film
    assert carts[0][:, 2].min() == 0.0
    assert carts[1][:, 2].min() - carts[0][:, 2].max() == pytest.approx(sep, abs=1e-12)
    assert A[2, 2] - carts[1][:, 2].max() == pytest.approx(vac, abs=1e-12)
    # the substrate is a rigid copy of its slab's super-cell: the same Gram matrix, the same distances
    ps, pf = ref.plane_cell(subs[0]), ref.plane_cell(film[0])
    sup_s, sup_f = Ms @ ps, Mf @ pf
    assert np.allclose(A[:2, :2] @ A[:2, :2].T, sup_s @ sup_s.T, rtol=1e-12, atol=0)
    # the film's strained primitive vectors M_f^-1 (A0, A1): its super-cell has the substrate super-cell's Gram matrix, and its
    # own super-cell vectors are stretched by |u_s| / |u_f|, |w_s| / |w_f|
    prim = np.linalg.inv(Mf) @ A[:2, :2]
    assert np.allclose((Mf @ prim) @ (Mf @ prim).T, sup_s @ sup_s.T, rtol=1e-12, atol=0)
    stretch = np.linalg.norm(A[:2, :2], axis=1) / np.linalg.norm(sup_f, axis=1)
    assert stretch == pytest.approx(np.linalg.norm(sup_s, axis=1) / np.linalg.norm(sup_f, axis=1), rel=1e-13)
    # every film row sits at the strained image of its slab position: in-plane fractions g with g M_f = f + m (mod the super-cell)
    f_slab = (film[1] @ np.linalg.inv(film[0]))[:, :2]
    b = np.arange(i * nf) % nf
    resid = fracs[1][:, :2] @ Mf - f_slab[b]
    q = np.arange(i * nf) // nf
    assert np.abs(resid - np.round(resid)).max() < 1e-9  # an integer vector of the film's surface lattice
    # ... and the images of one atom are pairwise inequivalent: i distinct points modulo the super-cell
    pts = np.round((fracs[1][b == 0, :2] % 1.0) * 1e6).astype(np.int64) % 10**6
    assert len({tuple(p) for p in pts}) == len(set(q[b == 0])) == i


def test_builder_stretch_is_the_reported_mismatch():
    """A matched pair: film fcc(100) a_f on substrate fcc(100) a_s = a_f sqrt 2 x 1.01 -> (2, 1), the film stretched by 1 %."""
    af = 3.0
    film = _slab(dref.fcc(af), (1, 0, 0), 1)
    subs = _slab(dref.fcc(af * math.sqrt(2.0) * 1.01), (1, 0, 0), 1)
    m = ref.match(ref.plane_cell(film[0]), ref.plane_cell(subs[0]), max_area=100.0)
    assert m["status"] == 0 and (m["i"], m["j"]) == (2, 1)
    assert m["ru"] == pytest.approx(0.01, abs=1e-12) and m["rw"] == pytest.approx(0.01, abs=1e-12) and abs(m["sin"]) < 1e-12
    A, carts, fracs, srcs, parts, area = ref.interface(film, subs, m["film_matrix"], m["subs_matrix"], 2.0, 8.0)
    sup_f = m["film_matrix"].astype(np.float64) @ ref.plane_cell(film[0])
    uf, wf = np.linalg.norm(sup_f, axis=1)
    us, ws = np.linalg.norm(A[0]), np.linalg.norm(A[1])
    assert abs(us / uf - 1.0) == pytest.approx(m["ru"], abs=1e-13) and abs(ws / wf - 1.0) == pytest.approx(m["rw"], abs=1e-13)
    assert len(carts[1]) == 2 * 4 and len(carts[0]) == 4
    # the strained film's nearest neighbours join its two planes: a_f / 2 up, a_f / 2 x 1.01 in the plane
    assert dref.shortest_pair(A, carts[1], (1, 1, 0)) == pytest.approx(0.5 * af * math.sqrt(1.0 + 1.01 ** 2), rel=1e-9)


# --- (c) the energy ----------------------------------------------------------------------------------------------------------------
def test_work_of_adhesion_and_units():
    assert ref.work_of_adhesion(-10.0, -6.0, -3.0, 4.0) == 0.25  # the interface is bound: W_ad > 0
    assert ref.EV_A2_TO_J_M2 == 16.02176634 == 1.602176634e-19 * 1e20
    assert 16 / ref.EV_A2_TO_J_M2 == pytest.approx(1 - 0.00136, abs=2e-5)  # the reference's 16 is 0.14 % low
