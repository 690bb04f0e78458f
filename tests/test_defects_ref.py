"""The restatements of tests/defects_ref.py and the pair potential of tests/pair_ref.py, pinned without a GPU: the Miller bases
by their geometry, the slabs by atom counts, distances and broken-bond counts known for fcc, the vacancy by its closed form in a
pair potential, and the host-side argument checks of ``alignn_amd.defects``."""

import numpy as np
import pytest

from alignn_amd import defects
from alignn_amd.synthetic import make_crystal
from tests import defects_ref as ref
from tests import pair_ref

HKLS = [(1, 0, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 1, 0), (1, -1, 0), (3, 2, 1)]
A = 4.0
RC = 3.4  # first neighbours only: between a / sqrt(2) = 2.83 and a


def _triclinic():
    lat, frac, _ = make_crystal(6, 77)
    lat = np.asarray(lat, dtype=np.float64)
    return lat, np.asarray(frac, dtype=np.float64) @ lat


PARENTS = {"fcc": ref.fcc(A), "triclinic": _triclinic()}


@pytest.mark.parametrize("name", list(PARENTS))
@pytest.mark.parametrize("hkl", HKLS)
def test_miller_basis_is_unimodular_and_in_plane(name, hkl):
    lat, _ = PARENTS[name]
    raw, b = ref.ase_basis(lat, hkl), ref.miller_basis(lat, hkl)
    assert abs(ref.det3i(raw)) == 1 and ref.det3i(b) == 1
    assert np.array_equal(b, defects.miller_basis(lat, hkl))
    assert np.array_equal(b[[0, 2]], raw[[0, 2]]) and np.array_equal(np.abs(b[1]), np.abs(raw[1]))
    assert b[0] @ np.array(hkl) == 0 and b[1] @ np.array(hkl) == 0
    C = b @ lat
    assert np.linalg.det(C) > 0
    if name == "fcc":
        area = np.linalg.norm(np.cross(C[0], C[1]))
        assert area == pytest.approx(A * A * np.linalg.norm(hkl), rel=1e-12)


def test_one_minus_one_zero_is_the_flipped_case():
    assert ref.det3i(ref.ase_basis(PARENTS["fcc"][0], (1, -1, 0))) == -1


def test_miller_basis_reduces_by_the_gcd():
    lat = PARENTS["triclinic"][0]
    assert np.array_equal(defects.miller_basis(lat, (2, 2, 2)), defects.miller_basis(lat, (1, 1, 1)))
    assert np.array_equal(defects.miller_basis(lat, (0, -3, 0)), defects.miller_basis(lat, (0, 1, 0)))


@pytest.mark.parametrize("name", list(PARENTS))
@pytest.mark.parametrize("hkl", HKLS)
def test_slab_atoms_and_distances(name, hkl):
    lat, pos = PARENTS[name]
    n = len(pos)
    b = ref.miller_basis(lat, hkl)
    layers = ref.layers_for(lat, b, 12.0)
    cell, cart, frac, src = ref.slab(lat, pos, b, layers, 10.0)
    assert len(cart) == n * layers and (np.bincount(src, minlength=n) == layers).all()
    assert (frac >= 0.0).all() and (frac < 1.0).all()
    assert np.linalg.det(cell) > 0
    # the slab is layers x the parent's volume plus the vacuum over its face
    area = np.linalg.norm(np.cross(cell[0], cell[1]))
    assert np.linalg.det(cell) == pytest.approx(layers * abs(np.linalg.det(lat)) + 10.0 * area, rel=1e-12)
    assert ref.shortest_pair(cell, cart) >= ref.shortest_pair(lat, pos) - 1e-9
    if name == "fcc":
        assert ref.shortest_pair(cell, cart) == pytest.approx(A / np.sqrt(2), rel=1e-12)
    # the positions are those of the fractions, and lie in the lower part of the cell
    back = frac @ cell - cart
    back = back @ np.linalg.inv(cell)
    assert np.abs(back - np.round(back)).max() < 1e-9


def test_supercell_order_and_removal():
    lat, pos = PARENTS["triclinic"]
    cell, cart, frac, src = ref.supercell(lat, pos, (2, 1, 3), beg=5)
    n = len(pos)
    assert np.array_equal(cell, np.array([2.0, 1.0, 3.0])[:, None] * lat) and len(cart) == 6 * n
    for img, (m0, m1, m2) in enumerate((a, b, c) for a in range(2) for b in range(1) for c in range(3)):
        want = pos + m0 * lat[0] + m1 * lat[1] + m2 * lat[2]
        assert np.abs(cart[img * n:(img + 1) * n] - want).max() < 1e-12
    assert np.array_equal(src, 5 + np.arange(6 * n) % n) and (frac >= 0).all() and (frac < 1).all()
    for a in (0, n + 2, 6 * n - 1):
        c2, cart2, frac2, src2 = ref.supercell(lat, pos, (2, 1, 3), removed=a, beg=5)
        keep = np.arange(6 * n) != a
        assert np.array_equal(cart2, cart[keep]) and np.array_equal(frac2, frac[keep]) and np.array_equal(src2, src[keep])
        assert np.array_equal(c2, cell)


def test_pair_potential_forces_and_stress_are_the_gradients():
    lat, pos = PARENTS["triclinic"]
    rng = np.random.default_rng(0)
    pos = pos + rng.normal(0.0, 0.05, pos.shape)
    efs = pair_ref.make_efs(4.5)
    e, f, s = efs(lat, pos)
    assert pair_ref.bond_count(lat, pos, 4.5) > 20
    h = 1e-5
    for i, k in ((0, 0), (3, 1), (5, 2)):
        d = np.zeros_like(pos)
        d[i, k] = h
        num = -(efs(lat, pos + d)[0] - efs(lat, pos - d)[0]) / (2 * h)
        assert num == pytest.approx(f[i, k], rel=1e-6, abs=1e-8)
    vol = abs(np.linalg.det(lat))
    for a, b in ((0, 0), (1, 2), (2, 2)):
        eps = np.zeros((3, 3))
        eps[a, b] = eps[b, a] = h if a != b else h
        Fp, Fm = np.eye(3) + eps, np.eye(3) - eps
        num = (efs(lat @ Fp, pos @ Fp)[0] - efs(lat @ Fm, pos @ Fm)[0]) / (2 * h) / vol
        want = s[a, b] + s[b, a] if a != b else s[a, b]
        assert num == pytest.approx(want, rel=1e-6, abs=1e-8)
    assert np.abs(f.sum(0)).max() < 1e-12


BROKEN = {(1, 0, 0): 8, (1, 1, 0): 12, (1, 1, 1): 12, (2, 1, 1): 20, (1, -1, 0): 12}


@pytest.mark.parametrize("hkl", list(BROKEN))
def test_fcc_slabs_lose_the_known_bonds(hkl):
    lat, pos = PARENTS["fcc"]
    efs = pair_ref.make_efs(RC)
    b = ref.miller_basis(lat, hkl)
    layers = ref.layers_for(lat, b, 12.0)
    cell, cart, _, _ = ref.slab(lat, pos, b, layers, 10.0)
    broken = layers * pair_ref.bond_count(lat, pos, RC) - pair_ref.bond_count(cell, cart, RC)
    assert broken == BROKEN[hkl]
    epa = efs(lat, pos)[0] / len(pos)
    phi1 = float(pair_ref.phi(A / np.sqrt(2), RC)[0])
    assert epa == pytest.approx(6 * phi1, rel=1e-12)
    area = np.linalg.norm(np.cross(cell[0], cell[1]))
    got = ref.surface_energy(efs(cell, cart)[0], len(cart), epa, cell)
    assert got == pytest.approx(-phi1 * broken / (2 * area), rel=1e-10)
    assert got > 0


def test_unrelaxed_vacancy_in_a_pair_potential():
    lat, pos = PARENTS["fcc"]
    efs = pair_ref.make_efs(RC)
    cell, cart, _, _ = ref.supercell(lat, pos, (2, 2, 2))
    assert min(np.linalg.norm(cell, axis=1)) > RC
    e_bulk = efs(cell, cart)[0]
    for a in (0, 3):
        c2, cart2, _, _ = ref.supercell(lat, pos, (2, 2, 2), removed=a)
        e_def = efs(c2, cart2)[0]
        assert e_def - e_bulk == pytest.approx(-2 * e_bulk / len(cart), rel=1e-10)
        # n_defect + 1 = n_bulk: the reference's formula at mu = 0 is e_defect - e_bulk, one atom's bonds
        assert ref.formation_energy(e_def, len(cart2), e_bulk, len(cart)) == pytest.approx(-2 * e_bulk / len(cart), rel=1e-10)
        assert ref.formation_energy(e_def, len(cart2), e_bulk, len(cart), mu=0.25) == pytest.approx(
            0.25 - 2 * e_bulk / len(cart), rel=1e-10)


def _fn(lats, poss):
    raise AssertionError("an argument error must come before any evaluation")


def test_argument_errors_come_before_any_device_work():
    lat, pos = PARENTS["fcc"]
    with pytest.raises(ValueError):
        defects.miller_basis(lat, (0, 0, 0))
    with pytest.raises(ValueError):
        defects.surface_energy(None, [lat], [pos], miller_indices=[(0, 0, 0)], forces_fn=_fn)
    with pytest.raises(ValueError):
        defects.surface_energy(None, [lat], [pos], miller_indices=[(1, 0, 0)], vacuum=-1.0, forces_fn=_fn)
    with pytest.raises(ValueError):
        defects.surface_energy(None, [lat], [pos], miller_indices=[(1, 0, 0)], thickness=0.0, forces_fn=_fn)
    with pytest.raises(ValueError):
        defects.surface_energy(None, [lat, lat], [pos, pos], miller_indices=[[(1, 0, 0)]] * 3, forces_fn=_fn)
    with pytest.raises(ValueError):  # a one-atom supercell
        defects.vacancy_formation(None, [lat], [pos[:1]], supercell=(1, 1, 1), forces_fn=_fn)
    with pytest.raises(ValueError):  # wrong label length
        defects.vacancy_formation(None, [lat], [pos], site_labels=[np.zeros(3, dtype=int)], supercell=(2, 2, 2), forces_fn=_fn)
    with pytest.raises(ValueError):
        defects.vacancy_formation(None, [lat], [pos], site_labels=[np.zeros(4)], supercell=(2, 2, 2), forces_fn=_fn)
    with pytest.raises(ValueError):
        defects.vacancy_formation(None, [lat], [pos], supercell=(2, 0, 2), forces_fn=_fn)
    with pytest.raises(ValueError):
        defects.vacancy_formation(None, [lat], [pos], supercell=(2, 2, 2), fixed=[np.zeros(4, dtype=bool)], forces_fn=_fn)
    with pytest.raises(ValueError):
        defects.vacancy_formation(None, [lat], [pos], supercell=(2, 2, 2), max_atoms_per_call=0, forces_fn=_fn)
    with pytest.raises(ValueError):
        defects.vacancy_formation(None, [lat], [pos[:, :2]], supercell=(2, 2, 2), forces_fn=_fn)
