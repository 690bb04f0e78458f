"""The numpy restatement of the primitive and conventional cells (tests/cells_ref.py, the definitions of include/alignn_cells.h)
against the table of the feature's issue and against what any such cell must satisfy: the density, the determinant of the
transformation, atoms that are copies of their source atoms, the symmetry of the output, and the same cell whatever basis or
supercell the crystal was given in."""

import numpy as np
import pytest

from tests import cells_ref as ref
from tests import sym_ref

TABLE = ref.table()
_CACHE = {}


def _conventional(name):
    if name not in _CACHE:
        A, pos, z = TABLE[name][:3]
        sym = sym_ref.find_symmetry(A, pos, z, 1e-3)
        _CACHE[name] = (sym, ref.conventional_cell(A, pos, z, sym=sym), ref.primitive_cell(A, pos, z, sym=sym))
    return _CACHE[name]


def test_the_table_has_every_row_of_the_issue():
    assert len(TABLE) == 23


@pytest.mark.parametrize("name", list(TABLE))
def test_the_restatement_reproduces_the_table(name):
    A, pos, z, system, n_t, mult, letter, lengths, angles, n_out = TABLE[name]
    sym, got, prim = _conventional(name)
    assert (got["crystal_system"], got["n_translations"], got["multiplicity"], got["centring"]) == (system, n_t, mult, letter)
    l, ang = ref.lengths_angles(got["lattice"])
    assert np.abs(l - lengths).max() <= 1e-4 and np.abs(ang - angles).max() <= 1e-3, (l, ang)
    assert len(got["positions"]) == n_out == len(got["source_atom"])
    assert prim["multiplicity"] == 1 and prim["centring"] == "P" and len(prim["positions"]) * n_t == len(pos)


@pytest.mark.parametrize("name", list(TABLE))
def test_what_every_cell_satisfies(name):
    A, pos, z = TABLE[name][:3]
    sym, conv, prim = _conventional(name)
    for got in (conv, prim):
        C, n_t, mult = got["lattice"], got["n_translations"], got["multiplicity"]
        dens_in, dens_out = len(pos) / abs(np.linalg.det(A)), len(got["positions"]) / abs(np.linalg.det(C))
        assert abs(dens_out - dens_in) <= 1e-12 * dens_in
        # the convention: transform_den = n_t, not reduced, and the handedness of the input is kept (det > 0)
        assert got["transform_den"] == n_t and ref.det3(got["transform_num"].tolist()) * n_t == mult * n_t ** 3
        # (a supercell's conventional cell is written from its primitive cell: products of small integers, a few ulps of 4 A)
        assert np.abs(C - ref.vec(A, got["transform_num"], n_t)).max() <= 1e-12
        # every atom is its source atom plus a vector of the primitive lattice
        P = prim["lattice"]
        d = (got["positions"] - pos[got["source_atom"]]) @ np.linalg.inv(P)
        assert np.abs((d - np.rint(d)) @ P).max() <= 1e-3
        f = got["positions"] @ np.linalg.inv(C)
        assert (f > -1e-12).all() and (f < 1.0 + 1e-12).all()  # (this inverse is not the one the wrap used: to rounding)
        assert (np.diff(got["source_atom"]) >= 0).all() and np.bincount(got["source_atom"]).max() == mult
        out = sym_ref.find_symmetry(C, got["positions"], z[got["source_atom"]], 1e-3)
        assert out["n_translations"] == mult and out["point_group_order"] == sym["point_group_order"]
        assert out["crystal_system"] == got["crystal_system"] == sym["crystal_system"]


def _sorted_shape(C):
    l, ang = ref.lengths_angles(C)
    return np.concatenate([np.sort(l), np.sort(ang)])


@pytest.mark.parametrize("name", list(TABLE))
def test_another_basis_or_a_supercell_gives_the_same_cell(name):
    A, pos, z = TABLE[name][:3]
    conv = _conventional(name)[1]
    want = _sorted_shape(conv["lattice"])
    others = [ref.rebase(A, pos, z, V) for V in ref.REBASES] + [sym_ref.supercell(A, pos, z, d) for d in ((2, 1, 1), (2, 2, 2))]
    # find_symmetry's limit holds: a row of the table that is itself rebased leaves its image range when rebased once more, or
    # when its longest vector is doubled
    inside = [o for o in others if max(sym_ref.image_range(o[0], 1e-3)) <= sym_ref.MAX_IMAGE_RANGE]
    assert len(inside) == len(others) or (name.endswith("_rebased") and len(inside) >= 2)
    for A2, pos2, z2 in inside:
        got = ref.conventional_cell(A2, pos2, z2)
        assert np.abs(_sorted_shape(got["lattice"]) - want).max() <= 1e-9
        assert got["centring"] == conv["centring"] and len(got["positions"]) == len(conv["positions"])
        assert got["multiplicity"] == conv["multiplicity"] and got["crystal_system"] == conv["crystal_system"]


def test_hermite_normal_form_is_canonical():
    rng = np.random.default_rng(3)
    for _ in range(20):
        nt = int(rng.integers(1, 9))
        ks = rng.integers(0, nt, size=(4, 3))
        H = ref.hermite(nt, ks.tolist())
        assert ref.hermite(nt, ks[::-1].tolist()) == H  # the same lattice from the generators in another order
        assert H[1][0] == H[2][0] == H[2][1] == 0 and all(H[c][c] > 0 for c in range(3))
        assert all(0 <= H[r][c] < H[c][c] for c in range(3) for r in range(c))
        for k in list(ks) + [[nt, 0, 0], [0, nt, 0], [0, 0, nt]]:  # every generator is an integer combination of the rows
            x = np.linalg.solve(np.array(H, dtype=np.float64).T, np.array(k, dtype=np.float64))
            assert np.abs(x - np.rint(x)).max() < 1e-9


def test_limits_raise_a_status():
    A, pos, z = TABLE["fcc"][:3]
    far = sym_ref.rebased(A, [[1, 2, 0], [0, 1, 3], [0, 0, 1]])
    with pytest.raises(ValueError):
        ref.conventional_cell(far, pos, z)  # (the symmetry search's own image range)
    flat = np.diag([3.0, 3.0, 23.0])  # primitive tetragonal: the search in the plane is short, the cell is found
    got = ref.conventional_cell(flat, np.zeros((1, 3)), None)
    assert got["crystal_system"] == "tetragonal" and got["centring"] == "P"
