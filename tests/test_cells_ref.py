"""The numpy restatement of the primitive and conventional cells (tests/cells_ref.py, the definitions of include/alignn_cells.h)
against the table of the feature's issue and against what any such cell must satisfy: the density, the determinant of the
transformation, atoms that are copies of their source atoms, the symmetry of the output, and the same cell whatever basis or
supercell the crystal was given in.

The rows of ``hard_table()`` - the centrings A, B and I, both rhombohedral settings, cells in no special orientation, strain and
noise below symprec, loops of more than 256 translations, atoms and lattice points - are held to the same: their textbook columns,
the properties of every cell, and decisions that are not close (a margin over symprec of 0.05, atoms 1e-6 off the faces of the new
cell), so that the device may be compared with them bit for bit in the integers (tests/test_gpu_cells_hard.py).  The operations of
the two largest rows are written down in closed form: the brute-force search would take 8 s and 14 s."""

import numpy as np
import pytest

from tests import cells_ref as ref
from tests import sym_ref

TABLE = ref.table()
HARD = ref.hard_table()
ROWS = {**TABLE, **HARD}
LARGE = ("tri_294", "mono_c_300")  # their operations in closed form
MARGIN, FACE_MARGIN = 0.05, 1e-6
_CACHE = {}


def _conventional(name):
    if name not in _CACHE:
        A, pos, z = ROWS[name][:3]
        sym = ref.known_operations(name, ROWS[name]) if name in LARGE else sym_ref.find_symmetry(A, pos, z, 1e-3)
        _CACHE[name] = (sym, ref.conventional_cell(A, pos, z, sym=sym), ref.primitive_cell(A, pos, z, sym=sym))
    return _CACHE[name]


def test_the_table_has_every_row_of_the_issue():
    assert len(TABLE) == 23


def test_the_hard_table_has_every_row_of_its_issue():
    assert not set(HARD) & set(TABLE)
    assert set(HARD) == {"ortho_a", "ortho_b", "ortho_i", "bcc_prim", "ortho_permuted", "rhombohedral_hex", "rhombohedral_reverse",
                         "rhombohedral_obtuse", "trigonal_p", "mono_acute", "fcc_rebased_far", "hcp_rot", "rhombohedral_rot",
                         "bcc_prim_rot", "mono_c_rot", "diamond_strained_noisy", "diamond_96", "tri_294", "mono_c_300"}
    assert [len(HARD[n][1]) for n in ("diamond_96",) + LARGE] == [96, 294, 300]


@pytest.mark.parametrize("name", list(HARD))
def test_the_decisions_of_the_hard_table_are_not_close(name):
    sym, conv, prim = _conventional(name)
    for kind, got in (("conventional", conv), ("primitive", prim)):
        print(f"{name} {kind}: margin over symprec {got['margin']:.3f}, face margin {got['face_margin']:.2e}, "
              f"largest pick {got['largest_pick']} points")
        assert got["margin"] >= MARGIN and got["face_margin"] >= FACE_MARGIN


def test_the_hard_table_reaches_what_it_is_there_for():
    conv = {name: _conventional(name)[1] for name in HARD}
    prim = {name: _conventional(name)[2] for name in HARD}
    assert [conv[n]["centring"] for n in ("ortho_a", "ortho_b", "ortho_i", "bcc_prim")] == ["A", "B", "I", "I"]
    assert conv["rhombohedral_reverse"]["reverse_setting"] and conv["rhombohedral_hex"]["reverse_setting"]
    assert not conv["rhombohedral_obtuse"]["reverse_setting"] and conv["rhombohedral_obtuse"]["centring"] == "R"
    assert conv["mono_acute"]["beta_negated"] and conv["trigonal_p"]["crystal_system"] == "trigonal"
    assert conv["fcc_rebased_far"]["largest_pick"] >= 2023 and np.abs(conv["fcc_rebased_far"]["transform_num"]).max() > 1
    # the axes of ortho_permuted come in the order of the rows given (c, a, b): by_length has something to do
    assert conv["ortho_permuted"]["transform_num"].tolist() != np.eye(3, dtype=np.int64).tolist()
    # only the rotations that keep the supercell are among its operations: the primitive cell of diamond_96 is reported
    # tetragonal; the conventional cell goes through the operations of that primitive cell
    assert (prim["diamond_96"]["crystal_system"], conv["diamond_96"]["crystal_system"]) == ("tetragonal", "cubic")
    assert (prim["tri_294"]["transform_den"], len(prim["tri_294"]["positions"])) == (294, 1)
    assert conv["mono_c_300"]["source_atom"].tolist() == np.repeat(np.arange(300), 2).tolist()
    # lengths that tie only to within symprec: the strained cube's c is 3.6e-5 A longer, and still the cube is found
    l = ref.lengths_angles(conv["diamond_strained_noisy"]["lattice"])[0]
    assert 1e-5 < l.max() - l.min() < 1e-4 and conv["diamond_strained_noisy"]["margin"] < 1.0


@pytest.mark.parametrize("name", list(ROWS))
def test_the_restatement_reproduces_the_table(name):
    A, pos, z, system, n_t, mult, letter, lengths, angles, n_out = ROWS[name]
    sym, got, prim = _conventional(name)
    assert (got["crystal_system"], got["n_translations"], got["multiplicity"], got["centring"]) == (system, n_t, mult, letter)
    l, ang = ref.lengths_angles(got["lattice"])
    assert np.abs(l - lengths).max() <= 1e-4 and np.abs(ang - angles).max() <= 1e-3, (l, ang)
    assert len(got["positions"]) == n_out == len(got["source_atom"])
    assert prim["multiplicity"] == 1 and prim["centring"] == "P" and len(prim["positions"]) * n_t == len(pos)


def _maps_onto_itself(C, positions, origin):
    """The twofold axis (y) through origin takes every atom onto an atom, to within a vector of the lattice C."""
    image = (positions - origin) * np.array([-1.0, 1.0, -1.0]) + origin
    d = (image[:, None] - positions[None]) @ np.linalg.inv(C)
    return bool((np.abs((d - np.rint(d)) @ C).max(axis=2).min(axis=1) <= 1e-9).all())


@pytest.mark.parametrize("name", list(ROWS))
def test_what_every_cell_satisfies(name):
    A, pos, z = ROWS[name][:3]
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
        if name == "mono_c_300":  # (a search over 600 atoms takes minutes: its two operations are known)
            assert _maps_onto_itself(C, got["positions"], ref.SHIFT @ A) and not _maps_onto_itself(C, got["positions"], np.zeros(3))
            assert got["crystal_system"] == sym["crystal_system"] == "monoclinic"
            continue
        out = sym_ref.find_symmetry(C, got["positions"], z[got["source_atom"]], 1e-3)
        if name == "diamond_96":  # the supercell keeps 16 of the 48 rotations; the cells that come out have them all
            assert out["n_translations"] == mult and (sym["point_group_order"], out["point_group_order"]) == (16, 48)
            assert (sym["crystal_system"], out["crystal_system"]) == ("tetragonal", "cubic")
            assert got["crystal_system"] == ("cubic" if got is conv else "tetragonal")
            continue
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
