"""The primitive and conventional cells on the device (csrc/cells.hip, alignn_amd/cells.py) against the restatement of
tests/cells_ref.py, the 23 structures of its table in one call: (a) every integer output equal, cells and positions within 1e-12 A
(products of small integers with the input cell, a few ulps of 4 A: four orders above that, nine below symprec); every structure
alone, and the batch rotated, give the batch's bits; ``sym=`` passed in gives the bits of ``sym=None``; a cell past the image range
and a conventional cell above the atom limit raise and leave the others intact; (b) ``on_conventional_cell`` of ``surface_energy``
and ``vacancy_formation`` on the pair potential of tests/pair_ref.py.

The largest structure of (a) has 8 atoms; the one above the atom limit has 520 (two per primitive cell would do no harm: the
limit is 1024 output atoms, so a centred cell needs more than 512 in the primitive one)."""

import numpy as np
import pytest
import torch

from alignn_amd import conventional_cell, find_symmetry, primitive_cell, surface_energy, vacancy_formation
from tests import cells_ref as ref
from tests import pair_ref, sym_ref
from tests.cells_ref import same_bits as _same_bits
from tests.sim_gpu import DEV

pytestmark = pytest.mark.gpu

ATOL = 1e-12
TABLE = ref.table()
NAMES = list(TABLE)
_CACHE = {}


def _call(fn, names, **kw):
    return fn([TABLE[n][0] for n in names], [TABLE[n][1] for n in names], [TABLE[n][2] for n in names], device=DEV, **kw)


def _batch(fn):
    if fn not in _CACHE:
        _CACHE[fn] = _call(fn, NAMES)
    return _CACHE[fn]


def _want(fn, name):
    key = (fn.__name__, name)
    if key not in _CACHE:
        A, pos, z = TABLE[name][:3]
        _CACHE[key] = getattr(ref, fn.__name__)(A, pos, z, 1e-3)
    return _CACHE[key]


@pytest.mark.parametrize("fn", [conventional_cell, primitive_cell])
def test_the_batch_equals_the_restatement(fn):
    res = _batch(fn)
    assert tuple(res.lattices.shape) == (len(NAMES), 3, 3) and res.lattices.dtype == torch.float64
    worst = 0.0
    for b, name in enumerate(NAMES):
        want = _want(fn, name)
        assert res.source_atom[b].dtype == torch.int32 and res.transform_num[b].dtype == torch.int64, name
        assert np.array_equal(res.transform_num[b].cpu().numpy(), want["transform_num"]), name
        assert np.array_equal(res.source_atom[b].cpu().numpy(), want["source_atom"]), name
        assert (res.transform_den[b], res.multiplicity[b], res.centring[b], res.crystal_system[b], res.n_translations[b]) == \
            (want["transform_den"], want["multiplicity"], want["centring"], want["crystal_system"], want["n_translations"]), name
        assert res.ns[b] == len(want["positions"]) == res.positions[b].shape[0], name
        d_cell = np.abs(res.lattices[b].cpu().numpy() - want["lattice"]).max()
        d_pos = np.abs(res.positions[b].cpu().numpy() - want["positions"]).max()
        print(f"{name}: {res.crystal_system[b]} {res.multiplicity[b]} {res.centring[b]}, {res.ns[b]} atoms, cell {d_cell:.1e} A, "
              f"positions {d_pos:.1e} A")
        assert d_cell <= ATOL and d_pos <= ATOL, name
        worst = max(worst, d_cell, d_pos)
    print(f"largest deviation: {worst:.2e} A")
    if fn is conventional_cell:  # the table itself
        for b, name in enumerate(NAMES):
            system, n_t, mult, letter, lengths, angles, n_out = TABLE[name][3:]
            assert (res.crystal_system[b], res.n_translations[b], res.multiplicity[b], res.centring[b], res.ns[b]) == \
                (system, n_t, mult, letter, n_out), name
            l, ang = ref.lengths_angles(res.lattices[b].cpu().numpy())
            assert np.abs(l - lengths).max() <= 1e-4 and np.abs(ang - angles).max() <= 1e-3, name


@pytest.mark.parametrize("fn", [conventional_cell, primitive_cell])
def test_every_structure_alone_and_the_batch_rotated_give_the_batchs_bits(fn):
    res = _batch(fn)
    for b, name in enumerate(NAMES):
        assert _same_bits(_call(fn, [name]), 0, res, b), name
    rolled = NAMES[5:] + NAMES[:5]
    other = _call(fn, rolled)
    for b, name in enumerate(rolled):
        assert _same_bits(other, b, res, NAMES.index(name)), name


@pytest.mark.parametrize("fn", [conventional_cell, primitive_cell])
def test_sym_passed_in_gives_the_same_bits(fn):
    sym = find_symmetry([TABLE[n][0] for n in NAMES], [TABLE[n][1] for n in NAMES], [TABLE[n][2] for n in NAMES], device=DEV)
    given, res = _call(fn, NAMES, sym=sym), _batch(fn)
    for b, name in enumerate(NAMES):
        assert _same_bits(given, b, res, b), name
    with pytest.raises(ValueError, match="sym was found for structures of"):
        _call(fn, NAMES[:3], sym=sym)


def _above_the_atom_limit():
    """520 atoms in the primitive cell of the base-centred monoclinic lattice of the table, in pairs under the twofold axis (y):
    monoclinic, C-centred, 1040 atoms in the conventional cell."""
    A = TABLE["mono_c"][0]
    x = np.random.default_rng(11).uniform(0.05, 0.95, (260, 3)) @ A
    return A, np.concatenate([x, x * np.array([-1.0, 1.0, -1.0])]), np.full(520, 14)


def test_limits_raise_and_leave_the_others_intact():
    fcc = TABLE["fcc"]
    far = (sym_ref.rebased(fcc[0], [[1, 2, 0], [0, 1, 3], [0, 0, 1]]), fcc[1], fcc[2])
    assert max(sym_ref.image_range(far[0], 1e-3)) > 8
    four = [TABLE["hcp"][:3], far, TABLE["rhombohedral"][:3], _above_the_atom_limit()]
    with pytest.raises(ValueError, match=r"structure 1: no symmetry operations.*structure 3: the new cell has more than 1024") as err:
        conventional_cell([s[0] for s in four], [s[1] for s in four], [s[2] for s in four], device=DEV)
    part, res = err.value.result, _batch(conventional_cell)
    assert part.ns == [2, 0, 3, 0] and part.multiplicity == [1, 0, 3, 0] and part.positions[1].shape == (0, 3)
    assert _same_bits(part, 0, res, NAMES.index("hcp")) and _same_bits(part, 2, res, NAMES.index("rhombohedral"))
    # the primitive cell of the large one is within the limit: the same 520 atoms
    prim = primitive_cell([four[3][0]], [four[3][1]], [four[3][2]], device=DEV)
    assert prim.ns == [520] and prim.crystal_system == ["monoclinic"] and prim.source_atom[0].tolist() == list(range(520))
    with pytest.raises(ValueError, match="structure 0: no symmetry operations"):
        primitive_cell([far[0]], [far[1]], device=DEV)


# --- (b) the wiring --------------------------------------------------------------------------------------------------------------
A0 = 4.0
KW = dict(forces_fn=pair_ref.make_forces_fn(3.4, stress=True), relax_structures=False, device=DEV)


def _cube():
    frac = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]], dtype=np.float64)
    return A0 * np.eye(3), frac * A0


def test_surface_energy_on_the_conventional_cell():
    """The sums of the pair potential run over the same pairs in another order and orientation: about 1e3 terms, 1e-13 relative;
    1e-10 leaves three orders."""
    A, pos = sym_ref.crystals(A0)["fcc"][:2]
    kw = dict(miller_indices=[(1, 0, 0)], thickness=7.0, vacuum=8.0, **KW)
    conv = surface_energy(None, [A], [pos], on_conventional_cell=True, **kw)
    cube = surface_energy(None, [_cube()[0]], [_cube()[1]], **kw)
    plain = surface_energy(None, [A], [pos], **kw)
    assert conv.n_slab[0].tolist() == cube.n_slab[0].tolist() and conv.layers[0].tolist() == cube.layers[0].tolist()
    assert abs(conv.area[0][0] - cube.area[0][0]) <= 1e-12 * cube.area[0][0] and abs(cube.area[0][0] - A0 * A0) <= 1e-12 * A0 * A0
    assert abs(conv.e_slab[0][0] - cube.e_slab[0][0]) <= 1e-10 * abs(cube.e_slab[0][0])
    assert abs(conv.epa[0] - cube.epa[0]) <= 1e-10 * abs(cube.epa[0])
    assert abs(conv.surf_en[0][0] - cube.surf_en[0][0]) <= 1e-10 * abs(cube.e_slab[0][0]) / cube.area[0][0]
    assert conv.src[0][0].tolist() == [0, 1, 2, 3]  # job 0 is the parent: the four atoms of the conventional cell
    # without the option (1, 0, 0) is a plane of the primitive cell: another surface
    assert abs(plain.area[0][0] - cube.area[0][0]) > 0.1 and abs(plain.surf_en[0][0] - cube.surf_en[0][0]) > 1e-3
    # the default is today's behaviour, bit for bit
    off = surface_energy(None, [A], [pos], on_conventional_cell=False, **kw)
    assert np.array_equal(off.e_slab[0], plain.e_slab[0]) and np.array_equal(off.surf_en[0], plain.surf_en[0])
    assert np.array_equal(off.area[0], plain.area[0]) and off.epa[0] == plain.epa[0]
    assert all(torch.equal(p, q) for p, q in zip(off.positions[0], plain.positions[0])) and torch.equal(off.lattices[0], plain.lattices[0])


def test_vacancy_formation_on_the_conventional_cell():
    A, pos, z = sym_ref.supercell(*sym_ref.crystals(A0)["fcc"][:3], (2, 2, 2))
    feats = np.arange(8.0).reshape(8, 1)  # (forces_fn ignores them; the rows go through source_atom)
    kw = dict(supercell=(2, 1, 1), **KW)
    conv = vacancy_formation(None, [A], [pos], [feats], on_conventional_cell=True, species=[z], site_labels="auto", **kw)
    assert conv.n_bulk == [8] and conv.labels[0].tolist() == [0] and conv.multiplicity[0].tolist() == [4]
    cube = vacancy_formation(None, [_cube()[0]], [_cube()[1]], site_labels=[np.zeros(4, dtype=np.int64)], **kw)
    assert abs(conv.e_bulk[0] - cube.e_bulk[0]) <= 1e-10 * abs(cube.e_bulk[0])
    assert abs(conv.e_defect[0][0] - cube.e_defect[0][0]) <= 1e-10 * abs(cube.e_bulk[0])
    plain = vacancy_formation(None, [A], [pos], site_labels="auto", species=[z], **kw)
    assert plain.n_bulk == [16]
    off = vacancy_formation(None, [A], [pos], site_labels="auto", species=[z], on_conventional_cell=False, **kw)
    assert off.n_bulk == [16] and off.e_bulk[0] == plain.e_bulk[0] and np.array_equal(off.e_defect[0], plain.e_defect[0])
    assert np.array_equal(off.formation_energy[0], plain.formation_energy[0])
    assert all(torch.equal(p, q) for p, q in zip(off.positions[0], plain.positions[0]))
    # labels given by hand follow their atoms: the four atoms of the cube keep the label of the atom they are copies of
    hand = vacancy_formation(None, [A], [pos], on_conventional_cell=True, site_labels=[np.arange(8) + 10], **kw)
    assert len(hand.labels[0]) == 1 and hand.multiplicity[0].tolist() == [4] and 10 <= hand.labels[0][0] < 18
