"""The primitive and conventional cells on the device (csrc/cells.hip, alignn_amd/cells.py) against the restatement of
tests/cells_ref.py on the structures of ``cells_ref.hard_table()``: the centrings A, B and I, both rhombohedral settings and an R
lattice given as its triple hexagonal cell, a trigonal structure on a P hexagonal lattice, a monoclinic cell found with an acute
beta, orthorhombic axes out of length order, cells in no special orientation, strain and noise below symprec, and the loops of
``cells_reduce_kernel`` that stride by the 256 threads of its workgroup past one pass: 294 pure translations, 300 atoms in and 600
out (three blocks of ``cells_fill_kernel``), 2023 lattice points in a pick.  One call of ``conventional_cell`` and one of
``primitive_cell`` over the whole table.

The operations: ``find_symmetry`` runs once on the device for the batch and is passed as ``sym=`` to both calls (what ``sym=None``
does by itself: the calls of every structure alone below take that way).  The restatement searches the operations of every row
itself (tests/sym_ref.py), except for ``tri_294`` and ``mono_c_300``: there it is given the device's own operations, converted to
the dict of ``cells_ref._cell``.  The symmetry search is pinned on its own in tests/test_gpu_symmetry.py; this module pins cells.hip
on equal inputs, and a brute-force search of 10 to 250 s on the host is avoided.

Before anything is compared the restatement's decisions are shown not to be close: a margin over symprec of 0.05 or more, and no
output atom within 1e-6 (fractional) of a face of its new cell - otherwise the two sides could differ legitimately.  Then every
integer output is equal and cells and positions agree within the 1e-12 A of tests/test_gpu_cells.py: the same products in the same
order without contraction, of integers below about 50 with cell entries below 32 A; a few ulps of 32 A is about 2e-14.  The
largest deviation, measured on an MI355X: 0.00e+00 A for both calls - every cell entry and every coordinate of the 19 structures
has the restatement's bits.

The status bits the kernels set from the operations they are given (``STATUS_SYMMETRY``, ``STATUS_TRANSLATIONS``) are produced
from doctored copies of a ``SymmetryResult``.  Every doctored value is one the kernel checks before it uses it (``k < 0 || k >=
R.n`` ahead of any use of k as an index; a translation is only rounded and measured; another structure's operations come with
their own row pointers): none can address memory outside the arrays."""

import dataclasses

import numpy as np
import pytest
import torch

from alignn_amd import conventional_cell, find_symmetry, primitive_cell
from tests import cells_ref as ref
from tests import sym_ref
from tests.cells_ref import same_bits as _same_bits
from tests.sim_gpu import DEV

pytestmark = pytest.mark.gpu

ATOL = 1e-12  # (that of tests/test_gpu_cells.py)
MARGIN, FACE_MARGIN = 0.05, 1e-6
HARD = ref.hard_table()
NAMES = list(HARD)
LARGE = ("tri_294", "mono_c_300")
FNS = [conventional_cell, primitive_cell]
_CACHE = {}


def _lists(rows):
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def _sym():
    if "sym" not in _CACHE:
        _CACHE["sym"] = find_symmetry(*_lists([HARD[n] for n in NAMES]), device=DEV)
    return _CACHE["sym"]


def _batch(fn):
    if fn not in _CACHE:
        _CACHE[fn] = fn(*_lists([HARD[n] for n in NAMES]), sym=_sym(), device=DEV)
    return _CACHE[fn]


def _operations(sym, b):
    """Structure b of a SymmetryResult, read from its packed arrays, as the dict cells_ref._cell takes."""
    pk, n = sym.packed, sym.ns[b]
    op, mp = pk["op_ptr"].cpu().numpy(), pk["map_ptr"].cpu().numpy()
    rot = pk["rotations"][op[b]:op[b + 1]].cpu().numpy().astype(np.int64)
    return dict(rotations=rot, translations=pk["translations"][op[b]:op[b + 1]].cpu().numpy(),
                atom_map=pk["atom_map"][mp[b]:mp[b + 1]].cpu().numpy().astype(np.int64).reshape(len(rot), n),
                n_translations=sum(1 for W in rot if np.array_equal(W, np.eye(3, dtype=np.int64))),
                point_group_order=len({tuple(W.reshape(-1)) for W in rot}))


def _want(fn, name):
    key = (fn.__name__, name)
    if key not in _CACHE:
        A, pos, z = HARD[name][:3]
        if ("ops", name) not in _CACHE:
            _CACHE["ops", name] = _operations(_sym(), NAMES.index(name)) if name in LARGE else sym_ref.find_symmetry(A, pos, z, 1e-3)
        _CACHE[key] = getattr(ref, fn.__name__)(A, pos, z, 1e-3, sym=_CACHE["ops", name])
    return _CACHE[key]


@pytest.mark.parametrize("fn", FNS)
def test_the_batch_equals_the_restatement(fn):
    for name in NAMES:  # the preconditions, before any comparison
        want = _want(fn, name)
        assert want["margin"] >= MARGIN and want["face_margin"] >= FACE_MARGIN, (name, want["margin"], want["face_margin"])
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
        print(f"{name}: {res.crystal_system[b]} {res.multiplicity[b]} {res.centring[b]}, {res.ns[b]} atoms, n_t {res.n_translations[b]}, "
              f"margin {want['margin']:.3f}, cell {d_cell:.1e} A, positions {d_pos:.1e} A")
        assert d_cell <= ATOL and d_pos <= ATOL, name
        worst = max(worst, d_cell, d_pos)
    print(f"largest deviation: {worst:.2e} A")
    if fn is conventional_cell:  # the table itself
        for b, name in enumerate(NAMES):
            system, n_t, mult, letter, lengths, angles, n_out = HARD[name][3:]
            assert (res.crystal_system[b], res.n_translations[b], res.multiplicity[b], res.centring[b], res.ns[b]) == \
                (system, n_t, mult, letter, n_out), name
            l, ang = ref.lengths_angles(res.lattices[b].cpu().numpy())
            assert np.abs(l - lengths).max() <= 1e-4 and np.abs(ang - angles).max() <= 1e-3, name


def test_the_cases_the_table_is_there_for():
    """By name: a change of the inputs cannot empty the module without this failing."""
    conv, prim = _batch(conventional_cell), _batch(primitive_cell)
    at = NAMES.index
    assert [conv.centring[at(n)] for n in ("ortho_a", "ortho_b", "ortho_i", "bcc_prim", "bcc_prim_rot")] == ["A", "B", "I", "I", "I"]
    # the reverse branch is taken (and then transform_num equals the restatement's, above), and is not taken
    for name, taken in (("rhombohedral_reverse", True), ("rhombohedral_rot", True), ("rhombohedral_hex", True), ("rhombohedral_obtuse", False)):
        assert _want(conventional_cell, name)["reverse_setting"] == taken and conv.centring[at(name)] == "R", name
        assert np.array_equal(conv.transform_num[at(name)].cpu().numpy(), _want(conventional_cell, name)["transform_num"]), name
    assert _want(conventional_cell, "mono_acute")["beta_negated"]
    assert (conv.crystal_system[at("trigonal_p")], conv.centring[at("trigonal_p")], conv.multiplicity[at("trigonal_p")]) == ("trigonal", "P", 1)
    assert conv.transform_num[at("ortho_permuted")].tolist() == [[0, 1, 0], [0, 0, 1], [1, 0, 0]]
    far = at("fcc_rebased_far")
    assert _want(primitive_cell, "fcc_rebased_far")["largest_pick"] >= 2023  # eight passes of the workgroup
    assert int(conv.transform_num[far].abs().max()) > 1 and int(prim.transform_num[far].abs().max()) > 1
    tri = at("tri_294")
    for res in (conv, prim):  # 294 > 256 pure translations
        assert (res.ns[tri], res.transform_den[tri], res.n_translations[tri], res.source_atom[tri].tolist()) == (1, 294, 294, [0])
    big = at("mono_c_300")  # two passes over the atoms; three blocks of the fill
    assert conv.ns[big] == 600 and conv.source_atom[big].tolist() == np.repeat(np.arange(300), 2).tolist()
    assert prim.ns[big] == 300 and prim.source_atom[big].tolist() == list(range(300))
    d96 = at("diamond_96")  # the two passes: 96 atoms, 48 translations, the primitive cell's own operations
    assert (conv.crystal_system[d96], conv.centring[d96], conv.ns[d96], conv.n_translations[d96]) == ("cubic", "F", 8, 48)
    assert (prim.crystal_system[d96], prim.ns[d96]) == ("tetragonal", 2)
    # source_atom composes through both passes: the atoms of the conventional cell are copies of the primitive cell's two, in
    # the numbering of the 96, four of each
    assert conv.source_atom[d96].tolist() == np.repeat(prim.source_atom[d96].cpu().numpy(), 4).tolist()
    assert len(set(prim.source_atom[d96].tolist())) == 2
    noisy = at("diamond_strained_noisy")  # lengths that tie only within symprec
    l = ref.lengths_angles(conv.lattices[noisy].cpu().numpy())[0]
    assert conv.crystal_system[noisy] == "cubic" and 1e-5 < l.max() - l.min() < 1e-4


@pytest.mark.parametrize("fn", FNS)
def test_what_the_device_output_satisfies_by_itself(fn):
    res, prim = _batch(fn), _batch(primitive_cell)
    for b, name in enumerate(NAMES):
        A, pos = HARD[name][:2]
        num, n_t, mult = res.transform_num[b].cpu().numpy().tolist(), res.n_translations[b], res.multiplicity[b]
        # the atom count scales with the cell volume, in integers
        assert ref.det3(num) * len(pos) == res.ns[b] * n_t ** 3 and res.ns[b] % mult == 0 and ref.det3(num) == mult * n_t ** 2, name
        C, out = res.lattices[b].cpu().numpy(), res.positions[b].cpu().numpy()
        f = out @ np.linalg.inv(C)  # (no atom is within 1e-6 of a face: the rounding of another inverse does not matter)
        assert (f >= 0.0).all() and (f < 1.0).all(), name
        # every atom is a copy of its source atom, moved by a vector of the crystal's lattice
        P = prim.lattices[b].cpu().numpy()
        d = (out - pos[res.source_atom[b].cpu().numpy()]) @ np.linalg.inv(P)
        assert np.abs((d - np.rint(d)) @ P).max() <= 1e-9, name
        assert np.abs(C - ref.vec(A, np.array(num), n_t)).max() <= ATOL, name


@pytest.mark.parametrize("fn", FNS)
def test_every_structure_alone_and_the_batch_rolled_give_the_batchs_bits(fn):
    res = _batch(fn)
    for b, name in enumerate(NAMES):  # (sym=None: the search runs inside the call)
        assert _same_bits(fn(*_lists([HARD[name]]), device=DEV), 0, res, b), name
    rolled = NAMES[5:] + NAMES[:5]
    other = fn(*_lists([HARD[n] for n in rolled]), device=DEV)
    for b, name in enumerate(rolled):
        assert _same_bits(other, b, res, NAMES.index(name)), name


# --- status bits from doctored operations ------------------------------------------------------------------------------------
TEXT = {ref.STATUS_INPUT: "no symmetry operations to work from (sym does not describe it)",
        ref.STATUS_TRANSLATIONS: "its pure translations form no lattice within symprec",
        ref.STATUS_RANGE: "the cell needs lattice vectors beyond", ref.STATUS_REDUCE: "its operations give no cell",
        ref.STATUS_ATOMS: "the new cell has more than"}
TABLE = ref.table()


def _pure_translations(sym, b):
    """The rows, within structure b, of its operations with W = I."""
    rot = _operations(sym, b)["rotations"]
    return [g for g, W in enumerate(rot) if np.array_equal(W, np.eye(3, dtype=np.int64))]


def _doctored(how):
    """-> (the three structures, their SymmetryResult, a copy with the operations of structure 1 doctored)."""
    rows = [TABLE[n] for n in ("hcp", "bcc_cube" if how in ("translation", "atom_map_identity") else "cscl", "wurtzite")]
    sym = find_symmetry(*_lists(rows), device=DEV)
    if how == "foreign":  # the operations of another two-atom structure, with their own row pointers
        bad = find_symmetry(*_lists([rows[0], TABLE["bcc_cube"], rows[2]]), device=DEV)
        assert bad.ns == sym.ns and bad.n_ops[1] != sym.n_ops[1]
        return rows, sym, bad
    pk = dict(sym.packed)
    for key in ("rotations", "translations", "atom_map"):
        pk[key] = pk[key].clone()
    n, op0, map0 = sym.ns[1], int(pk["op_ptr"][1]), int(pk["map_ptr"][1])
    pure = _pure_translations(sym, 1)
    if how == "atom_map":  # one entry of the identity's row set to n: past the atoms
        assert len(pure) == 1
        pk["atom_map"][map0 + pure[0] * n + 0] = n
    elif how == "translation":  # the centring translation moved by 3 symprec along a
        assert len(pure) == 2
        g = next(g for g in pure if float(pk["translations"][op0 + g].abs().max()) > 0.25)
        pk["translations"][op0 + g, 0] += 3.0 * 1e-3 / float(np.linalg.norm(rows[1][0][0]))
    elif how == "atom_map_identity":  # the centring translation said to map every atom onto itself: n_prim n_t = 4 != 2
        g = next(g for g in pure if float(pk["translations"][op0 + g].abs().max()) > 0.25)
        pk["atom_map"][map0 + g * n:map0 + (g + 1) * n] = torch.arange(n, dtype=torch.int32, device=pk["atom_map"].device)
    return rows, sym, dataclasses.replace(sym, packed=pk)


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("how", ["atom_map", "translation", "atom_map_identity", "foreign"])
def test_doctored_operations_set_the_status_of_the_restatement(fn, how):
    """``foreign``: a structure's rotations written in any basis of its lattice are a group of integer matrices of one of the
    arithmetic classes, so the operations of another two-atom structure give a cell (of that structure's kind) on both sides and
    nothing raises: there the device must return what the restatement returns from the same operations.  The status of
    ``n_prim * n_t != n`` comes from ``atom_map_identity``."""
    rows, sym, bad = _doctored(how)
    A, pos, z = rows[1][:3]
    status, want = 0, None
    try:
        want = getattr(ref, fn.__name__)(A, pos, z, 1e-3, sym=_operations(bad, 1))
    except ref.CellError as e:
        status = e.status
    assert (status != 0) == (how != "foreign")
    assert status == {"atom_map": ref.STATUS_INPUT, "translation": ref.STATUS_TRANSLATIONS, "atom_map_identity": ref.STATUS_INPUT,
                      "foreign": 0}[how]
    good = fn(*_lists(rows), sym=sym, device=DEV)
    if status:
        with pytest.raises(ValueError) as err:
            fn(*_lists(rows), sym=bad, device=DEV)
        text = str(err.value)
        assert f"structure 1: {TEXT[status]}" in text and "structure 0" not in text and "structure 2" not in text
        assert text.count("structure 1:") == 1
        part = err.value.result
        assert part.ns[1] == 0 and part.multiplicity[1] == 0 and part.positions[1].shape == (0, 3)
    else:
        part = fn(*_lists(rows), sym=bad, device=DEV)
        assert want["margin"] >= MARGIN  # (the atoms of these three lie on faces of their cells: the positions are not compared)
        assert np.array_equal(part.transform_num[1].cpu().numpy(), want["transform_num"])
        assert np.array_equal(part.source_atom[1].cpu().numpy(), want["source_atom"])
        assert (part.transform_den[1], part.multiplicity[1], part.centring[1], part.crystal_system[1], part.ns[1]) == \
            (want["transform_den"], want["multiplicity"], want["centring"], want["crystal_system"], len(want["positions"]))
        assert np.abs(part.lattices[1].cpu().numpy() - want["lattice"]).max() <= ATOL
    assert _same_bits(part, 0, good, 0) and _same_bits(part, 2, good, 2)
