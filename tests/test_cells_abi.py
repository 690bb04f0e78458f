"""CPU-side checks of include/alignn_cells.h, a header added after ``_abi.WORKFLOW_HEADERS``: it reads with the reader of
alignn_amd/_abi.py, the built library exports exactly the names it declares (no compute calls - there is no GPU here), the ctypes
layout of its argument block agrees with a C compiler's sizeof / offsetof and with the library's size query, and the limits come
from the header.  And the checks of the drivers that need no GPU: the arguments of ``primitive_cell`` / ``conventional_cell`` and
of ``on_conventional_cell`` in ``vacancy_formation`` and ``surface_energy``."""

import ctypes as C
import os

import numpy as np
import pytest

from alignn_amd import _abi, _lib, cells, conventional_cell, primitive_cell, surface_energy, symmetry, vacancy_formation
from alignn_amd.cells import HEADER, SIGNATURES, STRUCTS, CellsArgs, _load
from tests import abi_checks, cells_ref


def test_header_reads_and_the_library_exports_it():
    from alignn_amd.build import SOURCES, _headers, build

    assert "cells.hip" in SOURCES and HEADER in [os.path.normpath(h) for h in _headers()]  # (an edit of it rebuilds the library)
    assert "alignn_cells.h" in _abi.LATER_HEADERS and not set(_abi.LATER_HEADERS) & set(_abi.WORKFLOW_HEADERS)
    build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_cells_args"] == list(STRUCTS)
    assert set(sigs) == abi_checks.declared(HEADER) == set(SIGNATURES) == {"alignn_cells_reduce", "alignn_cells_fill",
                                                                           "alignn_cells_args_size"}
    lib = _load()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    assert abi_checks.exported(_lib.LIB_PATH, "alignn_cells_") == set(sigs)
    assert sigs["alignn_cells_reduce"] == sigs["alignn_cells_fill"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert sigs["alignn_cells_args_size"] == (C.c_size_t, [])


def test_limits_are_read_from_the_header():
    d = _abi.header("alignn_cells.h").defines
    assert d == {"ALIGNN_CELLS_MAX_ATOMS": 1024, "ALIGNN_CELLS_MAX_IMAGE_RANGE": 8, "ALIGNN_CELLS_MAX_ROTATIONS": 48,
                 "ALIGNN_CELLS_INFO": 8, "ALIGNN_CELLS_STATUS_SYMMETRY": 1, "ALIGNN_CELLS_STATUS_TRANSLATIONS": 2,
                 "ALIGNN_CELLS_STATUS_RANGE": 4, "ALIGNN_CELLS_STATUS_REDUCE": 8, "ALIGNN_CELLS_STATUS_ATOMS": 16}
    assert cells.MAX_ATOMS == d["ALIGNN_CELLS_MAX_ATOMS"] == symmetry.MAX_ATOMS == cells_ref.MAX_ATOMS
    assert cells.MAX_IMAGE_RANGE == d["ALIGNN_CELLS_MAX_IMAGE_RANGE"] == cells_ref.MAX_IMAGE_RANGE
    assert d["ALIGNN_CELLS_MAX_ROTATIONS"] == symmetry.MAX_LATTICE_OPS and cells.INFO == 8
    assert (cells.STATUS_SYMMETRY, cells.STATUS_TRANSLATIONS, cells.STATUS_RANGE, cells.STATUS_REDUCE, cells.STATUS_ATOMS) == \
        (cells_ref.STATUS_INPUT, cells_ref.STATUS_TRANSLATIONS, cells_ref.STATUS_RANGE, cells_ref.STATUS_REDUCE, cells_ref.STATUS_ATOMS)
    assert cells.CENTRINGS == cells_ref.CENTRINGS == "PIFABCR"


def test_argument_block_size_matches_the_library():
    assert _load().alignn_cells_args_size() == C.sizeof(CellsArgs) == 17 * 8 + 8 + 3 * 8 + 4 * 4
    blank = CellsArgs()
    assert blank.lattice is None and blank.n_structs == 0 and blank.conventional == 0


def test_argument_block_layout_matches_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_cells.h", STRUCTS, tmp_path)
    assert len(want) == 26 and seen == want


def test_entry_points_refuse_arguments_out_of_range():
    """The checks that come before any launch: no device is touched."""
    lib = _load()
    pointers = {name: 8 for name, kind in CellsArgs._fields_ if kind is C.c_void_p}  # (never followed: the scalars fail first)
    assert len(pointers) == 17
    good = dict(symprec=1e-3, n_ops_total=1, n_map_total=1, n_out_total=1, n_structs=1, n_atoms=1, conventional=1, max_out=1)
    for entry in (lib.alignn_cells_reduce, lib.alignn_cells_fill):
        assert entry(None, None) == 1  # hipErrorInvalidValue
        for bad in (dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_atoms=0), dict(symprec=0.0),
                    dict(symprec=float("nan")), dict(symprec=float("inf")), dict(conventional=2), dict(conventional=-1),
                    dict(n_ops_total=-1), dict(n_map_total=-1)):
            assert entry(C.byref(CellsArgs(**{**pointers, **good, **bad})), None) == 1, bad
        for name in ("lattice", "pos", "atom_ptr", "op_ptr", "map_ptr", "rotations", "translations", "atom_map", "info",
                     "transform_num", "transform_den", "cells", "points", "reps"):
            assert entry(C.byref(CellsArgs(**{**pointers, **good, name: None})), None) == 1, name
        assert entry(C.byref(CellsArgs(**{**pointers, **good, "n_structs": 0})), None) == 0  # nothing to do
    for bad in (dict(n_out_total=-1), dict(max_out=-1), dict(max_out=1025, n_out_total=2000), dict(max_out=2), dict(out_ptr=None),
                dict(out_pos=None), dict(source_atom=None)):
        assert lib.alignn_cells_fill(C.byref(CellsArgs(**{**pointers, **good, **bad})), None) == 1, bad
    assert lib.alignn_cells_fill(C.byref(CellsArgs(**{**pointers, **good, "n_out_total": 0, "max_out": 0})), None) == 0


# --- the drivers' checks that need no GPU ------------------------------------------------------------------------------------------
A = 3.6 * np.array([[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]])
POS = np.zeros((1, 3))


@pytest.mark.parametrize("fn", [primitive_cell, conventional_cell])
def test_ragged_inputs_raise(fn):
    with pytest.raises(ValueError, match="need the same number"):
        fn([A, A], [POS])
    with pytest.raises(ValueError, match="need the same number"):
        fn([], [])
    with pytest.raises(ValueError, match=r"positions\[1\]"):
        fn([A, A], [POS, np.zeros((2, 2))])
    with pytest.raises(ValueError, match=r"lattices\[0\]"):
        fn([np.eye(2)], [POS])
    with pytest.raises(ValueError, match="species needs one"):
        fn([A], [POS], [[1], [2]])
    with pytest.raises(ValueError, match=r"species\[0\]"):
        fn([A], [POS], [np.array([1, 2])])
    with pytest.raises(ValueError, match="1025 atoms"):
        fn([A], [np.zeros((1025, 3))])
    for symprec in (0.0, -1.0, float("nan"), True, "1e-3"):
        with pytest.raises(ValueError, match="symprec"):
            fn([A], [POS], symprec=symprec)
    with pytest.raises(ValueError, match="sym must be the SymmetryResult"):
        fn([A], [POS], sym=object())


def test_on_conventional_cell_is_one_bool_and_checks_its_inputs_first():
    fn = lambda lats, poss: None  # (never called: every check below comes before any device work)
    for flag in (1, 0, "yes", None, [True]):
        with pytest.raises(ValueError, match="on_conventional_cell is one bool"):
            vacancy_formation(None, [A], [POS], forces_fn=fn, on_conventional_cell=flag)
        with pytest.raises(ValueError, match="on_conventional_cell is one bool"):
            surface_energy(None, [A], [POS], miller_indices=[(1, 0, 0)], forces_fn=fn, on_conventional_cell=flag)
    with pytest.raises(ValueError, match="need the same number"):
        vacancy_formation(None, [A, A], [POS], forces_fn=fn, on_conventional_cell=True)
    with pytest.raises(ValueError, match=r"positions\[0\]"):
        surface_energy(None, [A], [np.zeros((3,))], miller_indices=[(1, 0, 0)], forces_fn=fn, on_conventional_cell=True)
    with pytest.raises(ValueError, match=r"species\[0\]"):
        surface_energy(None, [A], [POS], miller_indices=[(1, 0, 0)], forces_fn=fn, on_conventional_cell=True, species=[np.array([1, 2])])
    with pytest.raises(ValueError, match=r"site_labels\[0\]"):
        vacancy_formation(None, [A], [POS], forces_fn=fn, on_conventional_cell=True, site_labels=[np.array([0, 1])])
