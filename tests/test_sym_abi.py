"""CPU-side checks of the fifth header, include/alignn_sym.h: it reads with the reader of alignn_amd/_abi.py, the built library
exports exactly the names it declares (no compute calls - there is no GPU here), the
ctypes layout of its argument blocks agrees with a C compiler's sizeof / offsetof and with the library's size queries, and
every range check answers hipErrorInvalidValue before anything touches a device."""

import ctypes as C
import os

from alignn_amd import _abi, _lib
from alignn_amd.symmetry import (HEADER, INFO, MAX_ATOMS, MAX_CANDIDATES, MAX_IMAGE_RANGE, MAX_LATTICE_OPS, SIGNATURES,
                                 STATUS_IMAGES, STATUS_INPUT, STATUS_OVERFLOW, STRUCTS, ApplyArgs, FindArgs, _load)
from tests import abi_checks

NAMES = {"alignn_sym_search", "alignn_sym_fill", "alignn_sym_find_args_size", "alignn_sym_forces", "alignn_sym_stress",
         "alignn_sym_positions", "alignn_sym_apply_args_size"}


def test_header_reads_and_the_library_exports_exactly_its_names():
    from alignn_amd.build import SOURCES, _headers, build

    assert "symmetry.hip" in SOURCES and HEADER in [os.path.normpath(h) for h in _headers()]
    lib_path = build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_sym_find_args", "alignn_sym_apply_args"] == list(STRUCTS)
    assert set(sigs) == abi_checks.declared(HEADER) == set(SIGNATURES) == NAMES
    assert abi_checks.exported(lib_path, "alignn_sym_") == NAMES  # nothing of the prefix beside what the header declares
    lib = _load()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    for name in NAMES - {"alignn_sym_find_args_size", "alignn_sym_apply_args_size"}:
        assert sigs[name] == (C.c_int, [C.c_void_p, C.c_void_p]), name
    assert sigs["alignn_sym_find_args_size"] == sigs["alignn_sym_apply_args_size"] == (C.c_size_t, [])
    assert (MAX_ATOMS, MAX_IMAGE_RANGE, MAX_CANDIDATES, MAX_LATTICE_OPS, INFO) == (1024, 8, 256, 48, 8)
    assert (STATUS_IMAGES, STATUS_OVERFLOW, STATUS_INPUT) == (1, 2, 4)


def test_argument_block_sizes_match_the_library():
    lib = _load()
    assert lib.alignn_sym_find_args_size() == C.sizeof(FindArgs) == 23 * 8 + 4 * 4
    assert lib.alignn_sym_apply_args_size() == C.sizeof(ApplyArgs) == 12 * 8 + 2 * 4
    blank = FindArgs()
    assert blank.pos is None and blank.n_structs == 0 and blank.symprec == 0.0  # a field left out is NULL / 0


FIND_OK = dict(symprec=1e-3, n_structs=1, n_atoms=4, max_atoms=4, n_ops_total=0, n_map_total=0)
APPLY_OK = dict(n_structs=1, n_atoms=4, n_ops_total=2, n_map_total=8)


def test_entry_points_refuse_arguments_out_of_range():
    """The checks that come before any launch, every pointer NULL: no device is touched."""
    lib = _load()
    finds, applies = (lib.alignn_sym_search, lib.alignn_sym_fill), (lib.alignn_sym_forces, lib.alignn_sym_stress, lib.alignn_sym_positions)
    for fn in finds + applies:
        assert fn(None, None) == 1  # hipErrorInvalidValue
    nan, inf = float("nan"), float("inf")
    find_bad = [dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_atoms=0), dict(symprec=0.0), dict(symprec=-1e-3),
                dict(symprec=nan), dict(symprec=inf), dict(max_atoms=0), dict(max_atoms=5), dict(max_atoms=-1),
                dict(n_atoms=2000, max_atoms=MAX_ATOMS + 1), dict()]  # (dict(): in range, but every pointer NULL)
    for bad in find_bad:
        args = FindArgs(**{**FIND_OK, **bad})
        for fn in finds:
            assert fn(C.byref(args), None) == 1, bad
    for bad in (dict(n_ops_total=-1), dict(n_map_total=-1)):
        assert lib.alignn_sym_fill(C.byref(FindArgs(**{**FIND_OK, **bad})), None) == 1, bad
    apply_bad = [dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_ops_total=-1), dict(n_map_total=-1), dict()]
    for bad in apply_bad:
        args = ApplyArgs(**{**APPLY_OK, **bad})
        for fn in applies:
            assert fn(C.byref(args), None) == 1, bad
    # nothing to do: no structures
    for fn in finds:
        assert fn(C.byref(FindArgs(**{**FIND_OK, "n_structs": 0})), None) == 0
    for fn in applies:
        assert fn(C.byref(ApplyArgs(**{**APPLY_OK, "n_structs": 0})), None) == 0


def test_argument_block_layouts_match_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_sym.h", STRUCTS, tmp_path)
    assert len(want) == 2 + 26 + 14 and seen == want
