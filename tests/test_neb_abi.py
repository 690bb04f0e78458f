"""CPU-side checks of the third header, include/alignn_neb.h: it reads with the reader of alignn_amd/_abi.py, the built library
exports every name it declares (no compute calls - there is no GPU here), and the ctypes layout of its argument block agrees
with a C compiler's sizeof / offsetof and with the library's size query."""

import ctypes as C

from alignn_amd import _abi, _lib
from alignn_amd.neb import HEADER, MAX_IMAGES, SIGNATURES, STRUCTS, NebArgs, _load
from tests import abi_checks


def test_header_reads_and_the_library_exports_it():
    from alignn_amd.build import SOURCES, build

    assert "neb.hip" in SOURCES
    build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_neb_args"] == list(STRUCTS)
    assert set(sigs) == abi_checks.declared(HEADER) == set(SIGNATURES) == {"alignn_neb_interpolate", "alignn_neb_forces",
                                                                  "alignn_neb_args_size"}
    lib = _load()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    assert sigs["alignn_neb_forces"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert sigs["alignn_neb_args_size"] == (C.c_size_t, [])
    assert sigs["alignn_neb_interpolate"] == (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p])
    assert MAX_IMAGES == 64


def test_argument_block_size_matches_the_library():
    assert _load().alignn_neb_args_size() == C.sizeof(NebArgs) == 20 * 8 + 4 * 4
    blank = NebArgs()
    assert blank.fixed is None and blank.n_active == 0  # a field left out is NULL / 0


def test_entry_points_refuse_arguments_out_of_range():
    """The checks that come before any launch: no device is touched."""
    lib = _load()
    assert lib.alignn_neb_forces(None, None) == 1  # hipErrorInvalidValue
    for bad in (dict(max_images=2), dict(max_images=MAX_IMAGES + 1), dict(method=2), dict(climb=2), dict(n_active=-1), dict()):
        args = NebArgs(**{**dict(n_active=1, max_images=5, method=0, climb=0), **bad})  # (dict(): every pointer NULL)
        assert lib.alignn_neb_forces(C.byref(args), None) == 1, bad
    assert lib.alignn_neb_interpolate(None, None, None, None, None, -1, 0, None, None, None) == 1
    assert lib.alignn_neb_interpolate(None, None, None, None, None, 1, 4, None, None, None) == 1
    assert lib.alignn_neb_interpolate(None, None, None, None, None, 0, 0, None, None, None) == 0  # nothing to do


def test_argument_block_layout_matches_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_neb.h", STRUCTS, tmp_path)
    assert len(want) == 25 and seen == want
