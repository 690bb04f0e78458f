"""CPU-side checks of include/alignn_idpp.h, the first of the headers added after ``_abi.WORKFLOW_HEADERS``: it reads with the
reader of alignn_amd/_abi.py, the built library exports exactly the names it declares (no compute calls - there is no GPU here),
and the ctypes layout of its argument block agrees with a C compiler's sizeof / offsetof and with the library's size query."""

import ctypes as C
import os

from alignn_amd import _abi, _lib
from alignn_amd.idpp import HEADER, SIGNATURES, STRUCTS, IdppArgs, _load
from alignn_amd.neb import MAX_IMAGES
from tests import abi_checks


def test_header_reads_and_the_library_exports_it():
    from alignn_amd.build import SOURCES, _headers, build

    assert "idpp.hip" in SOURCES and HEADER in [os.path.normpath(h) for h in _headers()]  # (an edit of it rebuilds the library)
    assert "alignn_idpp.h" in _abi.LATER_HEADERS and not set(_abi.LATER_HEADERS) & set(_abi.WORKFLOW_HEADERS)
    build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_idpp_args"] == list(STRUCTS)
    assert set(sigs) == abi_checks.declared(HEADER) == set(SIGNATURES) == {"alignn_idpp_forces", "alignn_idpp_args_size"}
    lib = _load()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    assert abi_checks.exported(_lib.LIB_PATH, "alignn_idpp_") == set(sigs)
    assert sigs["alignn_idpp_forces"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert sigs["alignn_idpp_args_size"] == (C.c_size_t, [])
    assert _abi.header("alignn_idpp.h").defines == {}  # (the image limit is alignn_neb.h's)


def test_no_name_of_a_later_header_is_in_another_header():
    earlier = [(_abi.STRUCTS, _abi.SIGNATURES)] + [(_abi.header(n).structs, _abi.header(n).signatures) for n in _abi.WORKFLOW_HEADERS]
    for name in _abi.LATER_HEADERS:
        H = _abi.header(name)
        mine = set(H.structs) | set(H.signatures)
        for structs, sigs in earlier:
            assert not mine & (set(structs) | set(sigs)), name
        earlier.append((H.structs, H.signatures))


def test_argument_block_size_matches_the_library():
    assert _load().alignn_idpp_args_size() == C.sizeof(IdppArgs) == 14 * 8 + 4 * 4  # (3 ints and the padding of the last)
    blank = IdppArgs()
    assert blank.positions is None and blank.n_active == 0  # a field left out is NULL / 0


def test_entry_point_refuses_arguments_out_of_range():
    """The checks that come before any launch: no device is touched."""
    lib = _load()
    assert lib.alignn_idpp_forces(None, None) == 1  # hipErrorInvalidValue
    pointers = {name: 8 for name, kind in IdppArgs._fields_ if kind is C.c_void_p}  # (never followed: the scalars fail first)
    assert len(pointers) == 14
    for bad in (dict(max_images=2), dict(max_images=MAX_IMAGES + 1), dict(max_atoms=0), dict(n_active=-1), dict(n_active=65536)):
        args = IdppArgs(**{**pointers, **dict(n_active=1, max_images=5, max_atoms=8), **bad})
        assert lib.alignn_idpp_forces(C.byref(args), None) == 1, bad
    for name in pointers:  # every pointer is needed
        args = IdppArgs(**{**pointers, name: None}, n_active=1, max_images=5, max_atoms=8)
        assert lib.alignn_idpp_forces(C.byref(args), None) == 1, name
    args = IdppArgs(**pointers, n_active=0, max_images=3, max_atoms=1)
    assert lib.alignn_idpp_forces(C.byref(args), None) == 0  # nothing to do


def test_argument_block_layout_matches_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_idpp.h", STRUCTS, tmp_path)
    assert len(want) == 18 and seen == want
