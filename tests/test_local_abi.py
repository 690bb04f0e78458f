"""CPU-side checks of include/alignn_local.h, a header added after ``_abi.WORKFLOW_HEADERS``: it reads with the reader of
alignn_amd/_abi.py, the built library exports exactly the names it declares (no compute calls - there is no GPU here), the ctypes
layout of its argument blocks agrees with a C compiler's sizeof / offsetof and with the library's size queries, its limits are
those of alignn_order.h by value, and every entry point refuses an argument out of range before it looks at a pointer."""

import ctypes as C
import os

import alignn_amd
from alignn_amd import _abi, _lib, local_order, order
from alignn_amd.local_order import HEADER, SIGNATURES, STRUCTS, BondArgs, CnaArgs, _load
from tests import abi_checks

ENTRY = (C.c_int, [C.c_void_p, C.c_void_p])


def test_header_reads_and_the_library_exports_it():
    from alignn_amd.build import SOURCES, _headers, build

    assert "local_order.hip" in SOURCES and HEADER in [os.path.normpath(h) for h in _headers()]  # (an edit rebuilds the library)
    assert "alignn_local.h" in _abi.LATER_HEADERS and not set(_abi.LATER_HEADERS) & set(_abi.WORKFLOW_HEADERS)
    build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_local_cna_args", "alignn_local_bond_args"] == list(STRUCTS)
    assert set(sigs) == abi_checks.declared(HEADER) == set(SIGNATURES) == {
        "alignn_local_cna", "alignn_local_cna_counts", "alignn_local_cna_args_size", "alignn_local_bond_qlm",
        "alignn_local_bond_finish", "alignn_local_bond_args_size"}
    assert all(name.startswith("alignn_local_") for name in list(structs) + list(sigs))
    lib = _load()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    assert abi_checks.exported(_lib.LIB_PATH, "alignn_local_") == set(sigs)
    for name, sig in sigs.items():
        assert sig == ((C.c_size_t, []) if name.endswith("_size") else ENTRY), name


def test_the_package_exports_the_functions_and_results():
    assert alignn_amd.cna is local_order.cna and alignn_amd.bond_order is local_order.bond_order
    assert alignn_amd.CNAResult is local_order.CNAResult and alignn_amd.BondOrderResult is local_order.BondOrderResult


def test_limits_are_those_of_the_order_header_by_value():
    d, o = _abi.header("alignn_local.h").defines, _abi.header("alignn_order.h").defines
    for name in ("MAX_SPECIES", "MAX_IMAGE_RANGE", "MAX_NEIGHBORS", "MAX_L", "MAX_LS", "STATUS_IMAGES", "STATUS_NEIGHBORS"):
        assert d["ALIGNN_LOCAL_" + name] == o["ALIGNN_ORDER_" + name], name
    assert d["ALIGNN_LOCAL_CLASSES"] == len(local_order.CLASSES) == 5 and d["ALIGNN_LOCAL_SIGNATURES"] == len(local_order.SIGNATURES_COUNTED)
    assert d["ALIGNN_LOCAL_M_STRIDE"] == d["ALIGNN_LOCAL_MAX_L"] + 1 and d["ALIGNN_LOCAL_W3J_STRIDE"] == (2 * d["ALIGNN_LOCAL_MAX_L"] + 1) ** 2
    assert len(d) == 11 and local_order.MAX_NEIGHBORS == order.MAX_NEIGHBORS == 64
    assert local_order.ylm_norms().shape == (13, 13) and local_order.wigner_3j_table(12).size == d["ALIGNN_LOCAL_W3J_STRIDE"]


def test_argument_block_sizes_match_the_library():
    lib = _load()
    assert lib.alignn_local_cna_args_size() == C.sizeof(CnaArgs) == 12 * 8 + 10 * 4
    assert lib.alignn_local_bond_args_size() == C.sizeof(BondArgs) == 19 * 8 + 17 * 4 + 4  # (the padding of the last int)
    blank = BondArgs()
    assert blank.qlm is None and blank.n_ls == 0 and CnaArgs().adaptive == 0  # a field left out is NULL / 0


def test_argument_block_layouts_match_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_local.h", STRUCTS, tmp_path)
    assert len(want) == (1 + 22) + (1 + 36) and seen == want


FRAMES = dict(n_total_frames=4, frame0=0, frame_step=1, n_frames=4)
BAD_FRAMES = (dict(n_total_frames=-1), dict(frame0=-1), dict(frame_step=0), dict(n_frames=-1), dict(n_frames=5), dict(frame0=1),
              dict(frame_step=2))
BAD_COMMON = (dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_species=0), dict(n_species=9),
              dict(lattice_per_frame=2), dict(lattice_per_frame=-1))


def test_cna_entry_points_refuse_arguments_out_of_range():
    """The range checks come before any launch and before any pointer is looked at: every pointer is NULL here."""
    lib = _load()
    good = dict(n_structs=1, n_atoms=2, max_atoms=2, n_species=1, **FRAMES)
    for entry in (lib.alignn_local_cna, lib.alignn_local_cna_counts):
        assert entry(None, None) == 1  # hipErrorInvalidValue
        for bad in BAD_COMMON + BAD_FRAMES + (dict(adaptive=2), dict(adaptive=-1)):
            assert entry(C.byref(CnaArgs(**{**good, **bad})), None) == 1, bad
        assert entry(C.byref(CnaArgs(**good)), None) == 1  # in range, and the pointers are needed
        assert entry(C.byref(CnaArgs(**{**good, "n_structs": 0})), None) == 0  # no structures: nothing to do
        assert entry(C.byref(CnaArgs(**{**good, "n_frames": 0})), None) == 0  # no frame selected: nothing to do
    for bad in (dict(n_atoms=0), dict(max_atoms=0), dict(max_atoms=3), dict(max_atoms=65536, n_atoms=70000)):
        assert lib.alignn_local_cna(C.byref(CnaArgs(**{**good, **bad})), None) == 1, bad
    pointers = {name: 8 for name, kind in CnaArgs._fields_ if kind is C.c_void_p}  # (never followed: a NULL among them fails first)
    assert len(pointers) == 12
    for name in set(pointers) - {"counts", "fraction"}:
        assert lib.alignn_local_cna(C.byref(CnaArgs(**{**pointers, **good, name: None})), None) == 1, name
    for name in ("atom_ptr", "group", "group_count", "structure", "counts", "fraction"):
        assert lib.alignn_local_cna_counts(C.byref(CnaArgs(**{**pointers, **good, name: None})), None) == 1, name


def test_bond_entry_points_refuse_arguments_out_of_range():
    lib = _load()
    good = dict(n_structs=1, n_atoms=2, max_atoms=2, n_species=1, chunk0=0, chunk_frames=4, n_ls=2, l0=4, l1=6, **FRAMES)
    pointers = {name: 8 for name, kind in BondArgs._fields_ if kind is C.c_void_p}
    assert len(pointers) == 19
    for entry in (lib.alignn_local_bond_qlm, lib.alignn_local_bond_finish):
        assert entry(None, None) == 1
        for bad in BAD_COMMON + BAD_FRAMES + (dict(average=2), dict(average=-1), dict(n_ls=0), dict(n_ls=5), dict(l0=0), dict(l1=13),
                                              dict(l1=4), dict(n_ls=3, l2=0), dict(chunk0=-1), dict(chunk0=5), dict(chunk_frames=-1),
                                              dict(chunk_frames=5), dict(chunk0=2, chunk_frames=3)):
            assert entry(C.byref(BondArgs(**{**good, **bad})), None) == 1, bad
        assert entry(C.byref(BondArgs(**good)), None) == 1  # in range, and the pointers are needed
        for nothing in (dict(n_structs=0), dict(n_frames=0, chunk_frames=0), dict(chunk_frames=0), dict(chunk0=4, chunk_frames=0)):
            assert entry(C.byref(BondArgs(**{**good, **nothing})), None) == 0, nothing
        for bad in (dict(n_atoms=0), dict(max_atoms=0), dict(max_atoms=3)):
            assert entry(C.byref(BondArgs(**{**pointers, **good, **bad})), None) == 1, bad
    for name in ("traj", "lattice", "atom_ptr", "group", "group_count", "r_cut", "ynorm", "qlm", "n_neighbors", "status"):
        assert lib.alignn_local_bond_qlm(C.byref(BondArgs(**{**pointers, **good, name: None})), None) == 1, name
    for name in ("traj", "lattice", "atom_ptr", "group", "group_count", "r_cut", "w3j", "qlm", "s", "t", "q", "w"):
        assert lib.alignn_local_bond_finish(C.byref(BondArgs(**{**pointers, **good, name: None})), None) == 1, name
    for name in ("s_avg", "t_avg", "q_avg", "w_avg"):  # needed with average = 1 only
        assert lib.alignn_local_bond_finish(C.byref(BondArgs(**{**pointers, **good, "average": 1, name: None})), None) == 1, name
