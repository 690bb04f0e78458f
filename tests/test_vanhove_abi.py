"""CPU-side checks of include/alignn_vanhove.h, a header of ``_abi.ANALYSIS_HEADERS``: it reads with the reader of
alignn_amd/_abi.py, the built library exports exactly the names it declares (no compute calls - there is no GPU here), the ctypes
layout of its argument blocks agrees with a C compiler's sizeof / offsetof and with the library's size queries, the limits it
shares with alignn_traj.h and alignn_order.h are theirs by value, every entry point refuses an argument out of range before it
looks at a device pointer, and tests/vanhove_extents.py names every pointer field with an extent over the struct's own scalars."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import alignn_amd
from alignn_amd import _abi, _lib, order, trajectory, vanhove
from alignn_amd.vanhove import HEADER, SIGNATURES, STRUCTS, DistinctArgs, FqtArgs, SelfArgs, _load
from tests import abi_checks
from tests import gate_parity as gp
from tests import vanhove_extents as vx
from tests import workflow_extents as wx

ENTRY = (C.c_int, [C.c_void_p, C.c_void_p])
ENTRIES = {"alignn_vh_self", "alignn_vh_self_finish", "alignn_vh_distinct", "alignn_vh_distinct_finish", "alignn_vh_fqt_modes",
           "alignn_vh_fqt_correlate", "alignn_vh_fqt_bin"}
SIZES = {"alignn_vh_self_args_size", "alignn_vh_distinct_args_size", "alignn_vh_fqt_args_size"}


def test_header_reads_and_the_library_exports_it():
    from alignn_amd.build import SOURCES, _headers, build

    assert "vanhove.hip" in SOURCES and HEADER in [os.path.normpath(h) for h in _headers()]  # (an edit rebuilds the library)
    assert _abi.ANALYSIS_HEADERS == ("alignn_vanhove.h",)
    assert not set(_abi.ANALYSIS_HEADERS) & (set(_abi.WORKFLOW_HEADERS) | set(_abi.LATER_HEADERS))
    build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_vh_self_args", "alignn_vh_distinct_args", "alignn_vh_fqt_args"] == list(STRUCTS)
    assert set(sigs) == abi_checks.declared(HEADER) == set(SIGNATURES) == ENTRIES | SIZES
    assert all(name.startswith("alignn_vh_") for name in list(structs) + list(sigs))
    lib = _load()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    assert abi_checks.exported(_lib.LIB_PATH, "alignn_vh_") == set(sigs)
    for name, sig in sigs.items():
        assert sig == ((C.c_size_t, []) if name.endswith("_size") else ENTRY), name


def test_the_older_headers_declare_what_they_declared():
    """the entry points of the three headers whose kernels now share code with vanhove.hip"""
    assert set(_abi.header("alignn_traj.h").signatures) == {
        "alignn_traj_rdf_counts", "alignn_traj_rdf_normalise", "alignn_traj_rdf_args_size", "alignn_traj_com", "alignn_traj_corr",
        "alignn_traj_corr_args_size", "alignn_traj_vdos", "alignn_traj_fit", "alignn_traj_green_kubo"}
    assert set(_abi.header("alignn_order.h").signatures) == {
        "alignn_order_angles", "alignn_order_adf_finish", "alignn_order_steinhardt_mean", "alignn_order_angle_args_size",
        "alignn_order_sq_vectors", "alignn_order_sq_accumulate", "alignn_order_sq_bin", "alignn_order_sq_args_size"}
    assert set(_abi.header("alignn_local.h").signatures) == {
        "alignn_local_cna", "alignn_local_cna_counts", "alignn_local_cna_args_size", "alignn_local_bond_qlm",
        "alignn_local_bond_finish", "alignn_local_bond_args_size"}


def test_the_package_exports_the_functions_and_results():
    for name in ("van_hove_self", "van_hove_distinct", "intermediate_scattering", "VanHoveSelfResult", "VanHoveDistinctResult", "FqtResult"):
        assert getattr(alignn_amd, name) is getattr(vanhove, name) and name in vanhove.__all__, name
    assert order.reciprocal_vectors.__name__ == "reciprocal_vectors"


def test_limits_are_those_of_the_older_headers_by_value():
    d, t, o = _abi.header("alignn_vanhove.h").defines, _abi.header("alignn_traj.h").defines, _abi.header("alignn_order.h").defines
    for name in ("MAX_SPECIES", "MAX_BINS", "MAX_IMAGE_RANGE", "STATUS_IMAGES"):
        assert d["ALIGNN_VH_" + name] == t["ALIGNN_TRAJ_" + name], name
    assert d["ALIGNN_VH_MAX_HKL"] == o["ALIGNN_ORDER_MAX_HKL"] and d["ALIGNN_VH_MAX_Q_BINS"] == o["ALIGNN_ORDER_MAX_BINS"]
    assert d["ALIGNN_VH_MAX_SPECIES"] == o["ALIGNN_ORDER_MAX_SPECIES"] and d["ALIGNN_VH_FQT_FRAME_CHUNK"] == o["ALIGNN_ORDER_SQ_FRAME_CHUNK"]
    assert d["ALIGNN_VH_MAX_LAGS"] == vanhove.MAX_LAGS == 1024 and d["ALIGNN_VH_MAX_Q"] == vanhove.MAX_Q == 16 and len(d) == 9
    assert vanhove.MAX_BINS == trajectory.MAX_BINS == 4096 and vanhove.MAX_Q_BINS == order.MAX_BINS == 1024


def test_argument_block_sizes_match_the_library():
    lib = _load()
    assert lib.alignn_vh_self_args_size() == C.sizeof(SelfArgs) == 19 * 8 + 11 * 4 + 4  # (the padding of the last int)
    assert lib.alignn_vh_distinct_args_size() == C.sizeof(DistinctArgs) == 14 * 8 + 12 * 4
    assert lib.alignn_vh_fqt_args_size() == C.sizeof(FqtArgs) == 16 * 8 + 13 * 4 + 4
    blank = SelfArgs()
    assert blank.com is None and blank.n_q == 0 and DistinctArgs().lattice_per_frame == 0  # a field left out is NULL / 0


def test_argument_block_layouts_match_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_vanhove.h", STRUCTS, tmp_path)
    assert len(want) == (1 + 30) + (1 + 26) + (1 + 29) and seen == want


FRAMES = dict(n_total_frames=4, frame0=0, frame_step=1, n_frames=4)
BAD_FRAMES = (dict(n_total_frames=-1), dict(frame0=-1), dict(frame_step=0), dict(n_frames=-1), dict(n_frames=5), dict(frame0=1),
              dict(frame_step=2))
BAD_COMMON = (dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_species=0), dict(n_species=9), dict(n_lags=0),
              dict(n_lags=1025), dict(origin_stride=0), dict(origin_stride=-1), dict(n_bins=0))
BAD_LAGS = ([4], [0, 4], [-1, 2], [1, 1], [2, 1], [0, 2, 2])  # a lag >= n_frames, below 0, not strictly ascending


def _pointers(Args):
    """every pointer 8 (never followed: the refusals come first), the lags in host memory real: -> (fields, the array to keep)"""
    lags = np.array([0, 1, 3], dtype=np.int32)
    p = {name: 8 for name, kind in Args._fields_ if kind is C.c_void_p}
    p["lags_host"] = lags.ctypes.data
    return p, lags


def _refuses_lags(entry, Args, good, pointers):
    for bad in BAD_LAGS:
        lags = np.array(bad, dtype=np.int32)
        args = Args(**{**pointers, **good, "n_lags": len(bad), "lags_host": lags.ctypes.data})
        assert entry(C.byref(args), None) == 1, bad


def test_self_entry_points_refuse_arguments_out_of_range():
    """The range checks come before any launch and before any device pointer is looked at: every pointer is NULL here."""
    lib = _load()
    good = dict(r_max=6.0, n_structs=1, n_atoms=2, n_species=1, n_bins=10, n_lags=3, origin_stride=1, n_q=2, **FRAMES)
    pointers, keep = _pointers(SelfArgs)
    assert len(pointers) == 18
    for entry in (lib.alignn_vh_self, lib.alignn_vh_self_finish):
        assert entry(None, None) == 1  # hipErrorInvalidValue
        for bad in BAD_COMMON + BAD_FRAMES + (dict(n_bins=4097), dict(n_q=-1), dict(n_q=17), dict(r_max=0.0), dict(r_max=-1.0),
                                              dict(r_max=float("nan")), dict(r_max=float("inf"))):
            assert entry(C.byref(SelfArgs(**{**good, **bad})), None) == 1, bad
        assert entry(C.byref(SelfArgs(**good)), None) == 1  # in range, and the pointers are needed
        assert entry(C.byref(SelfArgs(**{**good, "n_structs": 0})), None) == 0  # no structures: nothing to do
        assert entry(C.byref(SelfArgs(**{**good, "n_frames": 0})), None) == 0  # no frame selected: nothing to do
        _refuses_lags(entry, SelfArgs, good, pointers)
    assert lib.alignn_vh_self(C.byref(SelfArgs(**{**pointers, **good, "n_atoms": 0})), None) == 1
    for name in ("traj", "atom_ptr", "group", "group_count", "lags", "lags_host", "q", "counts", "overflow", "sums", "fs_sum"):
        assert lib.alignn_vh_self(C.byref(SelfArgs(**{**pointers, **good, name: None})), None) == 1, name
    for name in ("group_count", "lags", "lags_host", "counts", "sums", "fs_sum", "moments", "alpha2", "p", "gs", "fs", "centres"):
        assert lib.alignn_vh_self_finish(C.byref(SelfArgs(**{**pointers, **good, name: None})), None) == 1, name
    del keep


def test_distinct_entry_points_refuse_arguments_out_of_range():
    lib = _load()
    good = dict(r_max=6.0, n_structs=1, n_atoms=2, max_atoms=2, n_species=1, n_bins=10, n_lags=3, origin_stride=1, **FRAMES)
    pointers, keep = _pointers(DistinctArgs)
    assert len(pointers) == 13
    for entry in (lib.alignn_vh_distinct, lib.alignn_vh_distinct_finish):
        assert entry(None, None) == 1
        for bad in BAD_COMMON + BAD_FRAMES + (dict(n_bins=4097), dict(lattice_per_frame=1), dict(lattice_per_frame=-1), dict(r_max=0.0),
                                              dict(r_max=float("nan"))):
            assert entry(C.byref(DistinctArgs(**{**good, **bad})), None) == 1, bad
        assert entry(C.byref(DistinctArgs(**good)), None) == 1
        assert entry(C.byref(DistinctArgs(**{**good, "n_structs": 0})), None) == 0
        assert entry(C.byref(DistinctArgs(**{**good, "n_frames": 0})), None) == 0
        _refuses_lags(entry, DistinctArgs, good, pointers)
    for bad in (dict(n_atoms=0), dict(max_atoms=0), dict(max_atoms=3)):
        assert lib.alignn_vh_distinct(C.byref(DistinctArgs(**{**pointers, **good, **bad})), None) == 1, bad
    for name in ("traj", "lattice", "atom_ptr", "group", "group_count", "lags", "lags_host", "counts", "status"):
        assert lib.alignn_vh_distinct(C.byref(DistinctArgs(**{**pointers, **good, name: None})), None) == 1, name
    for name in ("lattice", "group_count", "lags", "lags_host", "counts", "g", "volume", "centres"):
        assert lib.alignn_vh_distinct_finish(C.byref(DistinctArgs(**{**pointers, **good, name: None})), None) == 1, name
    del keep


def test_fqt_entry_points_refuse_arguments_out_of_range():
    lib = _load()
    good = dict(q_max=4.5, n_structs=1, n_atoms=2, n_species=1, n_bins=10, n_lags=3, origin_stride=1, n_vectors=5, max_vectors=5, **FRAMES)
    pointers, keep = _pointers(FqtArgs)
    assert len(pointers) == 15
    for entry in (lib.alignn_vh_fqt_modes, lib.alignn_vh_fqt_correlate, lib.alignn_vh_fqt_bin):
        assert entry(None, None) == 1
        for bad in BAD_COMMON + BAD_FRAMES + (dict(n_bins=1025), dict(lattice_per_frame=1), dict(q_max=0.0), dict(q_max=float("nan")),
                                              dict(n_vectors=-1), dict(max_vectors=-1), dict(max_vectors=6)):
            assert entry(C.byref(FqtArgs(**{**good, **bad})), None) == 1, bad
        assert entry(C.byref(FqtArgs(**good)), None) == 1
        assert entry(C.byref(FqtArgs(**{**good, "n_structs": 0})), None) == 0
        assert entry(C.byref(FqtArgs(**{**good, "n_frames": 0})), None) == 0
    for entry in (lib.alignn_vh_fqt_modes, lib.alignn_vh_fqt_correlate):
        assert entry(C.byref(FqtArgs(**{**good, "n_vectors": 0, "max_vectors": 0})), None) == 0  # no vectors: nothing to do
    _refuses_lags(lib.alignn_vh_fqt_correlate, FqtArgs, good, pointers)
    assert lib.alignn_vh_fqt_modes(C.byref(FqtArgs(**{**pointers, **good, "n_atoms": 0})), None) == 1
    for name in ("traj", "lattice", "atom_ptr", "group", "vec_ptr", "hkl", "modes"):
        assert lib.alignn_vh_fqt_modes(C.byref(FqtArgs(**{**pointers, **good, name: None})), None) == 1, name
    for name in ("group_count", "vec_ptr", "lags", "lags_host", "modes", "f_vec"):
        assert lib.alignn_vh_fqt_correlate(C.byref(FqtArgs(**{**pointers, **good, name: None})), None) == 1, name
    for name in ("vec_ptr", "vbin", "f_vec", "f", "n_vectors_bin", "centres"):
        assert lib.alignn_vh_fqt_bin(C.byref(FqtArgs(**{**pointers, **good, name: None})), None) == 1, name
    del keep


# --- tests/vanhove_extents.py against the header ---------------------------------------------------------------------------------------
CTYPE = {torch.float64: "double", torch.int32: "int32_t", torch.int64: "int64_t"}


def test_the_extents_table_names_every_struct_and_entry_point():
    h = _abi.header("alignn_vanhove.h")
    assert {s: t["header"] for s, t in vx.TABLE.items()} == {s: "alignn_vanhove.h" for s in h.structs}
    assert set(vx.entry_points()) == ENTRIES and len(vx.entry_points()) == sum(len(t["entries"]) for t in vx.TABLE.values()) == 7


@pytest.mark.parametrize("struct", list(vx.TABLE))
def test_every_pointer_field_has_an_extent_and_a_role_per_entry_point(struct):
    table, h = vx.TABLE[struct], wx.header_of(struct, vx.TABLE)
    cls = h.structs[struct]
    assert list(table["fields"]) == [n for n, t in cls._fields_ if t is C.c_void_p]  # every pointer field, no other, in the header's order
    known = {n for n, t in cls._fields_ if t is not C.c_void_p} | set(h.defines) | set(table["derived"])
    assert not set(table["derived"]) & {n for n, _ in cls._fields_} and not set(table["let"]) & known
    for field, spec in table["fields"].items():
        assert len(spec["roles"]) == len(table["entries"]) and set(spec["roles"]) <= set(vx.ROLES), field
        assert any(r != "unused" for r in spec["roles"]), field
        assert ("host" in spec["roles"]) == (field in vx.HOST), field
        assert not isinstance(spec["count"], dict)
        for expr in (spec["count"], spec["row"]):
            assert wx.names_used(struct, expr, vx.TABLE) <= known, (field, expr, wx.names_used(struct, expr, vx.TABLE) - known)
    # the dtype is the header's: the declaration of the field, read from the text; a const pointer is one no entry point writes
    with open(h.path) as f:
        text = _abi._uncomment(f.read())
    body = text[text.index("typedef struct " + struct):text.index("} " + struct)]
    for field, spec in table["fields"].items():
        m = re.search(rf"(const\s+)?{CTYPE[spec['dtype']]}\s*\*\s*{field}\s*;", body)
        assert m, (field, spec["dtype"])
        assert bool(m.group(1)) == (set(spec["roles"]) <= {"in", "host", "unused"}), field


def test_extents_follow_the_scalars():
    rep = gp.Report("vanhove extents")
    s = wx.Block(rep.guards, "alignn_vh_self_args", device="cpu", table=vx.TABLE)
    s.set(n_structs=3, n_atoms=76, n_species=3, n_bins=50, n_total_frames=9, n_frames=4, n_lags=3, n_q=2, r_max=6.0)
    assert s.extent("counts") == (3 * 4 * 3 * 50, 50) and s.extent("overflow") == (36, 3) and s.extent("fs_sum") == (72, 2)
    assert s.extent("traj") == (3 * 9 * 76, 3) and s.extent("com") == (36, 3) and s.extent("lags") == (3, 1) and s.extent("q") == (2, 1)
    d = wx.Block(rep.guards, "alignn_vh_distinct_args", device="cpu", table=vx.TABLE)
    d.set(n_structs=3, n_atoms=76, n_species=3, n_bins=50, n_total_frames=9, n_frames=9, n_lags=4)
    assert d.extent("counts") == (3 * 7 * 4 * 50, 50) and d.extent("lattice") == (27, 3) and d.extent("volume") == (3, 1)
    f = wx.Block(rep.guards, "alignn_vh_fqt_args", device="cpu", table=vx.TABLE)
    f.set(n_structs=3, n_atoms=76, n_species=3, n_bins=40, n_frames=9, n_lags=4, n_vectors=1959)
    assert f.extent("modes") == (2 * 9 * 3 * 1959, 2) and f.extent("f_vec") == (7 * 4 * 1959, 1959) and f.extent("f") == (3 * 7 * 4 * 40, 40)
    assert f.extent("n_vectors_bin") == (120, 40) and f.extent("hkl") == (3 * 1959, 3)
