"""CPU-side checks of include/alignn_voronoi.h, the header of ``_abi.STRUCTURE_HEADERS``: it reads with the reader of
alignn_amd/_abi.py, the built library exports exactly the names it declares (no compute calls - there is no GPU here), the ctypes
layout of its argument block agrees with a C compiler's sizeof / offsetof and with the library's size query, the limits it shares
with alignn_order.h are that header's by value and the restatement mirrors its own, both entry points refuse an argument out of
range before they look at a device pointer, and tests/voronoi_extents.py names every pointer field with an extent over the
struct's own scalars."""

import ctypes as C
import os
import re

import pytest
import torch

import alignn_amd
from alignn_amd import _abi, _lib, order
from alignn_amd.voronoi import (HEADER, MAX_FACES, MAX_NEIGHBORS, MAX_POLYGON, N_INDEX, SIGNATURES, STATUS_FACES, STATUS_POLYGON, STRUCTS,
                                VoroArgs, VoronoiResult, _load, voronoi, voronoi_census)
from tests import abi_checks
from tests import gate_parity as gp
from tests import voronoi_extents as vx
from tests import voronoi_ref as ref
from tests import workflow_extents as wx

ENTRY = (C.c_int, [C.c_void_p, C.c_void_p])
ENTRIES = {"alignn_voro_cells", "alignn_voro_means"}
SIZES = {"alignn_voro_args_size"}


def test_header_reads_and_the_library_exports_it():
    from alignn_amd.build import SOURCES, _headers, build

    assert "voronoi.hip" in SOURCES and HEADER in [os.path.normpath(h) for h in _headers()]  # (an edit rebuilds the library)
    assert _abi.STRUCTURE_HEADERS == ("alignn_voronoi.h",)
    assert not set(_abi.STRUCTURE_HEADERS) & (set(_abi.WORKFLOW_HEADERS) | set(_abi.LATER_HEADERS) | set(_abi.ANALYSIS_HEADERS))
    build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_voro_args"] == list(STRUCTS)
    assert set(sigs) == abi_checks.declared(HEADER) == set(SIGNATURES) == ENTRIES | SIZES
    assert all(name.startswith("alignn_voro_") for name in list(structs) + list(sigs))
    lib = _load()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    assert abi_checks.exported(_lib.LIB_PATH, "alignn_voro_") == set(sigs)
    for name, sig in sigs.items():
        assert sig == ((C.c_size_t, []) if name.endswith("_size") else ENTRY), name


def test_the_package_exports_the_functions_and_the_result():
    for name, thing in (("voronoi", voronoi), ("voronoi_census", voronoi_census), ("VoronoiResult", VoronoiResult)):
        assert getattr(alignn_amd, name) is thing, name
    import importlib

    assert {"voronoi", "voronoi_census", "VoronoiResult"} <= set(importlib.import_module("alignn_amd.voronoi").__all__)


def test_limits_are_mirrored():
    d, o = _abi.header("alignn_voronoi.h").defines, _abi.header("alignn_order.h").defines
    for name in ("MAX_SPECIES", "MAX_IMAGE_RANGE", "MAX_NEIGHBORS", "STATUS_IMAGES", "STATUS_NEIGHBORS"):
        assert d["ALIGNN_VORO_" + name] == o["ALIGNN_ORDER_" + name], name
    assert MAX_NEIGHBORS == order.MAX_NEIGHBORS == 64
    assert d["ALIGNN_VORO_MAX_POLYGON"] == MAX_POLYGON == ref.MAX_POLYGON == 32 and d["ALIGNN_VORO_MAX_FACES"] == MAX_FACES == ref.MAX_FACES == 32
    assert d["ALIGNN_VORO_INDEX"] == N_INDEX == ref.N_INDEX == 8 and d["ALIGNN_VORO_SQUARE"] == ref.SQUARE == 4.0
    assert (d["ALIGNN_VORO_STATUS_POLYGON"], d["ALIGNN_VORO_STATUS_FACES"]) == (STATUS_POLYGON, STATUS_FACES) == (4, 8) and len(d) == 11
    bits = [d[k] for k in d if "_STATUS_" in k]
    assert len(set(bits)) == 4 and all(b & (b - 1) == 0 for b in bits)  # four different single bits


def test_argument_block_size_matches_the_library():
    lib = _load()
    assert lib.alignn_voro_args_size() == C.sizeof(VoroArgs) == 19 * 8 + 3 * 8 + 10 * 4
    blank = VoroArgs()
    assert blank.face_j is None and blank.faces == 0 and blank.face_threshold == 0.0  # a field left out is NULL / 0


def test_argument_block_layout_matches_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_voronoi.h", STRUCTS, tmp_path)
    assert len(want) == 1 + 32 and seen == want


FRAMES = dict(n_total_frames=4, frame0=0, frame_step=1, n_frames=4)
BAD = (dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_species=0), dict(n_species=9), dict(lattice_per_frame=2),
       dict(lattice_per_frame=-1), dict(faces=2), dict(faces=-1), dict(face_threshold=-1.0), dict(face_threshold=float("nan")),
       dict(relative_face_threshold=float("inf")), dict(relative_face_threshold=-0.5), dict(edge_threshold=float("nan")),
       dict(edge_threshold=-1e-300), dict(n_total_frames=-1), dict(frame0=-1), dict(frame_step=0), dict(n_frames=-1), dict(n_frames=5),
       dict(frame0=1), dict(frame_step=2))


def test_entry_points_refuse_arguments_out_of_range():
    """The range checks come before any launch and before any device pointer is looked at: no pointer here is real."""
    lib = _load()
    good = dict(n_structs=1, n_atoms=2, max_atoms=2, n_species=1, faces=1, **FRAMES)
    pointers = {name: 8 for name, kind in VoroArgs._fields_ if kind is C.c_void_p}
    assert len(pointers) == 19
    for entry in (lib.alignn_voro_cells, lib.alignn_voro_means):
        assert entry(None, None) == 1  # hipErrorInvalidValue
        for bad in BAD:
            assert entry(C.byref(VoroArgs(**{**pointers, **good, **bad})), None) == 1, bad
        assert entry(C.byref(VoroArgs(**good)), None) == 1  # in range, and the pointers are needed
        assert entry(C.byref(VoroArgs(**{**good, "n_structs": 0})), None) == 0  # no structures: nothing to do
        assert entry(C.byref(VoroArgs(**{**good, "n_frames": 0})), None) == 0  # no frame selected: nothing to do
        assert entry(C.byref(VoroArgs(**{**pointers, **good, "n_atoms": 0})), None) == 1
    for bad in (dict(max_atoms=0), dict(max_atoms=3), dict(n_atoms=70000, max_atoms=65536)):
        assert lib.alignn_voro_cells(C.byref(VoroArgs(**{**pointers, **good, **bad})), None) == 1, bad
    for name in ("traj", "lattice", "atom_ptr", "group", "group_count", "r_cut", "volume", "area", "r_max", "n_faces", "index", "complete",
                 "status") + vx.FACES:
        assert lib.alignn_voro_cells(C.byref(VoroArgs(**{**pointers, **good, name: None})), None) == 1, name
    for name in ("atom_ptr", "group", "volume", "area", "n_faces", "complete", "mean", "n_complete"):
        assert lib.alignn_voro_means(C.byref(VoroArgs(**{**pointers, **good, name: None})), None) == 1, name


# --- tests/voronoi_extents.py against the header -------------------------------------------------------------------------------------
CTYPE = {torch.float64: "double", torch.int32: "int32_t", torch.int64: "int64_t"}


def test_the_extents_table_names_the_struct_and_both_entry_points():
    h = _abi.header("alignn_voronoi.h")
    assert {s: t["header"] for s, t in vx.TABLE.items()} == {s: "alignn_voronoi.h" for s in h.structs}
    assert set(vx.entry_points()) == ENTRIES and len(vx.entry_points()) == 2


@pytest.mark.parametrize("struct", list(vx.TABLE))
def test_every_pointer_field_has_an_extent_and_a_role_per_entry_point(struct):
    table, h = vx.TABLE[struct], wx.header_of(struct, vx.TABLE)
    cls = h.structs[struct]
    assert list(table["fields"]) == [n for n, t in cls._fields_ if t is C.c_void_p]  # every pointer field, no other, in the header's order
    known = {n for n, t in cls._fields_ if t is not C.c_void_p} | set(h.defines) | set(table["derived"])
    assert not set(table["derived"]) & {n for n, _ in cls._fields_} and not set(table["let"]) & known
    for field, spec in table["fields"].items():
        assert len(spec["roles"]) == len(table["entries"]) and set(spec["roles"]) <= set(wx.ROLES), field
        assert any(r != "unused" for r in spec["roles"]), field
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
        assert bool(m.group(1)) == (set(spec["roles"]) <= {"in", "unused"}), field


def test_extents_follow_the_scalars():
    rep = gp.Report("voronoi extents")
    b = wx.Block(rep.guards, "alignn_voro_args", device="cpu", table=vx.TABLE)
    b.set(n_structs=3, n_atoms=76, n_species=2, n_total_frames=9, n_frames=4, lattice_per_frame=0)
    assert b.extent("traj") == (3 * 9 * 76, 3) and b.extent("lattice") == (27, 3) and b.extent("r_cut") == (3, 1)
    assert b.extent("volume") == b.extent("complete") == (4 * 76, 1) and b.extent("index") == (4 * 76 * 8, 8)
    assert b.extent("mean") == (3 * 3 * 4 * 3, 3) and b.extent("n_complete") == (36, 1) and b.extent("group_count") == (9, 3)
    assert b.extent("face_j") == b.extent("face_area") == (4 * 76 * 32, 32) and b.extent("face_d") == (4 * 76 * 32 * 3, 3)
    b.set(lattice_per_frame=1)
    assert b.extent("lattice") == (9 * 3 * 9, 3)
