"""CPU-side checks of the sixth header, include/alignn_order.h: it reads with the reader of alignn_amd/_abi.py, the built library
exports exactly the names it declares (no compute calls - there is no GPU here), the
ctypes layout of its argument blocks agrees with a C compiler's sizeof / offsetof and with the library's size queries, and
every range check answers hipErrorInvalidValue before anything touches a device."""

import ctypes as C
import os

import alignn_amd
from alignn_amd import _abi, _lib
from alignn_amd.order import (HEADER, MAX_BINS, MAX_HKL, MAX_IMAGE_RANGE, MAX_L, MAX_LS, MAX_NEIGHBORS, MAX_SPECIES, SIGNATURES,
                              SQ_FRAME_CHUNK, STATUS_HKL, STATUS_IMAGES, STATUS_NEIGHBORS, STRUCTS, AngleArgs, SqArgs, _load)
from tests import abi_checks

ANGLE_CALLS = {"alignn_order_angles", "alignn_order_adf_finish", "alignn_order_steinhardt_mean"}
SQ_CALLS = {"alignn_order_sq_vectors", "alignn_order_sq_accumulate", "alignn_order_sq_bin"}
SIZES = {"alignn_order_angle_args_size", "alignn_order_sq_args_size"}
NAMES = ANGLE_CALLS | SQ_CALLS | SIZES


def test_header_reads_and_the_library_exports_exactly_its_names():
    from alignn_amd.build import SOURCES, _headers, build

    assert "order.hip" in SOURCES and HEADER in [os.path.normpath(h) for h in _headers()]
    lib_path = build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_order_angle_args", "alignn_order_sq_args"] == list(STRUCTS)
    assert set(sigs) == abi_checks.declared(HEADER) == set(SIGNATURES) == NAMES
    assert abi_checks.exported(lib_path, "alignn_order_") == NAMES  # nothing of the prefix beside what the header declares
    assert not any(name.startswith("alignn_traj_") for name in NAMES)
    lib = _load()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    for name in NAMES - SIZES:
        assert sigs[name] == (C.c_int, [C.c_void_p, C.c_void_p]), name
    for name in SIZES:
        assert sigs[name] == (C.c_size_t, []), name
    assert (MAX_SPECIES, MAX_IMAGE_RANGE, MAX_NEIGHBORS, MAX_BINS, MAX_L, MAX_LS, MAX_HKL, SQ_FRAME_CHUNK) == (8, 8, 64, 1024, 12, 4, 32, 64)
    assert (STATUS_IMAGES, STATUS_NEIGHBORS, STATUS_HKL) == (1, 2, 4)
    for name in ("adf", "steinhardt", "structure_factor", "ADFResult", "SteinhardtResult", "SQResult"):
        assert getattr(alignn_amd, name) is getattr(alignn_amd.order, name), name
    assert (alignn_amd.MAX_NEIGHBORS, alignn_amd.MAX_L, alignn_amd.MAX_HKL) == (MAX_NEIGHBORS, MAX_L, MAX_HKL)


def test_argument_block_sizes_match_the_library():
    lib = _load()
    assert lib.alignn_order_angle_args_size() == C.sizeof(AngleArgs) == 13 * 8 + 15 * 4 + 4  # (padded to the pointers' 8 bytes)
    assert lib.alignn_order_sq_args_size() == C.sizeof(SqArgs) == 17 * 8 + 10 * 4
    blank = AngleArgs()
    assert blank.traj is None and blank.counts is None and blank.n_frames == 0 and blank.l3 == 0  # a field left out is NULL / 0
    assert SqArgs().q_max == 0.0


ANGLE_OK = dict(n_structs=1, n_atoms=4, max_atoms=4, n_species=1, n_bins=50, n_total_frames=3, frame0=0, frame_step=1, n_frames=3,
                lattice_per_frame=0, n_ls=2, l0=4, l1=6)
SQ_OK = dict(q_max=6.0, n_structs=1, n_atoms=4, n_species=1, n_bins=50, n_total_frames=3, frame0=0, frame_step=1, n_frames=3,
             n_vectors=10, max_vectors=10)


def test_entry_points_refuse_arguments_out_of_range():
    """The checks that come before any launch, every pointer NULL: no device is touched."""
    lib = _load()
    angle_calls = [getattr(lib, name) for name in sorted(ANGLE_CALLS)]
    sq_calls = [getattr(lib, name) for name in sorted(SQ_CALLS)]
    for fn in angle_calls + sq_calls:
        assert fn(None, None) == 1  # hipErrorInvalidValue
    nan, inf = float("nan"), float("inf")
    angle_bad = [dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_species=0), dict(n_species=MAX_SPECIES + 1),
                 dict(n_bins=0), dict(n_bins=MAX_BINS + 1), dict(lattice_per_frame=2), dict(lattice_per_frame=-1), dict(frame0=-1),
                 dict(frame_step=0), dict(n_frames=-1), dict(n_frames=4), dict(frame0=1), dict(frame_step=2), dict(n_total_frames=-1),
                 dict(n_ls=-1), dict(n_ls=MAX_LS + 1), dict(l0=0), dict(l1=MAX_L + 1), dict(l1=4), dict(n_ls=3, l2=-1),
                 dict(n_ls=4, l2=8, l3=6), dict()]  # (dict(): in range, but every pointer NULL)
    for bad in angle_bad:
        args = AngleArgs(**{**ANGLE_OK, **bad})
        for fn in angle_calls:
            assert fn(C.byref(args), None) == 1, bad
    for bad in (dict(max_atoms=0), dict(max_atoms=5), dict(n_atoms=0), dict(n_atoms=70000, max_atoms=65536)):
        assert lib.alignn_order_angles(C.byref(AngleArgs(**{**ANGLE_OK, **bad})), None) == 1, bad
    assert lib.alignn_order_steinhardt_mean(C.byref(AngleArgs(**{**ANGLE_OK, "n_ls": 0})), None) == 1
    sq_bad = [dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_species=0), dict(n_species=MAX_SPECIES + 1),
              dict(n_bins=0), dict(n_bins=MAX_BINS + 1), dict(q_max=0.0), dict(q_max=-1.0), dict(q_max=nan), dict(q_max=inf),
              dict(frame0=-1), dict(frame_step=0), dict(n_frames=-1), dict(n_frames=4), dict(frame0=1), dict(n_total_frames=-1),
              dict(n_vectors=-1), dict(max_vectors=-1), dict(max_vectors=11), dict()]
    for bad in sq_bad:
        args = SqArgs(**{**SQ_OK, **bad})
        for fn in sq_calls:
            assert fn(C.byref(args), None) == 1, bad
    # nothing to do: no structures, or no frames selected
    for fn in angle_calls:
        assert fn(C.byref(AngleArgs(**{**ANGLE_OK, "n_structs": 0})), None) == 0
    for fn in sq_calls:
        assert fn(C.byref(SqArgs(**{**SQ_OK, "n_structs": 0})), None) == 0
    for fn in (lib.alignn_order_angles, lib.alignn_order_steinhardt_mean):
        assert fn(C.byref(AngleArgs(**{**ANGLE_OK, "n_frames": 0})), None) == 0
    assert lib.alignn_order_sq_accumulate(C.byref(SqArgs(**{**SQ_OK, "n_frames": 0})), None) == 0
    assert lib.alignn_order_sq_accumulate(C.byref(SqArgs(**{**SQ_OK, "n_vectors": 0, "max_vectors": 0})), None) == 0


def test_argument_block_layouts_match_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_order.h", STRUCTS, tmp_path)
    assert len(want) == 2 + 28 + 27 and seen == want
