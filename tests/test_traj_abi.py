"""CPU-side checks of the fourth header, include/alignn_traj.h: it reads with the reader of alignn_amd/_abi.py, the built library
exports exactly the names it declares (no compute calls - there is no GPU here), the
ctypes layout of its argument blocks agrees with a C compiler's sizeof / offsetof and with the library's size queries, and
every range check answers hipErrorInvalidValue before anything touches a device."""

import ctypes as C

from alignn_amd import _abi, _lib
from alignn_amd.trajectory import (HEADER, MAX_BINS, MAX_IMAGE_RANGE, MAX_SPECIES, SIGNATURES, STATUS_IMAGES, STRUCTS, CorrArgs,
                                   RdfArgs, _load)
from tests import abi_checks

NAMES = {"alignn_traj_rdf_counts", "alignn_traj_rdf_normalise", "alignn_traj_rdf_args_size", "alignn_traj_com",
         "alignn_traj_corr", "alignn_traj_corr_args_size", "alignn_traj_vdos", "alignn_traj_fit", "alignn_traj_green_kubo"}


def test_header_reads_and_the_library_exports_exactly_its_names():
    from alignn_amd.build import SOURCES, build

    assert "trajectory.hip" in SOURCES
    lib_path = build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_traj_rdf_args", "alignn_traj_corr_args"] == list(STRUCTS)
    assert set(sigs) == abi_checks.declared(HEADER) == set(SIGNATURES) == NAMES
    assert abi_checks.exported(lib_path, "alignn_traj_") == NAMES  # nothing of the prefix beside what the header declares
    lib = _load()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    for name in ("alignn_traj_rdf_counts", "alignn_traj_rdf_normalise", "alignn_traj_com", "alignn_traj_corr"):
        assert sigs[name] == (C.c_int, [C.c_void_p, C.c_void_p]), name
    assert sigs["alignn_traj_rdf_args_size"] == sigs["alignn_traj_corr_args_size"] == (C.c_size_t, [])
    assert sigs["alignn_traj_vdos"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int,
                                                  C.c_void_p, C.c_void_p])
    assert sigs["alignn_traj_fit"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p])
    assert sigs["alignn_traj_green_kubo"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p])
    assert (MAX_SPECIES, MAX_BINS, MAX_IMAGE_RANGE, STATUS_IMAGES) == (8, 4096, 8, 1)


def test_argument_block_sizes_match_the_library():
    lib = _load()
    assert lib.alignn_traj_rdf_args_size() == C.sizeof(RdfArgs) == 12 * 8 + 10 * 4
    assert lib.alignn_traj_corr_args_size() == C.sizeof(CorrArgs) == 7 * 8 + 10 * 4
    blank = RdfArgs()
    assert blank.traj is None and blank.n_frames == 0 and blank.r_max == 0.0  # a field left out is NULL / 0


RDF_OK = dict(r_max=6.0, n_structs=1, n_atoms=4, max_atoms=4, n_species=1, n_bins=50, n_total_frames=3, frame0=0, frame_step=1,
              n_frames=3, lattice_per_frame=0)
CORR_OK = dict(n_structs=1, n_atoms=4, n_species=1, n_total_frames=5, frame0=0, frame_step=1, n_frames=5, max_lag=4,
               origin_stride=1, mode=0)


def test_entry_points_refuse_arguments_out_of_range():
    """The checks that come before any launch, every pointer NULL: no device is touched."""
    lib = _load()
    for fn in (lib.alignn_traj_rdf_counts, lib.alignn_traj_rdf_normalise, lib.alignn_traj_com, lib.alignn_traj_corr):
        assert fn(None, None) == 1  # hipErrorInvalidValue
    rdf_bad = [dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_species=0), dict(n_species=MAX_SPECIES + 1),
               dict(n_bins=0), dict(n_bins=MAX_BINS + 1), dict(r_max=0.0), dict(r_max=-1.0), dict(r_max=float("nan")),
               dict(r_max=float("inf")), dict(lattice_per_frame=2), dict(lattice_per_frame=-1), dict(frame0=-1),
               dict(frame_step=0), dict(n_frames=-1), dict(n_frames=4), dict(frame0=1), dict(frame_step=2), dict(n_total_frames=-1),
               dict()]  # (dict(): in range, but every pointer NULL)
    for bad in rdf_bad:
        args = RdfArgs(**{**RDF_OK, **bad})
        assert lib.alignn_traj_rdf_counts(C.byref(args), None) == 1, bad
        assert lib.alignn_traj_rdf_normalise(C.byref(args), None) == 1, bad
    for bad in (dict(max_atoms=0), dict(max_atoms=5), dict(n_atoms=0)):
        assert lib.alignn_traj_rdf_counts(C.byref(RdfArgs(**{**RDF_OK, **bad})), None) == 1, bad
    corr_bad = [dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_species=0), dict(n_species=MAX_SPECIES + 1),
                dict(origin_stride=0), dict(mode=2), dict(mode=-1), dict(frame0=-1), dict(frame_step=0), dict(n_frames=-1),
                dict(n_frames=6), dict(frame0=1), dict(n_total_frames=-1), dict()]
    for bad in corr_bad:
        args = CorrArgs(**{**CORR_OK, **bad})
        assert lib.alignn_traj_corr(C.byref(args), None) == 1, bad
        assert lib.alignn_traj_com(C.byref(args), None) == 1, bad
    for bad in (dict(max_lag=-1), dict(max_lag=5), dict(n_atoms=0)):
        assert lib.alignn_traj_corr(C.byref(CorrArgs(**{**CORR_OK, **bad})), None) == 1, bad
    # nothing to do: no structures, or no frames selected
    for empty in (dict(n_structs=0), dict(n_frames=0)):
        assert lib.alignn_traj_rdf_counts(C.byref(RdfArgs(**{**RDF_OK, **empty})), None) == 0, empty
        assert lib.alignn_traj_corr(C.byref(CorrArgs(**{**CORR_OK, **empty, "max_lag": 0})), None) == 0, empty
        assert lib.alignn_traj_com(C.byref(CorrArgs(**{**CORR_OK, **empty})), None) == 0, empty
    assert lib.alignn_traj_rdf_normalise(C.byref(RdfArgs(**{**RDF_OK, "n_structs": 0})), None) == 0

    nan, inf = float("nan"), float("inf")
    vdos = lambda rows=1, K=4, dtau=1.0, nf=8, fmax=30.0, win=1: lib.alignn_traj_vdos(None, rows, K, dtau, nf, fmax, win, None, None)
    for bad in (dict(rows=-1), dict(K=-1), dict(dtau=0.0), dict(dtau=nan), dict(dtau=inf), dict(nf=1), dict(fmax=0.0),
                dict(fmax=nan), dict(win=2), dict(win=-1), dict()):
        assert vdos(**bad) == 1, bad
    assert vdos(rows=0) == 0
    fit = lambda rows=1, K=8, dtau=1.0, lo=2, hi=8: lib.alignn_traj_fit(None, rows, K, dtau, lo, hi, None, None)
    for bad in (dict(rows=-1), dict(rows=65536), dict(K=0), dict(dtau=0.0), dict(dtau=nan), dict(lo=-1), dict(lo=8), dict(hi=9),
                dict(lo=3, hi=3), dict()):
        assert fit(**bad) == 1, bad
    assert fit(rows=0) == 0
    gk = lambda rows=1, K=8, dtau=1.0, unit=0.1: lib.alignn_traj_green_kubo(None, rows, K, dtau, unit, None, None)
    for bad in (dict(rows=-1), dict(K=-1), dict(dtau=0.0), dict(dtau=nan), dict(unit=0.0), dict(unit=inf), dict()):
        assert gk(**bad) == 1, bad
    assert gk(rows=0) == 0


def test_argument_block_layouts_match_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_traj.h", STRUCTS, tmp_path)
    assert len(want) == 2 + 22 + 17 and seen == want
