"""CPU-side checks of the seventh header, include/alignn_phsym.h: it reads with the reader of alignn_amd/_abi.py, the built
library exports exactly the names it declares (no compute calls - there is no GPU here), the ctypes layout of its argument blocks agrees with a C compiler's sizeof / offsetof and with the library's size
queries, and every range check answers hipErrorInvalidValue before anything touches a device."""

import ctypes as C
import os
import sys

import alignn_amd  # noqa: F401  (the package exports the function ``phonons``: the module is taken from sys.modules)
from alignn_amd import _abi, _lib
from tests import abi_checks

PH = sys.modules["alignn_amd.phonons"]
SIZES = {"alignn_phsym_plan_args_size", "alignn_phsym_displace_args_size", "alignn_phsym_rows_args_size", "alignn_phsym_fc_args_size"}
ENTRIES = {"alignn_phsym_plan", "alignn_phsym_displace", "alignn_phsym_rows", "alignn_phsym_solve", "alignn_phsym_distribute"}
NAMES = SIZES | ENTRIES
BLOCKS = ["alignn_phsym_plan_args", "alignn_phsym_displace_args", "alignn_phsym_rows_args", "alignn_phsym_fc_args"]


def test_header_reads_and_the_library_exports_exactly_its_names():
    from alignn_amd.build import SOURCES, _headers, build

    assert "phonon_sym.hip" in SOURCES and PH.PHSYM_HEADER in [os.path.normpath(h) for h in _headers()]
    lib_path = build()
    structs, sigs = _abi.parse(open(PH.PHSYM_HEADER).read())
    assert list(structs) == BLOCKS == list(PH.PHSYM_STRUCTS)
    assert set(sigs) == abi_checks.declared(PH.PHSYM_HEADER) == set(PH.PHSYM_SIGNATURES) == NAMES
    assert abi_checks.exported(lib_path, "alignn_phsym_") == NAMES  # nothing of the prefix beside what the header declares
    lib = PH._load_phsym()
    assert lib is _lib.load()
    abi_checks.assert_typed(lib, sigs)
    for name in ENTRIES:
        assert sigs[name] == (C.c_int, [C.c_void_p, C.c_void_p]), name
    for name in SIZES:
        assert sigs[name] == (C.c_size_t, []), name
    assert (PH.PHSYM_MAX_ATOMS, PH.PHSYM_MAX_SITE_OPS, PH.PHSYM.defines["ALIGNN_PHSYM_N_CANDIDATES"]) == (32, 48, 13)
    assert PH.PHSYM_MAX_ATOMS * 3 == PH.MAX_DIM


def test_argument_block_sizes_match_the_library():
    lib = PH._load_phsym()
    assert lib.alignn_phsym_plan_args_size() == C.sizeof(PH.PlanArgs) == 18 * 8 + 2 * 4
    assert lib.alignn_phsym_displace_args_size() == C.sizeof(PH.DisplaceArgs) == 11 * 8 + 2 * 4
    assert lib.alignn_phsym_rows_args_size() == C.sizeof(PH.RowsArgs) == 8 * 8 + 3 * 4 + 4
    assert lib.alignn_phsym_fc_args_size() == C.sizeof(PH.FcArgs) == 22 * 8 + 3 * 4 + 4
    blank = PH.FcArgs()
    assert blank.fc is None and blank.n_items == 0 and PH.RowsArgs().delta == 0.0  # a field left out is NULL / 0


PLAN_OK = dict(n_structs=1, n_atoms=2, n_ops_total=4, n_map_total=8)
DISPLACE_OK = dict(n_jobs=2, n_structs=1, delta=0.01)
ROWS_OK = dict(n_pairs=1, n_structs=1, delta=0.01, drift=1)
FC_OK = dict(n_items=1, n_structs=1, n_ops_total=4, n_map_total=8, max_supercell_atoms=16)


def test_entry_points_refuse_arguments_out_of_range():
    """The checks that come before any launch, every pointer NULL: no device is touched."""
    lib = PH._load_phsym()
    for name in ENTRIES:
        assert getattr(lib, name)(None, None) == 1  # hipErrorInvalidValue
    nan, inf = float("nan"), float("inf")
    # (dict(): in range, but every pointer NULL)
    for bad in (dict(n_structs=-1), dict(n_structs=65536), dict(n_atoms=-1), dict(n_atoms=0), dict(n_ops_total=-1), dict(n_ops_total=0),
                dict(n_map_total=-1), dict(n_map_total=0), dict()):
        assert lib.alignn_phsym_plan(C.byref(PH.PlanArgs(**{**PLAN_OK, **bad})), None) == 1, bad
    for bad in (dict(n_jobs=-1), dict(n_structs=-1), dict(n_structs=0), dict(delta=0.0), dict(delta=-0.01), dict(delta=nan),
                dict(delta=inf), dict()):
        assert lib.alignn_phsym_displace(C.byref(PH.DisplaceArgs(**{**DISPLACE_OK, **bad})), None) == 1, bad
    for bad in (dict(n_pairs=-1), dict(n_structs=-1), dict(n_structs=0), dict(delta=0.0), dict(delta=nan), dict(delta=inf),
                dict(drift=-1), dict(drift=3), dict()):
        assert lib.alignn_phsym_rows(C.byref(PH.RowsArgs(**{**ROWS_OK, **bad})), None) == 1, bad
    for fn in (lib.alignn_phsym_solve, lib.alignn_phsym_distribute):
        for bad in (dict(n_items=-1), dict(n_items=65536), dict(n_structs=-1), dict(n_structs=0), dict(n_structs=65536),
                    dict(n_ops_total=-1), dict(n_ops_total=0), dict(n_map_total=-1), dict(n_map_total=0),
                    dict(max_supercell_atoms=0), dict()):
            assert fn(C.byref(PH.FcArgs(**{**FC_OK, **bad})), None) == 1, bad
    # nothing to do
    assert lib.alignn_phsym_plan(C.byref(PH.PlanArgs(**{**PLAN_OK, "n_structs": 0})), None) == 0
    assert lib.alignn_phsym_displace(C.byref(PH.DisplaceArgs(**{**DISPLACE_OK, "n_jobs": 0})), None) == 0
    assert lib.alignn_phsym_rows(C.byref(PH.RowsArgs(**{**ROWS_OK, "n_pairs": 0})), None) == 0
    for fn in (lib.alignn_phsym_solve, lib.alignn_phsym_distribute):
        assert fn(C.byref(PH.FcArgs(**{**FC_OK, "n_items": 0})), None) == 0


def test_argument_block_layouts_match_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_phsym.h", PH.PHSYM_STRUCTS, tmp_path)
    assert len(want) == 4 + 20 + 13 + 11 + 25 and seen == want
