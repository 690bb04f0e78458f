"""CPU-side checks of the fifth header, include/alignn_sym.h: it reads with the reader of alignn_amd/_abi.py, the built library
exports exactly the names it declares (no compute calls - there is no GPU here), no name collides with the other headers, the
ctypes layout of its argument blocks agrees with a C compiler's sizeof / offsetof and with the library's size queries, and
every range check answers hipErrorInvalidValue before anything touches a device."""

import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from alignn_amd import _abi, _lib
from alignn_amd.neb import SIGNATURES as NEB_SIGNATURES
from alignn_amd.neb import STRUCTS as NEB_STRUCTS
from alignn_amd.symmetry import (HEADER, INFO, MAX_ATOMS, MAX_CANDIDATES, MAX_IMAGE_RANGE, MAX_LATTICE_OPS, SIGNATURES,
                                 STATUS_IMAGES, STATUS_INPUT, STATUS_OVERFLOW, STRUCTS, ApplyArgs, FindArgs, _load)
from alignn_amd.thermo import SIGNATURES as THERMO_SIGNATURES
from alignn_amd.trajectory import SIGNATURES as TRAJ_SIGNATURES
from alignn_amd.trajectory import STRUCTS as TRAJ_STRUCTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"alignn_sym_search", "alignn_sym_fill", "alignn_sym_find_args_size", "alignn_sym_forces", "alignn_sym_stress",
         "alignn_sym_positions", "alignn_sym_apply_args_size"}


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(alignn_[a-z0-9_]+)\s*\(", text))


def _exported(lib_path):
    nm = "/opt/rocm/lib/llvm/bin/llvm-nm" if os.path.exists("/opt/rocm/lib/llvm/bin/llvm-nm") else shutil.which("nm")
    if nm is None:
        pytest.skip("no nm")
    out = subprocess.run([nm, "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("alignn_sym_")}


def test_header_reads_and_the_library_exports_exactly_its_names():
    from alignn_amd.build import SOURCES, _headers, build

    assert "symmetry.hip" in SOURCES and HEADER in [os.path.normpath(h) for h in _headers()]
    lib_path = build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_sym_find_args", "alignn_sym_apply_args"] == list(STRUCTS)
    assert set(sigs) == _declared(HEADER) == set(SIGNATURES) == NAMES
    assert _exported(lib_path) == NAMES  # nothing of the prefix beside what the header declares
    others = set(_abi.SIGNATURES) | set(THERMO_SIGNATURES) | set(NEB_SIGNATURES) | set(TRAJ_SIGNATURES)
    assert not set(sigs) & others  # no name in two headers
    assert not set(structs) & (set(_abi.STRUCTS) | set(NEB_STRUCTS) | set(TRAJ_STRUCTS))
    lib = _load()
    assert lib is _lib.load()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    for name in NAMES - {"alignn_sym_find_args_size", "alignn_sym_apply_args_size"}:
        assert sigs[name] == (C.c_int, [C.c_void_p, C.c_void_p]), name
    assert sigs["alignn_sym_find_args_size"] == sigs["alignn_sym_apply_args_size"] == (C.c_size_t, [])
    text = open(HEADER).read()
    for macro, value in (("MAX_ATOMS", MAX_ATOMS), ("MAX_IMAGE_RANGE", MAX_IMAGE_RANGE), ("MAX_CANDIDATES", MAX_CANDIDATES),
                         ("MAX_LATTICE_OPS", MAX_LATTICE_OPS), ("INFO", INFO), ("STATUS_IMAGES", STATUS_IMAGES),
                         ("STATUS_OVERFLOW", STATUS_OVERFLOW), ("STATUS_INPUT", STATUS_INPUT)):
        assert re.search(rf"#define\s+ALIGNN_SYM_{macro}\s+(\d+)", text).group(1) == str(value), macro


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


def _host_compiler():
    for cc in ("/opt/rocm/lib/llvm/bin/clang", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib/llvm/bin/clang")):
        if os.path.exists(cc):
            return cc
    return shutil.which("clang") or shutil.which("cc") or shutil.which("gcc")


def test_argument_block_layouts_match_the_compiler(tmp_path):
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C compiler")
    blocks = (("alignn_sym_find_args", FindArgs), ("alignn_sym_apply_args", ApplyArgs))
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "alignn_sym.h"', "int main(void) {"]
    want = []
    for name, block in blocks:
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        want.append((name, str(C.sizeof(block))))
        for field, _ in block._fields_:
            c_field = field.rstrip("_")  # (`in` is spelt `in_` on the Python side)
            lines.append(f'    printf("{name}.{field} %zu\\n", offsetof({name}, {c_field}));')
            want.append((f"{name}.{field}", str(getattr(block, field).offset)))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = [tuple(ln.split()) for ln in out if ln]
    assert len(want) == 2 + 26 + 14 and seen == want
