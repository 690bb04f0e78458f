"""CPU-side checks of the third header, include/alignn_neb.h: it reads with the reader of alignn_amd/_abi.py, the built library
exports every name it declares (no compute calls - there is no GPU here), and the ctypes layout of its argument block agrees
with a C compiler's sizeof / offsetof and with the library's size query."""

import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from alignn_amd import _abi, _lib
from alignn_amd.neb import HEADER, MAX_IMAGES, SIGNATURES, STRUCTS, NebArgs, _load
from alignn_amd.thermo import SIGNATURES as THERMO_SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(alignn_[a-z0-9_]+)\s*\(", text))


def test_header_reads_and_the_library_exports_it():
    from alignn_amd.build import SOURCES, build

    assert "neb.hip" in SOURCES
    build()
    structs, sigs = _abi.parse(open(HEADER).read())
    assert list(structs) == ["alignn_neb_args"] == list(STRUCTS)
    assert set(sigs) == _declared(HEADER) == set(SIGNATURES) == {"alignn_neb_interpolate", "alignn_neb_forces",
                                                                  "alignn_neb_args_size"}
    assert not set(sigs) & (set(_abi.SIGNATURES) | set(THERMO_SIGNATURES))  # no name in two headers; their tables are untouched
    assert not set(structs) & set(_abi.STRUCTS)
    lib = _load()
    assert lib is _lib.load()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert sigs["alignn_neb_forces"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert sigs["alignn_neb_args_size"] == (C.c_size_t, [])
    assert sigs["alignn_neb_interpolate"] == (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p])
    assert re.search(r"#define\s+ALIGNN_NEB_MAX_IMAGES\s+(\d+)", open(HEADER).read()).group(1) == str(MAX_IMAGES)


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


def _host_compiler():
    for cc in ("/opt/rocm/lib/llvm/bin/clang", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib/llvm/bin/clang")):
        if os.path.exists(cc):
            return cc
    return shutil.which("clang") or shutil.which("cc") or shutil.which("gcc")


def test_argument_block_layout_matches_the_compiler(tmp_path):
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "alignn_neb.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(alignn_neb_args));']
    lines += [f'    printf("{field} %zu\\n", offsetof(alignn_neb_args, {field}));' for field, _ in NebArgs._fields_]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = [tuple(ln.split()) for ln in out if ln]
    want = [("sizeof", str(C.sizeof(NebArgs)))] + [(field, str(getattr(NebArgs, field).offset)) for field, _ in NebArgs._fields_]
    assert len(want) == 25 and seen == want
