"""What the ABI tests of every header under include/ share (test_abi.py, test_*_abi.py, test_thermo_ref.py): the names a header
declares and the names the library exports, read without alignn_amd/_abi.py; the struct layouts a C compiler gives; and the check
that a bound library carries the types the header declares."""

import ctypes as C
import keyword
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def declared(path):
    """Every ``alignn_*`` name followed by ``(`` outside the comments of the header at ``path``."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(alignn_[a-z0-9_]+)\s*\(", text))


def exported(lib_path, prefix):
    """The dynamic symbols the library defines whose names begin with ``prefix``."""
    nm = "/opt/rocm/lib/llvm/bin/llvm-nm" if os.path.exists("/opt/rocm/lib/llvm/bin/llvm-nm") else shutil.which("nm")
    if nm is None:
        pytest.skip("no nm")
    out = subprocess.run([nm, "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith(prefix)}


def host_compiler():
    for cc in ("/opt/rocm/lib/llvm/bin/clang", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib/llvm/bin/clang")):
        if os.path.exists(cc):
            return cc
    return shutil.which("clang") or shutil.which("cc") or shutil.which("gcc")


def layouts(header_name, structs, tmp_path):
    """(seen, want): ``(struct, "sizeof" or field, bytes)`` of every struct of ``structs`` (C name -> ctypes class) as a C program
    that includes ``header_name`` prints them (compiled with -std=c11 -Wall -Werror), and as ctypes lays them out."""
    cc = host_compiler()
    if cc is None:
        pytest.skip("no host C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header_name}"', "int main(void) {"]
    want = []
    for name, st in structs.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        want.append((name, "sizeof", str(C.sizeof(st))))
        for field, _ in st._fields_:
            c_field = field[:-1] if field.endswith("_") and keyword.iskeyword(field[:-1]) else field  # in_ -> in
            lines.append(f'    printf("{name} {field} %zu\\n", offsetof({name}, {c_field}));')
            want.append((name, field, str(getattr(st, field).offset)))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    return [tuple(ln.split()) for ln in out if ln], want


def assert_typed(lib, sigs):
    """Every entry point of ``sigs`` carries, on ``lib``, the result and argument types the header gives it."""
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
