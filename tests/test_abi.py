"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/alignn_hip.h declares (no compute calls - there is no GPU here), and the ctypes table in
alignn_amd/_lib.py covers exactly that set.  The table and the argument structs are read from the header
(alignn_amd/_abi.py): the reader is checked on literal snippets, its struct layouts against a C compiler's
sizeof / offsetof of the real header, and their sizes against the library's."""

import ctypes as C
import keyword
import os
import re
import shutil
import subprocess

import pytest

from alignn_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "alignn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(alignn_[a-z0-9_]+)\s*\(", text))


def test_library_exports_every_declared_symbol():
    from alignn_amd.build import build

    build()
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    assert lib.alignn_version().decode().startswith("alignn_hip")


def test_ctypes_table_matches_header():
    assert set(_lib.SIGNATURES) == _declared()


def test_host_only_queries():
    lib = _lib.load()
    assert lib.alignn_col_stats_slabs(1) == 1
    assert lib.alignn_col_stats_slabs(10**7) == 1024 and lib.alignn_col_stats_slabs(3840) == 120
    assert lib.alignn_egc_slabs(0) == 1
    ws = lib.alignn_gemm_tn_workspace(10000, 256, 256)
    assert ws % (256 * 256 * 4) == 0 and 1 <= ws // (256 * 256 * 4) <= -(-10000 // 128)


# ---- the header reader (alignn_amd/_abi.py) on literal snippets -------------------------------------------------------------
def test_reader_on_fields_and_prototypes():
    structs, sigs = _abi.parse("""
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef void* handle_t; /* a comment with ; and ( and a fake prototype: int fake_entry(int x); */
        typedef struct inner {
            const float *a, *b;   /* several declarators; on one line */
            float* c, d;
            int32_t in, out;
            int64_t rows;
        } inner;
        /* int another_fake(void);
           over two lines */
        typedef struct outer {
            inner first, second;  /* by value */
            const inner* many;    /* a pointer to a struct */
            handle_t stream;
            size_t bytes;
            double x;
            int n;
        } outer;
        const char* name_of(void);
        int run(const outer* args, int64_t rows, float eps, double tol, size_t bytes, int flag, const uint8_t* mask, handle_t stream);
        size_t
        size_of(int which);
        #ifdef __cplusplus
        }
        #endif
    """)
    assert list(structs) == ["inner", "outer"]
    inner, outer = structs["inner"], structs["outer"]
    assert inner._fields_ == [("a", C.c_void_p), ("b", C.c_void_p), ("c", C.c_void_p), ("d", C.c_float), ("in_", C.c_int32),
                              ("out", C.c_int32), ("rows", C.c_int64)]
    assert outer._fields_ == [("first", inner), ("second", inner), ("many", C.c_void_p), ("stream", C.c_void_p),
                              ("bytes", C.c_size_t), ("x", C.c_double), ("n", C.c_int)]
    assert issubclass(inner, C.Structure) and inner.__name__ == "inner"
    assert C.sizeof(inner) == 48 and C.sizeof(outer) == 2 * 48 + 5 * 8 and outer.many.offset == 96 and inner.in_.offset == 28
    blank = outer()
    assert blank.many is None and blank.first.in_ == 0 and blank.x == 0.0  # a field left out is NULL / 0
    assert list(sigs) == ["name_of", "run", "size_of"]  # (nothing from inside the comments)
    assert sigs["name_of"] == (C.c_char_p, [])
    assert sigs["run"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_double, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p])
    assert sigs["size_of"] == (C.c_size_t, [C.c_int])


@pytest.mark.parametrize("text,where", [
    ("typedef struct s { int a;\n unsigned b; } s;", "line 2"),                 # an unknown type
    ("int f(int a,\n const foo_t* b);", "foo_t"),                               # ... also behind a pointer
    ("long f(void);", "long"),                                                  # ... and as a return type
    ("\ntypedef struct s { float a[3]; } s;", "line 2"),                        # an array field
    ("typedef struct s { int (*f)(int); } s;", "line 1"),                       # a function-pointer field
    ("typedef struct s { void v; } s;", "'v'"),                                 # no value of type void
    ("int f(void);\n\nstray\n;\nint g(void);", "line 3"),                      # text between declarations
    ("int f(void);\nint g(void)\n", "line 2"),                                 # an unfinished prototype
    ("typedef struct s { int a; } t;", "line 1"),                               # tag and name differ
    ("typedef struct s { struct { int a; } in; } s;", "line 1"),                # nested braces
    ("int f(void) { return 0; }", "line 1"),                                    # a definition
])
def test_reader_is_strict(text, where):
    with pytest.raises(ValueError, match=re.escape(where)):
        _abi.parse(text)


def test_derived_tables_of_the_real_header():
    assert _lib.SIGNATURES is _abi.SIGNATURES and len(_abi.SIGNATURES) == 162
    assert list(_abi.STRUCTS) == [
        "alignn_egc_fwd_args", "alignn_egc_bwd_args", "alignn_egc_wgrad_args", "alignn_mlp_params", "alignn_conv_params",
        "alignn_graph_csr", "alignn_model_batch", "alignn_model_desc", "alignn_ff_desc", "alignn_angle_args", "alignn_fire_args",
        "alignn_md_args"]
    assert _abi.SIGNATURES["alignn_version"] == (C.c_char_p, [])
    assert _abi.SIGNATURES["alignn_md_init_momenta"] == (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_double, C.c_void_p])
    assert _abi.SIGNATURES["alignn_egc_conv_fwd_scratch"] == (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int])
    assert _abi.STRUCTS["alignn_model_batch"].lg.offset == C.sizeof(_abi.STRUCTS["alignn_graph_csr"])
    assert "in_" in dict(_abi.STRUCTS["alignn_mlp_params"]._fields_)


# ---- layout against the compiler: sizeof / offsetof of every struct of the real header --------------------------------------
def _host_compiler():
    for cc in ("/opt/rocm/lib/llvm/bin/clang", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib/llvm/bin/clang")):
        if os.path.exists(cc):
            return cc
    return shutil.which("clang") or shutil.which("cc") or shutil.which("gcc")


def test_struct_layouts_match_the_compiler(tmp_path):
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "alignn_hip.h"', "int main(void) {"]
    for name, st in _abi.STRUCTS.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        for field, _ in st._fields_:
            c_field = field[:-1] if field.endswith("_") and keyword.iskeyword(field[:-1]) else field  # in_ -> in
            lines.append(f'    printf("{name} {field} %zu\\n", offsetof({name}, {c_field}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = [tuple(ln.split()) for ln in out if ln]
    want = []
    for name, st in _abi.STRUCTS.items():
        want.append((name, "sizeof", str(C.sizeof(st))))
        want += [(name, field, str(getattr(st, field).offset)) for field, _ in st._fields_]
    assert len(want) == 12 + sum(len(st._fields_) for st in _abi.STRUCTS.values()) > 300
    assert seen == want


# ---- sizes against the library ----------------------------------------------------------------------------------------------
def test_struct_sizes_match_the_library():
    lib = _lib.load()
    queries = {
        "alignn_egc_fwd_args": lambda: lib.alignn_egc_args_sizeof(0), "alignn_egc_bwd_args": lambda: lib.alignn_egc_args_sizeof(1),
        "alignn_egc_wgrad_args": lambda: lib.alignn_egc_args_sizeof(2),
        "alignn_mlp_params": lambda: lib.alignn_model_sizeof(0), "alignn_conv_params": lambda: lib.alignn_model_sizeof(1),
        "alignn_graph_csr": lambda: lib.alignn_model_sizeof(2), "alignn_model_batch": lambda: lib.alignn_model_sizeof(3),
        "alignn_model_desc": lambda: lib.alignn_model_sizeof(4),
        "alignn_ff_desc": lib.alignn_ff_desc_sizeof, "alignn_angle_args": lib.alignn_angle_args_sizeof,
        "alignn_fire_args": lib.alignn_fire_args_sizeof, "alignn_md_args": lib.alignn_md_args_sizeof}
    assert set(queries) == set(_abi.STRUCTS) and len(queries) == 12
    for name, query in queries.items():
        assert query() == C.sizeof(_abi.STRUCTS[name]), name
    assert [C.sizeof(st) for st in _abi.STRUCTS.values()] == [352, 424, 152, 104, 192, 104, 248, 728, 56, 312, 296, 336]
