"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/alignn_hip.h declares (no compute calls - there is no GPU here), and the ctypes table in
alignn_amd/_lib.py covers exactly that set.  The table and the argument structs are read from the header
(alignn_amd/_abi.py): the reader is checked on literal snippets, its struct layouts against a C compiler's
sizeof / offsetof of the real header, and their sizes against the library's.  The headers of the batched workflows
(``_abi.WORKFLOW_HEADERS``) have a test module each (test_*_abi.py); what spans them is here: their limits as ``_abi.defines``
reads them, ``_lib.bind``, and that no two headers declare the same name."""

import ctypes as C
import itertools
import re
import types

import pytest

from alignn_amd import _abi, _lib
from tests import abi_checks


def _declared():
    return abi_checks.declared(_abi.HEADER)


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
def test_struct_layouts_match_the_compiler(tmp_path):
    seen, want = abi_checks.layouts("alignn_hip.h", _abi.STRUCTS, tmp_path)
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


# ---- the limits of the headers: #define NAME literal ------------------------------------------------------------------------
def test_defines_on_literals():
    assert _abi.defines("""
        #ifndef GUARD_H
        #define GUARD_H
        #include <stdint.h>
        #define LIMIT 4096 /* a comment after the value */
        #  define MASK 0x10
        #define TAU 1e-4   /* a comment
                              over two lines */
        #define HALF -.5
        /* #define INSIDE_A_COMMENT 3 */
        int f(void);
        #endif
    """) == {"LIMIT": 4096, "MASK": 16, "TAU": 1e-4, "HALF": -0.5}
    found = _abi.defines("#define A 2\n#define B 2.0\n")
    assert (type(found["A"]), type(found["B"])) == (int, float)


LIMITS = {
    "alignn_hip.h": {},
    "alignn_thermo.h": {},
    "alignn_neb.h": {"ALIGNN_NEB_MAX_IMAGES": 64},
    "alignn_traj.h": {"ALIGNN_TRAJ_MAX_SPECIES": 8, "ALIGNN_TRAJ_MAX_BINS": 4096, "ALIGNN_TRAJ_MAX_IMAGE_RANGE": 8,
                      "ALIGNN_TRAJ_STATUS_IMAGES": 1},
    "alignn_sym.h": {"ALIGNN_SYM_MAX_ATOMS": 1024, "ALIGNN_SYM_MAX_IMAGE_RANGE": 8, "ALIGNN_SYM_MAX_CANDIDATES": 256,
                     "ALIGNN_SYM_MAX_LATTICE_OPS": 48, "ALIGNN_SYM_INFO": 8, "ALIGNN_SYM_STATUS_IMAGES": 1,
                     "ALIGNN_SYM_STATUS_OVERFLOW": 2, "ALIGNN_SYM_STATUS_INPUT": 4},
    "alignn_order.h": {"ALIGNN_ORDER_MAX_SPECIES": 8, "ALIGNN_ORDER_MAX_IMAGE_RANGE": 8, "ALIGNN_ORDER_MAX_NEIGHBORS": 64,
                       "ALIGNN_ORDER_MAX_BINS": 1024, "ALIGNN_ORDER_MAX_L": 12, "ALIGNN_ORDER_MAX_LS": 4, "ALIGNN_ORDER_MAX_HKL": 32,
                       "ALIGNN_ORDER_SQ_FRAME_CHUNK": 64, "ALIGNN_ORDER_STATUS_IMAGES": 1, "ALIGNN_ORDER_STATUS_NEIGHBORS": 2,
                       "ALIGNN_ORDER_STATUS_HKL": 4},
    "alignn_phsym.h": {"ALIGNN_PHSYM_MAX_ATOMS": 32, "ALIGNN_PHSYM_MAX_SITE_OPS": 48, "ALIGNN_PHSYM_N_CANDIDATES": 13,
                       "ALIGNN_PHSYM_TAU": 1e-4},
}


def _read(name):
    with open(abi_checks.INCLUDE + "/" + name) as f:
        return f.read()


def test_defines_of_the_real_headers():
    assert tuple(LIMITS) == ("alignn_hip.h",) + _abi.WORKFLOW_HEADERS
    for name, want in LIMITS.items():
        found = _abi.defines(_read(name))
        assert found == want and [type(found[k]) for k in want] == [type(v) for v in want.values()], name
        if name in _abi.WORKFLOW_HEADERS:
            assert _abi.header(name).defines == want and _abi.header(name) is _abi.header(name), name


@pytest.mark.parametrize("text,where", [
    ("#define A 1\n#define F(x) x", "line 2"),                                   # a function-like macro
    ("\n\n#define A (1)", "line 3"),                                             # not a literal: parentheses
    ("#define A 1 + 2", "'#define A 1 + 2'"),                                    # ... an expression
    ("#define A B", "line 1"),                                                   # ... another name
    ("#define A 1u", "line 1"),                                                  # ... a suffix
    ("#define A 010", "line 1"),                                                 # ... an octal literal
    ("#define A 1 \\\n 2", "line 1"),                                            # ... a continued line
    ("/* two\nlines */ #define A \"s\"", "line 2"),                              # ... a string, after a comment
    ("#define", "line 1"),                                                       # no name
])
def test_defines_is_strict(text, where):
    with pytest.raises(ValueError, match=re.escape(where)):
        _abi.defines(text)


# ---- one binder for the workflow headers (_lib.bind) -------------------------------------------------------------------------
def test_no_name_in_two_headers():
    read = {"alignn_hip.h": (_abi.STRUCTS, _abi.SIGNATURES)}
    for name in _abi.WORKFLOW_HEADERS:
        read[name] = (_abi.header(name).structs, _abi.header(name).signatures)
    assert len(read) == 7 and sum(len(sigs) for _, sigs in read.values()) == 162 + 3 + 3 + 9 + 7 + 8 + 9
    for (a, (structs_a, sigs_a)), (b, (structs_b, sigs_b)) in itertools.combinations(read.items(), 2):
        assert not set(sigs_a) & set(sigs_b), (a, b)
        assert not set(structs_a) & set(structs_b), (a, b)
        assert not (set(structs_a) | set(structs_b)) & (set(sigs_a) | set(sigs_b)), (a, b)


def test_every_argument_block_of_a_workflow_header_has_its_size_query(tmp_path):
    blocks = [s for name in _abi.WORKFLOW_HEADERS for s in _abi.header(name).structs]
    assert len(blocks) == 11
    odd = tmp_path / "alignn_odd.h"
    odd.write_text("typedef struct alignn_odd_args { int n; } alignn_odd_args;\nint alignn_odd(void);\n")
    with pytest.raises(ValueError, match="alignn_odd_args_size"):
        _abi.header(str(odd))
    odd.write_text("typedef struct alignn_odd_args { int n; } alignn_odd_args;\nint alignn_odd_args_size(void);\n")
    with pytest.raises(ValueError, match="alignn_odd_args_size"):  # (the query answers a size_t)
        _abi.header(str(odd))


def _stub(H, sizes):
    """An object with every entry point of ``H`` as a plain function, which takes ``restype`` / ``argtypes`` as attributes like
    a ctypes one; the size queries answer ``sizes``."""
    stub = types.SimpleNamespace()
    for name in H.signatures:
        setattr(stub, name, (lambda size: lambda *args: size)(sizes.get(name, 0)))
    return stub


def test_bind_refuses_a_library_of_another_header():
    H = _abi.header("alignn_traj.h")
    assert [C.sizeof(st) for st in H.structs.values()] == [136, 96]
    stub = _stub(H, {"alignn_traj_rdf_args_size": 136, "alignn_traj_corr_args_size": 104})
    with pytest.raises(RuntimeError, match="argument block alignn_traj_corr_args: library says 104 bytes, the header gives 96"):
        _lib.bind(H, stub)
    assert stub.alignn_traj_vdos.restype is C.c_int and stub.alignn_traj_rdf_args_size.restype is C.c_size_t
    with pytest.raises(RuntimeError, match="alignn_traj_corr_args"):  # (not remembered as bound: every call checks again)
        _lib.bind(H, stub)
    assert _lib.bind(H) is _lib.load()


def test_bind_returns_the_library_and_types_a_header_once(monkeypatch):
    lib = _lib.load()
    for name in _abi.WORKFLOW_HEADERS:
        H = _abi.header(name)
        assert _lib.bind(H) is lib and _lib._bound[H.path] is lib
        abi_checks.assert_typed(lib, H.signatures)
    typed = []
    monkeypatch.setattr(_lib, "_type", lambda lib, sigs: typed.append((lib, sigs)))
    for name in _abi.WORKFLOW_HEADERS:
        assert _lib.bind(_abi.header(name)) is lib
    assert typed == []
    neb = _abi.header("alignn_neb.h")
    monkeypatch.setitem(_lib._bound, neb.path, lib)  # (put back afterwards)
    other = _stub(neb, {"alignn_neb_args_size": C.sizeof(neb.structs["alignn_neb_args"])})
    assert _lib.bind(neb, other) is other and _lib.bind(neb, other) is other  # another library object: typed again, once
    assert typed == [(other, neb.signatures)]
