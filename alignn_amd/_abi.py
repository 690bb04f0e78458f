"""The ctypes view of include/alignn_hip.h, derived from the header itself: ``STRUCTS`` (C struct name -> ``ctypes.Structure``
subclass, in declaration order) and ``SIGNATURES`` (entry point -> ``(restype, argtypes)``).

The header is regular enough for a small reader: ``typedef struct NAME { fields } NAME;``, ``typedef T NAME;`` and prototypes,
inside one ``extern "C"`` block.  The reader is strict rather than general: a type it does not know, an array or
function-pointer field, or any text left between the declarations it recognises raises ``ValueError`` with the line.

The limits a header sets (``#define NAME literal``) are read by ``defines``, and ``header(name)`` reads one header under
include/ whole: the batched workflows bind theirs from that record (``_lib.bind``) and take their limits from it.
"""

from __future__ import annotations

import ctypes as C
import keyword
import os
import re
from functools import lru_cache
from typing import NamedTuple

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "alignn_hip.h")

# the headers of the batched workflows, in the order they were added (build.py compiles against them, the tests walk them)
WORKFLOW_HEADERS = ("alignn_thermo.h", "alignn_neb.h", "alignn_traj.h", "alignn_sym.h", "alignn_order.h", "alignn_phsym.h")
# the headers added after those, in the same form and read and bound the same way (build.py compiles against them too)
LATER_HEADERS = ("alignn_idpp.h", "alignn_cells.h", "alignn_local.h")
# the headers of the trajectory analyses added after those, a tuple of their own (the tests of the two above walk them whole)
ANALYSIS_HEADERS = ("alignn_vanhove.h",)
# the headers of the per-atom structure analyses added after those, again a tuple of their own (the tests pin the three above)
STRUCTURE_HEADERS = ("alignn_voronoi.h",)

# the ctypes class of a value of each type (None: there is no such value); behind a `*` every type is c_void_p
_BASE = {"void": None, "char": C.c_char, "uint8_t": C.c_uint8, "uint64_t": C.c_uint64, "int": C.c_int, "int32_t": C.c_int32,
         "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}

_ITEM = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;"  # struct: tag, fields, name
                   r"|typedef\s+([^;{}()]+);"                               # alias
                   r"|([^;{}()]+?\b\w+)\s*\(([^;{}()]*)\)\s*;")             # prototype: return type with the name, parameters
_GAP = re.compile(r'\s*(extern\s*"C"\s*\{)?\s*\}?\s*')
_DECLARATION = re.compile(r"\s*(?:const\s+)?(\w+)\b(.*)", re.S)
_DECLARATOR = re.compile(r"\s*(\**)\s*(\w+)\s*")
_DIRECTIVE = re.compile(r"^[ \t]*#[ \t]*define\b(.*)$", re.M)
_MACRO = re.compile(r"[ \t]+(\w+)(?![\w(])[ \t]*(.*?)[ \t]*")  # an object-like macro: its name, its replacement text
_INT = re.compile(r"[+-]?(?:0[xX][0-9a-fA-F]+|[1-9][0-9]*|0)")
_FLOAT = re.compile(r"[+-]?(?:[0-9]+\.[0-9]*|\.[0-9]+|[0-9]+(?=[eE]))(?:[eE][+-]?[0-9]+)?")


def _uncomment(text: str) -> str:
    """The text without its comments, every line where it was."""
    return re.sub(r"/\*.*?\*/", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)


def parse(text: str):
    """C declarations -> (structs, signatures)"""
    text = re.sub(r"^[ \t]*#.*$", "", _uncomment(text), flags=re.M)
    types, structs, sigs = dict(_BASE), {}, {}

    def fail(what, at):
        raise ValueError(f"line {text.count(chr(10), 0, at) + 1}: {what}")

    def gap(a, b):
        if not _GAP.fullmatch(text, a, b):
            junk = text[a:b]
            fail(f"cannot read {junk.strip()!r}", a + len(junk) - len(junk.lstrip()))

    def decl(s, at):
        """'const T *a, b' (at that offset of the text) -> [(name, ctype), ...]"""
        at += len(s) - len(s.lstrip())
        m = _DECLARATION.fullmatch(s)
        if not m or m.group(1) not in types:
            fail(f"unknown type in {s.strip()!r}", at)
        out = []
        for d in m.group(2).split(","):
            dm = _DECLARATOR.fullmatch(d)
            ctype = (C.c_void_p if dm.group(1) else types[m.group(1)]) if dm else None
            if ctype is None:
                fail(f"cannot read the declarator {d.strip()!r} of {s.strip()!r}", at)
            name = dm.group(2)
            out.append((name + "_" if keyword.iskeyword(name) else name, ctype))
        return out

    pos = 0
    for m in _ITEM.finditer(text):
        gap(pos, m.start())
        pos = m.end()
        tag, body, name, alias, head, params = m.groups()
        if tag is not None:
            if tag != name:
                fail(f"struct {tag} is named {name}", m.start())
            fields = [f for s in body.split(";") if s.strip() for f in decl(s, m.start(2) + body.find(s))]
            types[name] = structs[name] = type(name, (C.Structure,), {"_fields_": fields})
        elif alias is not None:
            (name, ctype), = decl(alias, m.start())
            types[name] = ctype
        else:
            (name, res), = decl(head, m.start(5))
            if re.match(r"\s*const\s+char\s*\*", head):
                res = C.c_char_p
            args = [] if params.strip() == "void" else [decl(p, m.start(6))[0][1] for p in params.split(",")]
            sigs[name] = (res, args)
    gap(pos, len(text))
    return structs, sigs


def defines(text: str) -> dict:
    """``#define NAME literal`` -> {NAME: int or float}.  A macro without replacement text (an include guard) is skipped; a
    function-like macro, or a replacement that is not one integer or floating literal, raises ``ValueError`` with the line."""
    text, out = _uncomment(text), {}
    for m in _DIRECTIVE.finditer(text):
        macro = _MACRO.fullmatch(m.group(1))
        name, value = macro.groups() if macro else (None, None)
        if value and _INT.fullmatch(value):
            out[name] = int(value, 0)
        elif value and _FLOAT.fullmatch(value):
            out[name] = float(value)
        elif value != "":
            raise ValueError(f"line {text.count(chr(10), 0, m.start()) + 1}: cannot read the macro {m.group().strip()!r}")
    return out


class Header(NamedTuple):
    """One header under include/: its path, its structs and signatures as ``parse`` gives them, its limits as ``defines`` does."""
    path: str
    structs: dict
    signatures: dict
    defines: dict


@lru_cache(maxsize=None)
def header(name: str) -> Header:
    """The header include/``name`` of a batched workflow (an absolute path is read where it is), read once.  Every struct ``S`` of
    such a header is an argument block and comes with its size query ``size_t S_size(void)`` (``_lib.bind`` asks it): one
    without is a ``ValueError``."""
    path = os.path.join(os.path.dirname(HEADER), name)
    with open(path) as f:
        text = f.read()
    structs, sigs = parse(text)
    for block in structs:
        if sigs.get(block + "_size") != (C.c_size_t, []):
            raise ValueError(f"{name}: the argument block {block} has no size query size_t {block}_size(void)")
    return Header(path, structs, sigs, defines(text))


with open(HEADER) as _f:
    STRUCTS, SIGNATURES = parse(_f.read())
