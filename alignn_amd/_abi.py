"""The ctypes view of include/alignn_hip.h, derived from the header itself: ``STRUCTS`` (C struct name -> ``ctypes.Structure``
subclass, in declaration order) and ``SIGNATURES`` (entry point -> ``(restype, argtypes)``).

The header is regular enough for a small reader: ``typedef struct NAME { fields } NAME;``, ``typedef T NAME;`` and prototypes,
inside one ``extern "C"`` block.  The reader is strict rather than general: a type it does not know, an array or
function-pointer field, or any text left between the declarations it recognises raises ``ValueError`` with the line.
"""

from __future__ import annotations

import ctypes as C
import keyword
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "alignn_hip.h")

# the ctypes class of a value of each type (None: there is no such value); behind a `*` every type is c_void_p
_BASE = {"void": None, "char": C.c_char, "uint8_t": C.c_uint8, "uint64_t": C.c_uint64, "int": C.c_int, "int32_t": C.c_int32,
         "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}

_ITEM = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;"  # struct: tag, fields, name
                   r"|typedef\s+([^;{}()]+);"                               # alias
                   r"|([^;{}()]+?\b\w+)\s*\(([^;{}()]*)\)\s*;")             # prototype: return type with the name, parameters
_GAP = re.compile(r'\s*(extern\s*"C"\s*\{)?\s*\}?\s*')
_DECLARATION = re.compile(r"\s*(?:const\s+)?(\w+)\b(.*)", re.S)
_DECLARATOR = re.compile(r"\s*(\**)\s*(\w+)\s*")


def parse(text: str):
    """C declarations -> (structs, signatures)"""
    text = re.sub(r"/\*.*?\*/", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
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


with open(HEADER) as _f:
    STRUCTS, SIGNATURES = parse(_f.read())
