"""include/poulpy_hip.h, the single source of truth for the C ABI, read into Python objects.

`parse()` is the one header parser: tools/gen_rust_ffi.py renders the Rust `extern "C"` block from it, and importing this module
builds the ctypes view of the header from it:

* one ``ctypes.Structure`` per ``typedef struct``, under its C name (``pz_glwe_op_params``, ...), in ``STRUCTS`` - the parameter
  structs, declared without a tag; a struct declared WITH its tag (``typedef struct pz_bdd_node {...} pz_bdd_node;``: an element type
  of an array argument, not a parameter block) is typed the same way and listed in ``TAGGED_STRUCTS``;
* a struct composed OF parameter structs and declared ``struct name {...};`` with its typedef on a line of its own
  (``pz_fhe_uint_prepare_params``) is typed the same way and listed in ``COMPOSITE_STRUCTS``; a pointer to one is passed as ``c_void_p``
  (``byref(...)``), like every pointer that is not to a parameter block.  (``STRUCTS`` is the list of the parameter BLOCKS, flat or
  with one block inside, which tests/test_abi_and_host.py pins; a struct that aggregates several of them is kept apart from it.)
* the enum constants (``PZ_OK``, ``PZ_AUTO_ADD``, ``PZ_K_FUSED_TAIL``, ...), in ``CONSTANTS``;
* ``PROTOTYPES``: ``name -> (restype, argtypes)`` of every ``pz_*`` function, which hal.load_library() applies.

Scalars map to their ctypes type; a pointer to a header struct to ``POINTER(struct)``; a ``const char*`` return to ``c_char_p``;
every other pointer, the module handle included, to ``c_void_p``, which accepts numpy ``.ctypes`` pointers, integer addresses
(torch ``data_ptr()``), ctypes arrays and ``byref(...)`` alike.
"""
from __future__ import annotations

import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "poulpy_hip.h")

SCALARS = {"size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "int": C.c_int, "uint32_t": C.c_uint32,
           "double": C.c_double, "float": C.c_float}
C_TYPE_NAMES = set(SCALARS) | {"char", "void"}


def strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def parse(header_text: str):
    """-> (structs, enums, funcs): [(name, [(field, C type)])], [(name, [(constant, value)])], [(name, C return type, [(param, C type)])],
    all in header order."""
    text = strip_comments(header_text)
    text = re.sub(r"#[^\n]*", " ", text)          # preprocessor lines
    text = text.replace('extern "C" {', " ")
    structs, enums, funcs = [], [], []
    for m in re.finditer(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in m.group(1).split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            # "uint64_t a, b" or "pz_blind_rotation_params br"
            first, rest = decl.split(" ", 1)
            for name in rest.split(","):
                fields.append((name.strip(), first))
        structs.append((m.group(2), fields))
    text_wo = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text_wo = re.sub(TAGGED_STRUCT, " ", text_wo, flags=re.S)
    text_wo = re.sub(COMPOSITE_STRUCT, " ", text_wo, flags=re.S)
    for m in re.finditer(r"(?:typedef\s+)?enum\s*\{(.*?)\}\s*(\w*)\s*;", text_wo, flags=re.S):
        vals, nxt = [], 0
        for item in m.group(1).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                name, v = [x.strip() for x in item.split("=")]
                nxt = int(v, 0)
            else:
                name = item
            vals.append((name, nxt))
            nxt += 1
        enums.append((m.group(2), vals))
    text_wo = re.sub(r"(?:typedef\s+)?enum\s*\{.*?\}\s*\w*\s*;", " ", text_wo, flags=re.S)
    text_wo = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", " ", text_wo)
    for m in re.finditer(r"([\w\s\*]+?)\b(pz_\w+)\s*\(([^()]*)\)\s*;", text_wo):
        ret = " ".join(m.group(1).split())
        name = m.group(2)
        args = []
        raw = " ".join(m.group(3).split())
        if raw and raw != "void":
            for k, a in enumerate(raw.split(",")):
                a = a.strip()
                mm = re.match(r"(.*?)(\w+)$", a)
                ty, nm = mm.group(1).strip(), mm.group(2)
                if not ty or nm in C_TYPE_NAMES or nm == "pz_module":   # unnamed parameter
                    ty, nm = a, f"arg{k}"
                args.append((nm, ty))
        funcs.append((name, ret, args))
    return structs, enums, funcs


TAGGED_STRUCT = r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;"


COMPOSITE_STRUCT = r"(?<![\w])(?<!typedef )struct\s+(\w+)\s*\{([^{}]*)\}\s*;"


def parse_composite(header_text: str):
    """-> [(name, [(field, C type)])] of the structs declared `struct name {...};` (their typedef follows on its own), in header order."""
    text = re.sub(r"#[^\n]*", " ", strip_comments(header_text))
    out = []
    for m in re.finditer(COMPOSITE_STRUCT, text, flags=re.S):
        fields = []
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if decl:
                first, rest = decl.split(" ", 1)
                fields += [(name.strip(), first) for name in rest.split(",")]
        out.append((m.group(1), fields))
    return out


def parse_tagged(header_text: str):
    """-> [(name, [(field, C type)])] of the structs declared with their tag, in header order."""
    text = re.sub(r"#[^\n]*", " ", strip_comments(header_text))
    out = []
    for m in re.finditer(TAGGED_STRUCT, text, flags=re.S):
        assert m.group(1) == m.group(3), m.group(0)
        fields = []
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if decl:
                first, rest = decl.split(" ", 1)
                fields += [(name.strip(), first) for name in rest.split(",")]
        out.append((m.group(3), fields))
    return out


def _ctype(decl: str, structs: dict, ret: bool = False):
    """C type of a parameter, field or return value -> ctypes type (None: a void return)."""
    toks = decl.replace("*", " * ").split()
    base = next(t for t in toks if t not in ("const", "*"))
    stars = toks.count("*")
    if stars == 0:
        return None if base == "void" else structs[base] if base in structs else SCALARS[base]
    if stars == 1 and base in structs:
        return C.POINTER(structs[base])
    if ret and stars == 1 and base == "char":
        return C.c_char_p
    return C.c_void_p


def _load():
    structs, enums, funcs = parse(open(HEADER).read())
    classes = {}
    for name, fields in structs:
        classes[name] = type(name, (C.Structure,), {"_fields_": [(f, _ctype(t, classes)) for f, t in fields],
                                                    "__doc__": f"{name} (include/poulpy_hip.h)"})
    tagged = {}
    for name, fields in parse_tagged(open(HEADER).read()):
        tagged[name] = type(name, (C.Structure,), {"_fields_": [(f, _ctype(t, classes)) for f, t in fields],
                                                   "__doc__": f"{name} (include/poulpy_hip.h)"})
    composite = {}
    for name, fields in parse_composite(open(HEADER).read()):
        composite[name] = type(name, (C.Structure,), {"_fields_": [(f, _ctype(t, classes)) for f, t in fields],
                                                      "__doc__": f"{name} (include/poulpy_hip.h)"})
    constants = {k: v for _, vals in enums for k, v in vals}
    known = {**classes, **tagged}
    protos = {name: (_ctype(ret, known, ret=True), [_ctype(t, known) for _, t in args]) for name, ret, args in funcs}
    return classes, tagged, composite, constants, protos


STRUCTS, TAGGED_STRUCTS, COMPOSITE_STRUCTS, CONSTANTS, PROTOTYPES = _load()
globals().update(STRUCTS)
globals().update(TAGGED_STRUCTS)
globals().update(COMPOSITE_STRUCTS)
globals().update(CONSTANTS)
