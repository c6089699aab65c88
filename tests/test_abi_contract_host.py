"""The hand-kept ctypes binding (speechdrivestemplates_amd/_lib.py) against the C header (include/sdt_hip.h), type by type.

Every value crosses this binding on its way to a kernel, and a drifted row fails silently: ``c_float`` where the header says ``double``,
``c_int`` where it says ``int64_t``, a forgotten ``restype`` on an ``int64_t`` size getter (truncated to 32 bits), a reordered structure
field.  The GPU tests call through the same table as the product code, so both sides would share the wrong row.  Here the header is
parsed (comments stripped; prototypes, structures, enumerators, macros) and compared with

  1. every row of ``_lib.SIGNATURES`` and every ``argtypes`` / ``restype`` that ``_lib.load()`` leaves on the library, argument by argument;
  2. the layout the C compiler gives the structures (gcc -std=c99: sizeof, offsetof, field sizes) and the values it gives the constants;
  3. (teeth) mutated COPIES of the table and of the structure classes, each of which the checks of 1 and 2 must reject by name;
  4. the number of arguments at every ``lib.sdt_*(...)`` call site of the package (ast), reached by a GPU test or not.

Host only: no GPU, exact equality of types, counts, sizes and offsets throughout."""
import ast
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO
from speechdrivestemplates_amd import _lib

HEADER = os.path.join(REPO, "include", "sdt_hip.h")
PACKAGE = os.path.join(REPO, "speechdrivestemplates_amd")

# C structure -> its ctypes mirror in _lib
STRUCT_MIRRORS = {"sdt_conv_geom": "ConvGeom", "sdt_norm_bwd": "NormBwd", "sdt_wt_desc": "WtDesc", "sdt_chain1d_layer": "ChainLayer"}

# (function, argument index) where the table may say c_void_p although the header names a structure type.  Only where the header documents
# that NULL may be passed or that the pointer is not a host pointer at all; everything else has to be the typed POINTER(...).
VOID_P_FOR_STRUCT = {
    # `table: device array of n_layers descriptors`: a DEVICE address (tensor.data_ptr()), which POINTER(WtDesc) would refuse
    ("sdt_weight_transpose_batched_f32", 0),
    # `inst`: the instance records live in device memory too (render.py uploads a numpy record array, render.INSTANCE, checked below)
    ("sdt_render_prepare_f64", 3),
}

# Header prototypes that are NOT rows of SIGNATURES: load() binds them one by one (the same set as tests/test_geometry.py's `extra`)
BOUND_OUTSIDE_TABLE = {"sdt_last_error", "sdt_abi_version", "sdt_get_conv_math", "sdt_conv_dw_workspace_bytes", "sdt_convsk_plan_bytes",
                       "sdt_convsk_workspace_bytes", "sdt_convsk_dw_plan_bytes", "sdt_convsk_dw_workspace_bytes", "sdt_convsk_plan_bytes_t",
                       "sdt_convsk_dw_plan_bytes_t", "sdt_convsk_get_spin_limit", "sdt_conv_dw_group_plan_bytes"}

RESTYPES = {"int": C.c_int, "int64_t": C.c_int64, "unsigned": C.c_uint, "const char*": C.c_char_p}


# ------------------------------------------------------------------------------------------------------------------------------------
# the header, parsed
# ------------------------------------------------------------------------------------------------------------------------------------
_SCALARS = {"int": "int", "int32_t": "int", "int64_t": "int64_t", "unsigned": "unsigned", "unsigned int": "unsigned", "uint32_t": "unsigned",
            "uint64_t": "uint64_t", "float": "float", "double": "double", "uint8_t": "uint8_t", "char": "char", "void": "void"}
_QUALIFIERS = ("const", "struct", "__restrict__", "restrict", "volatile")


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _declarator(decl, struct_names):
    """'const float* w' / 'int32_t dy[SDT_MAX_TAPS]' / 'void' -> (name or None, base class, pointer depth, array length expression or None)"""
    decl = decl.strip()
    array = None
    m = re.match(r"^(.*?)\[([^\]]+)\]$", decl)
    if m:
        decl, array = m.group(1).strip(), m.group(2).strip()
    if not re.match(r"^[\w\s\*]+$", decl):
        raise ValueError("cannot read the declaration %r" % decl)
    depth = decl.count("*")
    words = [w for w in re.findall(r"\w+", decl) if w not in _QUALIFIERS]
    known = lambda ws: " ".join(ws) in _SCALARS or " ".join(ws) in struct_names  # noqa: E731
    name = None
    if len(words) >= 2 and not known(words):
        name, words = words[-1], words[:-1]
    if not known(words):
        raise ValueError("unknown type in the declaration %r" % decl)
    base = " ".join(words)
    return name, _SCALARS.get(base, base), depth, array


def _return_type(text):
    return re.sub(r"\s*\*\s*", "*", " ".join(text.split()))


class Header(object):
    """prototypes: [(name, return type, [(name, class, depth)])] in header order; structs: {name: [(field, class, depth, array)]};
    enums: {enum name or '': [(enumerator, value)]}; defines: {macro: replacement text}; unparsed: statements nothing above could read"""

    def __init__(self, text):
        code = strip_comments(text)
        self.defines = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$", code, flags=re.M))
        code = re.sub(r"^[ \t]*#.*$", " ", code, flags=re.M)
        code, n_extern = re.subn(r'extern\s+"C"\s*\{', " ", code)
        self.prototypes, self.structs, self.enums, self.unparsed = [], {}, {}, []
        statements, depth, cur, stray = [], 0, [], 0
        for ch in code:
            if ch == "}" and depth == 0:
                stray += 1  # the brace that closes extern "C"
                continue
            depth += (ch == "{") - (ch == "}")
            if ch == ";" and depth == 0:
                statements.append(" ".join("".join(cur).split()))
                cur = []
            else:
                cur.append(ch)
        tail = "".join(cur).strip()
        if tail or stray != n_extern or depth != 0:
            self.unparsed.append("unbalanced text at the end of the header: %r (%d stray braces)" % (tail[:80], stray))
        struct_names = set(re.findall(r"typedef\s+struct\s+(\w+)", code))
        for st in statements:
            try:
                self._statement(st, struct_names)
            except ValueError as e:
                self.unparsed.append("%s: %s" % (e, st[:120]))
        self._by_name = {}
        for p in self.prototypes:
            self._by_name.setdefault(p[0], []).append(p)

    def _statement(self, st, struct_names):
        if not st:
            return
        m = re.match(r"^typedef struct (\w+) \{(.*)\} (\w+)$", st)
        if m:
            if m.group(1) != m.group(3):
                raise ValueError("structure tag and typedef name differ")
            fields = []
            for decl in m.group(2).split(";"):
                if not decl.strip():
                    continue
                parts = [p.strip() for p in decl.split(",")]
                first = _declarator(parts[0], struct_names)
                if first[2] and len(parts) > 1:
                    raise ValueError("several pointer declarators in one declaration")
                fields.append(first)
                type_words = parts[0][:parts[0].rindex(first[0])] if first[0] else None
                for more in parts[1:]:
                    fields.append(_declarator(type_words + " " + more, struct_names))
            if any(f[0] is None for f in fields):
                raise ValueError("a field without a name")
            self.structs[m.group(1)] = fields
            return
        m = re.match(r"^enum ?(\w*) ?\{(.*)\}$", st)
        if m:
            values, nxt = [], 0
            for item in m.group(2).split(","):
                if not item.strip():
                    continue
                mm = re.match(r"^\s*(\w+)\s*(?:=\s*(-?\d+))?\s*$", item)
                if not mm:
                    raise ValueError("cannot read the enumerator %r" % item)
                nxt = int(mm.group(2)) if mm.group(2) is not None else nxt
                values.append((mm.group(1), nxt))
                nxt += 1
            self.enums.setdefault(m.group(1), []).extend(values)
            return
        m = re.match(r"^([\w\s\*]+?)\b(sdt_\w+) ?\((.*)\)$", st)
        if m:
            ret = _return_type(m.group(1))
            params = [] if m.group(3).strip() == "void" else [_declarator(p, struct_names) for p in m.group(3).split(",")]
            for p in params:
                if p[3] is not None or (p[1] == "void" and p[2] == 0):
                    raise ValueError("cannot classify the parameter %r" % (p,))
            self.prototypes.append((m.group(2), ret, [p[:3] for p in params]))
            return
        raise ValueError("not a prototype, structure or enumeration")

    def proto(self, name):
        hits = self._by_name.get(name, [])
        assert len(hits) == 1, "%d prototypes of %s in the header" % (len(hits), name)
        return hits[0]

    def names(self):
        return [p[0] for p in self.prototypes]

    def enumerators(self):
        return dict(kv for values in self.enums.values() for kv in values)


_HEADER = [None]


def header():
    if _HEADER[0] is None:
        _HEADER[0] = Header(open(HEADER).read())
    return _HEADER[0]


# ------------------------------------------------------------------------------------------------------------------------------------
# ctypes types, classified the same way
# ------------------------------------------------------------------------------------------------------------------------------------
_CODES = {"i": "int", "q": "int64_t", "I": "unsigned", "Q": "uint64_t", "f": "float", "d": "double", "B": "uint8_t", "c": "char", "b": "char"}
if C.sizeof(C.c_long) == 8:
    _CODES.update({"l": "int64_t", "L": "uint64_t"})
elif C.sizeof(C.c_long) == 4:
    _CODES.update({"l": "int", "L": "unsigned"})


def ctype_class(t):
    """a ctypes type -> ('scalar', class) | ('void*',) | ('char*',) | ('ptr', what it points to) | ('struct', the class) | ('?', repr)"""
    if isinstance(t, type) and issubclass(t, C.Structure):
        return ("struct", t)
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return ("ptr", ctype_class(t._type_))
    if isinstance(t, type) and issubclass(t, C._SimpleCData):
        code = t._type_
        if code == "P":
            return ("void*",)
        if code == "z":
            return ("char*",)
        if code in _CODES:
            return ("scalar", _CODES[code])
    return ("?", repr(t))


def _show(cls):
    if cls[0] == "scalar":
        return cls[1]
    if cls[0] == "struct":
        return cls[1].__name__
    if cls[0] == "ptr":
        return "POINTER(%s)" % _show(cls[1])
    return cls[0] if cls[0] != "?" else cls[1]


def _show_param(p):
    return p[1] + "*" * p[2]


def param_mismatch(fn, idx, param, ctype, structs, void_ok):
    """None when the ctypes type `ctype` passes what the header's parameter `param` = (name, class, depth) takes, else what is wrong"""
    _name, base, depth = param
    got = ctype_class(ctype)
    want = None
    if depth == 0:
        ok = got == ("scalar", base)
        want = base
    elif base in structs:  # a structure of the header; structs[base] is None for one that has no ctypes mirror
        typed = ("struct", structs[base])
        for _ in range(depth):
            typed = ("ptr", typed)
        ok = (structs[base] is not None and got == typed) or (got == ("void*",) and depth == 1 and (fn, idx) in void_ok)
        want = _show(typed) if structs[base] is not None else "%s (no mirror: c_void_p, listed as an exception)" % _show_param(param)
    elif got == ("void*",):
        ok = True
    elif got == ("char*",):
        ok = base == "char" and depth == 1
    elif got[0] == "ptr":  # a typed pointer in the table has to point at what the header says
        ok = (depth >= 2 and got[1] == ("void*",)) or (depth == 1 and got[1] == ("scalar", base))
    else:
        ok = False
    if ok:
        return None
    return "%s argument %d (%s): the header says %s, the binding %s" % (fn, idx, param[0], want or _show_param(param), _show(got))


def argument_errors(hdr, table, structs, void_ok):
    """every disagreement between `table` (name -> argtypes) and the header's prototypes, as messages that start with the function's name"""
    errors = []
    for fn, argtypes in table.items():
        if fn not in hdr._by_name:
            errors.append("%s: bound but not declared in the header" % fn)
            continue
        params = hdr.proto(fn)[2]
        if argtypes is None:
            errors.append("%s: argtypes never set (the header declares %d parameters)" % (fn, len(params)))
            continue
        if len(argtypes) != len(params):
            errors.append("%s: the header declares %d parameters, the binding passes %d" % (fn, len(params), len(argtypes)))
            continue
        for idx, (param, ctype) in enumerate(zip(params, argtypes)):
            msg = param_mismatch(fn, idx, param, ctype, structs, void_ok)
            if msg:
                errors.append(msg)
    return errors


def restype_errors(hdr, restypes):
    """`restypes`: name -> the ctypes restype in force; every header prototype has to be there with the type its return type maps to"""
    errors = []
    for fn, ret, _params in hdr.prototypes:
        if ret not in RESTYPES:
            errors.append("%s: no ctypes mapping for the return type %r" % (fn, ret))
        elif fn not in restypes:
            errors.append("%s: not bound" % fn)
        elif restypes[fn] is not RESTYPES[ret]:
            errors.append("%s returns %s in the header, its restype is %s" % (fn, ret, getattr(restypes[fn], "__name__", restypes[fn])))
    return errors


def mirrors():
    """C structure -> ctypes class, None for a structure of the header that _lib does not mirror"""
    found = dict.fromkeys(header().structs)
    found.update({c: getattr(_lib, py) for c, py in STRUCT_MIRRORS.items()})
    return found


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. prototypes, argument by argument
# ------------------------------------------------------------------------------------------------------------------------------------
def test_parser_reads_every_declaration():
    hdr = header()
    assert hdr.unparsed == [], "the header has statements the parser cannot read:\n" + "\n".join(hdr.unparsed)
    crude = re.findall(r"\b(sdt_\w+)\s*\(", strip_comments(open(HEADER).read()))  # every `sdt_name(` outside a comment is a declaration
    assert len(hdr.prototypes) == len(crude), sorted(set(crude) ^ set(hdr.names()))
    assert sorted(hdr.names()) == sorted(crude)
    assert len(set(hdr.names())) == len(hdr.names()), "a function is declared twice"
    assert len(hdr.prototypes) >= 203
    assert set(STRUCT_MIRRORS) <= set(hdr.structs)
    assert set(hdr.structs) == set(STRUCT_MIRRORS) | {"sdt_render_instance"}, "a new structure needs a mirror and a layout check here"


def test_signature_table_matches_the_header():
    hdr = header()
    errors = argument_errors(hdr, _lib.SIGNATURES, mirrors(), VOID_P_FOR_STRUCT)
    assert errors == [], "\n".join(errors)
    # the exceptions are not a licence: each names a structure-pointer parameter that the table does pass as c_void_p
    for fn, idx in VOID_P_FOR_STRUCT:
        _name, base, depth = hdr.proto(fn)[2][idx]
        assert base in hdr.structs and depth == 1, (fn, idx)
        assert _lib.SIGNATURES[fn][idx] is C.c_void_p, "stale exception: %s argument %d is typed now" % (fn, idx)


def test_table_and_header_cover_the_same_functions():
    hdr = header()
    assert set(hdr.names()) - set(_lib.SIGNATURES) == BOUND_OUTSIDE_TABLE
    assert set(_lib.SIGNATURES) <= set(hdr.names()), sorted(set(_lib.SIGNATURES) - set(hdr.names()))
    assert len(_lib.SIGNATURES) + len(BOUND_OUTSIDE_TABLE) == len(hdr.prototypes)


def _loaded():
    try:
        return _lib.load()
    except ImportError:
        if os.path.exists(_lib.LIB_PATH):
            raise
        pytest.skip("libsdt_hip.so is absent and cannot be built here (no hipcc): nothing carries argtypes / restype to inspect")


def test_loaded_library_carries_the_header_types():
    """What load() actually left on the CDLL object (not the text of load()): argtypes and restype of EVERY declared function, the rows of
    the table and the twelve functions bound one by one."""
    hdr, lib = header(), _loaded()
    missing = [fn for fn in hdr.names() if not hasattr(lib, fn)]
    assert missing == [], "libsdt_hip.so does not export %s" % missing
    bound = {fn: getattr(lib, fn) for fn in hdr.names()}
    errors = argument_errors(hdr, {fn: f.argtypes for fn, f in bound.items()}, mirrors(), VOID_P_FOR_STRUCT)
    errors += restype_errors(hdr, {fn: f.restype for fn, f in bound.items()})
    assert errors == [], "\n".join(errors)
    for fn, argtypes in _lib.SIGNATURES.items():
        assert list(bound[fn].argtypes) == list(argtypes), fn
    assert lib.sdt_abi_version() == _lib.ABI_VERSION == int(hdr.defines["SDT_ABI_VERSION"])


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. structure layouts and constants against the compiler
# ------------------------------------------------------------------------------------------------------------------------------------
def probe_source(hdr):
    """a C program that prints what the compiler makes of the header: generated from the PARSED header, nothing is typed a second time"""
    out = ["#include <stdio.h>", "#include <stddef.h>", '#include "sdt_hip.h"', "int main(void) {"]
    for name, fields in hdr.structs.items():
        out.append('    printf("sizeof %s %%lu\\n", (unsigned long)sizeof(%s));' % (name, name))
        for f in fields:
            out.append('    printf("field %s %s %%lu %%lu\\n", (unsigned long)offsetof(%s, %s), (unsigned long)sizeof(((%s*)0)->%s));'
                       % (name, f[0], name, f[0], name, f[0]))
    for const in list(hdr.enumerators()) + sorted(hdr.defines):
        out.append('    printf("const %s %%lld\\n", (long long)(%s));' % (const, const))
    return "\n".join(out + ["    return 0;", "}", ""])


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{'sizeof': {struct: n}, 'fields': {struct: [(field, offset, size)]}, 'const': {name: value}} as gcc -std=c99 sees the header"""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    tmp = tmp_path_factory.mktemp("abi_probe")
    src, exe = str(tmp / "abi_probe.c"), str(tmp / "abi_probe")
    with open(src, "w") as f:
        f.write(probe_source(header()))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), src, "-o", exe])
    text = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    res = {"sizeof": {}, "fields": {}, "const": {}}
    for line in text.splitlines():
        w = line.split()
        if w[0] == "sizeof":
            res["sizeof"][w[1]] = int(w[2])
        elif w[0] == "field":
            res["fields"].setdefault(w[1], []).append((w[2], int(w[3]), int(w[4])))
        else:
            res["const"][w[1]] = int(w[2])
    return res


def _array_length(hdr, expr):
    return int(expr) if expr.isdigit() else int(hdr.defines[expr])


def struct_errors(hdr, compiled, cname, cls):
    """every disagreement between the ctypes structure `cls` and the C structure `cname`, as messages that name the structure and the field"""
    errors = []
    want = compiled["fields"][cname]
    got = [f[0] for f in cls._fields_]
    if got != [w[0] for w in want]:
        for i, (a, b) in enumerate(zip(got, [w[0] for w in want])):
            if a != b:
                errors.append("%s field %d is %s in the header, %s in %s" % (cname, i, b, a, cls.__name__))
        if len(got) != len(want):
            errors.append("%s has %d fields in the header, %s has %d" % (cname, len(want), cls.__name__, len(got)))
        return errors
    for (fname, off, size), parsed, (_n, ctype) in zip(want, hdr.structs[cname], cls._fields_):
        desc = getattr(cls, fname)
        if (desc.offset, desc.size) != (off, size):
            errors.append("%s.%s: offset %d size %d in C, offset %d size %d in %s" % (cname, fname, off, size, desc.offset, desc.size, cls.__name__))
        _pname, base, depth, array = parsed
        if array is not None:
            if not (isinstance(ctype, type) and issubclass(ctype, C.Array)) or ctype._length_ != _array_length(hdr, array):
                errors.append("%s.%s: an array of %s in C, %r in %s" % (cname, fname, array, ctype, cls.__name__))
                continue
            ctype = ctype._type_
        got_cls = ctype_class(ctype)
        ok = got_cls[0] in ("void*", "ptr") if depth else got_cls == ("scalar", base)
        if not ok:
            errors.append("%s.%s: %s in C, %s in %s" % (cname, fname, base + "*" * depth, _show(got_cls), cls.__name__))
    if C.sizeof(cls) != compiled["sizeof"][cname]:
        errors.append("%s: sizeof %d in C, %d in %s" % (cname, compiled["sizeof"][cname], C.sizeof(cls), cls.__name__))
    return errors


@pytest.mark.parametrize("cname", sorted(STRUCT_MIRRORS))
def test_structure_layout_matches_the_compiler(compiled, cname):
    hdr = header()
    assert [f[0] for f in hdr.structs[cname]] == [f[0] for f in compiled["fields"][cname]]
    errors = struct_errors(hdr, compiled, cname, getattr(_lib, STRUCT_MIRRORS[cname]))
    assert errors == [], "\n".join(errors)


def test_render_instance_record_matches_the_compiler(compiled):
    """sdt_render_instance has no ctypes mirror: render.py uploads a numpy record array whose dtype has to be the C layout"""
    from speechdrivestemplates_amd import render
    dt, hdr = render.INSTANCE, header()
    assert dt.itemsize == compiled["sizeof"]["sdt_render_instance"]
    assert list(dt.names) == [f[0] for f in compiled["fields"]["sdt_render_instance"]]
    kinds = {"int": "i", "int64_t": "i", "double": "f", "float": "f"}
    for (fname, off, size), parsed in zip(compiled["fields"]["sdt_render_instance"], hdr.structs["sdt_render_instance"]):
        sub, sub_off = dt.fields[fname][:2]
        assert (sub_off, sub.itemsize, sub.kind) == (off, size, kinds[parsed[1]]), fname
        assert parsed[2] == 0 and parsed[3] is None


def test_constants_match_the_header(compiled):
    hdr, const = header(), compiled["const"]
    for name, value in hdr.enumerators().items():  # the parser's reading of the enumerations is the compiler's
        assert const[name] == value, name
    assert const["SDT_MAX_TAPS"] == _lib.MAX_TAPS
    assert const["SDT_ABI_VERSION"] == _lib.ABI_VERSION
    assert (const["SDT_F32"], const["SDT_BF16"]) == (_lib.F32, _lib.BF16)
    assert [n for n, _v in hdr.enums["sdt_dtype"]] == ["SDT_F32", "SDT_BF16"]
    assert (const["SDT_CHAIN_PLAIN"], const["SDT_CHAIN_NORM"], const["SDT_CHAIN_UPADD"]) == (_lib.CHAIN_PLAIN, _lib.CHAIN_NORM, _lib.CHAIN_UPADD)
    assert const["SDT_OK"] == 0  # _lib.check: `status != 0` raises
    assert dict(hdr.enums["sdt_status"]) == {"SDT_OK": 0, "SDT_ERR_ARG": -1, "SDT_ERR_LAUNCH": -2, "SDT_ERR_UNSUPPORTED": -3}
    # every status the package compares against by value says which one it means; the value has to be the header's
    seen = []
    for path in package_sources():
        for n, line in enumerate(open(path).read().splitlines(), 1):
            m = re.search(r"\bstatus\s*[!=]=\s*(-\d+)\s*(?::|\)|and|or)?\s*(?:#\s*(SDT_\w+))?", line)
            if m:
                where = "%s:%d" % (os.path.relpath(path, REPO), n)
                assert m.group(2) in const, "%s compares a status with %s without naming the enumerator" % (where, m.group(1))
                assert const[m.group(2)] == int(m.group(1)), where
                seen.append(m.group(2))
    assert seen.count("SDT_ERR_UNSUPPORTED") >= 3 and set(seen) == {"SDT_ERR_UNSUPPORTED"}, seen
    # flag words that Python modules mirror as module constants
    from speechdrivestemplates_amd import gif, jpeg, prdc
    assert (gif.ERR_RANGE, gif.ERR_COUNT) == (const["SDT_GIF_ERR_RANGE"], const["SDT_GIF_ERR_COUNT"])
    assert (jpeg.ERR_STAGE, jpeg.ERR_RANGE) == (const["SDT_JPEG_ERR_STAGE"], const["SDT_JPEG_ERR_RANGE"])
    assert (prdc.ERR_REAL_ROWS, prdc.ERR_GEN_ROWS) == (const["SDT_PRDC_ERR_REAL_ROWS"], const["SDT_PRDC_ERR_GEN_ROWS"])


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. teeth: the checks above reject every kind of drift, on copies (never on _lib itself), and name the culprit
# ------------------------------------------------------------------------------------------------------------------------------------
def _table_copy():
    return {fn: list(argtypes) for fn, argtypes in _lib.SIGNATURES.items()}


def _rejected(table, fn, void_ok=VOID_P_FOR_STRUCT):
    errors = argument_errors(header(), table, mirrors(), void_ok)
    assert errors, "a mutated row of %s passes" % fn
    assert all(e.startswith(fn + ":") or e.startswith(fn + " ") for e in errors), errors
    return errors


def _scalar_positions(cls_name):
    return [(fn, i) for fn, argtypes in _lib.SIGNATURES.items() for i, t in enumerate(argtypes) if ctype_class(t) == ("scalar", cls_name)]


def test_teeth_float_for_double_and_int_for_int64():
    """EVERY float argument of the table bound as double (and back), every int64_t argument as int (and back): each is rejected by name"""
    assert argument_errors(header(), _table_copy(), mirrors(), VOID_P_FOR_STRUCT) == []
    for src, dst, dst_type in (("float", "double", C.c_double), ("double", "float", C.c_float), ("int64_t", "int", C.c_int),
                               ("int", "int64_t", C.c_int64), ("unsigned", "int", C.c_int), ("uint64_t", "int64_t", C.c_int64)):
        positions = _scalar_positions(src)
        assert positions, src
        for fn, i in positions:
            table = _table_copy()
            table[fn][i] = dst_type
            (msg,) = _rejected(table, fn)
            assert "argument %d " % i in msg and "says %s," % src in msg and msg.endswith("the binding " + dst), msg
    assert len(_scalar_positions("float")) >= 40 and len(_scalar_positions("int64_t")) >= 150


def test_teeth_swapped_and_dropped_arguments():
    """every adjacent pair of arguments of different class swapped; every row with one argument dropped (the last, and the first)"""
    swaps = 0
    for fn, argtypes in _lib.SIGNATURES.items():
        for i in range(len(argtypes) - 1):
            a, b = ctype_class(argtypes[i]), ctype_class(argtypes[i + 1])
            if a[0] == b[0] == "scalar" and a != b:
                table = _table_copy()
                table[fn][i], table[fn][i + 1] = table[fn][i + 1], table[fn][i]
                errors = _rejected(table, fn)
                assert len(errors) == 2 and "argument %d " % i in errors[0] and "argument %d " % (i + 1) in errors[1], errors
                swaps += 1
        if argtypes:
            for drop in (0, len(argtypes) - 1):
                table = _table_copy()
                del table[fn][drop]
                (msg,) = _rejected(table, fn)
                assert "declares %d parameters, the binding passes %d" % (len(argtypes), len(argtypes) - 1) in msg, msg
    assert swaps >= 100
    table = _table_copy()
    table["sdt_not_in_the_header"] = [C.c_int]
    assert _rejected(table, "sdt_not_in_the_header") == ["sdt_not_in_the_header: bound but not declared in the header"]
    table = _table_copy()
    table["sdt_convsk_grid"] = None
    assert "argtypes never set" in _rejected(table, "sdt_convsk_grid")[0]


def test_teeth_untyped_structure_pointers():
    """every POINTER(structure) of the table replaced by c_void_p, or by a pointer to ANOTHER structure; the listed exceptions typed as a
    pointer to the wrong structure; an exception that is not listed"""
    hdr, typed = header(), 0
    for fn, argtypes in _lib.SIGNATURES.items():
        for i, t in enumerate(argtypes):
            cls = ctype_class(t)
            if cls[0] == "ptr" and (cls[1][0] == "struct" or (cls[1][0] == "ptr" and cls[1][1][0] == "struct")):
                for wrong in (C.c_void_p, C.POINTER(_lib.WtDesc) if cls[1] != ("struct", _lib.WtDesc) else C.POINTER(_lib.ConvGeom)):
                    table = _table_copy()
                    table[fn][i] = wrong
                    (msg,) = _rejected(table, fn)
                    assert "argument %d " % i in msg and hdr.proto(fn)[2][i][0] in msg, msg
                typed += 1
    assert typed >= 20
    for fn, i in VOID_P_FOR_STRUCT:  # without its entry in the list each exception is a mismatch
        (msg,) = _rejected(_table_copy(), fn, void_ok=VOID_P_FOR_STRUCT - {(fn, i)})
        assert "argument %d " % i in msg, msg
    # a typed scalar pointer has to point at the header's element type
    table = _table_copy()
    assert ctype_class(table["sdt_conv_dw_group_plan"][3]) == ("ptr", ("scalar", "int64_t"))
    table["sdt_conv_dw_group_plan"][3] = C.POINTER(C.c_int32)
    assert "argument 3 " in _rejected(table, "sdt_conv_dw_group_plan")[0]


def test_teeth_return_types():
    """an int64_t (unsigned, const char*) return left at the default c_int, an int return widened, a function left unbound"""
    hdr = header()
    good = {fn: RESTYPES[ret] for fn, ret, _p in hdr.prototypes}
    assert restype_errors(hdr, good) == []
    n64 = 0
    for fn, ret, _p in hdr.prototypes:
        bad = dict(good)
        bad[fn] = C.c_int64 if ret == "int" else C.c_int
        (msg,) = restype_errors(hdr, bad)
        assert msg.startswith(fn + " returns " + ret), msg
        n64 += ret == "int64_t"
        del bad[fn]
        assert restype_errors(hdr, bad) == [fn + ": not bound"]
    assert n64 >= 35
    assert {ret for _fn, ret, _p in hdr.prototypes} == set(RESTYPES)


def _mutant(cls, fields):
    return type(cls.__name__, (C.Structure,), {"_fields_": fields})


def test_teeth_structure_fields(compiled):
    """every adjacent pair of fields swapped, every field widened or retyped: each is rejected and the message names structure and field"""
    hdr = header()
    for cname, cls in ((c, getattr(_lib, py)) for c, py in STRUCT_MIRRORS.items()):
        assert struct_errors(hdr, compiled, cname, _mutant(cls, list(cls._fields_))) == []
        fields = list(cls._fields_)
        for i in range(len(fields) - 1):
            swapped = fields[:i] + [fields[i + 1], fields[i]] + fields[i + 2:]
            errors = struct_errors(hdr, compiled, cname, _mutant(cls, swapped))
            assert errors and all(e.startswith(cname + " field") for e in errors) and fields[i][0] in errors[0], errors
            # the same two TYPES swapped under unchanged names (a layout change the names do not show)
            if fields[i][1] is not fields[i + 1][1]:
                retyped = fields[:i] + [(fields[i][0], fields[i + 1][1]), (fields[i + 1][0], fields[i][1])] + fields[i + 2:]
                errors = struct_errors(hdr, compiled, cname, _mutant(cls, retyped))
                assert errors and any(e.startswith("%s.%s:" % (cname, fields[i][0])) for e in errors), errors
        for i, (fname, ctype) in enumerate(fields):
            if ctype is C.c_int32:
                for wrong in (C.c_int64, C.c_float, C.c_int16):
                    errors = struct_errors(hdr, compiled, cname, _mutant(cls, fields[:i] + [(fname, wrong)] + fields[i + 1:]))
                    assert errors and any(e.startswith("%s.%s:" % (cname, fname)) for e in errors), (fname, wrong, errors)
            elif ctype is C.c_float:
                errors = struct_errors(hdr, compiled, cname, _mutant(cls, fields[:i] + [(fname, C.c_int32)] + fields[i + 1:]))
                assert errors == ["%s.%s: float in C, int in %s" % (cname, fname, cls.__name__)], errors
            elif isinstance(ctype, type) and issubclass(ctype, C.Array):
                short = ctype._type_ * (ctype._length_ - 1)
                errors = struct_errors(hdr, compiled, cname, _mutant(cls, fields[:i] + [(fname, short)] + fields[i + 1:]))
                assert errors and any(e.startswith("%s.%s:" % (cname, fname)) for e in errors), errors
        errors = struct_errors(hdr, compiled, cname, _mutant(cls, fields[:-1]))
        assert errors == ["%s has %d fields in the header, %s has %d" % (cname, len(fields), cls.__name__, len(fields) - 1)], errors


def test_teeth_parser_does_not_lose_declarations():
    """a prototype the parser cannot read is reported, it does not vanish; a new return type or structure is seen"""
    text = open(HEADER).read()
    marker = "int sdt_abi_version(void);"
    assert text.count(marker) == 1
    for extra, what in (("int sdt_new_a(int (*callback)(int), void* stream);", "sdt_new_a"), ("int sdt_new_b(size_t n);", "unknown type"),
                        ("int sdt_new_c(int n, ...);", "sdt_new_c"), ("int sdt_new_d(int taps[4]);", "sdt_new_d"),
                        ("int sdt_new_e(void* stream)", "sdt_new_e")):
        hdr = Header(text.replace(marker, marker + "\n" + extra))
        assert hdr.unparsed and any(what in u for u in hdr.unparsed), (extra, hdr.unparsed)
    hdr = Header(text.replace(marker, marker + "\nfloat sdt_new_f(double x);\n/* int sdt_in_a_comment(int); */ // int sdt_in_another(int);"))
    assert hdr.unparsed == [] and hdr.proto("sdt_new_f") == ("sdt_new_f", "float", [("x", "double", 0)])
    assert "sdt_in_a_comment" not in hdr.names() and "sdt_in_another" not in hdr.names()
    assert "sdt_new_f: no ctypes mapping for the return type 'float'" in restype_errors(hdr, {})
    assert len(hdr.prototypes) == len(header().prototypes) + 1


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. call sites pass as many arguments as the table says
# ------------------------------------------------------------------------------------------------------------------------------------
def package_sources():
    found = []
    for root, _dirs, files in os.walk(PACKAGE):
        found += [os.path.join(root, f) for f in files if f.endswith(".py")]
    return sorted(found)


def _entries(node, strings=False):
    """the entry points an expression denotes: `x.sdt_a`, `x.sdt_a if c else x.sdt_b`, `getattr(x, 'sdt_a')`; with `strings` also 'sdt_a'"""
    if isinstance(node, ast.Attribute) and node.attr.startswith("sdt_"):
        return [node.attr]
    if isinstance(node, ast.IfExp):
        a, b = _entries(node.body, strings), _entries(node.orelse, strings)
        return a + b if a and b else []
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "getattr" and len(node.args) == 2:
        return _entries(node.args[1], True)
    if strings and isinstance(node, ast.Constant) and isinstance(node.value, str) and re.match(r"^sdt_[a-z0-9_]*[a-z0-9]$", node.value):
        return [node.value]
    return []


def _tuple_lengths(scope):
    """{'ctx.args': {6}}: the lengths of the tuple displays assigned to a name inside `scope`"""
    found = {}
    for n in ast.walk(scope):
        if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.value, ast.Tuple) \
                and not any(isinstance(e, ast.Starred) for e in n.value.elts):
            found.setdefault(ast.unparse(n.targets[0]), set()).add(len(n.value.elts))
    return found


def _positional(call, lengths):
    """number of positional arguments of a call; `*name` counts when every tuple display assigned to `name` in the enclosing class (or
    module) has one and the same length; None when it cannot be told"""
    if call.keywords:
        return None
    n = 0
    for a in call.args:
        if not isinstance(a, ast.Starred):
            n += 1
        elif isinstance(a.value, ast.Tuple) and not any(isinstance(e, ast.Starred) for e in a.value.elts):
            n += len(a.value.elts)
        elif len(lengths.get(ast.unparse(a.value), ())) == 1:
            n += next(iter(lengths[ast.unparse(a.value)]))
        else:
            return None
    return n


def _forwarders(tree):
    """{'_call': (index of the entry-point parameter, named parameters, arguments the helper adds)} for helpers of the form
    `def _call(fn, device, *args): ... fn(*args, stream)` or `def _call(name, *args): ... getattr(lib, name)(*args)`"""
    found = {}
    for f in ast.walk(tree):
        if not isinstance(f, ast.FunctionDef) or f.args.vararg is None:
            continue
        named = [a.arg for a in f.args.args]
        for c in ast.walk(f):
            if not isinstance(c, ast.Call) or c.keywords:
                continue
            stars = [a for a in c.args if isinstance(a, ast.Starred)]
            if len(stars) != 1 or not isinstance(stars[0].value, ast.Name) or stars[0].value.id != f.args.vararg.arg:
                continue
            target = c.func
            if isinstance(target, ast.Call) and isinstance(target.func, ast.Name) and target.func.id == "getattr" and len(target.args) == 2:
                target = target.args[1]
            if isinstance(target, ast.Name) and target.id in named:
                found[f.name] = (named.index(target.id), len(named), len(c.args) - 1)
    return found


def call_sites(paths):
    """-> (calls [(where, entry point, number of positional arguments, or None when it cannot be counted)], references {name: [where]}).
    A call is `<anything>.sdt_X(...)` wherever it stands (inside `check(...)`, in a lambda: ast.walk visits every expression), a call of
    `a.sdt_X if c else a.sdt_Y` or of a local name bound to one of those, and a call through a forwarding helper of the module
    (`_call(lib.sdt_X, device, ...)`, `_call('sdt_X', ...)`), counted as the helper passes it on.  A reference is every other mention: an
    attribute that is never called, a string that spells an entry point."""
    calls, refs = [], {}
    for path in paths:
        tree = ast.parse(open(path).read(), path)
        rel = os.path.relpath(path, REPO)
        owner, lengths = {}, {id(tree): _tuple_lengths(tree)}
        for cls in ast.walk(tree):  # breadth first: an inner class comes later and overrides
            if isinstance(cls, ast.ClassDef):
                lengths[id(cls)] = _tuple_lengths(cls)
                for n in ast.walk(cls):
                    owner[id(n)] = id(cls)
        aliases = {}  # id(call) -> entry points, for `fn = lib.sdt_a if c else lib.sdt_b` ... `fn(...)` inside one function
        for f in ast.walk(tree):
            if isinstance(f, (ast.FunctionDef, ast.Lambda)):
                bound = {}
                for n in ast.walk(f):
                    if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name) and _entries(n.value):
                        bound.setdefault(n.targets[0].id, []).append(n.value)
                for n in ast.walk(f):
                    if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in bound:
                        aliases[id(n)] = bound[n.func.id]
        helpers, used = _forwarders(tree), set()

        def use(expr):
            for n in ast.walk(expr):
                used.add(id(n))

        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            where = "%s:%d" % (rel, node.lineno)
            count = _positional(node, lengths[owner.get(id(node), id(tree))])
            if _entries(node.func):
                use(node.func)
                calls += [(where, fn, count) for fn in _entries(node.func)]
            elif id(node) in aliases:
                for value in aliases[id(node)]:
                    use(value)
                    calls += [(where, fn, count) for fn in _entries(value)]
            elif isinstance(node.func, ast.Name) and node.func.id in helpers:
                at, named, added = helpers[node.func.id]
                if len(node.args) > at and _entries(node.args[at], True):
                    use(node.args[at])
                    calls += [(where, fn, None if count is None else count - named + added) for fn in _entries(node.args[at], True)]
        for node in ast.walk(tree):
            if id(node) in used:
                continue
            if isinstance(node, ast.Attribute) and node.attr.startswith("sdt_"):
                refs.setdefault(node.attr, []).append("%s:%d" % (rel, node.lineno))
            elif isinstance(node, ast.Constant) and isinstance(node.value, str) and re.match(r"^sdt_\w+$", node.value):
                refs.setdefault(node.value, []).append("%s:%d" % (rel, node.lineno))
    return calls, refs


# Declared entry points that no module of the package calls (in a form the pass can see).  Every other one has at least one call site
# whose argument count is checked.
NO_CALL_SITE = {
    # called as getattr(lib, 'sdt_tensor_hist_' + k)() in ops.tensor_hist_constants: no argument to count
    "sdt_tensor_hist_threads": "dynamic name", "sdt_tensor_hist_chunk": "dynamic name", "sdt_tensor_hist_buckets": "dynamic name",
    "sdt_tensor_hist_max_segments": "dynamic name",
    # the C API's fp32-only forms of entry points the package reaches through their *_t (element type) forms
    "sdt_colnorm_fwd_f32": "C API", "sdt_colnorm_bwd_f32": "C API", "sdt_l0_block_fwd_f32": "C API", "sdt_l0_block_bwd_f32": "C API",
    "sdt_convsk_supported": "C API", "sdt_convsk_plan_bytes": "C API", "sdt_convsk_plan_build": "C API",
    "sdt_convsk_dw_supported": "C API", "sdt_convsk_dw_plan_bytes": "C API", "sdt_convsk_dw_plan_build": "C API",
    # the Jacobi eigensolver on its own: the package runs it inside fgd / code_pca / code_axes launches; benchmarks and host tests call it
    "sdt_code_pca_eigh": "tools", "sdt_code_axes_eigh": "tools and tests",
    # introspection for tests, benchmarks and C callers: launch grid, spin limit, interval count, which compose kernel a shape takes
    "sdt_convsk_grid": "tests", "sdt_convsk_get_spin_limit": "tests", "sdt_convsk_set_spin_limit": "tests",
    "sdt_jpeg_intervals": "tools and tests", "sdt_strip_compose_vectorised": "tools and tests",
}

# Call sites whose argument count the pass cannot tell, by (file, entry point): `*(_p(t) for t in ctx.tabs)` spreads a run-time list
UNCOUNTABLE = {("speechdrivestemplates_amd/ops.py", "sdt_bone_loss_bwd_f32")}


def count_errors(calls, expected, uncountable=()):
    errors = []
    for where, fn, nargs in calls:
        if fn.startswith("sdt_debug_"):
            continue  # hooks of the -DSDT_TUNING library: not part of the header
        if fn not in expected:
            errors.append("%s calls %s, which the header does not declare" % (where, fn))
        elif nargs is None:
            if (where.rsplit(":", 1)[0], fn) not in uncountable:
                errors.append("%s calls %s with * or keyword arguments: the count cannot be checked" % (where, fn))
        elif nargs != expected[fn]:
            errors.append("%s passes %d arguments to %s, the table says %d" % (where, nargs, fn, expected[fn]))
    return errors


def test_call_sites_pass_what_the_table_says():
    hdr = header()
    expected = {fn: len(params) for fn, _ret, params in hdr.prototypes}
    for fn, argtypes in _lib.SIGNATURES.items():
        assert expected[fn] == len(argtypes), fn
    calls, refs = call_sites(package_sources())
    assert len(calls) >= 200
    errors = count_errors(calls, expected, UNCOUNTABLE)
    assert errors == [], "\n".join(errors)
    assert {(w.rsplit(":", 1)[0], fn) for w, fn, n in calls if n is None} == UNCOUNTABLE, "stale entry in UNCOUNTABLE"
    called = {fn for _w, fn, _n in calls}
    uncalled = set(expected) - called
    assert uncalled == set(NO_CALL_SITE), "entry points without a call site in the package: %s" % sorted(uncalled ^ set(NO_CALL_SITE))
    # nothing is merely mentioned: an attribute that is taken but never called would be a call site the pass does not see
    loose = {fn: w for fn, w in refs.items() if fn in expected and any(not x.startswith("speechdrivestemplates_amd/_lib.py:") for x in w)}
    assert loose == {}, loose


def test_teeth_call_site_counter(tmp_path):
    src = tmp_path / "m.py"
    src.write_text("def _call(fn, device, *args):\n"
                   "    check(fn(*args, stream(device)))\n"
                   "def _named(name, *args):\n"
                   "    check(getattr(load(), name)(*args))\n"
                   "class A:\n"
                   "    def f(ctx, lib, check, s):\n"
                   "        ctx.args = (1, 2, 3)\n"
                   "        check(lib.sdt_a(1, 2, s))\n"
                   "        g = lambda x: lib.sdt_b(x, s)\n"
                   "        (lib.sdt_c if s else lib.sdt_d)(1)\n"
                   "        h = lib.sdt_e\n"
                   "        lib.sdt_f(*s)\n"
                   "        lib.sdt_g(0, *ctx.args, s)\n"
                   "        fn = lib.sdt_h if s else lib.sdt_i\n"
                   "        fn(1, 2)\n"
                   "        _call(lib.sdt_j, s, 1, 2)\n"
                   "        _named('sdt_k', 1, 2, s)\n"
                   "        return getattr(lib, 'sdt_l')(g, h)\n"
                   "class B:\n"
                   "    def f(ctx, lib):\n"
                   "        ctx.args = (1, 2)\n"
                   "        lib.sdt_m(*ctx.args)\n"
                   "        lib.sdt_n(k=1)\n"
                   "        return 'sdt_o'\n")
    calls, refs = call_sites([str(src)])
    assert sorted((fn, n) for _w, fn, n in calls) == [
        ("sdt_a", 3), ("sdt_b", 2), ("sdt_c", 1), ("sdt_d", 1), ("sdt_f", None), ("sdt_g", 5), ("sdt_h", 2), ("sdt_i", 2), ("sdt_j", 3),
        ("sdt_k", 3), ("sdt_l", 2), ("sdt_m", 2), ("sdt_n", None)]
    assert sorted(refs) == ["sdt_e", "sdt_o"]
    expected = dict.fromkeys("sdt_a sdt_b sdt_c sdt_d sdt_f sdt_g sdt_h sdt_i sdt_j sdt_k sdt_l sdt_m".split(), 2)
    errors = count_errors(calls, expected)
    assert sorted(e.split(" ", 1)[1] for e in errors) == sorted([
        "passes 3 arguments to sdt_a, the table says 2", "passes 1 arguments to sdt_c, the table says 2",
        "passes 1 arguments to sdt_d, the table says 2", "calls sdt_f with * or keyword arguments: the count cannot be checked",
        "passes 5 arguments to sdt_g, the table says 2", "passes 3 arguments to sdt_j, the table says 2",
        "passes 3 arguments to sdt_k, the table says 2", "calls sdt_n, which the header does not declare"]), errors
