"""The C boundary read from its one statement, include/selfrecon_hip.h: the integer #defines, the argument structs as ctypes
classes and every prototype's (restype, argtypes).  _lib.py binds the library from this, so an entry point is declared once.

Pure Python: no torch, no library load.  The header is plain C99 in a regular style and this reads exactly that style; whatever it
does not understand raises AbiError naming the text -- a declaration skipped here would be a wrong call into a GPU kernel.

Mapping: every pointer (parameter or field, whatever it points at) is c_void_p, so callers pass addresses, byref() objects and ctypes
arrays; the scalar words map as _SCALARS says; a struct by value is its class; an array dimension is a literal or an earlier #define.
"""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "selfrecon_hip.h")    # (build._digest() hashes it)

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
            **{f"{u}int{n}_t": getattr(ctypes, f"c_{u}int{n}") for u in ("", "u") for n in (8, 16, 32, 64)}}
_POINTEE_ONLY = ("void", "char")
_RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}
_DECL = r"(const\s+)?(\w+)(\s*\*\s*|\s+)"                               # [const] word, then * or a blank
_NAME = r"(\w+)((?:\s*\[\s*\w+\s*\])*)"                                  # name [dim]...


class AbiError(ValueError):
    pass


def _ctype(word, star, structs, where):
    if word not in _SCALARS and word not in structs and not (star and word in _POINTEE_ONLY):
        raise AbiError(f"unknown type {word!r} in {where!r}")
    return ctypes.c_void_p if star else _SCALARS.get(word) or structs[word]


def _struct(name, body, defines, structs):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(_DECL + rf"({_NAME}(?:\s*,\s*{_NAME})*)", decl)
        if not m or ("*" in m.group(3) and "," in m.group(4)):                  # (`float* a, b` declares b a float: not written here)
            raise AbiError(f"cannot parse the field {decl!r} of {name}")
        base = _ctype(m.group(2), "*" in m.group(3), structs, decl)
        for field, dims in re.findall(_NAME, m.group(4)):
            t = base
            for dim in reversed(re.findall(r"\w+", dims)):
                if not dim.isdigit() and dim not in defines:
                    raise AbiError(f"undefined array dimension {dim!r} in {decl!r} of {name}")
                t = t * (int(dim) if dim.isdigit() else defines[dim])
            fields.append((field, t))
    if len({f for f, _ in fields}) != len(fields) or not fields:
        raise AbiError(f"struct {name} has no fields or repeats one")
    return type("".join(p.capitalize() for p in name.split("_")), (ctypes.Structure,), {"_fields_": fields})


def _prototype(ret, params, structs, where):
    ret = re.sub(r"\s*\*", "*", ret.strip())
    if ret not in _RETURNS:
        raise AbiError(f"unknown return type {ret!r} in {where!r}")
    argtypes = []
    for p in ([] if params.strip() == "void" else params.split(",")):
        m = re.fullmatch(_DECL + r"\w+", p.strip())
        if not m:
            raise AbiError(f"cannot parse the parameter {p.strip()!r} in {where!r}")
        argtypes.append(_ctype(m.group(2), "*" in m.group(3), structs, where))
    return _RETURNS[ret], argtypes


def parse(text):
    """(defines {name: int}, structs {C name: ctypes.Structure class}, functions {name: (restype, argtypes)}) of a header's text."""
    defines, structs, tagged, functions = {}, {}, {}, {}

    def fresh(name):
        if name in defines or name in structs or name in tagged or name in functions:
            raise AbiError(f"{name} is declared twice")
        return name

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*$", " ", text, flags=re.S | re.M)
    code = []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.fullmatch(r"\s*#\s*(\w+)\s*(\w*)\s*(.*?)\s*", line)
        if m.group(1) == "define" and m.group(2).startswith("SR_"):      # every SR_* define is an integer expression of earlier ones
            try:
                if not re.fullmatch(r"[\w\s()+*<-]+", m.group(3)):
                    raise SyntaxError
                value = int(eval(m.group(3), {"__builtins__": {}}, dict(defines)))
            except (SyntaxError, NameError, TypeError, ValueError) as e:
                raise AbiError(f"cannot evaluate {line.strip()!r}") from e
            defines[fresh(m.group(2))] = value
        elif not (m.group(1) in ("ifndef", "endif", "include") or (m.group(1) == "define" and not m.group(3))):     # (the include guard)
            raise AbiError(f"unknown preprocessor line {line.strip()!r}")
    code, end = "\n".join(code), 0
    for m in re.finditer(r"((?:[^;{]|\{[^}]*\})*);", code):
        end, s = m.end(), " ".join(m.group(1).split())
        if (d := re.fullmatch(r"typedef struct \{(.*)\} ?(\w+)", s)):
            structs[fresh(d.group(2))] = _struct(d.group(2), d.group(1), defines, structs)
        elif (d := re.fullmatch(r"struct (\w+) ?\{(.*)\}", s)):
            tagged[fresh(d.group(1))] = d.group(2)
        elif (d := re.fullmatch(r"typedef struct (\w+) (\w+)", s)):
            if d.group(1) not in tagged:
                raise AbiError(f"{s!r} names an undeclared struct")
            structs[fresh(d.group(2))] = _struct(d.group(2), tagged[d.group(1)], defines, structs)
        elif (d := re.fullmatch(r"([\w\s*]*[\s*])(\w+) ?\((.*)\)", s)):
            functions[fresh(d.group(2))] = _prototype(d.group(1), d.group(3), structs, s)
        else:
            raise AbiError(f"cannot parse the declaration {s!r}")
    if code[end:].strip():
        raise AbiError(f"cannot parse the declaration {' '.join(code[end:].split())!r}")
    return defines, structs, functions


def load():
    with open(HEADER) as fh:
        return parse(fh.read())
