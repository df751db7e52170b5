"""Parser of ``include/rechub_hip.h``, the one written copy of the C ABI: ``_lib.py`` derives its ctypes signatures, the
``RhPackItem`` layout and the ``RH_*`` constants from it.  It understands the plain C the header is written in and
raises ``ValueError`` on anything else; it never guesses a width."""
import ctypes
import os
import re

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rechub_hip.h")
_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
_POINTER = re.compile(r"(const\s+)?\w+\s*(\*\s*(const\s*)?)+\w*")


def _ctype(decl, where):
    """ctypes type of one parameter or field declaration (`const float* x`, `int64_t n`): any pointer is a c_void_p."""
    decl = decl.strip()
    if _POINTER.fullmatch(decl):
        return ctypes.c_void_p
    words = decl.split()
    if len(words) in (1, 2) and words[0] in _SCALARS and re.fullmatch(r"\w+", words[-1]):
        return _SCALARS[words[0]]
    raise ValueError(f"rechub_hip.h: cannot map `{decl}` in {where} to a ctypes type")


def parse(text):
    """-> ({name: (restype, [argtype, ...])} of every rh_* declaration, [(field, ctype), ...] of RhPackItem,
    {name: int} of every `#define RH_<NAME> <integer>`)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    macros = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(RH_\w*)(.*)$", text, flags=re.M):
        if not re.fullmatch(r"\s+(-?\d+|\(-?\d+\))\s*", value):
            raise ValueError(f"rechub_hip.h: #define {name}{value} is not an integer constant")
        macros[name] = int(value.strip(" \t()"))
    text = re.sub(r"#[ \t]*ifdef __cplusplus.*?#[ \t]*endif", " ", text, flags=re.S)  # extern "C" { and its }
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    struct = re.search(r"typedef\s+struct\s+RhPackItem\s*\{(.*?)\}\s*RhPackItem\s*;", text, flags=re.S)
    if struct is None:
        raise ValueError("rechub_hip.h: typedef struct RhPackItem not found")
    fields = [(f.split()[-1], _ctype(f, "RhPackItem")) for f in struct.group(1).split(";") if f.strip()]
    *decls, rest = (text[:struct.start()] + text[struct.end():]).split(";")
    if rest.strip():
        raise ValueError(f"rechub_hip.h: declaration cut off before `;`: {rest.strip()[:60]}")
    functions = {}
    for decl in decls:
        m = re.fullmatch(r"\s*(.*?)\s*\b(rh_\w+)\s*\((.*)\)\s*", decl, flags=re.S)
        if m is None:
            raise ValueError(f"rechub_hip.h: not a declaration of an rh_* function: {decl.strip()[:60]}")
        ret, name, params = m.groups()
        restype = ctypes.c_char_p if re.fullmatch(r"const\s+char\s*\*", ret) else _SCALARS.get(ret)
        if restype is None:
            raise ValueError(f"rechub_hip.h: cannot map the return type `{ret}` of {name}")
        params = [] if params.strip() == "void" else params.split(",")
        functions[name] = (restype, [_ctype(p, name) for p in params])
    return functions, fields, macros
