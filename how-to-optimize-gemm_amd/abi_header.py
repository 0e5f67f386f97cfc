"""include/mmult_hip.h as Python reads it.  The header is the one statement of the C ABI: the compiler holds the `extern "C"`
definitions to it, and api.py binds from what is parsed here, so no constant, export name or argument list is kept by hand.
  CONSTANTS   {"MMH_ERR_COMM": -6, ...}: every `#define MMH_<NAME> <integer expression>`, in header order
  PROTOTYPES  {"mmh_sgemm": (restype, [argtypes]), ...}: every mmh_* prototype as ctypes types, in header order
parse(path) reads any header of the same grammar (include/mmult_hip_q8.h: q8.py).  Parsed once at import; pure Python (ctypes for its type objects only: no library is loaded, no torch).  What the parser does
not know -- an operator in a constant, a type spelling in a prototype -- raises here, on the CPU, and names the place.
"""
from __future__ import annotations

import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmult_hip.h")


class HeaderError(ValueError):
    pass


def strip_comments(text: str) -> str:
    """Comments blanked out, line numbers kept."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)


def eval_int(expr: str) -> int:
    """The integer expressions the header uses: decimal literals (an `L` suffix allowed), parentheses, unary minus, `<<`."""
    tokens = re.findall(r"\d+L?|<<|[()-]|\S", expr)
    pos = 0

    def unary() -> int:
        nonlocal pos
        tok = tokens[pos] if pos < len(tokens) else ""
        pos += 1
        if tok == "-":
            return -unary()
        if tok == "(":
            v = shift()
            if pos >= len(tokens) or tokens[pos] != ")":
                raise HeaderError("unbalanced parenthesis")
            pos += 1
            return v
        if tok[:1].isdigit():
            return int(tok.rstrip("L"))
        raise HeaderError(f"unexpected {tok!r}")

    def shift() -> int:
        nonlocal pos
        v = unary()
        while pos < len(tokens) and tokens[pos] == "<<":
            pos += 1
            v <<= unary()
        return v

    v = shift()
    if pos != len(tokens):
        raise HeaderError(f"unexpected {tokens[pos]!r}")
    return v


def parse_constants(text: str, where: str = HEADER) -> dict:
    out = {}
    for no, line in enumerate(text.splitlines(), 1):
        m = re.match(r"\s*#\s*define\s+(MMH_\w+)\s+(\S.*)$", line)
        if m:
            try:
                out[m.group(1)] = eval_int(m.group(2))
            except HeaderError as e:
                raise HeaderError(f"{where}:{no}: #define {m.group(1)} {m.group(2).strip()}: {e}") from None
    return out


_SCALARS = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "float": C.c_float, "size_t": C.c_size_t}
_POINTEES = {"void", "int", "long", "float", "size_t", "int8_t", "int32_t"}
_HANDLE = re.compile(r"mmh_\w+_t")   # an opaque handle type: mmh_handle_t, mmh_shard_t, mmh_q8_weight_t


def ctype_of(spelling: str):
    """The ctypes type of a type as the header spells it (tokens joined by one blank: "const float *")."""
    if spelling in _SCALARS:
        return _SCALARS[spelling]
    if spelling in ("const char *", "char *"):
        return C.c_char_p
    words = spelling.split()
    if words[:1] == ["const"]:
        words = words[1:]
    # a handle, or one or two levels of pointer to a handle or a known pointee (const float **: where a pointer is returned)
    if _HANDLE.fullmatch(spelling) or (len(words) in (2, 3) and (words[0] in _POINTEES or _HANDLE.fullmatch(words[0]))
                                       and set(words[1:]) == {"*"}):
        return C.c_void_p
    raise HeaderError(f"unknown type {spelling!r}")


def parse_prototypes(text: str, where: str = HEADER) -> dict:
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)                  # preprocessor lines
    text = re.sub(r'extern\s+"C"\s*\{|^\s*\}\s*$', "", text, flags=re.M)
    out = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt or stmt.startswith("typedef "):
            continue
        m = re.fullmatch(r"(.+?)\b(mmh_\w+) ?\((.*)\)", stmt)
        if not m:
            raise HeaderError(f"{where}: not a prototype: {stmt!r}")
        ret, name, params = m.groups()
        try:
            argtypes = []
            for p in ([] if params.strip() == "void" else params.split(",")):
                pm = re.fullmatch(r"(.+?)\b(?!(?:const|void|char|int|long|float|size_t)\b)[A-Za-z_]\w*", p.strip())   # type, name
                if not pm:
                    raise HeaderError(f"unnamed or empty parameter {p.strip()!r}")
                argtypes.append(ctype_of(" ".join(re.findall(r"\w+|\*", pm.group(1)))))
            out[name] = (ctype_of(" ".join(re.findall(r"\w+|\*", ret))), argtypes)
        except HeaderError as e:
            raise HeaderError(f"{where}: {name}: {e}") from None
    return out


def parse(path: str):
    """(CONSTANTS, PROTOTYPES) of the header at `path`: its own #defines and prototypes (an #include is not followed)."""
    with open(path) as f:
        text = strip_comments(f.read())
    return parse_constants(text, path), parse_prototypes(text, path)


CONSTANTS, PROTOTYPES = parse(HEADER)


def constants(prefix: str) -> dict:
    """{name without `prefix`: value} of the constants that start with it, in header order."""
    return {name[len(prefix):]: v for name, v in CONSTANTS.items() if name.startswith(prefix)}
