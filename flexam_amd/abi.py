"""The one parse of include/flexam_hip.h: prototypes and constants of the C ABI, for the ctypes binding (hip.py) and the generator of
the replay dispatch table (gen_replay.py).

The type vocabulary is closed -- `int`, `int64_t`, `float`, `const char*`, any other `*` = pointer; return type `int` or
`const char*` -- and anything outside it raises with the prototype's name: a declared type is never guessed at, because a wrong width
does not fail, it truncates a stride."""
import os
import re
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flexam_hip.h")
_SCALARS = {"int": c_int, "int64_t": c_int64, "float": c_float}


def _code(header_text: str) -> str:
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S))


def ctype(c_type: str, where: str, returned: bool = False):
    """The ctypes type of a parameter (or return) type as the header spells it."""
    t = re.sub(r"\s*\*\s*", "*", " ".join(c_type.split()))
    if t == "const char*":
        return c_char_p
    if returned and t != "int":
        raise ValueError(f"{where}: return type '{c_type}' (int or const char* expected)")
    if re.fullmatch(r"[\w *]+\*", t):
        return c_void_p
    if t not in _SCALARS:
        raise ValueError(f"{where}: type '{c_type}' is outside the ABI's vocabulary (int, int64_t, float, const char*, pointers)")
    return _SCALARS[t]


def prototypes(header_text: str):
    """[(name, return type, [(C type, parameter name), ...])] of every flexam_* prototype, in header order."""
    out = []
    for stmt in _code(header_text).split(";"):
        stmt = " ".join(re.sub(r"^\s*#.*$", " ", stmt, flags=re.M).split())
        stmt = stmt[max(stmt.rfind("{"), stmt.rfind("}")) + 1:].strip()            # extern "C" {, the typedefs' bodies
        named = re.search(r"\b(flexam_\w+)\s*\(", stmt)
        if not named:
            continue
        m = re.fullmatch(r"([\w \*]+?)\s*\b(flexam_\w+)\s*\(([^()]*)\)", stmt)
        if not m:
            raise ValueError(f"{named.group(1)}: cannot parse the prototype '{stmt}'")
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        ctype(ret, name, returned=True)
        plist = []
        for prm in ([] if params in ("", "void") else params.split(",")):
            pm = re.fullmatch(r"(.*?)(\w+)", prm.strip())
            if not pm or not pm.group(1).strip():
                raise ValueError(f"{name}: cannot parse the parameter '{prm.strip()}'")
            ctype(pm.group(1), f"{name}({pm.group(2)})")
            plist.append((pm.group(1).strip(), pm.group(2)))
        out.append((name, ret, plist))
    return out


def signatures(protos):
    """{name: ([ctypes argument types], ctypes return type)} in header order."""
    return {n: ([ctype(t, n) for t, _ in p], ctype(r, n, returned=True)) for n, r, p in protos}


def stream_ordered(protos):
    """[(name, parameters)] of the asynchronous entry points: int-returning, last parameter `void* stream`."""
    return [(n, p) for n, r, p in protos if r == "int" and p and p[-1] == ("void*", "stream")]


def replayable(protos):
    """The stream-ordered launches flexam_replay can re-issue (flexam_replay itself is not a launch but a list of them); their
    order is their function id."""
    return [(n, p) for n, p in stream_ordered(protos) if n != "flexam_replay"]


def constants(header_text: str):
    """{name: value} of the header's object-like #defines: an integer, a float with an f suffix, or a product of integers, each
    optionally in parentheses; anything else raises (nothing is evaluated)."""
    out = {}
    for name, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S[^\n]*?)[ \t]*$", _code(header_text), flags=re.M):
        v = body[1:-1].strip() if body.startswith("(") and body.endswith(")") else body
        if re.fullmatch(r"-?\d+", v):
            out[name] = int(v)
        elif re.fullmatch(r"-?\d+\.\d*f", v):
            out[name] = float(v[:-1])
        elif re.fullmatch(r"\d+(\s*\*\s*\d+)+", v):
            out[name] = 1
            for f in v.split("*"):
                out[name] *= int(f)
        else:
            raise ValueError(f"{name}: cannot read the constant '{body}'")
    return out


_TEXT = open(HEADER).read()
PROTOTYPES = prototypes(_TEXT)
CONSTANTS = constants(_TEXT)
