"""What a public header under include/ declares, read with regular expressions (no compiler): the entry points with the kind of their result
and of every argument, the `typedef struct`s field by field, and the ctypes kind each C kind must be bound as.  Shared by
tests/test_components_host.py (the gate over all components) and the per-component host tests.  A kind is the C type with `const` dropped
and every `*` moved to its end: `const float* const* x` -> "float**", `const void *a, *b` -> "void*" twice, `float lp[6]` -> "float" with
dims [6]."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# C kind -> the ctypes type of a binding (compared by identity: on this ABI c_int is c_int32, c_longlong is c_int64, c_size_t is c_uint64,
# exactly as int / int32_t and long long / int64_t are one machine type).  Pointers: see ctypes_agrees.
SCALARS = {"void": None, "int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
           "long long": C.c_longlong, "size_t": C.c_size_t, "float": C.c_float}

_DECLARATOR = r"([\s*]*)(\w+)((?:\s*\[\d+\])*)"


def code(header):
    """the text of include/<header> without comments and preprocessor lines"""
    text = open(os.path.join(INCLUDE, header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)


def _declarations(text):
    """`T a, *b[3]` -> [(name, kind, dims)]: the base type is shared, stars and array lengths belong to each declarator"""
    first, *rest = [p.strip() for p in text.split(",")]
    base, stars, name, dims = re.fullmatch(r"(.*?\w)" + _DECLARATOR, first, flags=re.S).groups()
    base = " ".join(w for w in base.replace("*", " * ").split() if w != "const")
    base, base_stars = base.replace(" *", "").replace("*", ""), base.count("*")
    out = []
    for stars, name, dims in [(stars, name, dims)] + [re.fullmatch(_DECLARATOR, p, flags=re.S).groups() for p in rest]:
        out.append((name, base + "*" * (base_stars + stars.count("*")), [int(n) for n in re.findall(r"\[(\d+)\]", dims)]))
    return out


def entry_points(header):
    """[(name, return kind, [argument kinds])] in the header's order; every `sat_*(...)` declaration is one"""
    out = []
    for ret, name, args in re.findall(r"([\w\s*]+?)\b(sat_\w+)\s*\(([^()]*)\)\s*;", code(header)):
        params = [] if args.strip() in ("", "void") else [_declarations(a)[0] for a in args.split(",")]
        assert not any(dims for _, _, dims in params), (name, args)      # (no array arguments in this ABI)
        out.append((name, _declarations(ret + " _")[0][1], [kind for _, kind, _ in params]))
    return out


def names(header):
    return sorted(n for n, _, _ in entry_points(header))


def structs(header):
    """{typedef name: [(field, kind, dims)]} of every `typedef struct [tag] { ... } name;`"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", code(header), flags=re.S):
        out[name] = [f for decl in body.split(";") if decl.strip() for f in _declarations(decl)]
    return out


def define(header, name):
    """the value of `#define name value`, as text"""
    return re.search(r"^#define " + name + r" (\S+)", open(os.path.join(INCLUDE, header)).read(), flags=re.M).group(1)


def ctypes_agrees(kind, ctype, dims=()):
    """is `ctype` (with array lengths `dims`, outermost first) a correct binding of the C kind?  `char*` is c_char_p; any other pointer is
    c_void_p or a ctypes POINTER(...) (to a Structure or to c_int32: what it points to is not compared)"""
    for n in dims:
        if not (isinstance(ctype, type) and issubclass(ctype, C.Array) and ctype._length_ == n):
            return False
        ctype = ctype._type_
    if isinstance(ctype, type) and issubclass(ctype, C.Array):
        return False
    if kind == "char*":
        return ctype is C.c_char_p
    if kind.endswith("*"):
        return ctype is C.c_void_p or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
    return kind in SCALARS and ctype is SCALARS[kind]
