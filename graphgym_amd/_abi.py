"""The C headers under include/ as the Python side's statement of the ABI: `header(name)` reads one of them, once per
process, into ctypes prototypes, integer constants, structures and callback types.  Not a C parser: it knows the few
forms these headers use (commented, unconditional declarations of functions, enums with explicit values, integer
#defines, one flat struct, two callback typedefs) and refuses everything else, at import."""
import collections
import ctypes as C
import functools
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

# The whole type map.  Beside it any pointer is a c_void_p (callers pass addresses, byref() and ctypes arrays), and a
# return type alone may be `void` or `const char*`.
TYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
         "double": C.c_double, "size_t": C.c_size_t,
         "mp_stream_t": C.c_void_p, "mp_alloc_fn": C.c_void_p, "mp_free_fn": C.c_void_p}
RETURNS = {"void": None, "char*": C.c_char_p}

Header = collections.namedtuple("Header", "prototypes constants structs callbacks")


class HeaderError(ImportError):
    pass


def _ctype(decl, owner, is_return=False):
    """'const int32_t* rowptr' -> ('rowptr', c_void_p); a return type has no name"""
    words = [w for w in re.findall(r"\w+|\S", decl) if w != "const"]
    name = None if is_return else words.pop() if words else ""
    what = f"{owner}: the return" if is_return else f"{owner}: '{name}'"
    if name is not None and not re.fullmatch(r"[A-Za-z_]\w*", name):
        raise HeaderError(f"{owner}: '{decl.strip()}' does not end in a name")
    ctype = " ".join(words).replace(" *", "*")
    if is_return and ctype in RETURNS:
        return name, RETURNS[ctype]
    if re.fullmatch(r"\w+\*+", ctype):
        return name, C.c_void_p
    if ctype not in TYPES:
        raise HeaderError(f"{what} has type '{ctype}', which is not in the type map")
    return name, TYPES[ctype]


def _signature(ret, name, params):
    params = [] if params.strip() in ("", "void") else params.split(",")
    return _ctype(ret, name, True)[1], [_ctype(p, name)[1] for p in params]


def parse(text):
    """the Header of one header's text"""
    protos, consts, structs, callbacks = {}, {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", "", text, flags=re.S)         # the extern "C" brackets

    def constant(name, value):
        try:
            value = int(value, 0)
        except ValueError:
            raise HeaderError(f"constant {name}: '{value}' is not an integer literal") from None
        if consts.setdefault(name, value) != value:
            raise HeaderError(f"constant {name} is defined as {consts[name]} and as {value}")

    def directive(m):
        words = m.group(1).split()
        if words[0] == "define" and len(words) != 2:                            # two words: the include guard
            if len(words) != 3:
                raise HeaderError(f"#{m.group(1)}: not an integer constant")
            constant(words[1], words[2])
        return ""

    def enum(m):
        for item in filter(str.strip, m.group(1).split(",")):
            name, eq, value = (s.strip() for s in item.partition("="))
            if not eq:
                raise HeaderError(f"enumerator {name} has no explicit value")
            constant(name, value)
        return ""

    def struct(m):
        fields = [_ctype(f, m.group(2)) for f in filter(str.strip, m.group(1).split(";"))]
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        return ""

    def callback(m):
        ret, args = _signature(m.group(1), m.group(2), m.group(3))
        callbacks[m.group(2)] = C.CFUNCTYPE(ret, *args)
        return ""

    text = re.sub(r"^[ \t]*#[ \t]*(.*)$", directive, text, flags=re.M)
    text = re.sub(r"\benum\s+\w+\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"\btypedef\s+([^;(){}]+)\(\s*\*\s*(\w+)\s*\)\s*\(([^(){}]*)\)\s*;", callback, text)
    for stmt in filter(str.strip, text.split(";")):
        fn = re.fullmatch(r"\s*([^(){}]+?)\b(\w+)\s*\(([^(){}]*)\)\s*", stmt)
        alias = re.fullmatch(r"\s*typedef\s[\w\s*]*?\b(\w+)\s*", stmt)         # e.g. mp_stream_t: the type map says what it is
        if fn and fn.group(2) not in protos:
            protos[fn.group(2)] = _signature(*fn.groups())
        elif not (alias and alias.group(1) in TYPES):
            raise HeaderError(f"'{' '.join(stmt.split())}' is not a declaration this reader knows")
    return Header(protos, consts, structs, callbacks)


@functools.lru_cache(maxsize=None)
def header(name):
    path = os.path.join(INCLUDE, name)
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: the ctypes binding is derived from it (there is no copy in the package)")
    with open(path) as f:
        return parse(f.read())
