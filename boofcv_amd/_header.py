"""include/boofhip.h read as data: the one description of the C ABI that the ctypes binding (_lib.py) and the JNI generator
(scripts/gen_jni.py) are both derived from.  Pure text processing: no ctypes, no JNI names.

    parse(text) -> Header(functions, structs, constants, tagged, declared, forward)
    classify(ctype, pname) -> (kind, element type, is_const)
    load() -> parse() of HEADER, cached
"""
import collections
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "boofhip.h")

HANDLES = ("bhip_ctx", "bhip_surf", "bhip_klt", "bhip_bg")
ELEMENTS = ("float", "double", "uint8_t", "int", "int32_t", "int16_t", "long long", "char")   # what a pointer parameter may point at
_COMMENT = re.compile(r"/\*.*?\*/", re.S)
_FUNCTION = re.compile(r"^[ \t]*(int|void|const char\*)\s+(bhip_\w+)\s*\(([^;{}()]*)\)\s*;", re.M)

# functions: [(ret, name, [(ctype, pname)])] in header order; structs: {bhip_*_cfg: [(ctype, field)]}, the anonymous `typedef struct { } name;`
# ones; tagged: the same for `typedef struct name { } name;`; declared: the same for `struct name { }; typedef struct name name;` (the sets of
# the first two spellings are pinned by tests/test_header_binding.py and tests/test_threshold_reference.py; a new config struct is declared
# the third way -- or, now that tests/test_sift_reference.py pins that set too, the fourth: forward, `typedef struct name name; struct name { };`);
# constants: {BHIP_*: int}
Header = collections.namedtuple("Header", "functions structs constants tagged declared forward")


def _declarator(text):
    """'const float *dev_x' -> ('const float*', 'dev_x')"""
    text = " ".join(text.split())
    cut = max(text.rfind(" "), text.rfind("*")) + 1   # the name is what follows the last space or star
    return text[:cut].rstrip().replace(" *", "*"), text[cut:]


def parse_header(text):
    """every `int|void|const char* bhip_*(...);` declaration -> [(ret, name, [(ctype, pname)])]"""
    fns = []
    for m in _FUNCTION.finditer(_COMMENT.sub(" ", text)):
        ret, name, params = m.group(1), m.group(2), " ".join(m.group(3).split())
        fns.append((ret, name, [_declarator(p) for p in params.split(",")] if params and params != "void" else []))
    return fns


@functools.lru_cache(maxsize=None)   # a few hundred distinct (type, name) pairs for some two thousand parameters
def classify(ctype, pname):
    """-> (kind, C element type, is_const); kind is one of
    scalar       int / float / double / long long by value
    handle       bhip_ctx* / bhip_surf* / bhip_klt* / bhip_bg*          handle_out   a pointer to one of them, written by the call
    struct       bhip_*_cfg*
    address      void*, or a T* named dev_*: an opaque / device address  address_out  T**: one such address, written by the call
    array        T* in host memory                                       array2d      T* const*: a batch of host arrays
    A parameter type outside this list is an error: it has no binding until this function names one."""
    const = ctype.startswith("const ")
    base = ctype[6:] if const else ctype
    if base in ("int", "float", "double", "long long"):
        return ("scalar", base, const)
    if base.endswith("**") and base[:-2] in HANDLES:
        return ("handle_out", base[:-1], const)
    if base.endswith("*") and base[:-1] in HANDLES:
        return ("handle", base, const)
    if base.startswith("bhip_") and base.endswith("_cfg*"):
        return ("struct", base[:-1], const)
    if base == "void*":
        return ("address", "void", const)
    if base.endswith("* const*") and base[:-8] in ("float", "double", "uint8_t"):
        return ("array2d", base[:-8], True)
    if base.endswith("**") and base[:-2] in ELEMENTS:
        return ("address_out", base[:-2], const)
    if base.endswith("*") and base[:-1] in ELEMENTS:
        return ("address" if pname.startswith("dev_") else "array", base[:-1], const)
    raise ValueError("unmapped parameter type %r %s" % (ctype, pname))


def parse(text):
    """The whole header.  Every parameter is classified here, so an unmapped type fails the parse, not a later call."""
    functions = parse_header(text)
    for _, _, params in functions:
        for ctype, pname in params:
            classify(ctype, pname)
    text = _COMMENT.sub(" ", text)
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s*\{([^{}]*)\}\s*(bhip_\w+_cfg)\s*;", text):
        structs[m.group(2)] = [_declarator(f) for f in m.group(1).split(";") if f.strip()]
    tagged = {}
    for m in re.finditer(r"typedef\s+struct\s+(bhip_\w+_cfg)\s*\{([^{}]*)\}\s*\1\s*;", text):
        tagged[m.group(1)] = [_declarator(f) for f in m.group(2).split(";") if f.strip()]
    declared = {}
    for m in re.finditer(r"(?<!typedef)\s+struct\s+(bhip_\w+_cfg)\s*\{([^{}]*)\}\s*;\s*typedef\s+struct\s+\1\s+\1\s*;", text):
        declared[m.group(1)] = [_declarator(f) for f in m.group(2).split(";") if f.strip()]
    forward = {}
    for m in re.finditer(r"typedef\s+struct\s+(bhip_\w+_cfg)\s+\1\s*;\s*struct\s+\1\s*\{([^{}]*)\}\s*;", text):
        forward[m.group(1)] = [_declarator(f) for f in m.group(2).split(";") if f.strip()]
    constants = {}
    for m in re.finditer(r"typedef\s+enum\s*\{([^{}]*)\}\s*\w+\s*;", text):
        value = -1
        for item in m.group(1).split(","):
            name, _, explicit = (s.strip() for s in item.partition("="))
            if name:
                value = int(explicit, 0) if explicit else value + 1   # C: an enumerator without a value is the previous one plus 1
                constants[name] = value
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(BHIP_\w+)[ \t]+(\S+)[ \t]*$", text, flags=re.M):
        try:
            constants[m.group(1)] = int(m.group(2), 0)
        except ValueError:
            pass   # not an integer constant
    return Header(functions, structs, constants, tagged, declared, forward)


_cached = None


def load():
    global _cached
    if _cached is None:
        try:
            with open(HEADER) as f:
                text = f.read()
        except OSError as e:
            raise RuntimeError("the C ABI header %s cannot be read (%s): the binding is derived from it" % (os.path.abspath(HEADER), e))
        _cached = parse(text)
    return _cached
