"""ctypes binding of libboofhip.so, derived from include/boofhip.h (_header.py): constants, config structs and one signature per function.
Nothing of the C ABI is restated here; declare a new export in the header and it is bound.

The library is the product; there is no Python or CPU fallback.  Loading fails loudly when the shared object is missing
(run `python -m boofcv_amd.build` or `__graft_entry__.build()`), and creating a context fails loudly without a GPU.
"""
import ctypes as C
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# BHIP_LIB selects another build of the same ABI (scripts/ use libboofhip_exp.so, the -DBHIP_EXPERIMENTS build, for ablation runs)
LIB_PATH = os.environ.get("BHIP_LIB") or os.path.join(_HERE, "libboofhip.so")

_H = _header.load()   # parsed once per process (a few milliseconds)

# every typedef enum enumerator and every integer #define BHIP_* of the header: BHIP_OK, BHIP_ERR_*, BHIP_KLT_*, BHIP_BG_*, ...
globals().update(_H.constants)

P = C.POINTER
_vp, _i, _f, _d, _ll = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong
_fp, _dp, _ip, _u8p, _i16p, _i32p, _llp = P(C.c_float), P(C.c_double), P(C.c_int), P(C.c_uint8), P(C.c_int16), P(C.c_int32), P(C.c_longlong)

_CTYPES = {"int": _i, "float": _f, "double": _d, "long long": _ll, "uint8_t": C.c_uint8, "int16_t": C.c_int16, "int32_t": C.c_int32}

# the header's config structs (c = bhip_<key>_cfg) under the names the package uses: FhCfg(detectThreshold, extractRadius, ...), fields in header order
_STRUCT_NAMES = {"fh": "FhCfg", "surf": "SurfCfg", "ori": "OriCfg", "klt": "KltCfg", "disparity_bm": "DisparityBmCfg", "bg_basic": "BgBasicCfg",
                 "bg_gaussian": "BgGaussianCfg", "bg_gmm": "BgGmmCfg", "threshold": "ThresholdCfg", "sift": "SiftCfg", "csift": "CompleteSiftCfg"}
STRUCTS = {c: type(_STRUCT_NAMES[c[5:-4]], (C.Structure,), {"_fields_": [(name, _CTYPES[t]) for t, name in fields]})
           for c, fields in list(_H.structs.items()) + list(_H.tagged.items()) + list(_H.declared.items()) + list(_H.forward.items())}
globals().update((cls.__name__, cls) for cls in STRUCTS.values())


def _argtype(ctype, pname):
    kind, elem, _ = _header.classify(ctype, pname)
    if kind == "scalar":
        return _CTYPES[elem]
    if kind in ("handle", "address"):            # handles, void*, device addresses (dev_*)
        return _vp
    if kind in ("handle_out", "address_out"):    # bhip_x** and the T** of the device views
        return P(_vp)
    if kind == "struct":
        return P(STRUCTS[elem])
    if kind == "array2d":                        # T* const*
        return P(P(_CTYPES[elem]))
    return C.c_char_p if elem == "char" else P(_CTYPES[elem])   # host array


# name -> (restype, argtypes) for every function the header declares
SIGNATURES = {name: ({"int": _i, "void": None, "const char*": C.c_char_p}[ret], [_argtype(t, n) for t, n in params])
              for ret, name, params in _H.functions}

_lib = None


class BoofHipMissing(RuntimeError):
    pass


def _preload_process_hip_runtime():
    """One process must use ONE HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's);
    if libboofhip.so pulled in the system copy first and torch were imported later, the process would hold two runtimes and the
    second one finds no GPU.  So when a torch wheel with a bundled runtime is installed, load that copy first (without importing
    torch); libboofhip.so's NEEDED libamdhip64.so.7 then binds to it and device pointers / streams can be shared with torch."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """dlopen libboofhip.so (no GPU needed for this step) and attach the signatures."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BoofHipMissing("%s not found: build it with `python -m boofcv_amd.build` (hipcc, gfx950). "
                                 "There is no CPU fallback." % LIB_PATH)
        _preload_process_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here means the library and the header disagree
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib
