"""The ctypes binding (boofcv_amd/_lib.py) is derived from include/boofhip.h by boofcv_amd/_header.py.  These tests check the derivation
against witnesses that do not share its parser: the C compiler for struct layouts and constants, hand-written signatures for each
mapping rule.  No GPU and no built library needed."""
import ctypes as C
import os
import subprocess

import pytest

from boofcv_amd import _header, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_and_constants_match_the_c_compiler(tmp_path):
    """gcc's sizeof / offsetof of every config struct and its value of every constant, against the ctypes Structures and _lib.BHIP_*"""
    H = _header.load()
    assert len(H.structs) == 8 and len(H.constants) >= 38
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "boofhip.h"', "int main(void) {"]
    for cname, fields in H.structs.items():
        lines.append('\tprintf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for _, field in fields:
            lines.append('\tprintf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    for name in H.constants:
        lines.append('\tprintf("const %s %%lld\\n", (long long)%s);' % (name, name))
    lines += ["\treturn 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for line in out.splitlines():
        a, b, value = line.split()
        seen.add((a, b))
        if a == "const":
            assert getattr(_lib, b) == int(value), line
        elif b == "sizeof":
            assert C.sizeof(_lib.STRUCTS[a]) == int(value), line
        else:
            assert getattr(_lib.STRUCTS[a], b).offset == int(value), line
    assert len(seen) == len(H.constants) + sum(1 + len(f) for f in H.structs.values())
    # the public names, and a constant of each way the header spells them: multi-line enum with negative values, one-line enum, #define
    for name in ("FhCfg", "SurfCfg", "OriCfg", "KltCfg", "DisparityBmCfg", "BgBasicCfg", "BgGaussianCfg", "BgGmmCfg"):
        assert issubclass(getattr(_lib, name), C.Structure) and getattr(_lib, name) in _lib.STRUCTS.values()
    assert (_lib.BHIP_OK, _lib.BHIP_ERR_CAPACITY, _lib.BHIP_DISTORT_HOMOGRAPHY, _lib.BHIP_KLT_REFERENCE_THROWS, _lib.BHIP_TEMPLATE_MAX_CANDIDATES) == (0, -5, 2, 5, 65536)
    assert "BOOFHIP_H" not in H.constants


def test_one_export_per_mapping_rule():
    P, vp, i, f, d, ll = C.POINTER, C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong
    fp, u8p, ip, llp = P(C.c_float), P(C.c_uint8), P(C.c_int), P(C.c_longlong)
    expected = {
        "bhip_version": (C.c_char_p, []),                                                             # const char* result, (void)
        "bhip_fh_cfg_default": (None, [P(_lib.FhCfg)]),                                               # void result, struct pointer
        "bhip_ctx_create": (i, [i, P(vp)]),                                                           # handle out
        "bhip_surf_detect_f32": (i, [vp, P(fp), ip, ip, i, i, i]),                                    # T* const*
        "bhip_surf_detect_dev_f32": (i, [vp, vp, ll, i, i, i, i]),                                    # dev_ pointer, long long
        "bhip_surf_dev_view": (i, [vp, i, P(vp), P(vp), P(vp), ip]),                                  # const T** outputs
        "bhip_profile_report": (i, [vp, C.c_char_p, i]),                                              # char*
        "bhip_pyramid_layout": (i, [i, i, ip, i, ip, llp, llp]),                                      # long long*, no context
        "bhip_klt_create": (i, [vp, P(_lib.KltCfg), i, ip, i, i, f, i, i, i, i, P(vp)]),              # float scalar, struct, int array, handle out
        "bhip_bg_update_u8": (i, [vp, u8p, ll, ll, ll, ll, i, i, u8p, ll, ll, ll, i]),                # long long scalars beyond the sixth argument
        "bhip_template_intensity_dev_f32": (i, [vp, i, vp, ll, i, i, i, i, vp, ll, i, i, i, vp, ll, i, i, i, vp, ll, i]),   # the longest list
    }
    for name, sig in expected.items():
        assert _lib.SIGNATURES[name] == sig, name
    assert d in _lib.SIGNATURES["bhip_assoc_l2_f64"][1] and P(d) in _lib.SIGNATURES["bhip_assoc_l2_f64"][1]
    assert len(_lib.SIGNATURES) == len(_header.load().functions)


def test_unmapped_parameter_type_is_an_error():
    with pytest.raises(ValueError, match=r"struct foo\*.* p\b"):
        _header.parse("int bhip_x(struct foo* p);")
    with pytest.raises(ValueError, match="unsigned"):
        _header.classify("unsigned", "n")
    assert _header.parse("int bhip_x(const float* dev_p, long long n);").functions == [("int", "bhip_x", [("const float*", "dev_p"), ("long long", "n")])]
