"""boofcv_amd.api as a package of family modules, without a GPU: the public surface is the one the single module had, every name has one
home and imports run one way, and every family hands its host image views to C through the one validating marshaller of api/image.py."""
import ast
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import boofcv_amd
from boofcv_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ("core", "image", "associate", "detect", "filter", "surf", "klt", "disparity", "template", "distort", "background", "flow")   # import order
PRIVATE = {"_PinnedPool", "_host_map", "_kernel_model", "_check", "_NativeObject", "_klt_fetch"}


def _golden_names():
    lines = open(os.path.join(ROOT, "tests", "golden", "api_names.txt")).read().split("\n")
    return [n for n in lines if n and not n.startswith("#")]


def _tree(module):
    return ast.parse(open(os.path.join(ROOT, "boofcv_amd", "api", module + ".py")).read())


def _child(code):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)


def test_surface_is_the_single_modules():
    names = _golden_names()
    assert len(names) > 100 and PRIVATE <= set(names)
    for n in names:
        assert hasattr(api, n), "boofcv_amd.api lost " + n
        if not n.startswith("_"):
            assert getattr(boofcv_amd, n) is getattr(api, n), n
    extra = [k for k, v in vars(api).items() if not k.startswith("_") and (inspect.isclass(v) or inspect.isfunction(v)) and k not in names]
    assert not extra, "public names the single module did not have: %s" % extra
    assert {f[:-3] for f in os.listdir(os.path.join(ROOT, "boofcv_amd", "api")) if f.endswith(".py")} == set(MODULES) | {"__init__"}
    assert not os.path.exists(os.path.join(ROOT, "boofcv_amd", "api.py"))


def test_every_name_has_one_home_and_imports_run_one_way():
    homes = {"boofcv_amd.api." + m for m in MODULES}
    for k, v in vars(api).items():
        if inspect.isclass(v) or inspect.isfunction(v):
            assert v.__module__ in homes, (k, v.__module__)
    defined = {}
    for i, m in enumerate(MODULES):
        tree = _tree(m)
        assert ast.get_docstring(tree), m + " has no docstring"
        for node in tree.body:
            for name in ([node.name] if isinstance(node, (ast.ClassDef, ast.FunctionDef)) else
                         [t.id for t in node.targets if isinstance(t, ast.Name)] if isinstance(node, ast.Assign) else []):
                if name != "__all__":
                    assert name not in defined, "%s is defined in %s and in %s" % (name, defined.get(name), m)
                    defined[name] = m
        # relative imports: at module top only, and only of _lib and of modules earlier in the order
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level:
                assert node in tree.body, "%s imports %s inside a function" % (m, node.module)
                assert (node.level, node.module) == (2, None) or (node.level == 1 and node.module in MODULES[:i]), (m, node.module)
                assert not (node.level == 2 and [a.name for a in node.names] != ["_lib"]), m   # _lib.load() is looked up at every call
    assert set(_golden_names()) <= set(defined)


@pytest.mark.parametrize("module", MODULES)
def test_family_module_imports_on_its_own(module):
    r = _child("import boofcv_amd.api.%s as m; assert m.__doc__" % module)
    assert r.returncode == 0, r.stdout + r.stderr


# One host-view entry point per family module that has one, run in a child process against a library whose every function records its name
# and returns BHIP_OK.  (what it is, the call on fresh 16 x 12 inputs, the inputs' types, the calls the intact inputs make)
VIEWS_CHILD = """
import types
import numpy as np
from boofcv_amd import _lib, api

calls = []

class Fake:
    def __getattr__(self, name):
        def fn(*args):
            calls.append(name)
            return _lib.BHIP_OK
        return fn

fake = Fake()
_lib.load = lambda: fake
ctx = types.SimpleNamespace(_h=1, _children=set())
W, H = 16, 12
F32, U8 = api.GrayF32, api.GrayU8
f32, u8 = (lambda: F32(W, H)), (lambda: U8(W, H))

def template(image, templ):
    m = api.FactoryTemplateMatching.createIntensity(api.TemplateScoreType.SUM_ABSOLUTE_DIFFERENCE, U8, ctx)
    m.setInputImage(image)
    m.process(templ)

def klt(image, dx, dy):
    t = api.KltTracker(None, ctx)
    t.setImage(image, dx, dy)
    t.setDescriptionAll([[5, 5]], 2)

background = api.BackgroundStationaryBasic(0.05, 10.0, U8, ctx)
background.updateBackground(u8())      # the model now has its size: the next update is one call
surf = api.FactoryDetectDescribe.surfStable(None, None, None, F32, ctx)

ENTRIES = [
    ("detect: IntegralImageOps.transform", lambda a: api.IntegralImageOps.transform(a, ctx=ctx), (F32,), ["bhip_integral_f32"]),
    ("detect: IntegralImageFeatureIntensity.hessian", lambda a: api.IntegralImageFeatureIntensity.hessian(a, 1, 9, f32(), ctx), (F32,), ["bhip_hessian_f32"]),
    ("detect: NonMaxSuppression.process", lambda a: api.NonMaxSuppression(None, ctx).process(a), (F32,), ["bhip_nonmax_block_f32"]),
    ("detect: GradientCornerIntensity.process", lambda dx, dy: api.FactoryIntensityPointAlg.shiTomasi(2, ctx=ctx).process(dx, dy, F32(1, 1)), (F32, F32),
     ["bhip_corner_intensity_f32"]),
    ("filter: ConvolveImageNoBorder.horizontal", lambda a: api.ConvolveImageNoBorder.horizontal(api.Kernel1D_F32([1, 2, 1]), a, f32(), ctx), (F32,),
     ["bhip_conv_h_f32"]),
    ("filter: GradientSobel.process", lambda a: api.GradientSobel.process(a, f32(), f32(), ctx=ctx), (F32,), ["bhip_sobel_f32"]),
    ("filter: BlurImageOps.mean", lambda a: api.BlurImageOps.mean(a, None, 2, ctx=ctx), (F32,), ["bhip_mean_f32"]),
    ("surf: DetectDescribePoint.detectBatch", lambda a, b: surf.detectBatch([a, b]), (F32, F32), ["bhip_surf_detect_f32"]),
    ("klt: KltTracker.setImage + setDescriptionAll", klt, (F32, F32, F32), ["bhip_klt_set_description_f32"]),
    ("disparity: StereoDisparity.process", lambda l, r: api.FactoryStereoDisparity.blockMatch(api.ConfigDisparityBM(0, 4, 1, 1), ctx=ctx).process(l, r),
     (U8, U8), ["bhip_disparity_bm_u8_f32"]),
    ("template: TemplateMatchingIntensity.process", template, (U8, U8), ["bhip_template_intensity_u8"]),
    ("distort: DistortImageOps.distortSingle", lambda a: api.DistortImageOps.distortSingle(a, f32(), api.PixelTransformAffine_F32(),
                                                                                        api.InterpolationType.BILINEAR, api.BorderType.ZERO, ctx=ctx),
     (F32,), ["bhip_distort_model_f32"]),
    ("background: BackgroundStationaryBasic.updateBackground", background.updateBackground, (U8,), ["bhip_bg_update_u8"]),
    ("flow: DenseOpticalFlow.process", lambda a, b: api.FactoryDenseOpticalFlow.flowKlt(None, 2, F32, None, ctx).process(a, b, api.ImageFlow(W, H)),
     (F32, F32), ["bhip_flow_klt_f32"]),
]

def grow(im): im.height += 1
def narrow(im): im.stride = im.width - 1
def past(im): im.startIndex = im.data.size

for what, call, types_, expected in ENTRIES:
    for i in range(len(types_)):
        for damage in (grow, narrow, past):
            images = [T(W, H) for T in types_]
            damage(images[i])   # the fields are public and mutable, as in the reference
            del calls[:]
            try:
                call(*images)
            except api.IllegalArgumentException:
                pass
            else:
                raise AssertionError("%s: input %d after %s reached C: %s" % (what, i, damage.__name__, calls))
            assert not calls, "%s: input %d after %s: %s was called before the view was refused" % (what, i, damage.__name__, calls)
    del calls[:]
    call(*[T(W, H) for T in types_])
    assert calls == expected, (what, calls)
print("ok", len(ENTRIES), sorted({what.split(":")[0] for what, _, _, _ in ENTRIES}))
"""


def test_views_are_checked_at_every_familys_door():
    r = _child(VIEWS_CHILD)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok 14 ['background', 'detect', 'disparity', 'distort', 'filter', 'flow', 'klt', 'surf', 'template']" in r.stdout, r.stdout


@pytest.mark.parametrize("imageType, pointer", [(api.GrayF32, C.c_float), (api.GrayU8, C.c_uint8), (api.GrayS16, C.c_int16), (api.GrayS32, C.c_int32)])
def test_the_marshallers_tuples(imageType, pointer):
    whole = imageType(16, 12)
    whole.data[:] = np.arange(whole.data.size) % 100
    sub = whole.subimage(2, 3, 10, 9)
    ptr, startIndex, stride, width, height = view = sub._in()
    assert view[1:] == (3 * 16 + 2, 16, 8, 6)
    assert isinstance(ptr, C.POINTER(pointer)) and C.cast(ptr, C.c_void_p).value == sub.data.ctypes.data == whole.data.ctypes.data
    assert ptr[startIndex] == whole.array()[3, 2] == sub.array()[0, 0]
    out = sub._out()
    assert len(out) == 3 and out[1:] == (startIndex, stride) and C.cast(out[0], C.c_void_p).value == sub.data.ctypes.data
    sub.height += 7   # past the end of the array
    for form in (sub._in, sub._out):
        with pytest.raises(api.IllegalArgumentException):
            form()
