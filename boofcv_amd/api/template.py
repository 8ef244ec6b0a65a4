"""Template matching (F:alg/feature/detect/template, F:factory/feature/detect/template, F:struct/feature/Match.java)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .core import Float_MAX_VALUE, IllegalArgumentException, _check, _ctx
from .image import GrayF32, GrayU8
from .detect import ConfigExtract, FactoryFeatureExtractor

__all__ = ["FactoryTemplateMatching", "Match", "TemplateMatching", "TemplateMatchingIntensity", "TemplateScoreType"]


class TemplateScoreType:
    """F:factory/feature/detect/template/TemplateScoreType.java:28-64"""
    SUM_ABSOLUTE_DIFFERENCE, SUM_SQUARE_ERROR, NCC, CORRELATION = "SUM_ABSOLUTE_DIFFERENCE", "SUM_SQUARE_ERROR", "NCC", "CORRELATION"
    _ORDINAL = {SUM_ABSOLUTE_DIFFERENCE: _lib.BHIP_TEMPLATE_SAD, SUM_SQUARE_ERROR: _lib.BHIP_TEMPLATE_SSE, NCC: _lib.BHIP_TEMPLATE_NCC,
                CORRELATION: _lib.BHIP_TEMPLATE_CORRELATION}


class TemplateMatchingIntensity:
    """TemplateIntensityImage<GrayU8 | GrayF32> over TemplateSumAbsoluteDifference / TemplateSumSquaredError / TemplateNCC
    (F:alg/feature/detect/template/TemplateIntensityImage.java:56-125).  Rules, limits and deviations: bhip_template_intensity_u8 in
    include/boofhip.h.  The intensity image is written as a whole by every process(), 0 in the border, also with a mask."""

    def __init__(self, type, imageType, ctx=None):
        self.type, self.imageType = type, imageType
        self.ctx = _ctx(ctx)
        self.image = None
        self.intensity = GrayF32(0, 0)
        self.borderX0 = self.borderY0 = self.borderX1 = self.borderY1 = 0

    def setInputImage(self, image):
        self.image = image

    def process(self, template, mask=None):
        image = self.image
        for what, im in (("image", image), ("template", template), ("mask", mask)):
            if im is not None and not isinstance(im, self.imageType):
                raise IllegalArgumentException("the %s must be a %s" % (what, self.imageType.__name__))
        if image is None:
            raise IllegalArgumentException("setInputImage() has not been called")
        self.intensity.reshape(image.width, image.height)
        self.borderX0, self.borderY0 = template.width // 2, template.height // 2
        self.borderX1, self.borderY1 = template.width - self.borderX0, template.height - self.borderY0
        out = self.intensity
        fn = _lib.load().bhip_template_intensity_u8 if self.imageType is GrayU8 else _lib.load().bhip_template_intensity_f32
        m = mask._in() if mask is not None else (None, 0, 0, 0, 0)
        _check(self.ctx, fn(self.ctx._h, TemplateScoreType._ORDINAL[self.type], *image._in(), *template._in(), *m, *out._out()))

    def getIntensity(self): return self.intensity
    def isBorderProcessed(self): return False
    def isMaximize(self): return self.type == TemplateScoreType.NCC
    def getBorderX0(self): return self.borderX0
    def getBorderX1(self): return self.borderX1
    def getBorderY0(self): return self.borderY0
    def getBorderY1(self): return self.borderY1


@dataclass
class Match:
    """F:struct/feature/Match.java:28-52: the template's top-left corner and the fit score, higher is better"""
    x: int = 0
    y: int = 0
    score: float = 0.0


class TemplateMatching:
    """F:alg/feature/detect/template/TemplateMatching.java:69-176: the intensity, the strict block non-maximum suppression on its sub-image
    and the N best by QuickSelect (bhip_template_select_f32 in include/boofhip.h: which matches are kept is pinned, their order is that of
    the restated routine; a match shows its own candidate's score)."""

    def __init__(self, match, ctx=None):
        self.match = match
        self.ctx = _ctx(ctx if ctx is not None else getattr(match, "ctx", None))
        if match.isMaximize():
            config = ConfigExtract(2, -Float_MAX_VALUE, 0, True)
        else:
            config = ConfigExtract(2, -Float_MAX_VALUE, 0, True, True, False)
        self.extractor = FactoryFeatureExtractor.nonmax(config, self.ctx)
        self.template = self.mask = None
        self.maxMatches = 0
        self.imageWidth = self.imageHeight = 0
        self.results = []

    def setMinimumSeparation(self, radius):
        self.extractor.setSearchRadius(radius)

    def setTemplate(self, template, mask, maxMatches):
        self.template, self.mask, self.maxMatches = template, mask, maxMatches

    def setImage(self, image):
        self.match.setInputImage(image)
        self.imageWidth, self.imageHeight = image.width, image.height

    def process(self):
        match = self.match
        if self.mask is None:
            match.process(self.template)
        else:
            match.process(self.template, self.mask)
        intensity = match.getIntensity()
        offsetX = offsetY = 0
        if not match.isBorderProcessed():
            x0, x1 = match.getBorderX0(), self.imageWidth - match.getBorderX1()
            y0, y1 = match.getBorderY0(), self.imageHeight - match.getBorderY1()
            intensity = intensity.subimage(x0, y0, x1 + 1, y1 + 1)
        else:
            offsetX, offsetY = match.getBorderX0(), match.getBorderY0()
        self.extractor.process(intensity)
        cand = np.ascontiguousarray(self.extractor.foundMaxXY if match.isMaximize() else self.extractor.foundMinXY, dtype=np.int16)
        n = len(cand)
        N = max(min(int(self.maxMatches), n), 0)
        xy, score, got = np.zeros((max(N, 1), 2), np.int16), np.zeros(max(N, 1), np.float32), C.c_int(0)
        _check(self.ctx, _lib.load().bhip_template_select_f32(self.ctx._h, *intensity._in(), cand.ctypes.data_as(_lib._i16p), n, int(self.maxMatches),
                                                             1 if match.isMaximize() else 0, xy.ctypes.data_as(_lib._i16p),
                                                             score.ctypes.data_as(_lib._fp), C.byref(got)))
        self.results = [Match(int(xy[i, 0]) - offsetX, int(xy[i, 1]) - offsetY, float(score[i])) for i in range(got.value)]

    def getResults(self):
        return self.results


class FactoryTemplateMatching:
    """F:factory/feature/detect/template/FactoryTemplateMatching.java:47-113"""

    @staticmethod
    def createIntensity(type, imageType, ctx=None):
        """IllegalArgumentException where the factory throws it (an image class it has no evaluator for, an unknown type); CORRELATION on
        GrayF32, which the factory answers with TemplateCorrelationFFT, raises RuntimeError: use the Java path."""
        name = getattr(imageType, "__name__", str(imageType))
        if type == TemplateScoreType.CORRELATION:
            if imageType is GrayF32:
                raise RuntimeError("TemplateCorrelationFFT is not implemented on the GPU (use the Java path)")
            raise IllegalArgumentException("Image type not supported. " + name)
        if type not in (TemplateScoreType.SUM_ABSOLUTE_DIFFERENCE, TemplateScoreType.SUM_SQUARE_ERROR, TemplateScoreType.NCC):
            raise IllegalArgumentException("Unknown")
        if imageType is not GrayU8 and imageType is not GrayF32:
            raise IllegalArgumentException("Image type not supported. " + name)
        return TemplateMatchingIntensity(type, imageType, ctx)

    @staticmethod
    def createMatcher(type, imageType, ctx=None):
        return TemplateMatching(FactoryTemplateMatching.createIntensity(type, imageType, ctx))
