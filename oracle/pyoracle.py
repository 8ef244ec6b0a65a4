"""TEST INFRASTRUCTURE ONLY -- ctypes binding of oracle/liboracle.so (the CPU restatement of the Java reference).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this module.  The product package
(boofcv_amd) never does.
"""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "liboracle.so")


def build(force=False):
    """Compile liboracle.so with g++ (seconds)."""
    srcs = [os.path.join(_HERE, f) for f in ("oracle_capi.cpp", "boof_oracle.hpp", "boof_oracle_ip.hpp", "boof_oracle_int.hpp")]
    if not force and os.path.exists(_LIB_PATH) and all(os.path.getmtime(_LIB_PATH) >= os.path.getmtime(s) for s in srcs):
        return _LIB_PATH
    subprocess.check_call(["make", "-C", _HERE, "-B", "liboracle.so"], stdout=subprocess.DEVNULL)
    return _LIB_PATH


class _Image(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_float)), ("startIndex", C.c_int), ("stride", C.c_int), ("width", C.c_int), ("height", C.c_int)]


class FhCfg(C.Structure):
    """F:abst/feature/detect/interest/ConfigFastHessian.java:33-70"""
    _fields_ = [("detectThreshold", C.c_float), ("extractRadius", C.c_int), ("maxFeaturesPerScale", C.c_int), ("initialSampleSize", C.c_int),
                ("initialSize", C.c_int), ("numberScalesPerOctave", C.c_int), ("numberOfOctaves", C.c_int), ("scaleStepSize", C.c_int)]

    def __init__(self, detectThreshold=1.0, extractRadius=2, maxFeaturesPerScale=-1, initialSampleSize=1, initialSize=9,
                 numberScalesPerOctave=4, numberOfOctaves=4, scaleStepSize=6):
        super().__init__(detectThreshold, extractRadius, maxFeaturesPerScale, initialSampleSize, initialSize, numberScalesPerOctave,
                         numberOfOctaves, scaleStepSize)


class SurfCfg(C.Structure):
    """F:abst/feature/describe/ConfigSurfDescribe.java:34-78"""
    _fields_ = [("widthLargeGrid", C.c_int), ("widthSubRegion", C.c_int), ("widthSample", C.c_int), ("weightSigma", C.c_double),
                ("overLap", C.c_int), ("sigmaLargeGrid", C.c_double), ("sigmaSubRegion", C.c_double)]

    def __init__(self, widthLargeGrid=4, widthSubRegion=5, widthSample=3, weightSigma=4.5, overLap=2, sigmaLargeGrid=2.5, sigmaSubRegion=2.5):
        super().__init__(widthLargeGrid, widthSubRegion, widthSample, weightSigma, overLap, sigmaLargeGrid, sigmaSubRegion)


class OriCfg(C.Structure):
    """ConfigSlidingIntegral.java:34-54 / ConfigAverageIntegral.java:34-51 (windowSize unused by the average variant)"""
    _fields_ = [("objectRadiusToScale", C.c_double), ("samplePeriod", C.c_double), ("windowSize", C.c_double), ("radius", C.c_int),
                ("weightSigma", C.c_double), ("sampleWidth", C.c_int)]

    @staticmethod
    def sliding(samplePeriod=0.65, windowSize=np.pi / 3.0, radius=8, weightSigma=-1.0, sampleWidth=6):
        return OriCfg(0.5, samplePeriod, windowSize, radius, weightSigma, sampleWidth)

    @staticmethod
    def average(radius=6, samplePeriod=1.0, sampleWidth=6, weightSigma=-1.0):
        return OriCfg(0.5, samplePeriod, 0.0, radius, weightSigma, sampleWidth)


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB_PATH)
        P = C.POINTER
        IM = P(_Image)
        sig = {
            "orc_max_threads": (C.c_int, []),
            "orc_rand_new": (C.c_void_p, [C.c_int64]),
            "orc_rand_free": (None, [C.c_void_p]),
            "orc_rand_next_int": (C.c_int32, [C.c_void_p]),
            "orc_rand_next_int_bound": (C.c_int32, [C.c_void_p, C.c_int32]),
            "orc_rand_next_float": (C.c_float, [C.c_void_p]),
            "orc_rand_next_double": (C.c_double, [C.c_void_p]),
            "orc_rand_next_gaussian": (C.c_double, [C.c_void_p]),
            "orc_rand_next_boolean": (C.c_int, [C.c_void_p]),
            "orc_fill_uniform": (None, [C.c_void_p, IM, C.c_float, C.c_float]),
            "orc_fill_gaussian": (None, [C.c_void_p, IM, C.c_double, C.c_double, C.c_float, C.c_float]),
            "orc_integral": (None, [IM, IM]),
            "orc_block_unsafe": (C.c_float, [IM, C.c_int, C.c_int, C.c_int, C.c_int]),
            "orc_block_zero": (C.c_float, [IM, C.c_int, C.c_int, C.c_int, C.c_int]),
            "orc_convolve_sparse": (C.c_float, [IM, C.c_int, C.c_int, C.c_int, C.c_int]),
            "orc_convolve_sparse_blocks": (C.c_float, [IM, C.c_int, P(C.c_int), P(C.c_int), C.c_int, C.c_int]),
            "orc_hessian": (None, [IM, C.c_int, C.c_int, IM, C.c_int, C.c_int]),
            "orc_nonmax": (C.c_int, [IM, C.c_int, C.c_float, C.c_int, C.c_int, P(C.c_int16), C.c_int, C.c_int]),
            "orc_fh_detect": (C.c_int, [IM, P(FhCfg), P(C.c_double), C.c_int, C.c_int]),
            "orc_select_nbest": (C.c_int, [IM, P(C.c_int16), C.c_int, C.c_int, C.c_int, P(C.c_int16)]),
            "orc_orientation": (C.c_double, [IM, C.c_int, P(OriCfg), C.c_double, C.c_double, C.c_double]),
            "orc_sparse_gradient": (C.c_int, [IM, C.c_double, C.c_int, C.c_int, P(C.c_float), P(C.c_float)]),
            "orc_describe": (C.c_int, [IM, C.c_int, P(SurfCfg), C.c_double, C.c_double, C.c_double, C.c_double, P(C.c_double), P(C.c_uint8), C.c_int]),
            "orc_surf_is_inside": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]),
            "orc_surf_is_inside_region": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
            "orc_normalize_l2": (None, [P(C.c_double), C.c_int]),
            "orc_compute_pdf": (C.c_double, [C.c_double, C.c_double, C.c_double]),
            "orc_sparse_gradient_bounds": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, P(C.c_int)]),
            "orc_gaussian_width": (C.c_int, [C.c_double, C.c_int, P(C.c_double)]),
            "orc_gaussian2d_f64": (C.c_int, [C.c_double, C.c_int, P(C.c_double)]),
            "orc_gaussian1d_f32": (C.c_int, [C.c_double, C.c_int, P(C.c_float)]),
            "orc_surf_create": (C.c_void_p, [C.c_int, P(FhCfg), P(SurfCfg), P(OriCfg)]),
            "orc_surf_destroy": (None, [C.c_void_p]),
            "orc_surf_detect": (C.c_int, [C.c_void_p, IM, C.c_int]),
            "orc_surf_describe_points": (C.c_int, [C.c_void_p, IM, P(C.c_double), C.c_int, C.c_int]),
            "orc_surf_detect_u8": (C.c_int, [C.c_void_p, P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
            "orc_surf_detect_planar": (C.c_int, [C.c_void_p, P(_Image), C.c_int, C.c_int]),
            "orc_surf_describe_points_planar": (C.c_int, [C.c_void_p, P(C.c_double), C.c_int, C.c_int]),
            "orc_surf_fetch": (None, [C.c_void_p, P(C.c_double), P(C.c_double), P(C.c_uint8), P(C.c_double)]),
            "orc_surf_integral": (None, [C.c_void_p, P(C.c_float)]),
            "orc_associate_l2": (None, [P(C.c_double), C.c_int, P(C.c_double), C.c_int, C.c_int, C.c_double, C.c_int, P(C.c_int), P(C.c_double), C.c_int]),
            "orc_associate_euclidean": (None, [P(C.c_double), C.c_int, P(C.c_double), C.c_int, C.c_int, C.c_double, C.c_int, P(C.c_int), P(C.c_double), C.c_int]),
            "orc_associate_hamming": (None, [P(C.c_int32), C.c_int, P(C.c_int32), C.c_int, C.c_int, C.c_double, C.c_int, P(C.c_int), P(C.c_double), C.c_int]),
            "orc_euclidean_sq": (C.c_double, [P(C.c_double), P(C.c_double), C.c_int]),
            "orc_hamming_word": (C.c_int, [C.c_int32]),
            "orc_hamming": (C.c_int, [P(C.c_int32), P(C.c_int32), C.c_int]),
            "orc_brief_definition": (None, [C.c_int64, C.c_int, C.c_int, P(C.c_int), P(C.c_int)]),
            "orc_brief_describe": (None, [IM, C.c_int, C.c_int, P(C.c_int), P(C.c_int), P(C.c_double), C.c_int, P(C.c_int32)]),
            "orc_conv_h": (None, [P(C.c_float), C.c_int, C.c_int, IM, IM, C.c_int]),
            "orc_conv_v": (None, [P(C.c_float), C.c_int, C.c_int, IM, IM, C.c_int]),
            "orc_conv_norm_h": (None, [P(C.c_float), C.c_int, C.c_int, IM, IM, C.c_int]),
            "orc_conv_norm_v": (None, [P(C.c_float), C.c_int, C.c_int, IM, IM, C.c_int]),
            "orc_gaussian_blur": (None, [IM, IM, C.c_double, C.c_int, IM, C.c_int]),
            "orc_sobel": (None, [IM, IM, IM, C.c_int, C.c_int]),
            "orc_three": (None, [IM, IM, IM, C.c_int, C.c_int]),
            "orc_subsample": (None, [IM, IM, C.c_int]),
            "orc_conv2d": (None, [P(C.c_float), C.c_int, C.c_int, IM, IM]),
            "orc_blur_mean": (C.c_int, [IM, IM, C.c_int, C.c_int, IM]),
            "orc_blur_median": (C.c_int, [IM, IM, C.c_int]),
            "orc_integral_u8": (None, [P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_int32), C.c_int, C.c_int]),
            "orc_hessian_s32": (None, [P(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IM]),
            "orc_fh_detect_s32": (C.c_int, [P(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, P(FhCfg), P(C.c_double), C.c_int, C.c_int]),
            "orc_brief_u8": (None, [P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_int), P(C.c_int), P(C.c_double), C.c_int, P(C.c_int32)]),
            "orc_ssd_corner": (C.c_int, [IM, IM, C.c_int, C.c_int, C.c_float, P(C.c_float)]),
            "orc_conv_down_norm": (C.c_int, [C.c_int, P(C.c_float), C.c_int, IM, IM, C.c_int]),
            "orc_down_max_side": (C.c_int, [C.c_int, C.c_int, C.c_int]),
            "orc_down_offset": (C.c_int, [C.c_int, C.c_int]),
            "orc_pyramid": (C.c_long, [P(C.c_float), C.c_int, C.c_double, P(C.c_int), C.c_int, IM, P(C.c_float), C.c_long, P(C.c_int), P(C.c_double)]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


MAX_VALUE_F32 = np.float32(3.4028234663852886e38)  # Float.MAX_VALUE
MAX_VALUE_F64 = 1.7976931348623157e308  # Double.MAX_VALUE


def _fp(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


class Gray:
    """GrayF32 view over a float32 numpy buffer: pixel(x,y) = buf[startIndex + y*stride + x]  (T:struct/image/ImageBase.java:34-52)."""

    def __init__(self, width, height, buf=None, startIndex=0, stride=None):
        self.width, self.height = int(width), int(height)
        self.stride = int(stride if stride is not None else width)
        self.startIndex = int(startIndex)
        if buf is None:
            buf = np.zeros(self.startIndex + self.stride * self.height, dtype=np.float32)
        assert buf.dtype == np.float32 and buf.flags["C_CONTIGUOUS"]
        self.buf = buf

    @staticmethod
    def from_array(a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        return Gray(a.shape[1], a.shape[0], a.reshape(-1))

    def array(self):
        """(height,width) strided view of the pixels."""
        return np.lib.stride_tricks.as_strided(self.buf[self.startIndex:], shape=(self.height, self.width), strides=(4 * self.stride, 4))

    def c(self):
        return C.byref(_Image(_fp(self.buf), self.startIndex, self.stride, self.width, self.height))

    def sub_image_of(self, pad_x=5, pad_y=7, fill=0.0):
        """BoofTesting.createSubImageOf (I:testing/BoofTesting.java:71): same pixels inside a larger buffer."""
        W, H = self.width + 2 * pad_x, self.height + 2 * pad_y
        big = np.full(W * H, fill, dtype=np.float32)
        g = Gray(self.width, self.height, big, startIndex=pad_y * W + pad_x, stride=W)
        g.array()[:, :] = self.array()
        return g


class JavaRandom:
    """java.util.Random (48-bit LCG)."""

    def __init__(self, seed):
        self._h = lib().orc_rand_new(int(seed))

    def __del__(self):
        try:
            lib().orc_rand_free(self._h)
        except Exception:
            pass

    def nextInt(self, bound=None):
        return lib().orc_rand_next_int(self._h) if bound is None else lib().orc_rand_next_int_bound(self._h, bound)

    def nextFloat(self):
        return lib().orc_rand_next_float(self._h)

    def nextDouble(self):
        return lib().orc_rand_next_double(self._h)

    def nextGaussian(self):
        return lib().orc_rand_next_gaussian(self._h)

    def nextBoolean(self):
        return bool(lib().orc_rand_next_boolean(self._h))

    def fillUniform(self, img, lo, hi):
        lib().orc_fill_uniform(self._h, img.c(), lo, hi)
        return img

    def fillGaussian(self, img, mean, sigma, lo, hi):
        lib().orc_fill_gaussian(self._h, img.c(), mean, sigma, lo, hi)
        return img


def noise_image(width, height, seed, lo=0.0, hi=100.0):
    """S-noise(W,H,seed) of SURVEY 8d: ImageMiscOps.fillUniform with java.util.Random(seed)."""
    return JavaRandom(seed).fillUniform(Gray(width, height), lo, hi)


def integral(img):
    out = Gray(img.width, img.height)
    lib().orc_integral(img.c(), out.c())
    return out


def hessian(ii, skip, size, naive=False, threads=1):
    out = Gray(ii.width // skip, ii.height // skip)
    lib().orc_hessian(ii.c(), skip, size, out.c(), 1 if naive else 0, threads)
    return out


def nonmax(intensity, radius, threshold, border, naive=False, threads=1):
    cap = intensity.width * intensity.height
    out = np.zeros((cap, 2), dtype=np.int16)
    n = lib().orc_nonmax(intensity.c(), radius, threshold, border, 1 if naive else 0, _fp(out, C.c_int16), cap, threads)
    return out[:n].copy()


def select_nbest(intensity, corners, target, positive=True):
    """SelectNBestFeatures.process: corners = (n,2) int16 (x,y); returns the kept points in the reference's output order."""
    xy = np.ascontiguousarray(corners, dtype=np.int16).reshape(-1, 2)
    out = np.zeros((max(len(xy), 1), 2), dtype=np.int16)
    n = lib().orc_select_nbest(intensity.c(), _fp(xy, C.c_int16), len(xy), target, 1 if positive else 0, _fp(out, C.c_int16))
    return out[:n].copy()


def fh_detect(ii, cfg=None, threads=1):
    cfg = cfg or FhCfg()
    cap = 1 << 16
    while True:
        out = np.zeros((cap, 3), dtype=np.float64)
        n = lib().orc_fh_detect(ii.c(), C.byref(cfg), _fp(out, C.c_double), cap, threads)
        if n <= cap:
            return out[:n].copy()
        cap = n


def orientation(ii, x, y, objectRadius, kind="sliding", cfg=None):
    k = 0 if kind == "sliding" else 1
    cfg = cfg or (OriCfg.sliding() if k == 0 else OriCfg.average())
    return lib().orc_orientation(ii.c(), k, C.byref(cfg), x, y, objectRadius)


def describe(ii, x, y, angle, scale, stable=True, cfg=None, normalize=True):
    cfg = cfg or SurfCfg()
    desc = np.zeros(cfg.widthLargeGrid * cfg.widthLargeGrid * 4, dtype=np.float64)
    white = C.c_uint8(0)
    if lib().orc_describe(ii.c(), 1 if stable else 0, C.byref(cfg), x, y, angle, scale, _fp(desc, C.c_double), C.byref(white), 1 if normalize else 0) != 0:
        raise ValueError("Weighting kernel has an unexpected size")   # DescribePointSurf.java:241-243: widthLargeGrid * widthSubRegion is odd
    return desc, bool(white.value)


class Surf:
    """FactoryDetectDescribe.surfStable / surfFast (F:factory/feature/detdesc/FactoryDetectDescribe.java:118-135,209-226)."""

    def __init__(self, stable=True, fh=None, sd=None, ori=None):
        self.stable = stable
        self.fh = fh or FhCfg()
        self.sd = sd or SurfCfg()
        self.ori = ori or (OriCfg.sliding() if stable else OriCfg.average())
        self.dof = self.sd.widthLargeGrid * self.sd.widthLargeGrid * 4
        self._h = lib().orc_surf_create(1 if stable else 0, C.byref(self.fh), C.byref(self.sd), C.byref(self.ori))
        if not self._h:
            raise ValueError("Weighting kernel has an unexpected size")   # surfFast on an odd widthLargeGrid * widthSubRegion, see orc_surf_create
        self.n = 0

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().orc_surf_destroy(self._h)
        except Exception:
            pass

    def detect(self, img, threads=1):
        self.n = lib().orc_surf_detect(self._h, img.c(), threads)
        self._bands = 1
        self._shape = (img.width, img.height)
        return self.n

    def detect_u8(self, img_u8, threads=1):
        """FactoryDetectDescribe.surfStable / surfFast on a GrayU8 frame ((H, W) uint8 array)."""
        a = np.ascontiguousarray(img_u8, dtype=np.uint8)
        h, w = a.shape
        self.n = lib().orc_surf_detect_u8(self._h, _fp(a, C.c_uint8), 0, w, w, h, threads)
        self._bands = 1
        self._shape = (w, h)
        return self.n

    def detect_planar(self, bands, threads=1):
        """FactoryDetectDescribe.surfColorStable / surfColorFast on a Planar<GrayF32> given as a list of Gray bands."""
        arr = (_Image * len(bands))(*[_Image(_fp(b.buf), b.startIndex, b.stride, b.width, b.height) for b in bands])
        self.n = lib().orc_surf_detect_planar(self._h, arr, len(bands), threads)
        self._bands = len(bands)
        return self.n

    def describe_points_planar(self, xys, threads=1):
        xys = np.ascontiguousarray(xys, dtype=np.float64)
        self.n = lib().orc_surf_describe_points_planar(self._h, _fp(xys, C.c_double), len(xys), threads)
        return self.n

    def describe_points(self, xys, img=None, threads=1):
        xys = np.ascontiguousarray(xys, dtype=np.float64)
        self.n = lib().orc_surf_describe_points(self._h, img.c() if img is not None else None, _fp(xys, C.c_double), len(xys), threads)
        self._bands = 1
        return self.n

    def fetch(self):
        n = self.n
        xys = np.zeros((n, 3)); ang = np.zeros(n); white = np.zeros(n, dtype=np.uint8); desc = np.zeros((n, self.dof * getattr(self, "_bands", 1)))
        lib().orc_surf_fetch(self._h, _fp(xys, C.c_double), _fp(ang, C.c_double), _fp(white, C.c_uint8), _fp(desc, C.c_double))
        return xys, ang, white, desc

    def integral(self):
        w, h = self._shape
        out = np.zeros((h, w), dtype=np.float32)
        lib().orc_surf_integral(self._h, _fp(out))
        return out


def associate_l2(src, dst, maxErr=MAX_VALUE_F64, backwards=True, threads=1, sqrt_score=False):
    """AssociateGreedy + ScoreAssociateEuclideanSq_F64 (or ScoreAssociateEuclidean_F64 when sqrt_score)
    -> (pairs int32[ns], fitQuality float64[ns])."""
    src = np.ascontiguousarray(src, dtype=np.float64); dst = np.ascontiguousarray(dst, dtype=np.float64)
    ns, nd = len(src), len(dst)
    dof = src.shape[1] if ns else (dst.shape[1] if nd else 0)
    pairs = np.zeros(ns, dtype=np.int32); fit = np.zeros(ns, dtype=np.float64)
    fn = lib().orc_associate_euclidean if sqrt_score else lib().orc_associate_l2
    fn(_fp(src, C.c_double), ns, _fp(dst, C.c_double), nd, dof, maxErr, int(backwards), _fp(pairs, C.c_int), _fp(fit, C.c_double), threads)
    return pairs, fit


def associate_surf_basic(src, srcWhite, dst, dstWhite, maxErr=MAX_VALUE_F64, backwards=True, sqrt_score=False):
    """AssociateSurfBasic.associate (F:alg/feature/associate/AssociateSurfBasic.java:83-124, sort :133-147): features are split by
    Laplacian sign, each sign is associated on its own (positive first), matches carry the indices of the original lists.
    Returns (matches [(src, dst, fitScore)], unassociatedSrc) in the reference's order."""
    src = np.ascontiguousarray(src, dtype=np.float64); dst = np.ascontiguousarray(dst, dtype=np.float64)
    sw = np.asarray(srcWhite, dtype=bool); dw = np.asarray(dstWhite, dtype=bool)
    matches, unassoc = [], []
    if len(src) == 0 or len(dst) == 0:
        return matches, unassoc
    for sign in (True, False):
        si = np.flatnonzero(sw == sign); di = np.flatnonzero(dw == sign)
        if len(si) == 0:
            continue
        if len(di) == 0:
            # WrapAssociateGreedy on an empty destination list: nothing matches, every source is unassociated
            unassoc.extend(int(i) for i in si)
            continue
        pairs, fit = associate_l2(src[si], dst[di], maxErr, backwards, 1, sqrt_score)
        for k in range(len(si)):
            if pairs[k] >= 0:
                matches.append((int(si[k]), int(di[pairs[k]]), float(fit[k])))
        unassoc.extend(int(si[k]) for k in range(len(si)) if pairs[k] < 0)
    return matches, unassoc


def associate_hamming(src, dst, maxErr=MAX_VALUE_F64, backwards=True, threads=1):
    """AssociateGreedy + ScoreAssociateHamming_B on int32 words."""
    src = np.ascontiguousarray(src, dtype=np.int32); dst = np.ascontiguousarray(dst, dtype=np.int32)
    ns, nd = len(src), len(dst)
    words = src.shape[1] if ns else (dst.shape[1] if nd else 0)
    pairs = np.zeros(ns, dtype=np.int32); fit = np.zeros(ns, dtype=np.float64)
    lib().orc_associate_hamming(_fp(src, C.c_int32), ns, _fp(dst, C.c_int32), nd, words, maxErr, int(backwards), _fp(pairs, C.c_int), _fp(fit, C.c_double), threads)
    return pairs, fit


def brief_definition(seed=123, radius=16, numPoints=512):
    sp = np.zeros((numPoints, 2), dtype=np.int32); cmp_ = np.zeros((numPoints, 2), dtype=np.int32)
    lib().orc_brief_definition(seed, radius, numPoints, _fp(sp, C.c_int), _fp(cmp_, C.c_int))
    return sp, cmp_


def brief_describe(img, xy, radius, samplePoints, compare):
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    n = len(xy); npts = len(samplePoints)
    out = np.zeros((n, (npts + 31) // 32), dtype=np.int32)
    sp = np.ascontiguousarray(samplePoints, dtype=np.int32); cp = np.ascontiguousarray(compare, dtype=np.int32)
    lib().orc_brief_describe(img.c(), radius, npts, _fp(sp, C.c_int), _fp(cp, C.c_int), _fp(xy, C.c_double), n, _fp(out, C.c_int32))
    return out


def _kernel(k):
    k = np.ascontiguousarray(k, dtype=np.float32)
    return k, _fp(k)


def conv(kind, kernel, offset, src, threads=1):
    """kind in {'h','v','norm_h','norm_v'}; returns a new Gray (border of the no-border variants left at 0)."""
    k, kp = _kernel(kernel)
    out = Gray(src.width, src.height)
    getattr(lib(), "orc_conv_" + kind)(kp, len(k), offset, src.c(), out.c(), threads)
    return out


def conv2d(kernel2d, offset, src, out=None):
    """ConvolveImageNoBorder.convolve(Kernel2D_F32): the frame of `out` is left untouched."""
    k = np.ascontiguousarray(kernel2d, dtype=np.float32)
    assert k.ndim == 2 and k.shape[0] == k.shape[1]
    out = out or Gray(src.width, src.height)
    lib().orc_conv2d(_fp(k), k.shape[0], offset, src.c(), out.c())
    return out


def blur_mean(src, radiusX, radiusY=None):
    out = Gray(src.width, src.height); st = Gray(src.width, src.height)
    if lib().orc_blur_mean(src.c(), out.c(), radiusX, radiusX if radiusY is None else radiusY, st.c()) != 0:
        raise ValueError("Radius must be > 0")
    return out


def blur_median(src, radius):
    out = Gray(src.width, src.height)
    if lib().orc_blur_median(src.c(), out.c(), radius) != 0:
        raise ValueError("Radius must be > 0")
    return out


def integral_u8(img_u8):
    """IntegralImageOps.transform(GrayU8, GrayS32): (H, W) uint8 -> (H, W) int32."""
    a = np.ascontiguousarray(img_u8, dtype=np.uint8)
    h, w = a.shape
    out = np.zeros((h, w), dtype=np.int32)
    lib().orc_integral_u8(_fp(a, C.c_uint8), 0, w, w, h, _fp(out, C.c_int32), 0, w)
    return out


def hessian_s32(ii_s32, skip, size):
    """IntegralImageFeatureIntensity.hessian(GrayS32, skip, size, intensity) -> (H/skip, W/skip) float32."""
    a = np.ascontiguousarray(ii_s32, dtype=np.int32)
    h, w = a.shape
    out = Gray(w // skip, h // skip)
    lib().orc_hessian_s32(_fp(a, C.c_int32), 0, w, w, h, skip, size, out.c())
    return out.array().copy()


def fh_detect_s32(ii_s32, cfg=None, threads=1):
    """FastHessianFeatureDetector<GrayS32>.detect on the integral image of a GrayU8 frame."""
    cfg = cfg or FhCfg()
    a = np.ascontiguousarray(ii_s32, dtype=np.int32)
    h, w = a.shape
    cap = 1 << 16
    while True:
        out = np.zeros((cap, 3), dtype=np.float64)
        n = lib().orc_fh_detect_s32(_fp(a, C.c_int32), 0, w, w, h, C.byref(cfg), _fp(out, C.c_double), cap, threads)
        if n <= cap:
            return out[:n].copy()
        cap = n


def brief_describe_u8(img_u8, xy, radius, samplePoints, compare):
    a = np.ascontiguousarray(img_u8, dtype=np.uint8)
    h, w = a.shape
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    sp = np.ascontiguousarray(samplePoints, dtype=np.int32); cp = np.ascontiguousarray(compare, dtype=np.int32)
    n = len(cp)
    out = np.zeros((len(xy), (n + 31) // 32), dtype=np.int32)
    lib().orc_brief_u8(_fp(a, C.c_uint8), 0, w, w, h, radius, n, _fp(sp, C.c_int), _fp(cp, C.c_int), _fp(xy, C.c_double), len(xy), _fp(out, C.c_int32))
    return out


def corner_intensity(derivX, derivY, radius, kind="shitomasi", kappa=0.04):
    """FactoryIntensityPointAlg.shiTomasi / harris (unweighted, GrayF32) .process(derivX, derivY, intensity) -> (H, W) float32."""
    k = {"shitomasi": 0, "harris": 1, "mocksum": 2}[kind]
    out = np.zeros((derivX.height, derivX.width), dtype=np.float32)
    if lib().orc_ssd_corner(derivX.c(), derivY.c(), radius, k, np.float32(kappa), _fp(out)) != 0:
        raise ValueError("corner intensity rejected")
    return out


def conv_down(kind, kernel, src, skip, out=None):
    """ConvolveImageDownNormalized.horizontal ('h') / vertical ('v').  `out` defaults to a zeroed image of the
    smallest legal size; raises ValueError where the reference throws (or would read outside the image)."""
    k, kp = _kernel(kernel)
    if out is None:
        out = Gray(src.width // skip, src.height) if kind == "h" else Gray(src.width, src.height // skip)
    if lib().orc_conv_down_norm(int(kind == "v"), kp, len(k), src.c(), out.c(), skip) != 0:
        raise ValueError("down convolution rejected")
    return out


def pyramid(kernel, sigma, scales, src):
    """PyramidDiscreteSampleBlur(kernel, sigma, scales).process(src) -> (list of layer arrays, sigmas)."""
    k, kp = _kernel(kernel)
    sc = np.asarray(scales, dtype=np.int32)
    cap = int(sum((src.width // max(int(v), 1) + 1) * (src.height // max(int(v), 1) + 1) for v in sc))
    out = np.zeros(cap, dtype=np.float32)
    dims = np.zeros(2 * len(sc), dtype=np.int32)
    sig = np.zeros(len(sc), dtype=np.float64)
    n = lib().orc_pyramid(kp, len(k), float(sigma), sc.ctypes.data_as(C.POINTER(C.c_int)), len(sc), src.c(), _fp(out), cap,
                          dims.ctypes.data_as(C.POINTER(C.c_int)), _fp(sig, C.c_double))
    if n < 0:
        raise ValueError("pyramid rejected")
    layers, off = [], 0
    for i in range(len(sc)):
        w, h = int(dims[2 * i]), int(dims[2 * i + 1])
        layers.append(out[off:off + w * h].reshape(h, w).copy())
        off += w * h
    return layers, sig


def gaussian_blur(src, sigma, radius, threads=1):
    out = Gray(src.width, src.height); storage = Gray(src.width, src.height)
    lib().orc_gaussian_blur(src.c(), out.c(), sigma, radius, storage.c(), threads)
    return out


def gradient(kind, src, border_zero=False, threads=1):
    dx = Gray(src.width, src.height); dy = Gray(src.width, src.height)
    getattr(lib(), "orc_" + kind)(src.c(), dx.c(), dy.c(), int(border_zero), threads)
    return dx, dy


def gaussian1d_f32(sigma, radius):
    out = np.zeros(4096, dtype=np.float32)
    w = lib().orc_gaussian1d_f32(sigma, radius, _fp(out))
    return out[:w].copy()


def gaussian_width(sigma, width):
    out = np.zeros(width * width + 64, dtype=np.float64)
    w = lib().orc_gaussian_width(sigma, width, _fp(out, C.c_double))
    return out[:w * w].reshape(w, w).copy()


def gaussian2d_f64(sigma, radius):
    out = np.zeros(65 * 65, dtype=np.float64)
    w = lib().orc_gaussian2d_f64(sigma, radius, _fp(out, C.c_double))
    return out[:w * w].reshape(w, w).copy()
