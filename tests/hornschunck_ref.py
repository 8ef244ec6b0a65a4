"""numpy float32 restatement of the reference's Horn-Schunck dense optical flow (test reference, not product code; never imported by boofcv_amd/).

Written from the cited BoofCV sources (F: = main/boofcv-feature/src/main/java/boofcv/):
  FactoryDenseOpticalFlow.hornSchunck     F:factory/flow/FactoryDenseOpticalFlow.java:122-138
  HornSchunck.process, the averages       F:alg/flow/HornSchunck.java:92-191
  HornSchunck_F32                         F:alg/flow/HornSchunck_F32.java:36-175
  HornSchunck_U8                          F:alg/flow/HornSchunck_U8.java:38-177
  ConfigHornSchunck                       F:factory/flow/ConfigHornSchunck.java:28-44   (alpha = 20, numIterations = 1000)

float32 throughout, no fused multiply-add, every sum in the operand order of the source.  The reference's loops are restated as rules (w =
width-1, h = height-1): the interior, the last row and the last column of derivX / derivY, and one clamped rule for derivT (its interior loop and
borderDerivT are the same expression) and for the average (innerAverageFlow and computeBorder are the same expression under getExtend's clamp);
average_as_written is the two routines literally, for the check that they are.

Deviations from the reference, shared with the library (include/boofhip.h, bhip_flow_hs_dev_f32):
  - derivY(w, h) is never written by the reference and keeps what the reused array held; it is 0 here, the value of a freshly constructed instance
  - HornSchunck_F32.computeDerivT :114 indexes image1 with image2.stride in its fourth tap; image1's pixel (x+1, y+1) is read here whatever the strides
  - a flow whose size differs from the images is refused by the mirrors (the Java indexes past it)
  - numIterations <= 0 gives the zero flow, as the Java loop does
"""
import numpy as np

F = np.float32
C_SIDE, C_DIAG = F(0.1666667), F(0.08333333)


def _taps(img):
    """(x,y), (x+1,y), (x,y+1), (x+1,y+1) of every pixel, coordinates clamped to the image"""
    H, W = img.shape
    p = np.pad(img, ((0, 1), (0, 1)), "edge")
    return p[:H, :W], p[:H, 1:], p[1:, :W], p[1:, 1:]


def _trunc_div(s, d):
    """Java's int division: toward zero"""
    return (np.abs(s) // d) * np.sign(s)


def derivatives_f32(image1, image2):
    """HornSchunck_F32.computeDerivX / Y / T -> (derivX, derivY, derivT) float32 [H, W]"""
    a, b = np.ascontiguousarray(image1, np.float32), np.ascontiguousarray(image2, np.float32)
    H, W = a.shape
    w, h = W - 1, H - 1
    A00, A10, A01, A11 = _taps(a)
    B00, B10, B01, B11 = _taps(b)
    dX, dY = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    gx = F(0.25) * ((((A10 - A00) + (A11 - A01)) + (B10 - B00)) + (B11 - B01))     # :46-53  d0 + d1 + d2 + d3
    dX[:h, :w] = gx[:h, :w]
    dX[h, :w] = (F(0.5) * ((A10 - A00) + (B10 - B00)))[h, :w]                      # :60-65; column w stays 0 (:56-58)
    gy = F(0.25) * ((((A01 - A00) + (A11 - A10)) + (B01 - B00)) + (B11 - B10))     # :78-85
    dY[:h, :w] = gy[:h, :w]
    dY[:h, w] = (F(0.5) * ((A01 - A00) + (B01 - B00)))[:h, w]                      # :88-93; row h stays 0 (:95-97), (w, h) by definition
    dT = F(0.25) * ((((B00 - A00) + (B10 - A10)) + (B01 - A01)) + (B11 - A11))     # :105-126 and borderDerivT :129-146
    return dX, dY, dT.astype(np.float32)


def derivatives_u8(image1, image2):
    """HornSchunck_U8.computeDerivX / Y / T -> (derivX, derivY, derivT) int16 [H, W] (GrayS16)"""
    a, b = np.ascontiguousarray(image1, np.uint8).astype(np.int32), np.ascontiguousarray(image2, np.uint8).astype(np.int32)
    H, W = a.shape
    w, h = W - 1, H - 1
    A00, A10, A01, A11 = _taps(a)
    B00, B10, B01, B11 = _taps(b)
    dX, dY = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    dX[:h, :w] = _trunc_div((A10 - A00) + (A11 - A01) + (B10 - B00) + (B11 - B01), 4)[:h, :w]
    dX[h, :w] = _trunc_div((A10 - A00) + (B10 - B00), 2)[h, :w]
    dY[:h, :w] = _trunc_div((A01 - A00) + (A11 - A10) + (B01 - B00) + (B11 - B10), 4)[:h, :w]
    dY[:h, w] = _trunc_div((A01 - A00) + (B01 - B00), 2)[:h, w]
    dT = _trunc_div((B00 - A00) + (B10 - A10) + (B01 - A01) + (B11 - A11), 4)      # the interior :112-119; the border: border_deriv_t_u8
    return dX.astype(np.int16), dY.astype(np.int16), dT.astype(np.int16)


def border_deriv_t_u8(d0, d1, d2, d3):
    """HornSchunck_U8.borderDerivT :131-139 as written: the four differences as float, (short)((d0+d1+d2+d3)/4)"""
    s = ((F(d0) + F(d1)) + F(d2)) + F(d3)
    return np.int16(np.trunc(s / F(4)))


def average(flow):
    """averageFlow of borderAverageFlow + innerAverageFlow: flow [H, W, 2] -> [H, W, 2]"""
    p = np.pad(flow, ((1, 1), (1, 1), (0, 0)), "edge")     # getExtend :184-191
    f0, f1, f2, f3 = p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]      # left, right, up, down
    f4, f5, f6, f7 = p[:-2, :-2], p[:-2, 2:], p[2:, :-2], p[2:, 2:]            # up-left, up-right, down-left, down-right
    return C_SIDE * (((f0 + f1) + f2) + f3) + C_DIAG * (((f4 + f5) + f6) + f7)


def average_as_written(flow):
    """HornSchunck.borderAverageFlow :154-182 then innerAverageFlow :125-149, literally"""
    H, W = flow.shape[:2]
    out = np.zeros_like(flow)

    def ext(x, y):
        return flow[min(max(y, 0), H - 1), min(max(x, 0), W - 1)]

    def border(x, y):
        f0, f1, f2, f3 = ext(x - 1, y), ext(x + 1, y), ext(x, y - 1), ext(x, y + 1)
        f4, f5, f6, f7 = ext(x - 1, y - 1), ext(x + 1, y - 1), ext(x - 1, y + 1), ext(x + 1, y + 1)
        out[y, x] = C_SIDE * (f0 + f1 + f2 + f3) + C_DIAG * (f4 + f5 + f6 + f7)

    for y in range(H):
        border(0, y)
        border(W - 1, y)
    for x in range(1, W - 1):
        border(x, 0)
        border(x, H - 1)
    for y in range(1, H - 1):
        for x in range(1, W - 1):
            f0, f1, f2, f3 = flow[y, x - 1], flow[y, x + 1], flow[y - 1, x], flow[y + 1, x]
            f4, f5, f6, f7 = flow[y - 1, x - 1], flow[y - 1, x + 1], flow[y + 1, x - 1], flow[y + 1, x + 1]
            out[y, x] = C_SIDE * (f0 + f1 + f2 + f3) + C_DIAG * (f4 + f5 + f6 + f7)
    return out


def find_flow(derivX, derivY, derivT, alpha, numIterations):
    """findFlow (HornSchunck_F32.java:149-175, HornSchunck_U8.java:151-177) from the zero flow -> [H, W, 2] float32"""
    dx, dy, dt = (np.ascontiguousarray(d).astype(np.float32) for d in (derivX, derivY, derivT))   # float dx = derivX.data[i]: exact for GrayS16
    alpha2 = F(alpha) * F(alpha)                                                                # HornSchunck.java:68
    flow = np.zeros(dx.shape + (2,), np.float32)
    with np.errstate(all="ignore"):
        den = (alpha2 + dx * dx) + dy * dy
        for _ in range(numIterations):
            avg = average(flow)
            u, v = avg[:, :, 0], avg[:, :, 1]
            r = ((dx * u + dy * v) + dt) / den
            flow = np.stack((u - dx * r, v - dy * r), axis=2).astype(np.float32)
    return flow


def horn_schunck(image1, image2, alpha=20.0, numIterations=1000, u8=False):
    """DenseOpticalFlow.process of FactoryDenseOpticalFlow.hornSchunck -> (flow [H, W, 2] float32, (derivX, derivY, derivT))"""
    d = derivatives_u8(image1, image2) if u8 else derivatives_f32(image1, image2)
    return find_flow(*d, alpha, numIterations), d
