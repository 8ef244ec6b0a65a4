"""Line-by-line Python restatement of the reference's binary image operations, the oracle of the GPU tests (plain loops: the images are small).

  ImplBinaryInnerOps, ImplBinaryBorderOps     I:alg/filter/binary/impl/*.java   (the border loops keep their order: every x top then bottom, then every y
                                              left then right, so corners and images 1 or 2 pixels wide come out as in Java)
  BinaryImageOps erode / dilate numTimes      I:alg/filter/binary/BinaryImageOps.java:158-361 (the tmp1 / tmp2 ping-pong)
  ImplBinaryImageOps logic, relabel, labelToBinary    impl/ImplBinaryImageOps.java
  LinearContourLabelChang2004.process + ContourTracer  :96-152, ContourTracer.java: padded copy, the -1 marks, steps 1-3, both rules

Images are numpy uint8 [H,W] holding 0 and 1 (the inner loops' signed-byte sums are restated for those values only)."""
import numpy as np

FOUR, EIGHT = 4, 8


class _Border:
    """ImageBorderValue.wrap(input, value).get(x, y)"""

    def __init__(self, img, value):
        self.img, self.value = img, value

    def get(self, x, y):
        h, w = self.img.shape
        return int(self.img[y, x]) if 0 <= x < w and 0 <= y < h else self.value


# ---- ImplBinaryInnerOps ----
_N4 = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))
_N8 = tuple((dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1))


def _inner(inp, out, cells, rule):
    h, w = inp.shape
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            total = sum(int(inp[y + dy, x + dx]) for dx, dy in cells)
            out[y, x] = rule(total, int(inp[y, x]))


def _inner_erode4(i, o): _inner(i, o, _N4, lambda t, c: 1 if t == 5 else 0)
def _inner_dilate4(i, o): _inner(i, o, _N4, lambda t, c: 1 if t > 0 else 0)
def _inner_edge4(i, o): _inner(i, o, _N4[1:], lambda t, c: 0 if t == 4 else c)
def _inner_erode8(i, o): _inner(i, o, _N8, lambda t, c: 1 if t == 9 else 0)
def _inner_dilate8(i, o): _inner(i, o, _N8, lambda t, c: 1 if t > 0 else 0)
def _inner_edge8(i, o): _inner(i, o, [c for c in _N8 if c != (0, 0)], lambda t, c: 0 if t == 8 else c)
def _inner_noise(i, o): _inner(i, o, [c for c in _N8 if c != (0, 0)], lambda t, c: 0 if t < 2 else 1 if t > 6 else c)


# ---- ImplBinaryBorderOps: top / bottom / left / right give the get() arguments of each sum as written there; rule(total, input pixel) ----
def _border_loops(inp, out, value, top, bottom, left, right, rule):
    g = _Border(inp, value)
    H, W = inp.shape
    h, w = H - 1, W - 1
    for x in range(W):
        out[0, x] = rule(sum(g.get(*c) for c in top(x)), g.get(x, 0))
        out[h, x] = rule(sum(g.get(*c) for c in bottom(x, h)), g.get(x, h))
    for y in range(H):
        out[y, 0] = rule(sum(g.get(*c) for c in left(y)), g.get(0, y))
        out[y, w] = rule(sum(g.get(*c) for c in right(y, w)), g.get(w, y))


def _border_4(inp, out, value, rule, centre):
    c = (lambda *p: [p]) if centre else (lambda *p: [])
    _border_loops(inp, out, value,
                  lambda x: c(x, 0) + [(x - 1, 0), (x + 1, 0), (x, 1)],
                  lambda x, h: c(x, h) + [(x - 1, h), (x + 1, h), (x, h - 1)],
                  lambda y: c(0, y) + [(1, y), (0, y - 1), (0, y + 1)],
                  lambda y, w: c(w, y) + [(w - 1, y), (w, y - 1), (w, y + 1)], rule)


def _border_8(inp, out, value, rule, centre):
    c = (lambda *p: [p]) if centre else (lambda *p: [])
    _border_loops(inp, out, value,
                  lambda x: c(x, 0) + [(x - 1, 0), (x + 1, 0), (x - 1, 1), (x, 1), (x + 1, 1)],
                  lambda x, h: c(x, h) + [(x - 1, h), (x + 1, h), (x - 1, h - 1), (x, h - 1), (x + 1, h - 1)],
                  lambda y: c(0, y) + [(1, y), (0, y - 1), (1, y - 1), (0, y + 1), (1, y + 1)],
                  lambda y, w: c(w, y) + [(w - 1, y), (w - 1, y - 1), (w, y - 1), (w - 1, y + 1), (w, y + 1)], rule)


def _border_erode4(i, o): _border_4(i, o, 0, lambda t, c: 1 if t == 4 else 0, True)
def _border_dilate4(i, o): _border_4(i, o, 0, lambda t, c: 1 if t > 0 else 0, True)
def _border_erode8(i, o): _border_8(i, o, 1, lambda t, c: 1 if t == 6 else 0, True)
def _border_dilate8(i, o): _border_8(i, o, 0, lambda t, c: 1 if t > 0 else 0, True)
def _border_noise(i, o): _border_8(i, o, 0, lambda t, c: 0 if t < 2 else c, False)


def _border_edge(i, o, outsideZero, eight):
    if outsideZero:   # edge_outside0
        H, W = i.shape
        for x in range(W):
            o[0, x] = i[0, x]
            o[H - 1, x] = i[H - 1, x]
        for y in range(H):
            o[y, 0] = i[y, 0]
            o[y, W - 1] = i[y, W - 1]
    elif eight:
        _border_8(i, o, 1, lambda t, c: 0 if t == 5 else c, False)
    else:
        _border_4(i, o, 1, lambda t, c: 0 if t == 3 else c, False)


# ---- BinaryImageOps ----
def _check(input):
    input = np.asarray(input, np.uint8)
    assert input.ndim == 2
    return input


def _once(inner, border, input):
    out = np.zeros_like(input)
    inner(input, out)
    border(input, out)
    return out


def _times(inner, border, input, numTimes):
    input = _check(input)
    output = _once(inner, border, input)
    if numTimes > 1:
        tmp1, tmp2 = np.zeros_like(input), output
        for _ in range(1, numTimes):
            inner(tmp2, tmp1)
            border(tmp2, tmp1)
            tmp1, tmp2 = tmp2, tmp1
        if tmp2 is not output:
            output[...] = tmp2
    return output


def erode4(input, numTimes):
    if numTimes <= 0:
        raise ValueError("numTimes must be >= 1")
    return _times(_inner_erode4, _border_erode4, input, numTimes)


def dilate4(input, numTimes): return _times(_inner_dilate4, _border_dilate4, input, numTimes)
def erode8(input, numTimes): return _times(_inner_erode8, _border_erode8, input, numTimes)
def dilate8(input, numTimes): return _times(_inner_dilate8, _border_dilate8, input, numTimes)
def edge4(input, outsideZero): return _once(_inner_edge4, lambda i, o: _border_edge(i, o, outsideZero, False), _check(input))
def edge8(input, outsideZero): return _once(_inner_edge8, lambda i, o: _border_edge(i, o, outsideZero, True), _check(input))
def removePointNoise(input): return _once(_inner_noise, _border_noise, _check(input))


MORPH = {"erode4": erode4, "dilate4": dilate4, "erode8": erode8, "dilate8": dilate8}


def logicAnd(a, b): return ((a == 1) & (a == b)).astype(np.uint8)
def logicOr(a, b): return ((a == 1) | (b == 1)).astype(np.uint8)
def logicXor(a, b): return (a != b).astype(np.uint8)
def invert(a): return (a == 0).astype(np.uint8)


def relabel(img, labels):
    """ImplBinaryImageOps.relabel, except that a pixel outside the table stays (the library's documented deviation; the reference throws)"""
    out = img.copy()
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            v = int(img[y, x])
            if 0 <= v < len(labels):
                out[y, x] = labels[v]
    return out


def labelToBinary(img, selected=None):
    if selected is None:
        return (img != 0).astype(np.uint8)
    sel = np.asarray(selected, bool)
    return sel[img].astype(np.uint8)


# ---- LinearContourLabelChang2004 + ContourTracer ----
class _Tracer:
    def __init__(self, rule):
        self.rule = rule
        n = rule
        self.next = [((i + n // 2) % n + (2 if n == 8 else 1)) % n for i in range(n)]
        self.off = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)] if n == 8 else [(1, 0), (0, 1), (-1, 0), (0, -1)]

    def setInputs(self, binary, labeled):
        self.binary, self.labeled = binary, labeled

    def _checkOne(self, x, y):
        if self.binary[y, x] == 1:
            return True
        self.binary[y, x] = -1   # marked so that it is not searched again
        return False

    def _searchOne(self):
        for _ in range(self.rule):
            dx, dy = self.off[self.dir]
            if self._checkOne(self.x + dx, self.y + dy):
                return True
            self.dir = (self.dir + 1) % self.rule
        return False

    def _moveToNext(self):
        dx, dy = self.off[self.dir]
        self.x += dx
        self.y += dy

    def _add(self):
        self.labeled[self.y - 1, self.x - 1] = self.label   # binary has the one-pixel border that labeled lacks

    def trace(self, label, initialX, initialY, external):
        initialDir = (7 if external else 3) if self.rule == 8 else (0 if external else 2)
        self.label, self.dir, self.x, self.y = label, initialDir, initialX, initialY
        self._add()
        if not self._searchOne():
            return
        initialDir = self.dir
        self._moveToNext()
        self.dir = self.next[self.dir]
        while True:
            self._searchOne()
            if self.x == initialX and self.y == initialY and self.dir == initialDir:
                return
            self._add()
            self._moveToNext()
            self.dir = self.next[self.dir]


def contourLabels(binary, rule):
    """-> (labeled int32 [H,W], contours.size) of LinearContourLabelChang2004(rule).process(binary, labeled) on a fresh object"""
    binary = _check(binary)
    H, W = binary.shape
    border = np.zeros((H + 2, W + 2), np.int8)          # Java bytes: the -1 mark is != 0 and != 1
    border[1:-1, 1:-1] = binary.astype(np.int8)
    labeled = np.zeros((H, W), np.int32)
    tracer = _Tracer(rule)
    tracer.setInputs(border, labeled)
    contours = 0
    endY, endX = H + 1, W + 1

    def scanForOne(y, x, end):
        while x < end and border[y, x] != 1:
            x += 1
        return x

    for y in range(1, endY):
        x = scanForOne(y, 1, endX)
        while x < endX:
            label = int(labeled[y - 1, x - 1])
            handled = False
            if label == 0 and border[y - 1, x] != 1:      # step 1: an external contour of a new blob
                contours += 1
                tracer.trace(contours, x, y, True)
                handled = True
                label = contours
            if border[y + 1, x] == 0:                     # step 2: an internal contour (the pixel below is unmarked and white)
                if label == 0:
                    label = int(labeled[y - 1, x - 2])
                tracer.trace(label, x, y, False)
                handled = True
            if not handled:                               # step 3
                if labeled[y - 1, x - 1] == 0:
                    labeled[y - 1, x - 1] = labeled[y - 1, x - 2]
            x = scanForOne(y, x + 1, endX)
    return labeled, contours


def floodLabels(binary, rule):
    """Independent statement of the result: connected components of the pixels equal to 1, numbered from 1 in the raster order of each
    component's first pixel (plain flood fill)."""
    binary = _check(binary)
    H, W = binary.shape
    out = np.zeros((H, W), np.int32)
    nb = [(1, 0), (-1, 0), (0, 1), (0, -1)] + ([(1, 1), (-1, 1), (1, -1), (-1, -1)] if rule == 8 else [])
    n = 0
    for y in range(H):
        for x in range(W):
            if binary[y, x] != 1 or out[y, x]:
                continue
            n += 1
            out[y, x] = n
            stack = [(x, y)]
            while stack:
                cx, cy = stack.pop()
                for dx, dy in nb:
                    px, py = cx + dx, cy + dy
                    if 0 <= px < W and 0 <= py < H and binary[py, px] == 1 and not out[py, px]:
                        out[py, px] = n
                        stack.append((px, py))
    return out, n
