// Device helpers of the KLT arithmetic that klt.hip (one wave per track) and flow.hip (one lane per pixel) share: BilinearRectangle region(),
// KltTracker.computeSubImageBounds and setAllowedBounds.  Citations: klt.hip.
#pragma once
#include "common.h"
#include <cfloat>
#include <cmath>

// ---- BilinearRectangle_F32.region ----
struct KltRegion {
	int xt, yt, regW, regH;
	bool bR, bB, bad;
	float ax, ay, bx, by, a0, a1, a2, a3;
};
__device__ __forceinline__ KltRegion kltRegion(float tlx, float tly, int w, int h, int W, int H) {
	KltRegion R;
	// region() :65 throws on this test; a NaN corner passes it in Java and then reads from pixel 0, which the integer test below also
	// allows only when the patch fits
	R.bad = tlx < 0 || tly < 0 || tlx + w > W || tly + h > H || w <= 0 || h <= 0;
	R.xt = tlx == tlx ? (int)fminf(fmaxf(tlx, -1.0f), 1.0e9f) : 0;
	R.yt = tly == tly ? (int)fminf(fmaxf(tly, -1.0f), 1.0e9f) : 0;
	if (R.xt < 0 || R.yt < 0 || R.xt + w > W || R.yt + h > H) R.bad = true;   // :89 "requested region is out of bounds"
	R.ax = tlx - R.xt;
	R.ay = tly - R.yt;
	R.bx = 1.0f - R.ax;
	R.by = 1.0f - R.ay;
	R.a0 = R.bx * R.by;
	R.a1 = R.ax * R.by;
	R.a2 = R.ax * R.ay;
	R.a3 = R.bx * R.ay;
	R.bR = R.xt + w == W;
	R.bB = R.yt + h == H;
	R.regW = R.bR ? w - 1 : w;
	R.regH = R.bB ? h - 1 : h;
	return R;
}
// output pixel (j, i) of region(); the image border cases are handleBorder :128-172 as written (including the bottom-only corner, which
// reads row regHeight of the image and mixes with by / ay)
template <class T>
__device__ __forceinline__ float kltRegionAt(const KltRegion& R, const T* p, int stride, int j, int i) {
	const T* q = p + (long long)(R.yt + i) * stride + R.xt + j;
	if (j < R.regW && i < R.regH) {
		const float XY = q[0], xY = q[1], Xy = q[stride], xy = q[stride + 1];
		return R.a0 * XY + R.a1 * xY + R.a2 * xy + R.a3 * Xy;
	}
	if (i < R.regH) return R.by * q[0] + R.ay * q[stride];   // right border column
	if (j == R.regW) return q[0];                             // corner, right and bottom border
	if (!R.bR && j == R.regW - 1) {
		const float XY = q[0], Xy = p[(long long)R.regH * stride + R.xt + R.regW];
		return R.by * XY + R.ay * Xy;
	}
	return R.bx * q[0] + R.ax * q[1];                         // bottom border row
}

// ---- KltTracker.computeSubImageBounds :421-457 ----
struct KltSub {
	int dx0, dy0, dx1, dy1;
	float sx0, sy0;
	bool bad;
};
__device__ __forceinline__ KltSub kltSubBounds(float cx, float cy, int r, int wF, int W, int H) {
	KltSub B;
	B.dx0 = 0; B.dy0 = 0; B.dx1 = wF; B.dy1 = wF;
	B.sx0 = cx - r;
	B.sy0 = cy - r;
	const float sx1 = B.sx0 + wF, sy1 = B.sy0 + wF;
	if (B.sx0 < 0) { B.dx0 = (int)-floorf(B.sx0); B.sx0 += B.dx0; }
	if (sx1 > W) { B.dx1 -= (int)ceilf(sx1 - W); B.dx1 -= (B.sx0 + (B.dx1 - B.dx0) > W ? 1 : 0); }
	if (B.sy0 < 0) { B.dy0 = (int)-floorf(B.sy0); B.sy0 += B.dy0; }
	if (sy1 > H) { B.dy1 -= (int)ceilf(sy1 - H); B.dy1 -= (B.sy0 + (B.dy1 - B.dy0) > H ? 1 : 0); }
	B.bad = B.sx0 < 0 || B.sy0 < 0 || B.sx0 + (B.dx1 - B.dx0) > W || B.sy0 + (B.dy1 - B.dy0) > H;
	return B;
}

struct KltBounds {
	float aL, aR, aT, aB, oL, oR, oT, oB;
	__device__ __forceinline__ KltBounds(int r, int W, int H) {   // setAllowedBounds :330-344
		aL = r; aT = r; aR = W - r - 1; aB = H - r - 1;
		oL = -r; oT = -r; oR = W + r - 1; oB = H + r - 1;
	}
	__device__ __forceinline__ bool inside(float x, float y) const { return !(x < aL || x > aR) && !(y < aT || y > aB); }
	__device__ __forceinline__ bool outside(float x, float y) const { return x < oL || x > oR || y < oT || y > oB; }
};
