// Device-side Fast-Hessian response of ONE pixel of one level (shared by k_hessian and the on-demand outer levels of k_nms_scalespace).
// Reference: ImplIntegralImageFeatureIntensity.hessianInner / hessianBorder (see hessian.hip).
#pragma once
#include "common.h"

struct HessLevel {
	int size;
	int bS, bL, rF, rS;     // blockSmall, blockLarge, radiusFeature, radiusSkinny
	int border, lost;       // border (in output pixels), lostPixel
	float norm;
	// kernelDerivXX / YY / XY parameters for the border path
	int r1, r2, r3, b;
};

// T = float (GrayF32 integral image) or int (GrayS32: exact integer box sums, converted where the reference converts -- at the
// assignment / compound assignment into a float: ImplIntegralImageFeatureIntensity.java:245-390)
template <class T>
__device__ __forceinline__ T block_zero(const T* __restrict__ d, int stride, int W, int H, int x0, int y0, int x1, int y1) {
	x0 = min(x0, W - 1);
	y0 = min(y0, H - 1);
	x1 = min(x1, W - 1);
	y1 = min(y1, H - 1);
	// branch-free: the four corners are always fetched (from coordinates clamped into the image) and zeroed afterwards, so the
	// 40 taps of a border pixel are independent loads in flight together
	const int cx0 = max(x0, 0), cy0 = max(y0, 0), cx1 = max(x1, 0), cy1 = max(y1, 0);
	const T vbr = d[(long long)cy1 * stride + cx1], vtr = d[(long long)cy0 * stride + cx1];
	const T vbl = d[(long long)cy1 * stride + cx0], vtl = d[(long long)cy0 * stride + cx0];
	const T br = (x1 >= 0 && y1 >= 0) ? vbr : T(0);
	const T tr = (y0 >= 0 && x1 >= 0) ? vtr : T(0);
	const T bl = (x0 >= 0 && y1 >= 0) ? vbl : T(0);
	const T tl = (x0 >= 0 && y0 >= 0) ? vtl : T(0);
	return br - tr - bl + tl;
}

// The 32 taps of hessianInner, by box: xx(r, k) = row r (top, bottom) and column k * blockSmall of the Dxx lobes; yy(k, s) = row k * blockSmall
// and side s (left, right) of the Dyy lobes; xy(r, c) = row r (y1..y4) and column c (0, blockSmall, blockSmall + 1, 2 * blockSmall + 1) of the Dxy
// quadrants.  One expression for every tap source (global memory here, LDS in k_hessian_rows): the order of the sums, the T(3) products and
// the conversions are the reference's.
template <class T, class Taps>
__device__ __forceinline__ void hessianInnerExpr(const Taps& t, float& Dxx, float& Dyy, float& Dxy) {
	Dxx = (float)(t.xx(1, 3) - t.xx(0, 3) - t.xx(1, 0) + t.xx(0, 0));
	Dxx -= (float)(T(3) * (t.xx(1, 2) - t.xx(0, 2) - t.xx(1, 1) + t.xx(0, 1)));

	Dyy = (float)(t.yy(3, 1) - t.yy(3, 0) - t.yy(0, 1) + t.yy(0, 0));
	Dyy -= (float)(T(3) * (t.yy(2, 1) - t.yy(2, 0) - t.yy(1, 1) + t.yy(1, 0)));

	Dxy = (float)(t.xy(1, 1) - t.xy(0, 1) - t.xy(1, 0) + t.xy(0, 0));
	Dxy -= (float)(t.xy(1, 3) - t.xy(0, 3) - t.xy(1, 2) + t.xy(0, 2));
	Dxy += (float)(t.xy(3, 3) - t.xy(2, 3) - t.xy(3, 2) + t.xy(2, 2));
	Dxy -= (float)(t.xy(3, 1) - t.xy(2, 1) - t.xy(3, 0) + t.xy(2, 0));
}

__device__ __forceinline__ float hessianDeterminant(float Dxx, float Dyy, float Dxy, float norm) {
	Dxx *= norm;
	Dxy *= norm;
	Dyy *= norm;
	return Dxx * Dyy - 0.81f * Dxy * Dxy;
}

// rows and columns of the Dxy quadrants relative to (y1, first column): 0, bS, bS + 1, 2 bS + 1
__host__ __device__ __forceinline__ int hessXyOffset(int i, int bS) { return i == 0 ? 0 : i == 1 ? bS : i == 2 ? bS + 1 : 2 * bS + 1; }

// taps of the output pixel whose first tap column is `col` (row yy of the image), gathered from the integral image d
template <class T>
struct HessTapsGlobal {
	const T* __restrict__ d;
	long long top, l, y1, stride;
	int bS, bL;
	__device__ __forceinline__ HessTapsGlobal(const T* __restrict__ d_, int stride_, const HessLevel& L, int yy, int col)
		: d(d_), top((long long)(yy - L.rS - 1) * stride_ + col), l((long long)(yy - L.rF - 1) * stride_ + (L.rF - L.rS) + col),
		  y1((long long)(yy - L.bS - 1) * stride_ + (L.rF - L.bS) + col), stride(stride_), bS(L.bS), bL(L.bL) {}
	__device__ __forceinline__ T xx(int r, int k) const { return d[top + (long long)(r * bL) * stride + k * bS]; }
	__device__ __forceinline__ T yy(int k, int s) const { return d[l + (long long)(k * bS) * stride + s * bL]; }
	__device__ __forceinline__ T xy(int r, int c) const { return d[y1 + (long long)hessXyOffset(r, bS) * stride + hessXyOffset(c, bS)]; }
};

// det(Hessian) of output pixel (x, y) of a level with geometry L on the octave lattice `skip` (w x h outputs): hessianInner inside the
// level's border, the clamped border form outside.  d = integral image of this frame.
template <class T>
__device__ __forceinline__ float hessianCompute(const T* __restrict__ d, int stride, int W, int H, const HessLevel& L, int skip, int w, int h, int x, int y) {
	const bool inner = x >= L.border && x < w - L.border && y >= L.border && y < h - L.border;
	const int xx = x * skip, yy = y * skip;
	float Dxx, Dyy, Dxy;
	if (inner) {
		// hessianInner: the first inner column sits at offset `lost`, then +skip per output pixel
		const int col = L.lost + (x - L.border) * skip;
		hessianInnerExpr<T>(HessTapsGlobal<T>(d, stride, L, yy, col), Dxx, Dyy, Dxy);
	} else {
		// computeHessian via convolveSparse: ret = 0; ret += block_zero(...) * scale, block by block (float scales for GrayF32, int for GrayS32)
		T ret = 0;
		ret += block_zero<T>(d, stride, W, H, xx - L.r2 - 1, yy - L.r3 - 1, xx + L.r2, yy + L.r3) * T(1);
		ret += block_zero<T>(d, stride, W, H, xx - L.r1 - 1, yy - L.r3 - 1, xx + L.r1, yy + L.r3) * T(-3);
		Dxx = (float)ret;
		ret = 0;
		ret += block_zero<T>(d, stride, W, H, xx - L.r3 - 1, yy - L.r2 - 1, xx + L.r3, yy + L.r2) * T(1);
		ret += block_zero<T>(d, stride, W, H, xx - L.r3 - 1, yy - L.r1 - 1, xx + L.r3, yy + L.r1) * T(-3);
		Dyy = (float)ret;
		ret = 0;
		const int b = L.b;
		ret += block_zero<T>(d, stride, W, H, xx - b - 1, yy - b - 1, xx - 1, yy - 1) * T(1);
		ret += block_zero<T>(d, stride, W, H, xx, yy - b - 1, xx + b, yy - 1) * T(-1);
		ret += block_zero<T>(d, stride, W, H, xx, yy, xx + b, yy + b) * T(1);
		ret += block_zero<T>(d, stride, W, H, xx - b - 1, yy, xx - 1, yy + b) * T(-1);
		Dxy = (float)ret;
	}
	return hessianDeterminant(Dxx, Dyy, Dxy, L.norm);
}

static inline HessLevel bhipMakeHessLevel(int size, int skip) {
	HessLevel L;
	L.size = size;
	L.bS = size / 3;
	L.bL = size - L.bS - 1;
	L.rF = size / 2;
	L.rS = L.bL / 2;
	const int borderOrig = L.rF + 1 + (skip - (L.rF + 1) % skip);
	L.border = borderOrig / skip;
	L.lost = borderOrig - L.rF - 1;
	L.norm = 1.0f / (float)(size * size);
	const int blockW = size / 3, blockH = size - blockW - 1;
	L.r1 = blockW / 2;
	L.r2 = blockW + L.r1;
	L.r3 = blockH / 2;
	L.b = size / 3;
	return L;
}

