// Device functions the SIFT describe kernels (sift_describe.hip) and the dense descriptors (dense.hip) share.
#pragma once
#include "common.h"

// georegression UtilAngle.dist: circular distance in [0, pi] (describe.hip restates the same)
__device__ __forceinline__ double siftAngleDist(double a, double b) {
	double diff = a - b;
	if (diff > M_PI) diff = diff - 2.0 * M_PI;
	else if (diff < -M_PI) diff = 2.0 * M_PI + diff;
	return fabs(diff);
}
// UtilAngle.domain2PI: (-pi, pi] to [0, 2 pi)
__device__ __forceinline__ double siftDomain2PI(double a) { return a < 0 ? a + 2.0 * M_PI : a; }
// Math.atan2: where an argument is zero the Java specification fixes the result to the doubles nearest pi/2 and pi (and the signed zeros);
// those are selected here, so that a sample on a bin edge does not depend on the device library's rounding.  Everything else is the library's
__device__ __forceinline__ double siftAtan2(double y, double x) {
	if (x == 0.0) {
		if (y > 0.0) return M_PI_2;
		if (y < 0.0) return -M_PI_2;
		if (y != y) return y;
		return signbit(x) ? copysign(M_PI, y) : y;
	}
	if (y == 0.0) return x > 0.0 ? y : x < 0.0 ? copysign(M_PI, y) : x;   // (x is NaN in the last case)
	return atan2(y, x);
}
// GradientThree with the EXTENDED border at (x, y), from the scale image itself
__device__ __forceinline__ void siftGradient(const float* __restrict__ img, int S, int W, int H, int x, int y, float& dx, float& dy) {
	const int xl = max(x - 1, 0), xr = min(x + 1, W - 1), yt = max(y - 1, 0), yb = min(y + 1, H - 1);
	const float* row = img + (long long)y * S;
	dx = (row[xr] - row[xl]) * 0.5f;
	dy = (img[(long long)yb * S + x] - img[(long long)yt * S + x]) * 0.5f;
}
