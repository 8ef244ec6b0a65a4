// What more than one boofcv-ip unit needs (conv.hip, pyramid.hip, gradient.hip, corner.hip): the separable-convolution parameter block with
// its tap expressions, the guarded 16-byte row load, and the launchers' layout predicates.
#ifndef BHIP_IP_DEV_H
#define BHIP_IP_DEV_H
#include "common.h"
#include <type_traits>

#define BHIP_MAX_TAPS 255

struct ConvParams {
	const float* in;
	float* out;
	long long inImageStride, outImageStride;   // floats between the images of a batch (blockIdx.z)
	int inStride, outStride, width, height;
	int kw, koff;
	int unrolled;   // first tap assigns instead of adding to 0
	int mode;       // 0 = no border (frame untouched), 1 = normalised border, 2 = normalised naive (kernel wider than image),
	                // 3 = normalised border pixels only (interior untouched: the mean blur fills it with running sums)
	int borderOnly; // general kernel only: the grid covers just the koff + (kw-koff-1) border columns (rows) of the filtered axis
	float k[BHIP_MAX_TAPS];
};

// Interior taps.  The loads of one output are independent: issue them together (a run-time tap loop waits for each load before the next).
// Unrolled widths (ConvolveImageUnrolled_SB_F32_F32 / ConvolveDownNoBorderUnrolled_F32_F32): total = s[0]*k[0]; total += s[i]*k[i] ...
template <int KW>
__device__ __forceinline__ float tapsFirstAssigns(const float* __restrict__ s, long long step, const float* k) {
	float v[KW];
#pragma unroll
	for (int i = 0; i < KW; i++) v[i] = s[i * step];
	float total = v[0] * k[0];
#pragma unroll
	for (int i = 1; i < KW; i++) total += v[i] * k[i];
	return total;
}
__device__ __forceinline__ float tapsUnrolled(const float* __restrict__ s, long long step, const float* k, int kw) {
	switch (kw) {
	case 3: return tapsFirstAssigns<3>(s, step, k);
	case 5: return tapsFirstAssigns<5>(s, step, k);
	case 7: return tapsFirstAssigns<7>(s, step, k);
	case 9: return tapsFirstAssigns<9>(s, step, k);
	default: return tapsFirstAssigns<11>(s, step, k);
	}
}
// Standard form (ConvolveImageStandard_SB / ConvolveDownNoBorderStandard): total = 0; total += s[i]*k[i] in order, loads four at a time
__device__ __forceinline__ float tapsStandard(const float* __restrict__ s, long long step, const float* k, int kw) {
	float total = 0;
	int i = 0;
	for (; i + 4 <= kw; i += 4) {
		const float v0 = s[i * step], v1 = s[(i + 1) * step], v2 = s[(i + 2) * step], v3 = s[(i + 3) * step];
		total += v0 * k[i];
		total += v1 * k[i + 1];
		total += v2 * k[i + 2];
		total += v3 * k[i + 3];
	}
	for (; i < kw; i++) total += s[i * step] * k[i];
	return total;
}

// One output value from `s` (taps `step` floats apart in LDS), exactly the reference's expression for the pixel's position class:
//   interior            total = s0*k0 (unrolled widths) or 0 + s0*k0 (standard), then total += s_i*k_i in tap order
//   border, normalised  weight += k; total += s*k over the taps inside the image, total / weight   (ConvolveNormalized_JustBorder_SB)
// KW > 0: compile-time width (the reference's unrolled widths 3..11), KW == 0: run-time width.  Returns false when the pixel is not written.
// kc: where the coefficients are read from -- the kernel arguments by default; the tiled kernels pass their LDS copy (a run-time index into
// the argument block is a memory access per tap)
template <int KW>
__device__ __forceinline__ bool convOne(const ConvParams& P, const float* s, int step, int pos, int extent, float& result, const float* kc = nullptr) {
	if (!kc) kc = P.k;
	const int kw = KW > 0 ? KW : P.kw;
	const int offL = P.koff, offR = kw - P.koff - 1;
	const bool interior = pos >= offL && pos < extent - offR;
	if (interior && P.mode != 2) {
		if (P.mode == 3) return false;
		float total;
		if (KW > 0) {
			float v[KW > 0 ? KW : 1];
#pragma unroll
			for (int i = 0; i < KW; i++) v[i] = s[i * step];
			total = v[0] * kc[0];
#pragma unroll
			for (int i = 1; i < KW; i++) total += v[i] * kc[i];
		} else {
			total = P.unrolled ? s[0] * kc[0] : 0.0f + s[0] * kc[0];
			int i = 1;
			for (; i + 4 <= kw; i += 4) {
				const float v0 = s[i * step], v1 = s[(i + 1) * step], v2 = s[(i + 2) * step], v3 = s[(i + 3) * step];
				total += v0 * kc[i];
				total += v1 * kc[i + 1];
				total += v2 * kc[i + 2];
				total += v3 * kc[i + 3];
			}
			for (; i < kw; i++) total += s[i * step] * kc[i];
		}
		result = total;
		return true;
	}
	if (P.mode == 0) return false;
	const int k0 = max(0, offL - pos);
	const int k1 = min(kw, extent - pos + offL);
	float total = 0, weight = 0;
	for (int k = k0; k < k1; k++) {
		const float w = kc[k];
		weight += w;
		total += s[k * step] * w;
	}
	result = total / weight;
	return true;
}

// 16-byte load of in[gx .. gx+3] of a row of `width` floats; elements outside [0,width) read as 0 (they are never used as taps)
__device__ __forceinline__ float4 loadRow4(const float* __restrict__ row, int gx, int width) {
	if (gx >= 0 && gx + 3 < width) return *reinterpret_cast<const float4*>(row + gx);
	float4 v;
	v.x = (gx >= 0 && gx < width) ? row[gx] : 0.0f;
	v.y = (gx + 1 >= 0 && gx + 1 < width) ? row[gx + 1] : 0.0f;
	v.z = (gx + 2 >= 0 && gx + 2 < width) ? row[gx + 2] : 0.0f;
	v.w = (gx + 3 >= 0 && gx + 3 < width) ? row[gx + 3] : 0.0f;
	return v;
}

// One value of the fused one-pass kernels (k_blur_fused, k_pyr_layer_fused) from its KW taps in registers
template <int KW>
__device__ __forceinline__ float blurTapsInterior(const float (&v)[KW], const float* k) {
	float total = v[0] * k[0];
#pragma unroll
	for (int i = 1; i < KW; i++) total += v[i] * k[i];
	return total;
}
// first: index of tap 0 along the filtered axis (pos - R); extent: image size along that axis.  Taps outside [0, extent) are skipped.
template <int KW>
__device__ __forceinline__ float blurTapsBorder(const float (&v)[KW], const float* k, int first, int extent) {
	float total = 0, weight = 0;
#pragma unroll
	for (int i = 0; i < KW; i++) {
		const bool in = first + i >= 0 && first + i < extent;
		const float w = k[i];
		weight = in ? weight + w : weight;
		total = in ? total + v[i] * w : total;
	}
	return total / weight;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ConvolveImageNormalized.horizontal / vertical (F32) along an axis of `extent` pixels: the naive form (mode 2) when the kernel is at least as
// wide as the image, else border re-normalisation (mode 1) with the kernel re-normalised first when |sum - 1| > 1e-4 (Kernel1D_F32.computeSum
// is a sequential fp32 sum).  P.k / P.kw must be set.
static void setNormalizedMode(ConvParams& P, int extent) {
	const int kw = P.kw;
	if (kw >= extent) {
		P.mode = 2;
		return;
	}
	P.mode = 1;
	float sum = 0;
	for (int i = 0; i < kw; i++) sum += P.k[i];
	float diff = sum - 1.0f;
	if (diff < 0) diff = -diff;
	if (diff > 1e-4f) {
		float total = 0;
		for (int i = 0; i < kw; i++) total += P.k[i];
		for (int i = 0; i < kw; i++) P.k[i] /= total;
	}
}

// both sides of a launch allow 16-byte vector accesses: base, row stride and image stride
template <class T>
static bool vec4(DevImg<T> v) { return aligned16(v.data) && v.stride % 4 == 0 && v.imageStride % 4 == 0; }

// dx and dy of one gradient (or one corner intensity) are addressed with one row stride and one image stride
template <class T>
static bool sameLayout(DevImg<T> a, DevImg<T> b) { return a.stride == b.stride && a.imageStride == b.imageStride; }

#endif
