// Stationary background models on a batch of independent camera streams: BackgroundStationaryBasic, BackgroundStationaryGaussian and
// BackgroundStationaryGmm on GrayU8 / GrayF32 and Planar<GrayU8> / Planar<GrayF32> with 1..4 bands.
//
// Reference (F: = main/boofcv-feature/src/main/java/boofcv/):
//   BackgroundStationaryBasic_SB updateBackground / segment       F:alg/background/stationary/BackgroundStationaryBasic_SB.java:58-123
//   BackgroundStationaryBasic_PL                                  F:alg/background/stationary/BackgroundStationaryBasic_PL.java:66-142
//   BackgroundStationaryGaussian_SB                               F:alg/background/stationary/BackgroundStationaryGaussian_SB.java:58-142
//   BackgroundStationaryGaussian_PL                               F:alg/background/stationary/BackgroundStationaryGaussian_PL.java:72-180
//   BackgroundStationaryGmm, _SB, _MB                             F:alg/background/stationary/BackgroundStationaryGmm.java:48-78, BackgroundStationaryGmm_SB.java:50-100,
//                                                                 BackgroundStationaryGmm_MB.java:54-105
//   BackgroundGmmCommon updateMixture / updateWeightAndPrune / checkBackground   F:alg/background/BackgroundGmmCommon.java:78-375
//   BackgroundModelStationary.updateBackground(frame, segment)    F:alg/background/BackgroundModelStationary.java:48-51 (update, then segment)
//
// One kernel template k_background<ALG, T, B, K, SB, SEG>: algorithm, pixel type, number of bands, largest number of Gaussians, the single-band
// (Gray*, *_SB classes) or multi-band (Planar, *_PL / *_MB classes) form of the arithmetic, and update (with or without masks, a
// workgroup-uniform run-time branch) or segment.
//
// Layout: the model of a stream is `C` dense float planes [component][h][w] (Basic: C = B, the bands; Gaussian: C = 2B, plane 2b the mean and
// 2b+1 the variance of band b, the reference's band order; GMM: C = K * (2 + B), plane g * (2 + B) + k = weight, variance, means of Gaussian g),
// so the lanes of a wave read and write consecutive floats of every plane.  The reference's interleaved GMM row exists only in
// bhip_bg_fetch_model / bhip_bg_store_model.
//
// Tile: a workgroup of 256 owns 64 * PX columns x 4 rows of one stream; a lane owns PX consecutive pixels of one row, PX = 4, 2 or 1 so that
// PX * C stays within about 64 registers (bgPx).  The lane's first column is where the address of the first frame's mask row (of the frame row
// when there are no masks) is a multiple of PX elements: the mask and a GrayU8 frame are then read and written PX bytes at a time at any view
// layout, and only the lanes cut by the left or right edge fall back to single bytes.  Accesses whose address is not a multiple of their size
// (model planes of an odd width, later frames at an odd frame stride) are done element by element.  No access leaves a view.
//
// Multi-frame form: the launch walks the T frames of its stream in order with the pixel's model in registers: the model is read once and written
// once, mask t is what updateBackground(frame_t, mask_t) writes after frames 0 .. t.
//
// The mixture lives in a compile-time-sized vector value (BgVec); "slot i" with a run-time i is always a chain of selects over the K slots (bgSel,
// and `if (g == i)` inside unrolled loops), never an indexed access: no instantiation uses scratch (DESIGN.md has the registers of each).  Every loop bound is a template parameter or T.  No atomics, no LDS, no
// communication between workgroups.
//
// Units: background.hip holds the host side and instantiates the Basic and Gaussian kernels (40 small ones); the 160 GMM kernels, fully
// unrolled mixtures that take most of the library's compile time, are instantiated by the background_gmm_*.hip units -- one per band form,
// pixel type and range of K (1..6 and 7..8, about equal shares of the work); the `extern template` lines at the end of this file keep them
// out of every other unit -- so that they compile side by side and none takes longer than the library's other units.
#ifndef BHIP_BACKGROUND_DEV_H
#define BHIP_BACKGROUND_DEV_H
#include "common.h"

#define BG_LANES 64
#define BG_ROWS 4

struct BgParams {
	const void* frames;          // [stream][frame][band][h][w] view: strides in elements
	long long fStreamStride, fFrameStride, fBandStride;
	int fStride;
	uint8_t* masks;              // nullptr: update without masks
	long long mStreamStride, mFrameStride;
	int mStride;
	float* model;                // [stream][C][h][w]
	const int* state;            // [stream][2]: initialised, BackgroundGmmCommon.unknownValue
	int w, h, T;
	int unknownValue;            // BackgroundModel.unknownValue & 0xFF
	int neverInit;               // BackgroundStationaryGaussian with width 1: `background.width == 1` stays true, every frame initialises
	float learnRate;             // Basic, Gaussian: learnRate.  GMM: learningRate = 1 / learningPeriod
	float minusLearn;            // 1.0f - learnRate
	float threshold;             // Basic: thresholdSq.  Gaussian: threshold
	float initialVariance;
	float minimumDifference, adjustedMinimumDifference;
	float decay, maxDistance, significantWeight;   // maxDistance: the multi-band form's maxDistance * numBands where SB is false
};

// pixels a lane owns for a model of C components
__host__ __device__ constexpr int bgPx(int C) { return C <= 16 ? 4 : C <= 32 ? 2 : 1; }
__host__ __device__ constexpr int bgComponents(int alg, int B, int K) { return alg == BHIP_BG_BASIC ? B : alg == BHIP_BG_GAUSSIAN ? 2 * B : K * (2 + B); }

// ---- PX consecutive elements of a row; `in`: the elements inside the image.  One access when all are and the address allows it ----
template <int PX>
__device__ __forceinline__ void bgLoad(const float* p, unsigned int in, float* v) {
	if (PX > 1 && in == (1u << PX) - 1 && ((uintptr_t)p & (4 * PX - 1)) == 0) {
		if constexpr (PX == 4) { const float4 u = *(const float4*)p; v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w; }
		if constexpr (PX == 2) { const float2 u = *(const float2*)p; v[0] = u.x; v[1] = u.y; }
	} else {
#pragma unroll
		for (int j = 0; j < PX; j++) {
			v[j] = 0.0f;
			if (in >> j & 1u) v[j] = p[j];
		}
	}
}
// GImageGray.getF on GrayU8: data & 0xFF as float
template <int PX>
__device__ __forceinline__ void bgLoad(const uint8_t* p, unsigned int in, float* v) {
	if (PX > 1 && in == (1u << PX) - 1 && ((uintptr_t)p & (PX - 1)) == 0) {
		unsigned int u = 0;
		if constexpr (PX == 4) u = *(const unsigned int*)p;
		if constexpr (PX == 2) u = *(const unsigned short*)p;
#pragma unroll
		for (int j = 0; j < PX; j++) v[j] = (float)((u >> (8 * j)) & 255u);
	} else {
#pragma unroll
		for (int j = 0; j < PX; j++) {
			v[j] = 0.0f;
			if (in >> j & 1u) v[j] = (float)p[j];
		}
	}
}
template <int PX>
__device__ __forceinline__ void bgStore(float* p, unsigned int in, const float* v) {
	if (PX > 1 && in == (1u << PX) - 1 && ((uintptr_t)p & (4 * PX - 1)) == 0) {
		if constexpr (PX == 4) *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
		if constexpr (PX == 2) *(float2*)p = make_float2(v[0], v[1]);
	} else {
#pragma unroll
		for (int j = 0; j < PX; j++)
			if (in >> j & 1u) p[j] = v[j];
	}
}
template <int PX>
__device__ __forceinline__ void bgStore(uint8_t* p, unsigned int in, const int* v) {
	if (PX > 1 && in == (1u << PX) - 1 && ((uintptr_t)p & (PX - 1)) == 0) {
		unsigned int u = 0;
#pragma unroll
		for (int j = 0; j < PX; j++) u |= ((unsigned int)v[j] & 255u) << (8 * j);
		if constexpr (PX == 4) *(unsigned int*)p = u;
		if constexpr (PX == 2) *(unsigned short*)p = (unsigned short)u;
	} else {
#pragma unroll
		for (int j = 0; j < PX; j++)
			if (in >> j & 1u) p[j] = (uint8_t)(v[j] & 255);
	}
}

// ---- Basic: s[b] = background of band b ----
template <int B>
__device__ __forceinline__ void basicUpdate(float* s, const float* px, bool inited, const BgParams& P) {
#pragma unroll
	for (int b = 0; b < B; b++) {
		if (!inited) s[b] = px[b];                                   // GConvertImage.convert(frame, background)
		else s[b] = P.minusLearn * s[b] + P.learnRate * px[b];       // Basic_SB.java:85, Basic_PL.java:95
	}
}
template <int B, bool SB>
__device__ __forceinline__ int basicSegment(const float* s, const float* px, const BgParams& P) {
	if constexpr (SB) {
		const float diff = s[0] - px[0];
		return diff * diff <= P.threshold ? 0 : 1;                   // Basic_SB.java:111-116
	} else {
		double sumErrorSq = 0;                                       // Basic_PL.java:125-135: float products summed in a double
#pragma unroll
		for (int b = 0; b < B; b++) {
			const float diff = s[b] - px[b];
			sumErrorSq += (double)(diff * diff);
		}
		return sumErrorSq <= (double)P.threshold ? 0 : 1;
	}
}

// ---- Gaussian: s[2b] = mean, s[2b+1] = variance of band b ----
template <int B>
__device__ __forceinline__ void gaussianUpdate(float* s, const float* px, bool inited, const BgParams& P) {
#pragma unroll
	for (int b = 0; b < B; b++) {
		if (!inited) {                                               // Gaussian_SB.java:65-69, Gaussian_PL.java:79-86
			s[2 * b] = px[b];
			s[2 * b + 1] = P.initialVariance;
		} else {                                                     // Gaussian_SB.java:87-93, Gaussian_PL.java:108-114
			const float inputValue = px[b], meanBG = s[2 * b], varianceBG = s[2 * b + 1];
			const float diff = meanBG - inputValue;
			s[2 * b] = P.minusLearn * meanBG + P.learnRate * inputValue;
			s[2 * b + 1] = P.minusLearn * varianceBG + P.learnRate * diff * diff;
		}
	}
}
template <int B, bool SB>
__device__ __forceinline__ int gaussianSegment(const float* s, const float* px, const BgParams& P) {
	if constexpr (SB) {                                              // Gaussian_SB.java:120-135
		const float diff = s[0] - px[0];
		const float chisq = diff * diff / s[1];
		if (chisq <= P.threshold) return 0;
		return (diff >= P.minimumDifference || -diff >= P.minimumDifference) ? 1 : 0;
	} else {                                                         // Gaussian_PL.java:144-173
		float mahalanobis = 0;
#pragma unroll
		for (int b = 0; b < B; b++) {
			const float diff = s[2 * b] - px[b];
			mahalanobis += diff * diff / s[2 * b + 1];
		}
		if (mahalanobis <= P.threshold) return 0;
		if (P.minimumDifference == 0) return 1;
		float sumAbsDiff = 0;
#pragma unroll
		for (int b = 0; b < B; b++) sumAbsDiff += fabsf(s[2 * b] - px[b]);
		return sumAbsDiff >= P.adjustedMinimumDifference ? 1 : 0;
	}
}

// ---- GMM: s[g * G + 0 / 1 / 2 + i] = weight / variance / mean of band i of Gaussian g, G = 2 + B ----
// gmmUpdate / gmmCheck copy the mixture they are handed into a vector value (BgVec), work on that and copy it back: one block of loads at
// the start, one block of stores at the end.  Worked on through the pointer (or in a local float[]), the select chains below end in scratch:
// the compiler merges their loads from different branches into one load at a computed address before it has promoted the array to registers.
// A vector value is never an addressable array; its element accesses are constant once the loops are unrolled.
template <int N>
using BgVec = float __attribute__((ext_vector_type(N)));
template <int N>
__device__ __forceinline__ void bgCopy(BgVec<N>& dst, const float* src) {
#pragma unroll
	for (int c = 0; c < N; c++) dst[c] = src[c];
}
template <int N>
__device__ __forceinline__ void bgCopy(float* dst, const BgVec<N>& src) {
#pragma unroll
	for (int c = 0; c < N; c++) dst[c] = src[c];
}

// element k of the Gaussian in slot i, 0 <= i < K (slot 0 for any other i)
template <int K, int G>
__device__ __forceinline__ float bgSel(const BgVec<K * G>& s, int i, int k) {
	float r = s[k];
#pragma unroll
	for (int g = 1; g < K; g++) r = i == g ? s[g * G + k] : r;
	return r;
}

// BackgroundGmmCommon.updateWeightAndPrune, :188-234.  The reference's loop does not advance when it prunes; an iteration either advances i or
// lowers ng, so it ends within K iterations
template <int K, int B>
__device__ __forceinline__ void gmmWeightAndPrune(BgVec<K * (2 + B)>& s, int ng, int best, float bestWeight, const BgParams& P) {
	constexpr int G = 2 + B;
	int i = 0;
	float weightTotal = 0;
#pragma unroll
	for (int it = 0; it < K; it++) {
		if (i < ng) {
			float weight = bgSel<K, G>(s, i, 0);
			weight = weight - P.learnRate * (weight + P.decay);
			if (weight <= 0) {
				const int last = ng - 1;
				float moved[G];                                      // copy the last Gaussian into this location
#pragma unroll
				for (int k = 0; k < G; k++) moved[k] = bgSel<K, G>(s, last, k);
#pragma unroll
				for (int g = 0; g < K; g++)
					if (g == i) {
#pragma unroll
						for (int k = 0; k < G; k++) s[g * G + k] = moved[k];
					}
				if (last == best) best = i;                          // the best Gaussian just got moved to here
#pragma unroll
				for (int g = 0; g < K; g++)
					if (g == last) s[g * G + 1] = 0;                 // mark it as unused
				ng -= 1;
			} else {
#pragma unroll
				for (int g = 0; g < K; g++)
					if (g == i) s[g * G] = weight;
				weightTotal += weight;
				i++;
			}
		}
	}
	if (best != -1) {                                                // undo the change to the best model
		weightTotal -= bgSel<K, G>(s, best, 0);
		weightTotal += bestWeight;
#pragma unroll
		for (int g = 0; g < K; g++)
			if (g == best) s[g * G] = bestWeight;
	}
#pragma unroll
	for (int g = 0; g < K; g++)
		if (g < ng) s[g * G] /= weightTotal;
}

// the search both updateMixture and checkBackground start with: the first strict minimum of the Mahalanobis distance below the bound, among the
// Gaussians in use (variance > 0 ends the list).  Returns ng
template <int K, int B, bool SB>
__device__ __forceinline__ int gmmSearch(const BgVec<K * (2 + B)>& s, const float* px, float& bestDistance, int& best) {
	constexpr int G = 2 + B;
	int ng = K;
	bool open = true;
#pragma unroll
	for (int g = 0; g < K; g++) {
		if (open) {
			const float variance = s[g * G + 1];
			if (variance <= 0) {
				ng = g;
				open = false;
			} else {
				float mahalanobis;
				if constexpr (SB) {                                  // :256-257
					const float delta = px[0] - s[g * G + 2];
					mahalanobis = delta * delta / variance;
				} else {                                             // :126-131
					mahalanobis = 0;
#pragma unroll
					for (int i = 0; i < B; i++) {
						const float delta = px[i] - s[g * G + 2 + i];
						mahalanobis += delta * delta / variance;
					}
				}
				if (mahalanobis < bestDistance) {
					bestDistance = mahalanobis;
					best = g;
				}
			}
		}
	}
	return ng;
}

// BackgroundGmmCommon.updateMixture: (float, ...) :240-304 where SB, (float[], ...) :112-183 otherwise
template <int K, int B, bool SB>
__device__ __forceinline__ int gmmUpdate(float* mix, const float* px, int unknownValue, const BgParams& P) {
	constexpr int G = 2 + B;
	BgVec<K * G> s;
	bgCopy<K * G>(s, mix);
	int result = 1;                                                  // didn't match any model and can't create a new one
	float bestDistance = P.maxDistance;
	int best = -1;
	const int ng = gmmSearch<K, B, SB>(s, px, bestDistance, best);
	const bool found = SB ? bestDistance != P.maxDistance : best != -1;
	if (found) {
		float weight = bgSel<K, G>(s, best, 0);
		const float variance = bgSel<K, G>(s, best, 1);
		weight += P.learnRate * (1.0f - weight);
		float upd[G];
		upd[0] = 1;                                                  // set to one so that it can't possibly go negative
		if constexpr (SB) {
			const float mean = bgSel<K, G>(s, best, 2);
			const float delta = px[0] - mean;
			upd[1] = variance + (P.learnRate / weight) * (delta * delta * 1.2f - variance);
			upd[2] = mean + delta * P.learnRate / weight;
		} else {
			float sumDeltaSq = 0;
#pragma unroll
			for (int i = 0; i < B; i++) {
				const float mean = bgSel<K, G>(s, best, 2 + i);
				const float delta = px[i] - mean;
				upd[2 + i] = mean + delta * P.learnRate / weight;
				sumDeltaSq += delta * delta;
			}
			sumDeltaSq /= (float)B;
			upd[1] = variance + (P.learnRate / weight) * (sumDeltaSq * 1.2f - variance);
		}
#pragma unroll
		for (int g = 0; g < K; g++)
			if (g == best) {
#pragma unroll
				for (int k = 0; k < G; k++) s[g * G + k] = upd[k];
			}
		gmmWeightAndPrune<K, B>(s, ng, best, weight, P);
		result = weight >= P.significantWeight ? 0 : 1;
	} else if (ng < K) {                                             // no good fit: a new model, there is room
#pragma unroll
		for (int g = 0; g < K; g++)
			if (g == ng) {
				s[g * G] = 1;
				s[g * G + 1] = P.initialVariance;
#pragma unroll
				for (int i = 0; i < B; i++) s[g * G + 2 + i] = px[i];
			}
		if (ng == 0) result = unknownValue;                          // there are no models
		else gmmWeightAndPrune<K, B>(s, ng + 1, ng, P.learnRate, P);
	}
	bgCopy<K * G>(mix, s);
	return result;
}

// BackgroundGmmCommon.checkBackground, :311-375
template <int K, int B, bool SB>
__device__ __forceinline__ int gmmCheck(const float* mix, const float* px, int unknownValue, const BgParams& P) {
	constexpr int G = 2 + B;
	BgVec<K * G> s;
	bgCopy<K * G>(s, mix);
	float bestDistance = P.maxDistance;
	int best = -1;
	const int ng = gmmSearch<K, B, SB>(s, px, bestDistance, best);
	if (ng == 0) return unknownValue;
	const float bestWeight = best == -1 ? 0.0f : bgSel<K, G>(s, best, 0);
	return bestWeight >= P.significantWeight ? 0 : 1;
}

template <int ALG, class T, int B, int K, bool SB, bool SEG>
__global__ __launch_bounds__(256) void k_background(BgParams P) {
	constexpr int C = bgComponents(ALG, B, K), PX = bgPx(C);
	const long long st = blockIdx.z;
	const int y = blockIdx.y * BG_ROWS + (threadIdx.x >> 6);
	if (y >= P.h) return;
	const T* frow = (const T*)P.frames + st * P.fStreamStride + (long long)y * P.fStride;
	uint8_t* mrow = P.masks ? P.masks + st * P.mStreamStride + (long long)y * P.mStride : nullptr;
	// the lane's first column: the row's address at xa is a multiple of PX elements, xa <= 0 < xa + PX
	const int xa = -(int)((mrow ? (uintptr_t)mrow : (uintptr_t)frow / sizeof(T)) % PX);
	const int x = xa + (blockIdx.x * BG_LANES + (threadIdx.x & 63)) * PX;
	if (x >= P.w) return;
	unsigned int in = 0;
#pragma unroll
	for (int j = 0; j < PX; j++)
		if (x + j >= 0 && x + j < P.w) in |= 1u << j;

	const long long plane = (long long)P.w * P.h;
	float* mp = P.model + st * plane * C + (long long)y * P.w + x;
	const int commonUnknown = P.state[2 * st + 1];
	bool inited = P.state[2 * st] != 0 && !P.neverInit;

	float s[PX][C];
	if (inited) {
#pragma unroll
		for (int c = 0; c < C; c++) {
			float v[PX];
			bgLoad<PX>(mp + c * plane, in, v);
#pragma unroll
			for (int j = 0; j < PX; j++) s[j][c] = v[j];
		}
	} else {
#pragma unroll
		for (int j = 0; j < PX; j++)
#pragma unroll
			for (int c = 0; c < C; c++) s[j][c] = 0;                 // BackgroundStationaryGmm.java:71-72 model.zero(); Basic / Gaussian: overwritten by the first frame
	}

	for (int t = 0; t < P.T; t++) {
		float px[PX][B];
#pragma unroll
		for (int b = 0; b < B; b++) {
			float v[PX];
			bgLoad<PX>(frow + t * P.fFrameStride + b * P.fBandStride + x, in, v);
#pragma unroll
			for (int j = 0; j < PX; j++) px[j][b] = v[j];
		}
		int r[PX];
#pragma unroll
		for (int j = 0; j < PX; j++) {
			r[j] = 0;
			if (!(in >> j & 1u)) continue;
			if constexpr (SEG) {
				if (!inited) r[j] = P.unknownValue;                  // ImageMiscOps.fill(segmented, unknownValue)
				else if constexpr (ALG == BHIP_BG_BASIC) r[j] = basicSegment<B, SB>(s[j], px[j], P);
				else if constexpr (ALG == BHIP_BG_GAUSSIAN) r[j] = gaussianSegment<B, SB>(s[j], px[j], P);
				else r[j] = gmmCheck<K, B, SB>(s[j], px[j], P.unknownValue, P);
			} else if constexpr (ALG == BHIP_BG_BASIC) {
				basicUpdate<B>(s[j], px[j], inited, P);
				if (mrow) r[j] = basicSegment<B, SB>(s[j], px[j], P);
			} else if constexpr (ALG == BHIP_BG_GAUSSIAN) {
				gaussianUpdate<B>(s[j], px[j], inited, P);
				if (mrow) r[j] = P.neverInit ? P.unknownValue : gaussianSegment<B, SB>(s[j], px[j], P);
			} else {
				r[j] = gmmUpdate<K, B, SB>(s[j], px[j], commonUnknown, P);
			}
		}
		if (mrow) bgStore<PX>(mrow + t * P.mFrameStride + x, in, r);
		inited = !P.neverInit;
	}

	if constexpr (!SEG) {
#pragma unroll
		for (int c = 0; c < C; c++) {
			float v[PX];
#pragma unroll
			for (int j = 0; j < PX; j++) v[j] = s[j][c];
			bgStore<PX>(mp + c * plane, in, v);
		}
	}
}

// ---- dispatch: (algorithm, pixel type, bands, Gaussians, form, mode) -> instantiation ----
template <int ALG, class T, int B, int K, bool SB>
void bgLaunch2(bool seg, dim3 grid, hipStream_t st, const BgParams& P) {
	if (seg) hipLaunchKernelGGL((k_background<ALG, T, B, K, SB, true>), grid, dim3(256), 0, st, P);
	else hipLaunchKernelGGL((k_background<ALG, T, B, K, SB, false>), grid, dim3(256), 0, st, P);
}
template <int ALG, class T, int B, bool SB>
static void bgLaunch1(int K, bool seg, dim3 grid, hipStream_t st, const BgParams& P) {
	if constexpr (ALG != BHIP_BG_GMM) {
		bgLaunch2<ALG, T, B, 1, SB>(seg, grid, st, P);
	} else {
		switch (K) {
		case 1: bgLaunch2<ALG, T, B, 1, SB>(seg, grid, st, P); break;
		case 2: bgLaunch2<ALG, T, B, 2, SB>(seg, grid, st, P); break;
		case 3: bgLaunch2<ALG, T, B, 3, SB>(seg, grid, st, P); break;
		case 4: bgLaunch2<ALG, T, B, 4, SB>(seg, grid, st, P); break;
		case 5: bgLaunch2<ALG, T, B, 5, SB>(seg, grid, st, P); break;
		case 6: bgLaunch2<ALG, T, B, 6, SB>(seg, grid, st, P); break;
		case 7: bgLaunch2<ALG, T, B, 7, SB>(seg, grid, st, P); break;
		default: bgLaunch2<ALG, T, B, 8, SB>(seg, grid, st, P); break;
		}
	}
}

// One GMM form: the update and the segment kernel of (pixel type, bands, Gaussians, single-band).  Every form is declared here and
// instantiated by one BG_GMM_LAUNCH line of a background_gmm_<bands>_<type>_k<Gaussians>.hip unit.
#define BG_GMM_LAUNCH(T, B, K, SB) template void bgLaunch2<BHIP_BG_GMM, T, B, K, SB>(bool, dim3, hipStream_t, const BgParams&)
#define BG_GMM_EXTERN(T, B, SB)                                                                                                      \
	extern BG_GMM_LAUNCH(T, B, 1, SB); extern BG_GMM_LAUNCH(T, B, 2, SB); extern BG_GMM_LAUNCH(T, B, 3, SB); extern BG_GMM_LAUNCH(T, B, 4, SB); \
	extern BG_GMM_LAUNCH(T, B, 5, SB); extern BG_GMM_LAUNCH(T, B, 6, SB); extern BG_GMM_LAUNCH(T, B, 7, SB); extern BG_GMM_LAUNCH(T, B, 8, SB)
BG_GMM_EXTERN(uint8_t, 1, true);
BG_GMM_EXTERN(float, 1, true);
BG_GMM_EXTERN(uint8_t, 1, false);
BG_GMM_EXTERN(float, 1, false);
BG_GMM_EXTERN(uint8_t, 2, false);
BG_GMM_EXTERN(float, 2, false);
BG_GMM_EXTERN(uint8_t, 3, false);
BG_GMM_EXTERN(float, 3, false);
BG_GMM_EXTERN(uint8_t, 4, false);
BG_GMM_EXTERN(float, 4, false);
#undef BG_GMM_EXTERN

#endif

