// ---------------------------------------------------------------------------------------------------------------
// Thresholding: FactoryThresholdBinary.threshold(ConfigThreshold, GrayU8 | GrayF32) -> InputToBinary, the GrayU8 0/1 image
//   FIXED          GlobalFixedBinaryFilter -> ImplThresholdImageOps.threshold      I:alg/filter/binary/impl/ImplThresholdImageOps.java:46-134
//   GLOBAL_OTSU    GlobalBinaryFilter.Otsu, GThresholdImageOps.computeOtsu         I:alg/filter/binary/GThresholdImageOps.java:56-142
//   LOCAL_MEAN     ImplThresholdImageOps.localMean                                 :226-270 (GrayU8), :424-468 (GrayF32)
//   LOCAL_GAUSSIAN ImplThresholdImageOps.localGaussian                             :272-323, :470-520
//   BLOCK_*        ThresholdBlock + ThresholdBlockMinMax_* / Mean_* / Otsu         I:alg/filter/binary/ThresholdBlock.java:90-170
// and the GrayU8 blurs the local forms are made of (BlurImageOps.mean / gaussian on GrayU8, I:alg/filter/blur/BlurImageOps.java:75-141).
//
// Every streaming kernel gives a lane 16 (GrayU8) or 4 (GrayF32) neighbouring pixels of a row: one 16-byte load, and one 16- or 4-byte store,
// where all of them are inside the image, single elements at the right edge.  Views start anywhere (gfx950 global memory takes unaligned vector
// accesses), and only the width x height pixels of an output view are stored.
//
// GrayU8 blurs.  ImplConvolveMean, ConvolveImageNoBorder with a divisor, ConvolveNormalized_JustBorder_SB and ConvolveNormalizedNaive_SB all
// evaluate, for an output pixel, (total + weight/2) / weight over the taps inside the image, weight = the sum of those taps (the all-ones
// table kernel for the mean), in int arithmetic with a GrayU8 image between the two passes.  Integer sums are order free, so one formula
// covers the interior, the border and the kernel-wider-than-the-image forms.
// ---------------------------------------------------------------------------------------------------------------
#include "common.h"
#include <cfloat>
#include <climits>
#include <algorithm>

// Java's (int) of a double: NaN -> 0, saturating
__host__ __device__ static inline int javaD2I(double v) {
	if (v != v) return 0;
	if (v >= 2147483647.0) return INT_MAX;
	if (v <= -2147483648.0) return INT_MIN;
	return (int)v;
}

// ---- the pixels of a lane: 16 neighbouring GrayU8 pixels (one 16-byte load, one 16-byte store) or 4 GrayF32 pixels (16-byte load, 4-byte store) ----
template <class T> struct PixT;
template <> struct PixT<uint8_t> { using type = int; static constexpr int N = 16; };
template <> struct PixT<float> { using type = float; static constexpr int N = 4; };

__device__ __forceinline__ void loadLane(const uint8_t* p, int n, int v[16]) {
	if (n >= 16) {
		uint4 q;
		__builtin_memcpy(&q, p, 16);
		const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
		for (int j = 0; j < 16; j++) v[j] = (w[j >> 2] >> (8 * (j & 3))) & 255;
	} else
		for (int j = 0; j < 16; j++) v[j] = j < n ? p[j] : 0;
}
__device__ __forceinline__ void loadLane(const float* p, int n, float v[4]) {
	if (n >= 4) {
		float4 w;
		__builtin_memcpy(&w, p, 16);
		v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
	} else
		for (int j = 0; j < 4; j++) v[j] = j < n ? p[j] : 0.0f;
}
// N 0/1 (or byte) results of a lane
template <int N>
__device__ __forceinline__ void storeLane(uint8_t* p, int n, const int v[N]) {
	if (n >= N) {
		uint32_t w[N / 4];
#pragma unroll
		for (int j = 0; j < N / 4; j++) w[j] = (uint32_t)v[4 * j] | ((uint32_t)v[4 * j + 1] << 8) | ((uint32_t)v[4 * j + 2] << 16) | ((uint32_t)v[4 * j + 3] << 24);
		__builtin_memcpy(p, w, N);
	} else
		for (int j = 0; j < n; j++) p[j] = (uint8_t)v[j];
}
template <class V>
__device__ __forceinline__ int cmpOut(V px, V thr, int mode) {
	return mode == BHIP_CMP_LE ? (px <= thr ? 1 : 0) : mode == BHIP_CMP_GT ? (px > thr ? 1 : 0) : (px <= thr ? 0 : 1);
}

// grid of the streaming kernels: x covers the row in lanes of N pixels, y strides over the rows, z is the image
template <class T>
static inline dim3 streamGrid(int width, int height, int batch) {
	return dim3((width + 256 * PixT<T>::N - 1) / (256 * PixT<T>::N), std::min(height, 1024), batch);
}

// ---------------------------------------------------------------------------------------------------------------
// FIXED, and the apply pass of GLOBAL_OTSU (imageThr: one int per image, computed on the device)
// ---------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void k_thresh_global(const T* __restrict__ in, long long inImageStride, int inStride, uint8_t* __restrict__ out,
													   long long outImageStride, int outStride, int width, int height, typename PixT<T>::type thr,
													   const int* __restrict__ imageThr, int mode) {
	using V = typename PixT<T>::type;
	constexpr int N = PixT<T>::N;
	const int x = (blockIdx.x * 256 + threadIdx.x) * N;
	if (x >= width) return;
	if (imageThr) thr = (V)imageThr[blockIdx.z];
	const int n = width - x;
	const T* src = in + (long long)blockIdx.z * inImageStride + x;
	uint8_t* dst = out + (long long)blockIdx.z * outImageStride + x;
	for (int y = blockIdx.y; y < height; y += gridDim.y) {
		V v[N];
		int o[N];
		loadLane(src + (long long)y * inStride, n, v);
#pragma unroll
		for (int j = 0; j < N; j++) o[j] = cmpOut<V>(v[j], thr, mode);
		storeLane<N>(dst + (long long)y * outStride, n, o);
	}
}
template <class T>
static int launchThresholdGlobal(bhip_ctx* ctx, DevImg<const T> in, DevImg<uint8_t> out, typename PixT<T>::type thr, const int* imageThr, int mode) {
	ProfScope prof(ctx, sizeof(T) == 1 ? "k_thresh_global_u8" : "k_thresh_global_f32", (sizeof(T) + 1.0) * in.width * in.height * in.batch);
	hipLaunchKernelGGL(k_thresh_global<T>, streamGrid<T>(in.width, in.height, in.batch), dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data,
					   out.imageStride, out.stride, in.width, in.height, thr, imageThr, mode);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
int bhip_launch_threshold_global(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<uint8_t> out, int thr, const int* imageThr, int mode) {
	return launchThresholdGlobal<uint8_t>(ctx, in, out, thr, imageThr, mode);
}
int bhip_launch_threshold_global(bhip_ctx* ctx, DevImg<const float> in, DevImg<uint8_t> out, float thr, const int* imageThr, int mode) {
	return launchThresholdGlobal<float>(ctx, in, out, thr, imageThr, mode);
}

// ImageStatistics.histogram(GrayU8, minValue, int[length]), length <= 256: counts per workgroup in LDS, then one global add per bin that was
// hit (hist[batch][length] zeroed by the caller).  A value outside [minValue, minValue + length) is dropped (the reference throws)
__global__ __launch_bounds__(256) void k_hist_u8(const uint8_t* __restrict__ in, long long inImageStride, int inStride, int width, int height, int minValue,
												 int length, int* __restrict__ hist) {
	__shared__ int h[256];
	h[threadIdx.x] = 0;
	__syncthreads();
	const int x = (blockIdx.x * 256 + threadIdx.x) * 16;
	if (x < width) {
		const int n = width - x;
		const uint8_t* src = in + (long long)blockIdx.z * inImageStride + x;
		for (int y = blockIdx.y; y < height; y += gridDim.y) {
			int v[16];
			loadLane(src + (long long)y * inStride, n, v);
#pragma unroll
			for (int j = 0; j < 16; j++)
				if (j < n && (unsigned)(v[j] - minValue) < (unsigned)length) atomicAdd(&h[v[j] - minValue], 1);
		}
	}
	__syncthreads();
	if ((int)threadIdx.x < length && h[threadIdx.x]) atomicAdd(&hist[(long long)blockIdx.z * length + threadIdx.x], h[threadIdx.x]);
}
int bhip_launch_hist_u8(bhip_ctx* ctx, DevImg<const uint8_t> in, int* hist, int minValue, int length) {
	ProfScope prof(ctx, "k_hist_u8", 1.0 * in.width * in.height * in.batch);
	dim3 grid((in.width + 4095) / 4096, std::min(in.height, 128), in.batch);
	hipLaunchKernelGGL(k_hist_u8, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, in.width, in.height, minValue, length, hist);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
// GThresholdImageOps.computeOtsu(int[], 256, width*height) (:105-142, its own loop) and GlobalBinaryFilter.process (:57-62):
// thr[image] = (int)(otsu * scale), `scale` already turned into 1/scale (or 0) by the caller when thresholding up
__global__ __launch_bounds__(64) void k_otsu_global(const int* __restrict__ hist, int totalPixels, double scale, int* __restrict__ thr) {
	if (threadIdx.x != 0) return;
	const int* histogram = hist + blockIdx.x * 256;
	const int length = 256;
	const double dlength = length;
	double sum = 0;
	for (int i = 0; i < length; i++) sum += (i / dlength) * histogram[i];
	double sumB = 0;
	int wB = 0;
	double varMax = 0;
	int threshold = 0;
	for (int i = 0; i < length; i++) {
		wB += histogram[i];
		if (wB == 0) continue;
		const int wF = totalPixels - wB;
		if (wF == 0) break;
		sumB += (i / dlength) * histogram[i];
		const double mB = sumB / wB;
		const double mF = (sum - sumB) / wF;
		const double varBetween = (double)wB * (double)wF * (mB - mF) * (mB - mF);
		if (varBetween > varMax) {
			varMax = varBetween;
			threshold = i;
		}
	}
	thr[blockIdx.x] = javaD2I((double)threshold * scale);
}
int bhip_launch_otsu_global(bhip_ctx* ctx, const int* hist, int batch, int totalPixels, double scale, int* thr) {
	hipLaunchKernelGGL(k_otsu_global, dim3(batch), dim3(64), 0, ctx->stream, hist, totalPixels, scale, thr);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// compare against a blurred image: the tail of localMean / localGaussian.  down: px <= blur * scale; up: px * scale > blur, in float
// ---------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void k_local_compare(const T* __restrict__ in, long long inImageStride, int inStride, const T* __restrict__ blur,
													   long long blurImageStride, int blurStride, uint8_t* __restrict__ out, long long outImageStride,
													   int outStride, int width, int height, float scale, int down) {
	using V = typename PixT<T>::type;
	constexpr int N = PixT<T>::N;
	const int x = (blockIdx.x * 256 + threadIdx.x) * N;
	if (x >= width) return;
	const int n = width - x;
	const T* src = in + (long long)blockIdx.z * inImageStride + x;
	const T* bl = blur + (long long)blockIdx.z * blurImageStride + x;
	uint8_t* dst = out + (long long)blockIdx.z * outImageStride + x;
	for (int y = blockIdx.y; y < height; y += gridDim.y) {
		V v[N], m[N];
		int o[N];
		loadLane(src + (long long)y * inStride, n, v);
		loadLane(bl + (long long)y * blurStride, n, m);
#pragma unroll
		for (int j = 0; j < N; j++) o[j] = down ? ((float)v[j] <= (float)m[j] * scale ? 1 : 0) : ((float)v[j] * scale > (float)m[j] ? 1 : 0);
		storeLane<N>(dst + (long long)y * outStride, n, o);
	}
}
template <class T>
int bhip_launch_local_compare(bhip_ctx* ctx, DevImg<const T> in, DevImg<const T> blur, DevImg<uint8_t> out, float scale, bool down) {
	ProfScope prof(ctx, sizeof(T) == 1 ? "k_local_compare_u8" : "k_local_compare_f32", (2.0 * sizeof(T) + 1.0) * in.width * in.height * in.batch);
	hipLaunchKernelGGL(k_local_compare<T>, streamGrid<T>(in.width, in.height, in.batch), dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, blur.data,
					   blur.imageStride, blur.stride, out.data, out.imageStride, out.stride, in.width, in.height, scale, down ? 1 : 0);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_local_compare<uint8_t>(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, DevImg<uint8_t>, float, bool);
template int bhip_launch_local_compare<float>(bhip_ctx*, DevImg<const float>, DevImg<const float>, DevImg<uint8_t>, float, bool);

// ---------------------------------------------------------------------------------------------------------------
// GrayU8 blurs.  taps == nullptr: the all-ones kernel of the mean.
// ---------------------------------------------------------------------------------------------------------------
// One direction, any radius: a lane computes one pixel from the taps inside the image.  The path for radii beyond the fused kernel and for
// kernels wider than the image.
template <bool VERTICAL>
__global__ __launch_bounds__(256) void k_blur_u8_pass(const uint8_t* __restrict__ in, long long inImageStride, int inStride, uint8_t* __restrict__ out,
													  long long outImageStride, int outStride, int width, int height, const int32_t* __restrict__ taps, int radius) {
	const int x = blockIdx.x * 256 + threadIdx.x;
	if (x >= width) return;
	const uint8_t* src = in + (long long)blockIdx.z * inImageStride;
	for (int y = blockIdx.y; y < height; y += gridDim.y) {
		const int pos = VERTICAL ? y : x, extent = VERTICAL ? height : width;
		const int lo = std::max(pos - radius, 0), hi = std::min(pos + radius, extent - 1);
		int total = 0, weight = 0;
		for (int p = lo; p <= hi; p++) {
			const int w = taps ? taps[p - pos + radius] : 1;
			const int v = VERTICAL ? src[(long long)p * inStride + x] : src[(long long)y * inStride + p];
			total += v * w;
			weight += w;
		}
		out[(long long)blockIdx.z * outImageStride + (long long)y * outStride + x] = (uint8_t)((total + weight / 2) / weight);
	}
}
int bhip_launch_blur_u8_pass(bhip_ctx* ctx, bool vertical, const int32_t* devTaps, int radius, DevImg<const uint8_t> in, DevImg<uint8_t> out) {
	ProfScope prof(ctx, vertical ? "k_blur_u8_cols" : "k_blur_u8_rows", 2.0 * in.width * in.height * in.batch);
	dim3 grid((in.width + 255) / 256, std::min(in.height, 32768), in.batch);
	if (vertical)
		hipLaunchKernelGGL(k_blur_u8_pass<true>, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width,
						   in.height, devTaps, radius);
	else
		hipLaunchKernelGGL(k_blur_u8_pass<false>, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width,
						   in.height, devTaps, radius);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// Both directions in one launch, radius <= BHIP_THRESH_FUSED_MAX_RADIUS: a workgroup stages a FT_W x FT_H tile with its halo in LDS (zero
// outside the image: such taps add nothing to a total, and the weight comes from the clipped tap range), takes the horizontal pass to bytes
// in LDS for every tile row and halo row, then the vertical pass, then -- COMPARE -- the local threshold's compare, and stores.  One read of
// the input (plus halo) and one write.  LDS: (FT_H + 2R) x (FT_W + 2R) + (FT_H + 2R) x FT_W bytes = 6 + 4 KiB at R = 16.
// Both passes give a lane four neighbouring pixels and read LDS in 4-byte words; the taps and their prefix sums are kernel arguments, so a
// tap (the same for every lane) comes from the scalar side.
#define FT_W 64
#define FT_H 32
#define FT_R BHIP_THRESH_FUSED_MAX_RADIUS
#define FT_PITCH (FT_W + 2 * FT_R)
struct FusedTaps {
	int k[2 * FT_R + 1];     // Kernel1D_S32 taps
	int pre[2 * FT_R + 2];   // pre[i] = k[0] + ... + k[i-1]
};
// (total + weight/2) / weight for 0 <= total + weight/2 < 2^24 with rcp ~ 1 / weight: the float quotient is within one of the integer one
__device__ __forceinline__ int divRound(int total, int weight, float rcp) {
	const int n = total + weight / 2;
	int q = (int)((float)n * rcp);
	const int r = n - q * weight;
	if (r < 0) q--;
	else if (r >= weight) q++;
	return q;
}
template <bool COMPARE>
__global__ __launch_bounds__(256) void k_blur_u8_fused(const uint8_t* __restrict__ in, long long inImageStride, int inStride, uint8_t* __restrict__ out,
													   long long outImageStride, int outStride, int width, int height, FusedTaps taps, int radius, float scale,
													   int down) {
	__shared__ __attribute__((aligned(16))) uint8_t tile[(FT_H + 2 * FT_R) * FT_PITCH];
	__shared__ __attribute__((aligned(16))) uint8_t hbuf[(FT_H + 2 * FT_R) * FT_W];
	const int tid = threadIdx.x;
	const int kw = 2 * radius + 1;
	const int x0 = blockIdx.x * FT_W, y0 = blockIdx.y * FT_H;
	const uint8_t* src = in + (long long)blockIdx.z * inImageStride;
	// stage: rows y0 - radius .. y0 + FT_H + radius, columns x0 - radius .. x0 + FT_W + radius, four columns per lane and step
	const int rows = FT_H + 2 * radius, quads = (FT_W + 2 * radius + 3) / 4;
	for (int i = tid; i < rows * quads; i += 256) {
		const int ry = i / quads, q = i - ry * quads;
		const int gy = y0 - radius + ry, gx = x0 - radius + 4 * q;
		uint32_t w = 0;
		if (gy >= 0 && gy < height) {
			const uint8_t* p = src + (long long)gy * inStride + gx;
			if (gx >= 0 && gx + 3 < width) __builtin_memcpy(&w, p, 4);
			else
				for (int j = 0; j < 4; j++)
					if (gx + j >= 0 && gx + j < width) w |= (uint32_t)p[j] << (8 * j);
		}
		*reinterpret_cast<uint32_t*>(&tile[ry * FT_PITCH + 4 * q]) = w;
	}
	__syncthreads();
	// horizontal pass: hbuf[ry][lx .. lx+3] for every staged row; rows and columns outside the image hold 0.  Output j of the lane takes tap
	// t = c - j from the byte at tile column lx + c
	const int hwords = (kw + 3 + 3) / 4;
	for (int i = tid; i < rows * (FT_W / 4); i += 256) {
		const int ry = i / (FT_W / 4), lx = (i - ry * (FT_W / 4)) * 4;
		const int gy = y0 - radius + ry, gx = x0 + lx;
		uint32_t res = 0;
		if (gy >= 0 && gy < height && gx < width) {
			int total[4] = {0, 0, 0, 0};
			const uint8_t* t = &tile[ry * FT_PITCH + lx];
			for (int wi = 0; wi < hwords; wi++) {
				const uint32_t w = *reinterpret_cast<const uint32_t*>(t + 4 * wi);
#pragma unroll
				for (int b = 0; b < 4; b++) {
					const int v = (w >> (8 * b)) & 255, c = 4 * wi + b;
#pragma unroll
					for (int j = 0; j < 4; j++) {
						const int tap = c - j;
						const int coef = tap >= 0 && tap < kw ? taps.k[tap] : 0;   // uniform
						total[j] += v * coef;
					}
				}
			}
#pragma unroll
			for (int j = 0; j < 4; j++) {
				if (gx + j >= width) break;
				const int weight = taps.pre[min(kw, width - (gx + j) + radius)] - taps.pre[max(0, radius - (gx + j))];
				res |= (uint32_t)divRound(total[j], weight, __builtin_amdgcn_rcpf((float)weight)) << (8 * j);
			}
		}
		*reinterpret_cast<uint32_t*>(&hbuf[ry * FT_W + lx]) = res;
	}
	__syncthreads();
	// vertical pass, four pixels of a row per lane
	uint8_t* dst = out + (long long)blockIdx.z * outImageStride;
	for (int i = tid; i < FT_H * (FT_W / 4); i += 256) {
		const int ly = i / (FT_W / 4), lx = (i - ly * (FT_W / 4)) * 4;
		const int gy = y0 + ly, gx = x0 + lx;
		if (gy >= height || gx >= width) continue;
		int total[4] = {0, 0, 0, 0};
		for (int k = 0; k < kw; k++) {
			const uint32_t w = *reinterpret_cast<const uint32_t*>(&hbuf[(ly + k) * FT_W + lx]);
			const int c = taps.k[k];
			total[0] += (int)(w & 255) * c; total[1] += (int)((w >> 8) & 255) * c; total[2] += (int)((w >> 16) & 255) * c; total[3] += (int)(w >> 24) * c;
		}
		const int weight = taps.pre[min(kw, height - gy + radius)] - taps.pre[max(0, radius - gy)];
		const float rcp = __builtin_amdgcn_rcpf((float)weight);
		int o[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int m = divRound(total[j], weight, rcp);
			if (COMPARE) {
				const int px = tile[(ly + radius) * FT_PITCH + lx + radius + j];
				o[j] = down ? ((float)px <= (float)m * scale ? 1 : 0) : ((float)px * scale > (float)m ? 1 : 0);
			} else
				o[j] = m;
		}
		storeLane<4>(dst + (long long)gy * outStride + gx, width - gx, o);
	}
}
// hostTaps: the 2*radius+1 Kernel1D_S32 taps in host memory, nullptr = the mean
int bhip_launch_blur_u8_fused(bhip_ctx* ctx, const int32_t* hostTaps, int radius, DevImg<const uint8_t> in, DevImg<uint8_t> out, bool compare, float scale, bool down) {
	if (radius < 1 || radius > FT_R) return bhip_fail(ctx, BHIP_ERR_INVALID, "fused GrayU8 blur radius");
	FusedTaps taps{};
	for (int i = 0; i < 2 * radius + 1; i++) {
		taps.k[i] = hostTaps ? hostTaps[i] : 1;
		taps.pre[i + 1] = taps.pre[i] + taps.k[i];
	}
	if (255LL * taps.pre[2 * radius + 1] + taps.pre[2 * radius + 1] / 2 >= (1 << 24)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "kernel sum beyond the fused GrayU8 blur");
	const double halo = (double)(FT_W + 2 * radius) * (FT_H + 2 * radius) / (FT_W * FT_H);
	ProfScope prof(ctx, compare ? "k_local_u8_fused" : "k_blur_u8_fused", (1.0 + halo) * in.width * in.height * in.batch);
	dim3 grid((in.width + FT_W - 1) / FT_W, (in.height + FT_H - 1) / FT_H, in.batch);
	if (compare)
		hipLaunchKernelGGL(k_blur_u8_fused<true>, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width,
						   in.height, taps, radius, scale, down ? 1 : 0);
	else
		hipLaunchKernelGGL(k_blur_u8_fused<false>, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width,
						   in.height, taps, radius, scale, down ? 1 : 0);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Block thresholds, three stages.  Block (bx, by) of the nbx x nby stats grid covers x in [bx*bw, bx == nbx-1 ? width : (bx+1)*bw) and the
// same in y: the last block of a direction takes the remainder (ThresholdBlock.process / computeStatistics :90-170).
//   1. statistics per block: min/max, mean or a 256-bin histogram
//   2. one record per block from the 3x3 neighbourhood of statistics clipped at the grid's border (or the block alone)
//   3. a streaming apply pass: pixel -> block -> record
// ---------------------------------------------------------------------------------------------------------------
struct BlockGeom {
	int width, height, bw, bh, nbx, nby;
};
struct BlockRec {
	int thr;      // the threshold: an int, or the bits of a float
	int always;   // ThresholdBlockMinMax's textureless block: every pixel is 1
};
__device__ __forceinline__ void blockRect(const BlockGeom& g, int bx, int by, int& x0, int& y0, int& w, int& h) {
	x0 = bx * g.bw; y0 = by * g.bh;
	w = (bx == g.nbx - 1 ? g.width : x0 + g.bw) - x0;
	h = (by == g.nby - 1 ? g.height : y0 + g.bh) - y0;
}
__device__ __forceinline__ int waveSum(int v) {
	for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

// stage 1, min / max: one wave per block (a workgroup of four waves with four blocks measured 10 % slower here, 5 % faster for the histograms).  The reference starts from min = max = pixel(x0, y0) and walks `if (v < min) .. else if (v > max)`:
// the true extrema for integers; for floats the extrema of the values that are not NaN, unless the first pixel is NaN, which then stays in both.
template <class T>
__global__ __launch_bounds__(64) void k_block_minmax(const T* __restrict__ in, long long inImageStride, int inStride, BlockGeom g, typename PixT<T>::type* __restrict__ stats) {
	using V = typename PixT<T>::type;
	const int blk = blockIdx.x, lane = threadIdx.x;
	const int bx = blk % g.nbx, by = blk / g.nbx;
	int x0, y0, w, h;
	blockRect(g, bx, by, x0, y0, w, h);
	const T* src = in + (long long)blockIdx.z * inImageStride + (long long)y0 * inStride + x0;
	const V first = (V)src[0];
	V mn = first, mx = first;
	for (int i = lane; i < w * h; i += 64) {
		const int yy = i / w, xx = i - yy * w;
		const V v = (V)src[(long long)yy * inStride + xx];
		if (v < mn) mn = v;
		if (v > mx) mx = v;
	}
	for (int d = 32; d > 0; d >>= 1) {
		const V a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
		if (a < mn) mn = a;
		if (b > mx) mx = b;
	}
	if (lane == 0) {
		V* s = stats + ((long long)blockIdx.z * g.nbx * g.nby + blk) * 2;
		s[0] = mn; s[1] = mx;   // first is NaN: no comparison above was true, both are still NaN
	}
}
// stage 1, GrayU8 mean: int sum, (int)(scale*sum/(w*h) + 0.5) in double, stored as a byte (wraps above 255) and read back & 0xFF
__global__ __launch_bounds__(64) void k_block_mean_u8(const uint8_t* __restrict__ in, long long inImageStride, int inStride, BlockGeom g, double scale, int* __restrict__ stats) {
	const int blk = blockIdx.x, lane = threadIdx.x;
	const int bx = blk % g.nbx, by = blk / g.nbx;
	int x0, y0, w, h;
	blockRect(g, bx, by, x0, y0, w, h);
	const uint8_t* src = in + (long long)blockIdx.z * inImageStride + (long long)y0 * inStride + x0;
	int sum = 0;
	for (int i = lane; i < w * h; i += 64) {
		const int yy = i / w, xx = i - yy * w;
		sum += src[(long long)yy * inStride + xx];
	}
	sum = waveSum(sum);
	if (lane == 0) stats[(long long)blockIdx.z * g.nbx * g.nby + blk] = javaD2I(scale * sum / (w * h) + 0.5) & 0xFF;
}
// stage 1, GrayF32 mean: `sum += pixel` in raster order over the block is the one order-sensitive sum, so a block is one lane's serial chain
// (neighbouring lanes walk neighbouring blocks of a block row, so a wave's loads of one step fall into a few cache lines)
__global__ __launch_bounds__(64) void k_block_mean_f32(const float* __restrict__ in, long long inImageStride, int inStride, BlockGeom g, float scale, float* __restrict__ stats) {
	const int blk = blockIdx.x * 64 + threadIdx.x;
	if (blk >= g.nbx * g.nby) return;
	const int bx = blk % g.nbx, by = blk / g.nbx;
	int x0, y0, w, h;
	blockRect(g, bx, by, x0, y0, w, h);
	const float* src = in + (long long)blockIdx.z * inImageStride + (long long)y0 * inStride + x0;
	float sum = 0;
	for (int yy = 0; yy < h; yy++) {
		const float* r = src + (long long)yy * inStride;
		for (int xx = 0; xx < w; xx++) sum += r[xx];
	}
	stats[(long long)blockIdx.z * g.nbx * g.nby + blk] = scale * sum / (float)(w * h);
}
// stage 1, Otsu: 256-bin int histogram of a block, counted in LDS by one wave (four waves, four blocks per workgroup)
__global__ __launch_bounds__(256) void k_block_hist(const uint8_t* __restrict__ in, long long inImageStride, int inStride, BlockGeom g, int* __restrict__ stats) {
	__shared__ int hists[4][256];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	int* hist = hists[wave];
	for (int i = lane; i < 256; i += 64) hist[i] = 0;
	__syncthreads();
	const int blk = blockIdx.x * 4 + wave;
	const bool live = blk < g.nbx * g.nby;
	if (live) {
		const int bx = blk % g.nbx, by = blk / g.nbx;
		int x0, y0, w, h;
		blockRect(g, bx, by, x0, y0, w, h);
		const uint8_t* src = in + (long long)blockIdx.z * inImageStride + (long long)y0 * inStride + x0;
		for (int i = lane; i < w * h; i += 64) {
			const int yy = i / w, xx = i - yy * w;
			atomicAdd(&hist[src[(long long)yy * inStride + xx]], 1);
		}
	}
	__syncthreads();
	if (!live) return;
	int* s = stats + ((long long)blockIdx.z * g.nbx * g.nby + blk) * 256;
	for (int i = lane; i < 256; i += 64) s[i] = hist[i];
}

struct BlockRecParams {
	int kind;   // BHIP_THRESHOLD_BLOCK_MIN_MAX / _MEAN
	int local, down;
	double scale, minimumSpread;
};
__device__ __forceinline__ void neighbourhood(const BlockGeom& g, int local, int bx, int by, int& bx0, int& by0, int& bx1, int& by1) {
	if (local) {
		bx1 = std::min(g.nbx - 1, bx + 1); by1 = std::min(g.nby - 1, by + 1);
		bx0 = std::max(0, bx - 1); by0 = std::max(0, by - 1);
	} else {
		bx0 = bx1 = bx; by0 = by1 = by;
	}
}
// stage 2, min / max and mean: one lane per block, the neighbourhood in block raster order
template <class T>
__global__ __launch_bounds__(64) void k_block_record(BlockGeom g, BlockRecParams p, const typename PixT<T>::type* __restrict__ stats, BlockRec* __restrict__ rec) {
	using V = typename PixT<T>::type;
	const int blk = blockIdx.x * 64 + threadIdx.x;
	if (blk >= g.nbx * g.nby) return;
	const int bx = blk % g.nbx, by = blk / g.nbx;
	int bx0, by0, bx1, by1;
	neighbourhood(g, p.local, bx, by, bx0, by0, bx1, by1);
	const V* s = stats + (long long)blockIdx.z * g.nbx * g.nby * (p.kind == BHIP_THRESHOLD_BLOCK_MIN_MAX ? 2 : 1);
	BlockRec r;
	r.always = 0;
	if (p.kind == BHIP_THRESHOLD_BLOCK_MIN_MAX) {
		if constexpr (std::is_same_v<T, uint8_t>) {
			int mn = INT_MAX, mx = -INT_MAX;
			for (int y = by0; y <= by1; y++)
				for (int x = bx0; x <= bx1; x++) {
					const int lmn = s[(y * g.nbx + x) * 2], lmx = s[(y * g.nbx + x) * 2 + 1];
					if (lmn < mn) mn = lmn;
					if (lmx > mx) mx = lmx;
				}
			r.always = mx - mn <= javaD2I(p.minimumSpread) ? 1 : 0;
			r.thr = javaD2I(p.scale * ((mx + mn) / 2));
		} else {
			float mn = FLT_MAX, mx = -FLT_MAX;
			for (int y = by0; y <= by1; y++)
				for (int x = bx0; x <= bx1; x++) {
					const float lmn = s[(y * g.nbx + x) * 2], lmx = s[(y * g.nbx + x) * 2 + 1];
					if (lmn < mn) mn = lmn;
					if (lmx > mx) mx = lmx;
				}
			r.always = mx - mn <= (float)p.minimumSpread ? 1 : 0;
			r.thr = __float_as_int((float)p.scale * (mx + mn) / 2.0f);
		}
	} else {
		const int count = (by1 - by0 + 1) * (bx1 - bx0 + 1);
		V mean = 0;
		for (int y = by0; y <= by1; y++)
			for (int x = bx0; x <= bx1; x++) mean += s[y * g.nbx + x];
		if constexpr (std::is_same_v<T, uint8_t>) r.thr = mean / count;
		else r.thr = __float_as_int(mean / (float)count);
	}
	rec[(long long)blockIdx.z * g.nbx * g.nby + blk] = r;
}
// stage 2, Otsu: one wave per block sums the neighbourhood's histograms (integer counts: order free) and evaluates ComputeOtsu.compute
// (I:alg/filter/binary/ComputeOtsu.java:71-170).  The reference's loop carries wB, a count, and sumB = sum of (i / 256.0) * histogram[i]: every
// term is a multiple of 1/256 below 2^32, so every partial sum is exact in double whatever the order, and sumB at bin i is S_i / 256.0 with the
// integer prefix sum S_i = sum of j * histogram[j], j <= i.  With both as prefix scans, varBetween of a bin is the reference's expression on
// the reference's operands, evaluated by the lane that owns the bin; the loop's `continue` (wB == 0) and `break` (wF == 0) drop exactly the
// bins dropped here, and its strict `>` keeps the first bin of the largest value: the argmax below with the smaller bin on ties.
__global__ __launch_bounds__(256) void k_block_otsu(BlockGeom g, int local, int down, int useOtsu2, double tuning, double scale, const int* __restrict__ stats,
													BlockRec* __restrict__ rec) {
	const int blk = blockIdx.x * 4 + (threadIdx.x >> 6);   // four waves, four blocks
	if (blk >= g.nbx * g.nby) return;
	const int bx = blk % g.nbx, by = blk / g.nbx;
	int bx0, by0, bx1, by1;
	neighbourhood(g, local, bx, by, bx0, by0, bx1, by1);
	const int* s = stats + (long long)blockIdx.z * g.nbx * g.nby * 256;
	const int lane = threadIdx.x & 63, i0 = 4 * lane;   // the lane owns bins i0 .. i0+3
	int h[4] = {0, 0, 0, 0};
	for (int y = by0; y <= by1; y++)
		for (int x = bx0; x <= bx1; x++) {
			const int4 v = *reinterpret_cast<const int4*>(s + (long long)(y * g.nbx + x) * 256 + i0);
			h[0] += v.x; h[1] += v.y; h[2] += v.z; h[3] += v.w;
		}
	// inclusive prefix sums of the counts (wB) and of bin * count (S) over the 256 bins
	int wB[4];
	long long S[4];
	wB[0] = h[0]; S[0] = (long long)i0 * h[0];
#pragma unroll
	for (int j = 1; j < 4; j++) { wB[j] = wB[j - 1] + h[j]; S[j] = S[j - 1] + (long long)(i0 + j) * h[j]; }
	int cw = wB[3];
	long long cs = S[3];
	for (int d = 1; d < 64; d <<= 1) {
		const int a = __shfl_up(cw, d);
		const long long b = __shfl_up(cs, d);
		if (lane >= d) { cw += a; cs += b; }
	}
	const int totalPixels = __shfl(cw, 63);
	const long long Sall = __shfl(cs, 63);
	const int offW = cw - wB[3];
	const long long offS = cs - S[3];
	const double dlength = 256.0;
	const double sum = (double)Sall / dlength;
	double best = 0, bestMB = 0, bestMF = 0;   // the reference starts from variance = 0 (selectedMB = selectedMF = 0) and takes strictly larger values only
	int bestI = 256;                           // 256: no bin
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const int w = offW + wB[j];
		const int wF = totalPixels - w;
		if (w == 0 || wF == 0) continue;
		const double sumB = (double)(offS + S[j]) / dlength;
		const double mB = sumB / w;
		const double mF = (sum - sumB) / wF;
		const double varBetween = (double)w * (double)wF * (mB - mF) * (mB - mF);
		if (varBetween > best) { best = varBetween; bestI = i0 + j; bestMB = mB; bestMF = mF; }
	}
	for (int d = 32; d > 0; d >>= 1) {
		const double ob = __shfl_xor(best, d), omb = __shfl_xor(bestMB, d), omf = __shfl_xor(bestMF, d);
		const int oi = __shfl_xor(bestI, d);
		if (ob > best || (ob == best && oi < bestI)) { best = ob; bestI = oi; bestMB = omb; bestMF = omf; }
	}
	if (lane != 0) return;
	double variance = best;
	double threshold = useOtsu2 ? 256 * (bestMB + bestMF) / 2.0 : (bestI < 256 ? bestI : 0);
	variance += 0.001;
	const int adjustment = javaD2I(tuning * threshold * tuning * threshold / variance + 0.5);
	threshold += down ? -adjustment : adjustment;
	threshold = javaD2I(scale * (threshold > 0 ? threshold : 0) + 0.5);   // Math.max(threshold, 0)
	BlockRec r;
	r.thr = (int)threshold;
	r.always = 0;
	rec[(long long)blockIdx.z * g.nbx * g.nby + blk] = r;
}
// stage 3
template <class T>
__global__ __launch_bounds__(256) void k_block_apply(const T* __restrict__ in, long long inImageStride, int inStride, uint8_t* __restrict__ out, long long outImageStride,
													 int outStride, BlockGeom g, const BlockRec* __restrict__ rec, int mode) {
	using V = typename PixT<T>::type;
	constexpr int N = PixT<T>::N;
	const int x = (blockIdx.x * 256 + threadIdx.x) * N;
	if (x >= g.width) return;
	const int n = g.width - x;
	const T* src = in + (long long)blockIdx.z * inImageStride + x;
	uint8_t* dst = out + (long long)blockIdx.z * outImageStride + x;
	const BlockRec* rb = rec + (long long)blockIdx.z * g.nbx * g.nby;
	const int bxFirst = min(x / g.bw, g.nbx - 1);
	const int left = bxFirst == g.nbx - 1 ? g.width : (bxFirst + 1) * g.bw;   // where the lane's first block ends
	for (int y = blockIdx.y; y < g.height; y += gridDim.y) {
		const BlockRec* row = rb + min(y / g.bh, g.nby - 1) * g.nbx;
		V v[N];
		int o[N];
		loadLane(src + (long long)y * inStride, n, v);
		int bx = bxFirst, end = left;
		BlockRec r = row[bx];
#pragma unroll
		for (int j = 0; j < N; j++) {
			if (x + j >= end && bx < g.nbx - 1) {
				bx++;
				end = bx == g.nbx - 1 ? g.width : end + g.bw;
				r = row[bx];
			}
			V thr;
			if constexpr (std::is_same_v<T, uint8_t>) thr = r.thr;
			else thr = __int_as_float(r.thr);
			o[j] = r.always ? 1 : cmpOut<V>(v[j], thr, mode);
		}
		storeLane<N>(dst + (long long)y * outStride, n, o);
	}
}

size_t bhip_block_threshold_scratch(int kind, int nbx, int nby, int images) {
	const size_t blocks = (size_t)nbx * nby * images;
	const size_t stats = kind == BHIP_THRESHOLD_BLOCK_OTSU ? 1024 : kind == BHIP_THRESHOLD_BLOCK_MIN_MAX ? 8 : 4;
	return ((blocks * sizeof(BlockRec) + 15) & ~(size_t)15) + blocks * stats;   // the records, then the statistics from a 16-byte boundary
}
// Scratch: bhip_block_threshold_scratch(kind, nbx, nby, chunk) bytes, where `chunk` <= batch images are in flight at a time (the Otsu
// histograms are 1 KiB per block, so a large batch goes through in several rounds of the three stages).
template <class T>
int bhip_launch_block_threshold(bhip_ctx* ctx, const ThreshBlocks& c, DevImg<const T> in, DevImg<uint8_t> out, void* scratch, int chunk) {
	using V = typename PixT<T>::type;
	const BlockGeom g{in.width, in.height, c.bw, c.bh, c.nbx, c.nby};
	const int nb = c.nbx * c.nby;
	const bool up = !c.down;
	for (int b0 = 0; b0 < in.batch; b0 += chunk) {
		const int nimg = std::min(chunk, in.batch - b0);
		const T* src = in.data + (long long)b0 * in.imageStride;
		uint8_t* dst = out.data + (long long)b0 * out.imageStride;
		BlockRec* rec = (BlockRec*)scratch;
		void* stats = (char*)scratch + (((size_t)nb * chunk * sizeof(BlockRec) + 15) & ~(size_t)15);
		int mode = up ? BHIP_CMP_NOT_LE : BHIP_CMP_LE;
		if (c.kind == BHIP_THRESHOLD_BLOCK_OTSU) {
			if constexpr (std::is_same_v<T, uint8_t>) {
				{
					ProfScope prof(ctx, "k_block_hist", 1.0 * in.width * in.height * nimg + 1024.0 * nb * nimg);
					hipLaunchKernelGGL(k_block_hist, dim3((nb + 3) / 4, 1, nimg), dim3(256), 0, ctx->stream, src, in.imageStride, in.stride, g, (int*)stats);
				}
				ProfScope prof(ctx, "k_block_otsu", 1024.0 * 9 * nb * nimg);
				hipLaunchKernelGGL(k_block_otsu, dim3((nb + 3) / 4, 1, nimg), dim3(256), 0, ctx->stream, g, c.local, c.down, c.useOtsu2, c.tuning, c.scale, (const int*)stats, rec);
			} else
				return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "BLOCK_OTSU is GrayU8 only");
		} else {
			if (c.kind == BHIP_THRESHOLD_BLOCK_MIN_MAX) {
				ProfScope prof(ctx, "k_block_minmax", (double)sizeof(T) * in.width * in.height * nimg);
				hipLaunchKernelGGL(k_block_minmax<T>, dim3(nb, 1, nimg), dim3(64), 0, ctx->stream, src, in.imageStride, in.stride, g, (V*)stats);
				if (up) mode = BHIP_CMP_GT;
			} else {
				ProfScope prof(ctx, "k_block_mean", (double)sizeof(T) * in.width * in.height * nimg);
				if constexpr (std::is_same_v<T, uint8_t>)
					hipLaunchKernelGGL(k_block_mean_u8, dim3(nb, 1, nimg), dim3(64), 0, ctx->stream, src, in.imageStride, in.stride, g, c.scale, (int*)stats);
				else
					hipLaunchKernelGGL(k_block_mean_f32, dim3((nb + 63) / 64, 1, nimg), dim3(64), 0, ctx->stream, src, in.imageStride, in.stride, g, (float)c.scale,
									   (float*)stats);
			}
			const BlockRecParams p{c.kind, c.local, c.down, c.scale, c.minimumSpread};
			hipLaunchKernelGGL(k_block_record<T>, dim3((nb + 63) / 64, 1, nimg), dim3(64), 0, ctx->stream, g, p, (const V*)stats, rec);
		}
		ProfScope prof(ctx, sizeof(T) == 1 ? "k_block_apply_u8" : "k_block_apply_f32", (sizeof(T) + 1.0) * in.width * in.height * nimg);
		hipLaunchKernelGGL(k_block_apply<T>, streamGrid<T>(in.width, in.height, nimg), dim3(256), 0, ctx->stream, src, in.imageStride, in.stride, dst, out.imageStride,
						   out.stride, g, rec, mode);
		BHIP_HIP(ctx, hipGetLastError());
	}
	return BHIP_OK;
}
template int bhip_launch_block_threshold<uint8_t>(bhip_ctx*, const ThreshBlocks&, DevImg<const uint8_t>, DevImg<uint8_t>, void*, int);
template int bhip_launch_block_threshold<float>(bhip_ctx*, const ThreshBlocks&, DevImg<const float>, DevImg<uint8_t>, void*, int);
