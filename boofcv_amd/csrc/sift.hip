// SIFT detector: the scale space and the DoG extrema.  All fp32 / fp64 with the reference's evaluation order and no FMA contraction.
//
// Reference:
//   SiftScaleSpace.initialize / computeOctaveScales / applyGaussian   F:alg/feature/detect/interest/SiftScaleSpace.java:170-245
//   PyramidOps.scaleImageUp / scaleDown2                              I:alg/transform/pyramid/impl/ImplPyramidOps.java:44-85
//     ImplBilinearPixel_F32.get (EXTENDED)                            I:alg/interpolate/impl/ImplBilinearPixel_F32.java:48-90
//   ConvolveImageNormalized.horizontal / vertical                     I:alg/filter/convolve/ConvolveImageNormalized.java:48-93 (expressions: ip_dev.h)
//   SiftDetector.detectFeatures / isScaleSpaceExtremum / processFeatureCandidate / isEdge   F:alg/feature/detect/interest/SiftDetector.java:199-331
//     ConvolveImageSparse.horizontal / vertical / convolve            I:alg/filter/convolve/ConvolveImageSparse.java:41-80
//     KernelMath.convolve1D_F32 / convolve2D                          I:alg/filter/kernel/KernelMath.java:142-166, 338-356
//     FastHessianFeatureDetector.polyPeak(float)                      F:alg/feature/detect/interest/FastHessianFeatureDetector.java:336-350
//   NonMaxLimiter.process (the QuickSelect cut)                       F:abst/feature/detect/extract/NonMaxLimiter.java:80-83
// The order QuickSelect leaves is unpinned against the ddogleg jar (the routine is the project's restatement, select_dev.h); the kept set is
// pinned whenever no two |value| around the cut are equal.
//
// k_sift_level, one scale level in one launch: a 256-lane workgroup takes a 64 x 64 tile of the level.  It stages the source tile with the
// kernel's reach on every side in LDS (16-byte loads), forms the horizontally filtered rows -- the float values the reference stores in
// tempBlur, border columns with the re-normalised expression -- into a second LDS plane, filters those vertically, and writes octave[i] and
// dog[i-1] = octave[i] - octave[i-1], the centre tap coming from the staged tile.  Geometry and LDS budget: DESIGN.md.
#include "ip_dev.h"
#include "select_dev.h"

// ---------------- the small kernels: one pixel per lane, any strides ----------------
__global__ __launch_bounds__(256) void k_sift_u8_to_f32(const uint8_t* __restrict__ in, long long inImageStride, int inStride, float* __restrict__ out,
														   long long outImageStride, int outStride, int width) {
	const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
	if (x >= width) return;
	out[(long long)blockIdx.z * outImageStride + (long long)y * outStride + x] = (float)in[(long long)blockIdx.z * inImageStride + (long long)y * inStride + x];
}

// out(x, y) = interp.get(x * fdiv, y * fdiv), fdiv = 1 / (float)scale.  The coordinates are finite and >= 0, so get_fast and get_border are
// one expression: floor is truncation, and a clamped read is the plain read wherever get_fast is taken (x <= width - 2)
__global__ __launch_bounds__(256) void k_sift_scale_up(const float* __restrict__ in, long long inImageStride, int inStride, int inWidth, int inHeight,
														  float* __restrict__ out, long long outImageStride, int outStride, int outWidth, float fdiv) {
	const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
	if (x >= outWidth) return;
	const float sx = (float)x * fdiv, sy = (float)y * fdiv;
	const int xt = (int)sx, yt = (int)sy;
	const float ax = sx - (float)xt, ay = sy - (float)yt;
	const int x0 = min(xt, inWidth - 1), x1 = min(xt + 1, inWidth - 1), y0 = min(yt, inHeight - 1), y1 = min(yt + 1, inHeight - 1);
	const float* img = in + (long long)blockIdx.z * inImageStride;
	const float p00 = img[(long long)y0 * inStride + x0], p10 = img[(long long)y0 * inStride + x1];
	const float p11 = img[(long long)y1 * inStride + x1], p01 = img[(long long)y1 * inStride + x0];
	float val = (1.0f - ax) * (1.0f - ay) * p00;
	val += ax * (1.0f - ay) * p10;
	val += ax * ay * p11;
	val += (1.0f - ax) * ay * p01;
	out[(long long)blockIdx.z * outImageStride + (long long)y * outStride + x] = val;
}

__global__ __launch_bounds__(256) void k_sift_scale_down2(const float* __restrict__ in, long long inImageStride, int inStride, float* __restrict__ out,
															 long long outImageStride, int outStride, int outWidth) {
	const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
	if (x >= outWidth) return;
	out[(long long)blockIdx.z * outImageStride + (long long)y * outStride + x] = in[(long long)blockIdx.z * inImageStride + (long long)(2 * y) * inStride + 2 * x];
}

__global__ __launch_bounds__(256) void k_sift_subtract(const float* __restrict__ a, long long aImageStride, int aStride, const float* __restrict__ b,
														  long long bImageStride, int bStride, float* __restrict__ out, long long outImageStride, int outStride, int width) {
	const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
	if (x >= width) return;
	out[(long long)blockIdx.z * outImageStride + (long long)y * outStride + x] =
		a[(long long)blockIdx.z * aImageStride + (long long)y * aStride + x] - b[(long long)blockIdx.z * bImageStride + (long long)y * bStride + x];
}

static int siftGrid(bhip_ctx* ctx, int width, int height, int batch, dim3& grid) {
	if (batch > 65535 || height > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "SIFT on the GPU: at most 65535 frames and rows per call");
	grid = dim3((width + 255) / 256, height, batch);
	return BHIP_OK;
}

int bhip_launch_sift_u8_to_f32(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<float> out) {
	dim3 grid;
	BHIP_TRY(siftGrid(ctx, in.width, in.height, in.batch, grid));
	ProfScope prof(ctx, "k_sift_u8_to_f32", 5.0 * in.width * in.height * in.batch);
	hipLaunchKernelGGL(k_sift_u8_to_f32, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

int bhip_launch_sift_scale_up(bhip_ctx* ctx, DevImg<const float> in, DevImg<float> out, int scale) {
	dim3 grid;
	BHIP_TRY(siftGrid(ctx, out.width, out.height, in.batch, grid));
	ProfScope prof(ctx, "k_sift_scale_up", 4.0 * ((double)in.width * in.height + (double)out.width * out.height) * in.batch);
	hipLaunchKernelGGL(k_sift_scale_up, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, in.width, in.height, out.data, out.imageStride, out.stride,
					   out.width, 1 / (float)scale);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

int bhip_launch_sift_scale_down2(bhip_ctx* ctx, DevImg<const float> in, DevImg<float> out) {
	dim3 grid;
	BHIP_TRY(siftGrid(ctx, out.width, out.height, in.batch, grid));
	ProfScope prof(ctx, "k_sift_scale_down2", 8.0 * out.width * out.height * in.batch);
	hipLaunchKernelGGL(k_sift_scale_down2, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, out.width);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

int bhip_launch_sift_subtract(bhip_ctx* ctx, DevImg<const float> a, DevImg<const float> b, DevImg<float> out) {
	dim3 grid;
	BHIP_TRY(siftGrid(ctx, a.width, a.height, a.batch, grid));
	ProfScope prof(ctx, "k_sift_subtract", 12.0 * a.width * a.height * a.batch);
	hipLaunchKernelGGL(k_sift_subtract, grid, dim3(256), 0, ctx->stream, a.data, a.imageStride, a.stride, b.data, b.imageStride, b.stride, out.data, out.imageStride,
					   out.stride, a.width);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------- k_sift_level ----------------
#define SL_TW BHIP_SIFT_TILE_W
#define SL_TH BHIP_SIFT_TILE_H
static_assert(SL_TW == 64 && SL_TH == 64, "k_sift_level: a lane per tile column, four waves of 16 tile rows each");

struct SiftLevelParams {
	const float* in;
	float* out;
	float* dog;
	long long inImageStride, outImageStride, dogImageStride;
	int inStride, outStride, dogStride, width, height;
	float k[BHIP_SIFT_FUSED_MAX_TAPS];
};

// the reference's interior expression for KW taps: the unrolled widths 3 .. 11 assign the first product (blurTapsInterior), the standard
// form of every other width adds it to 0 (convOne)
template <int KW>
__device__ __forceinline__ float siftTapsInterior(const float (&v)[KW], const float* k) {
	if constexpr (KW <= 11) {
		return blurTapsInterior<KW>(v, k);
	} else {
		float total = 0.0f + v[0] * k[0];
#pragma unroll
		for (int i = 1; i < KW; i++) total += v[i] * k[i];
		return total;
	}
}

template <int KW>
__global__ __launch_bounds__(256) void k_sift_level(SiftLevelParams P) {
	constexpr int R = KW / 2, PADL = (R + 3) & ~3, SW = SL_TW + 2 * PADL, ROWS = SL_TH + KW - 1;
	__shared__ __attribute__((aligned(16))) float src[ROWS * SW];   // source rows y0 - R .., columns x0 - PADL ..; 0 outside the image
	__shared__ float hf[ROWS * SL_TW];                              // tempBlur of the same rows, columns x0 ..
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int x0 = blockIdx.x * SL_TW, y0 = blockIdx.y * SL_TH;
	const int W = P.width, H = P.height;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	// stage: 16-byte chunks, consecutive lanes take consecutive chunks of a row
	constexpr int CH = SW / 4;
	for (int c = threadIdx.x; c < ROWS * CH; c += 256) {
		const int r = c / CH, q = c - r * CH;
		const int y = y0 - R + r;
		float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (y >= 0 && y < H) v = loadRow4(img + (long long)y * P.inStride, x0 - PADL + 4 * q, W);
		*reinterpret_cast<float4*>(src + r * SW + 4 * q) = v;
	}
	__syncthreads();
	// horizontal: lane = tile column, wave w takes tile rows w, w + 4, ...
	const int gx = x0 + lane;
	if (gx < W) {
		const bool interiorX = gx >= R && gx < W - R;
		for (int r = wave; r < ROWS; r += 4) {
			const int y = y0 - R + r;
			if (y < 0 || y >= H) continue;
			const float* s = src + r * SW + PADL - R + lane;
			float v[KW];
#pragma unroll
			for (int i = 0; i < KW; i++) v[i] = s[i];
			hf[r * SL_TW + lane] = interiorX ? siftTapsInterior<KW>(v, P.k) : blurTapsBorder<KW>(v, P.k, gx - R, W);
		}
	}
	__syncthreads();
	if (gx >= W) return;
	// vertical: wave w takes tile rows 16 w .. 16 w + 15 of its column, four at a time out of one register window
	float* outImg = P.out + (long long)blockIdx.z * P.outImageStride;
	float* dogImg = P.dog + (long long)blockIdx.z * P.dogImageStride;
#pragma unroll 1
	for (int g = 0; g < 4; g++) {
		const int t0 = wave * 16 + g * 4;   // first tile row of the group
		if (y0 + t0 >= H) break;
		float col[KW + 3];
#pragma unroll
		for (int i = 0; i < KW + 3; i++) col[i] = hf[(t0 + i) * SL_TW + lane];
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const int y = y0 + t0 + q;
			if (y >= H) break;
			float v[KW];
#pragma unroll
			for (int i = 0; i < KW; i++) v[i] = col[q + i];
			const float val = (y >= R && y < H - R) ? siftTapsInterior<KW>(v, P.k) : blurTapsBorder<KW>(v, P.k, y - R, H);
			outImg[(long long)y * P.outStride + gx] = val;
			dogImg[(long long)y * P.dogStride + gx] = val - src[(t0 + q + R) * SW + PADL + lane];
		}
	}
}

int bhip_launch_sift_level(bhip_ctx* ctx, const float* kernel, int kw, DevImg<const float> in, DevImg<float> out, DevImg<float> dog, bool* done) {
	*done = false;
	const int width = in.width, height = in.height, batch = in.batch;
	if (kw < 3 || kw > BHIP_SIFT_FUSED_MAX_TAPS || kw % 2 == 0 || kw >= width || kw >= height) return BHIP_OK;   // the naive form included
	if (!vec4(in) || batch > 65535 || (height + SL_TH - 1) / SL_TH > 65535) return BHIP_OK;
	ConvParams N;   // the kernel as ConvolveImageNormalized uses it (re-normalised when its sum is off by more than 1e-4)
	N.kw = kw;
	for (int i = 0; i < kw; i++) N.k[i] = kernel[i];
	setNormalizedMode(N, std::min(width, height));
	SiftLevelParams P;
	P.in = in.data; P.out = out.data; P.dog = dog.data;
	P.inImageStride = in.imageStride; P.outImageStride = out.imageStride; P.dogImageStride = dog.imageStride;
	P.inStride = in.stride; P.outStride = out.stride; P.dogStride = dog.stride; P.width = width; P.height = height;
	for (int i = 0; i < BHIP_SIFT_FUSED_MAX_TAPS; i++) P.k[i] = i < kw ? N.k[i] : 0.0f;
	const dim3 grid((width + SL_TW - 1) / SL_TW, (height + SL_TH - 1) / SL_TH, batch);
	ProfScope prof(ctx, "k_sift_level", 12.0 * width * height * batch);
	switch (kw) {
#define SL_CASE(KWT) case KWT: hipLaunchKernelGGL(k_sift_level<KWT>, grid, dim3(256), 0, ctx->stream, P); break
		SL_CASE(3); SL_CASE(5); SL_CASE(7); SL_CASE(9); SL_CASE(11); SL_CASE(13); SL_CASE(15); SL_CASE(17); SL_CASE(19); SL_CASE(21); SL_CASE(23); SL_CASE(25);
		SL_CASE(27);
#undef SL_CASE
	}
	BHIP_HIP(ctx, hipGetLastError());
	*done = true;
	return BHIP_OK;
}

// ---------------- candidates ----------------
struct SiftRec {
	double x, y, scale;
	int px, py;
	bool white;
};

// FastHessianFeatureDetector.polyPeak(float)
__device__ __forceinline__ float siftPolyPeak(float lower, float middle, float upper) {
	const float a = 0.5f * lower - middle + 0.5f * upper;
	const float b = 0.5f * upper - 0.5f * lower;
	if (a == 0.0f) return 0.0f;
	return -b / (2.0f * a);
}

// entries of frame b's list after the cut
__device__ __forceinline__ int siftListLength(const SiftCandParams& P, int b, int& nMin) {
	nMin = min(P.nMin[b], P.listCap);
	const int n = nMin + min(P.nMax[b], P.listCap);
	return (P.sel && n > P.maxFeatures) ? P.maxFeatures : n;
}

// entry i of frame b's list through isScaleSpaceExtremum, isEdge and processFeatureCandidate: false when a test rejects it
__device__ bool siftEntry(const SiftCandParams& P, int b, int i, SiftRec& r) {
	int nMin;
	if (i >= siftListLength(P, b, nMin)) return false;
	const int e = P.sel ? P.sel[(long long)b * 2 * P.listCap + i] : i;
	const bool maximum = e >= nMin;
	const int16_t* p = maximum ? P.xyMax + ((long long)b * P.listCap + (e - nMin)) * 2 : P.xyMin + ((long long)b * P.listCap + e) * 2;
	const int x = p[0], y = p[1];
	const int W = P.width, H = P.height, S = P.stride;
	if (x <= 1 || y <= 1 || x >= W - 1 || y >= H - 1) return false;
	const float* lo = P.lower + (long long)b * P.imageStride;
	const float* tg = P.target + (long long)b * P.imageStride;
	const float* up = P.upper + (long long)b * P.imageStride;
	const float signAdj = maximum ? 1.0f : -1.0f;
	float value = tg[(long long)y * S + x];   // LocalExtreme.getValue(): the pixel, the sign put back
	value *= signAdj;
	for (int dy = -1; dy <= 1; dy++)
		for (int dx = -1; dx <= 1; dx++) {
			float v = lo[(long long)(y + dy) * S + x + dx];
			if (v * signAdj >= value) return false;
			v = up[(long long)(y + dy) * S + x + dx];
			if (v * signAdj >= value) return false;
		}
	// isEdge: the kernels of createSparseDerivatives with the zeros (and their signs) that KernelMath leaves, EXTENDED border
	const float kdd[5] = {1.0f, 0.0f, -2.0f, 0.0f, 1.0f};
	const float kxy[9] = {1.0f, -0.0f, -1.0f, -0.0f, 0.0f, 0.0f, -1.0f, 0.0f, 1.0f};
	auto ext = [&](int xx, int yy) { return tg[(long long)min(max(yy, 0), H - 1) * S + min(max(xx, 0), W - 1)]; };
	float fxx = 0, fyy = 0, fxy = 0;
	for (int t = 0; t < 5; t++) fxx += ext(x + t - 2, y) * kdd[t];
	for (int t = 0; t < 5; t++) fyy += ext(x, y + t - 2) * kdd[t];
	for (int t = 0; t < 3; t++)
		for (int u = 0; u < 3; u++) fxy += ext(x + u - 1, y + t - 1) * kxy[t * 3 + u];
	const double xx = fxx, xy = fxy, yy = fyy;
	const double Tr = xx + yy;
	const double det = xx * yy - xy * xy;
	if (det <= 0) return false;
	if (Tr * Tr >= P.edgeThreshold * det) return false;
	// processFeatureCandidate
	const float x0 = tg[(long long)y * S + x - 1] * signAdj, x2 = tg[(long long)y * S + x + 1] * signAdj;
	const float y0 = tg[(long long)(y - 1) * S + x] * signAdj, y2 = tg[(long long)(y + 1) * S + x] * signAdj;
	const float s0 = lo[(long long)y * S + x] * signAdj, s2 = up[(long long)y * S + x] * signAdj;
	r.x = P.pixelScaleToInput * (double)((float)x + siftPolyPeak(x0, value, x2));
	r.y = P.pixelScaleToInput * (double)((float)y + siftPolyPeak(y0, value, y2));
	const double sigmaInterp = siftPolyPeak(s0, value, s2);
	if (sigmaInterp < 0) r.scale = P.sigmaLower * (-sigmaInterp) + (1 + sigmaInterp) * P.sigmaTarget;
	else r.scale = P.sigmaUpper * sigmaInterp + (1 - sigmaInterp) * P.sigmaTarget;
	r.white = !maximum;
	r.px = x;
	r.py = y;
	return true;
}

// one lane per list entry; a wave's survivors are 64 bits (two words) of the frame's bitmap, every word of which this grid writes
__global__ __launch_bounds__(256) void k_sift_candidates(SiftCandParams P, unsigned int* __restrict__ bitmap, int words) {
	const int b = blockIdx.y;
	const int i = blockIdx.x * 256 + threadIdx.x;
	SiftRec r;
	const bool ok = siftEntry(P, b, i, r);
	const unsigned long long m = __ballot(ok);
	if ((threadIdx.x & 63) == 0) {
		unsigned int* bm = bitmap + (long long)b * words + (i >> 5);
		bm[0] = (unsigned int)m;
		bm[1] = (unsigned int)(m >> 32);
	}
}

// the survivors at their rank behind the frame's running count
__global__ __launch_bounds__(256) void k_sift_emit(SiftCandParams P, const unsigned int* __restrict__ bitmap, const unsigned int* __restrict__ prefix, int words) {
	const int b = blockIdx.y;
	const int i = blockIdx.x * 256 + threadIdx.x;
	const unsigned int word = bitmap[(long long)b * words + (i >> 5)];
	if (!((word >> (i & 31)) & 1u)) return;
	const long long pos = (long long)P.count[b] + prefix[(long long)b * words + (i >> 5)] + __popc(word & ((1u << (i & 31)) - 1u));
	if (pos >= P.cap) return;
	SiftRec r;
	if (!siftEntry(P, b, i, r)) return;   // (it passed in k_sift_candidates)
	const long long o = (long long)b * P.cap + pos;
	P.x[o] = r.x;
	P.y[o] = r.y;
	P.scale[o] = r.scale;
	P.white[o] = r.white ? 1 : 0;
	P.where[o * 4 + 0] = (int16_t)P.octave;
	P.where[o * 4 + 1] = (int16_t)P.j;
	P.where[o * 4 + 2] = (int16_t)r.px;
	P.where[o * 4 + 3] = (int16_t)r.py;
}

__global__ void k_sift_advance(int* __restrict__ count, const int* __restrict__ nPass, int batch) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b < batch) count[b] += nPass[b];
}

int bhip_launch_sift_candidates(bhip_ctx* ctx, const SiftCandParams& P, unsigned int* bitmap, unsigned int* prefix, int* nPass) {
	if (P.batch <= 0 || P.listCap <= 0) return BHIP_OK;
	if (P.batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "SIFT on the GPU: at most 65535 frames per call");
	const int blocks = (2 * P.listCap + 255) / 256;
	const int words = blocks * 8;
	{
		ProfScope prof(ctx, "k_sift_candidates");
		hipLaunchKernelGGL(k_sift_candidates, dim3(blocks, P.batch), dim3(256), 0, ctx->stream, P, bitmap, words);
	}
	BHIP_TRY(bhip_launch_word_prefix(ctx, bitmap, words, P.batch, prefix, nPass));
	{
		ProfScope prof(ctx, "k_sift_emit");
		hipLaunchKernelGGL(k_sift_emit, dim3(blocks, P.batch), dim3(256), 0, ctx->stream, P, bitmap, prefix, words);
		hipLaunchKernelGGL(k_sift_advance, dim3((P.batch + 255) / 256), dim3(256), 0, ctx->stream, P.count, nPass, P.batch);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// NonMaxLimiter.process :80-83, one wave per frame: keys -intensity = the pixel for a minimum and its negation for a maximum, then the
// sequential select on lane 0.  A list that is not cut keeps its order
__global__ __launch_bounds__(64) void k_sift_select(SiftCandParams P, float* __restrict__ keyBuf, int* __restrict__ selBuf) {
	const int b = blockIdx.x, lane = threadIdx.x;
	const int nMin = min(P.nMin[b], P.listCap), n = nMin + min(P.nMax[b], P.listCap);
	float* key = keyBuf + (long long)b * 2 * P.listCap;
	int* sel = selBuf + (long long)b * 2 * P.listCap;
	const float* tg = P.target + (long long)b * P.imageStride;
	const bool cut = n > P.maxFeatures;
	for (int i = lane; i < n; i += 64) {
		sel[i] = i;
		if (cut) {
			const int16_t* p = i >= nMin ? P.xyMax + ((long long)b * P.listCap + (i - nMin)) * 2 : P.xyMin + ((long long)b * P.listCap + i) * 2;
			const float v = tg[(long long)p[1] * P.stride + p[0]];
			key[i] = i >= nMin ? -v : v;   // LocalExtreme.intensity is -val for a minimum, val for a maximum; the key is its (exact) negation
		}
	}
	if (!cut) return;
	__threadfence_block();
	__builtin_amdgcn_wave_barrier();
	if (lane == 0) quickSelectIndexSeq(key, P.maxFeatures, n, sel);
}

int bhip_launch_sift_select(bhip_ctx* ctx, const SiftCandParams& P, float* key, int* sel) {
	if (P.batch <= 0 || P.listCap <= 0) return BHIP_OK;
	ProfScope prof(ctx, "k_sift_select");
	hipLaunchKernelGGL(k_sift_select, dim3(P.batch), dim3(64), 0, ctx->stream, P, key, sel);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
