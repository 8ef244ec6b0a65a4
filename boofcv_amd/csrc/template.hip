// Template matching intensity on GrayU8 / GrayF32: FactoryTemplateMatching.createIntensity(SUM_ABSOLUTE_DIFFERENCE | SUM_SQUARE_ERROR | NCC), with and without a mask.
//
// Reference (F: = main/boofcv-feature/src/main/java/boofcv/):
//   TemplateIntensityImage.process / processInner / processInnerMask   F:alg/feature/detect/template/TemplateIntensityImage.java:56-125
//   TemplateSumAbsoluteDifference.F32 / .U8                            F:alg/feature/detect/template/TemplateSumAbsoluteDifference.java:46-128
//   TemplateSumSquaredError.F32 / .U8                                  F:alg/feature/detect/template/TemplateSumSquaredError.java:46-144
//   TemplateNCC.F32 / .U8 (evaluate, evaluateMask, setupTemplate)      F:alg/feature/detect/template/TemplateNCC.java:54-274
//   FactoryTemplateMatching.createIntensity                            F:factory/feature/detect/template/FactoryTemplateMatching.java:47-99
//
// Image W x H, template tw x th: w = W-tw+1, h = H-th+1, bx0 = tw/2, by0 = th/2.  intensity[y+by0][x+bx0] = evaluate(x, y) for x < w, y < h, every
// other pixel of the W x H intensity image is 0 (k_template_border).  The arithmetic of evaluate, restated: include/boofhip.h,
// bhip_template_intensity_u8.  Every output pixel sees its template elements in the reference's order (rows outer, columns inner) with the
// reference's separate fp32 operations; the parallelism is across output pixels and the batch only.
//
// Kernel shape: a workgroup of 256 owns TPL_TW = 64 x TPL_TH = 16 output pixels of one image; a lane owns TPL_R = 4 horizontally adjacent ones.
// The template is walked in chunks of TPL_CH = 16 rows.  Per chunk the workgroup stages, as 32-bit elements (GrayU8 widened to int),
//   the image rows the chunk meets, TPL_TH + chunk - 1 of them, 64 + roundup4(tw) columns (zero outside the image: they only feed outputs that are not stored),
//   the chunk's template rows and mask rows (NCC: the template as T - templateMean, the mask as float),
// so the template height is not limited; the width is, by the staged row: tw <= BHIP_TEMPLATE_MAX_WIDTH = 160.  A lane slides an 8-element
// register window along each template row: per four template columns one 16-byte LDS read of the image (the 16 lanes of a tile row read 256
// contiguous bytes), one broadcast 16-byte read of the template and one of the mask feed 16 comparisons.  The accumulators stay in registers
// across chunks.  NCC walks the chunks twice (image sum, then imageSigma and top); its template statistics come from k_template_stats, one
// lane per template, sequential fp32 in the reference's order.
// LDS: image 31 * 224 * 4 = 27776 B, template and mask 16 * 160 * 4 = 10240 B each; 48256 B per workgroup, three workgroups per CU.
//
// Deviation from the reference: the masked process() of the reference leaves the border as an earlier call left it; here the whole intensity
// view is written on every call (the result of a freshly constructed object).
#include "common.h"

#define TPL_TW 64
#define TPL_TH 16
#define TPL_R 4
#define TPL_CH 16
#define TPL_TPITCH BHIP_TEMPLATE_MAX_WIDTH              // multiple of 4
#define TPL_IPITCH (TPL_TW + BHIP_TEMPLATE_MAX_WIDTH)   // 224: columns 4*tx + x + 7 <= 60 + (tw4 - 4) + 7 < 64 + tw4
#define TPL_IROWS (TPL_TH + TPL_CH - 1)

// UtilEjml.F_EPS = (float)Math.pow(2, -21) (EJML's definition; parity unpinned against the jar)
#define TPL_NCC_EPS 4.76837158203125e-07f

struct TplKernelParams {
	const void* img;
	long long iImageStride;
	int iStride, W, H;
	const void* tpl;
	long long tImageStride;   // 0: one template for the batch
	int tStride, tw, th;
	const void* mask;
	long long mImageStride;
	int mStride;
	const float* stats;       // NCC: [template][2] = templateMean, templateSigma
	float* out;
	long long oImageStride;
	int oStride;
};

template <bool U8> struct TplElem { typedef float type; };
template <> struct TplElem<true> { typedef int type; };
template <class E> struct TplVec4 { typedef float4 type; };
template <> struct TplVec4<int> { typedef int4 type; };

// per output pixel state; which members are live depends on the score
template <class E>
struct TplAcc {
	E row;         // SAD / SSE: rowTotal; NCC pass 0: the image sum
	float total;   // SAD / SSE: total; NCC: imageMean, set after pass 0
	float sigma, top;
};

// NCC stages the template and the mask as the 32-bit patterns of floats whatever E is
template <class E> __device__ __forceinline__ E tplBits(float f);
template <> __device__ __forceinline__ float tplBits<float>(float f) { return f; }
template <> __device__ __forceinline__ int tplBits<int>(float f) { return __float_as_int(f); }
__device__ __forceinline__ float tplFloat(float e) { return e; }
__device__ __forceinline__ float tplFloat(int e) { return __int_as_float(e); }

// one template element against one image element
template <int SCORE, bool U8, bool MASKED, int PASS, class E>
__device__ __forceinline__ void tplStep(TplAcc<E>& a, E v, E t, E m) {
	if constexpr (SCORE == BHIP_TEMPLATE_SAD) {
		if constexpr (U8) {
			// int rowTotal += m * |I - T| (both below 2^8: the 24-bit multiply is exact)
			if constexpr (MASKED) a.row += __mul24(m, (int)__builtin_amdgcn_sad_u8((unsigned int)v, (unsigned int)t, 0u));
			else a.row = (int)__builtin_amdgcn_sad_u8((unsigned int)v, (unsigned int)t, (unsigned int)a.row);
		} else {
			if constexpr (MASKED) a.row += m * fabsf(v - t);
			else a.row += fabsf(v - t);
		}
	} else if constexpr (SCORE == BHIP_TEMPLATE_SSE) {
		if constexpr (U8) {
			// |e| <= 255 and m <= 255: e * e < 2^16 and m * e * e < 2^24, so the 24-bit multiplies are exact and (m * e) * e = m * (e * e); it is the
			// row total that wraps in Java: added in unsigned arithmetic and read back as two's complement
			const int e = v - t;
			const unsigned int ee = (unsigned int)__mul24(e, e);
			if constexpr (MASKED) a.row = (int)((unsigned int)a.row + __umul24((unsigned int)m, ee));
			else a.row = (int)((unsigned int)a.row + ee);
		} else {
			const float e = v - t;
			if constexpr (MASKED) a.row += (m * e) * e;
			else a.row += e * e;
		}
	} else {
		if constexpr (PASS == 0) {
			if constexpr (U8) a.row = (int)((unsigned int)a.row + (unsigned int)v);
			else a.row += v;
		} else {
			// t = T - templateMean, m = (float)mask
			const float diff = (float)v - a.total;
			a.sigma += diff * diff;
			if constexpr (MASKED) a.top += (tplFloat(m) * diff) * tplFloat(t);
			else a.top += diff * tplFloat(t);
		}
	}
}

// rows r0 .. r0+rows-1, columns c0 .. c0+cols-1 of image `src` (W x H, row stride `stride`) into dst[row][col] (pitch TPL_IPITCH), widened to E; 0 outside
template <class T, class E>
__device__ __forceinline__ void tplStageImage(E* dst, const T* src, int stride, int W, int H, int r0, int rows, int c0, int cols) {
	for (int r = threadIdx.x >> 6; r < rows; r += 4) {
		const int gy = r0 + r;
		for (int c = threadIdx.x & 63; c < cols; c += 64) {
			const int gx = c0 + c;
			E v = 0;
			if (gy < H && gx < W) v = (E)src[(long long)gy * stride + gx];
			dst[r * TPL_IPITCH + c] = v;
		}
	}
}

template <int SCORE, bool U8, bool MASKED>
__global__ __launch_bounds__(256) void k_template_intensity(TplKernelParams P) {
	typedef typename TplElem<U8>::type E;
	typedef typename TplVec4<E>::type E4;
	typedef typename std::conditional<U8, uint8_t, float>::type T;
	constexpr bool NCC = SCORE == BHIP_TEMPLATE_NCC;
	__shared__ __attribute__((aligned(16))) E simg[TPL_IROWS * TPL_IPITCH];
	__shared__ __attribute__((aligned(16))) E stpl[TPL_CH * TPL_TPITCH];
	__shared__ __attribute__((aligned(16))) E smask[MASKED ? TPL_CH * TPL_TPITCH : 4];
	const int W = P.W, H = P.H, tw = P.tw, th = P.th;
	const int w = W - tw + 1, h = H - th + 1;
	const int tw4 = (tw + 3) & ~3;
	const long long b = blockIdx.z;
	const T* img = (const T*)P.img + b * P.iImageStride;
	const T* tpl = (const T*)P.tpl + b * P.tImageStride;
	const T* mask = MASKED ? (const T*)P.mask + b * P.mImageStride : nullptr;
	const int ox0 = blockIdx.x * TPL_TW, oy0 = blockIdx.y * TPL_TH;
	const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
	float tMean = 0.f, tSigma = 0.f;
	if constexpr (NCC) {
		const float* st = P.stats + (P.tImageStride ? 2 * b : 0);
		tMean = st[0];
		tSigma = st[1];
	}
	const float area = (float)(tw * th);
	TplAcc<E> acc[TPL_R];
#pragma unroll
	for (int r = 0; r < TPL_R; r++) { acc[r].row = 0; acc[r].total = 0.f; acc[r].sigma = 0.f; acc[r].top = 0.f; }

	auto walk = [&](auto passTag) {
		constexpr int PASS = decltype(passTag)::value;
		for (int j0 = 0; j0 < th; j0 += TPL_CH) {
			const int ch = min(TPL_CH, th - j0);
			__syncthreads();   // the previous chunk has been read
			tplStageImage<T, E>(simg, img, P.iStride, W, H, oy0 + j0, TPL_TH + ch - 1, ox0, TPL_TW + tw4);
			if (!(NCC && PASS == 0)) {
				for (int i = threadIdx.x; i < ch * tw4; i += 256) {
					const int r = i / tw4, c = i - r * tw4;
					E tv = 0, mv = 0;
					if (c < tw) {
						const T t = tpl[(long long)(j0 + r) * P.tStride + c];
						if constexpr (NCC) tv = tplBits<E>((float)t - tMean);
						else tv = (E)t;
						if constexpr (MASKED) {
							const T m = mask[(long long)(j0 + r) * P.mStride + c];
							if constexpr (NCC) mv = tplBits<E>((float)m);
							else mv = (E)m;
						}
					}
					stpl[r * TPL_TPITCH + c] = tv;
					if constexpr (MASKED) smask[r * TPL_TPITCH + c] = mv;
				}
			}
			__syncthreads();
			for (int j = 0; j < ch; j++) {
				const E* irow = simg + (ty + j) * TPL_IPITCH + TPL_R * tx;
				const E* trow = stpl + j * TPL_TPITCH;
				const E* mrow = smask + (MASKED ? j * TPL_TPITCH : 0);
				if constexpr (!NCC) {
#pragma unroll
					for (int r = 0; r < TPL_R; r++) acc[r].row = 0;
				}
				// four template columns from x on: win[0..3] = image columns 4*tx + x .., the next four are read here; `valid` of the columns exist
				E4 cur = *(const E4*)irow;
				auto group = [&](int x, auto validTag, int valid) {
					constexpr int VALID = decltype(validTag)::value;   // 4: all of them (the main loop), 0: `valid` < 4 of them (the tail)
					const E4 nxt = *(const E4*)(irow + x + 4);
					const E win[8] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z, nxt.w};
					E t[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0};
					if constexpr (!(NCC && PASS == 0)) {
						const E4 t4 = *(const E4*)(trow + x);
						t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w;
						if constexpr (MASKED) {
							const E4 m4 = *(const E4*)(mrow + x);
							m[0] = m4.x; m[1] = m4.y; m[2] = m4.z; m[3] = m4.w;
						}
					}
#pragma unroll
					for (int k = 0; k < (VALID ? 4 : 3); k++) {
						if (VALID || k < valid) {
#pragma unroll
							for (int r = 0; r < TPL_R; r++) tplStep<SCORE, U8, MASKED, PASS, E>(acc[r], win[r + k], t[k], m[k]);
						}
					}
					cur = nxt;
				};
				int x = 0;
#pragma unroll 2
				for (; x + 4 <= tw; x += 4) group(x, std::integral_constant<int, 4>(), 4);
				if (x < tw) group(x, std::integral_constant<int, 0>(), tw - x);
				if constexpr (SCORE == BHIP_TEMPLATE_SAD) {
#pragma unroll
					for (int r = 0; r < TPL_R; r++) acc[r].total += (float)acc[r].row;   // total += rowTotal
				} else if constexpr (SCORE == BHIP_TEMPLATE_SSE) {
					const float div = 255.0f * 255.0f;
#pragma unroll
					for (int r = 0; r < TPL_R; r++) acc[r].total += (float)acc[r].row / div;   // total += rowTotal / div
				}
			}
		}
	};

	walk(std::integral_constant<int, 0>());
	if constexpr (NCC) {
#pragma unroll
		for (int r = 0; r < TPL_R; r++) acc[r].total = (float)acc[r].row / area;   // imageMean = imageSum / area
		walk(std::integral_constant<int, 1>());
	}

	const int oy = oy0 + ty;
	if (oy >= h) return;
	float* o = P.out + b * P.oImageStride + (long long)(oy + th / 2) * P.oStride + tw / 2;
#pragma unroll
	for (int r = 0; r < TPL_R; r++) {
		const int ox = ox0 + TPL_R * tx + r;
		if (ox >= w) continue;
		float v = acc[r].total;
		if constexpr (NCC) {
			const float imageSigma = sqrtf(acc[r].sigma / area);
			v = acc[r].top / (TPL_NCC_EPS + imageSigma * tSigma);
		}
		o[ox] = v;
	}
}

// TemplateNCC.setupTemplate: one lane per template, sequential fp32
template <class T>
__global__ __launch_bounds__(64) void k_template_stats(const T* tpl, long long imageStride, int stride, int tw, int th, float* stats) {
	if (threadIdx.x != 0) return;
	const T* t = tpl + (long long)blockIdx.x * imageStride;
	const float area = (float)(tw * th);
	float mean = 0.f;
	for (int y = 0; y < th; y++)
		for (int x = 0; x < tw; x++) mean += (float)t[(long long)y * stride + x];
	mean /= area;
	float sigma = 0.f;
	for (int y = 0; y < th; y++)
		for (int x = 0; x < tw; x++) {
			const float diff = (float)t[(long long)y * stride + x] - mean;
			sigma += diff * diff;
		}
	stats[2 * blockIdx.x] = mean;
	stats[2 * blockIdx.x + 1] = sqrtf(sigma / area);
}

// the pixels TemplateIntensityImage.processInner never writes: 0
__global__ __launch_bounds__(256) void k_template_border(float* out, long long imageStride, int stride, int W, int H, int x0, int x1, int y0, int y1) {
	const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (x >= W || y >= H) return;
	if (x < x0 || x >= x1 || y < y0 || y >= y1) out[(long long)blockIdx.z * imageStride + (long long)y * stride + x] = 0.f;
}

size_t bhip_template_scratch(int batch) { return (size_t)batch * 2 * sizeof(float); }

template <int SCORE, class T>
static void tplLaunch(bhip_ctx* ctx, const TplKernelParams& P, dim3 grid, bool masked) {
	constexpr bool U8 = sizeof(T) == 1;
	if (masked) hipLaunchKernelGGL((k_template_intensity<SCORE, U8, true>), grid, dim3(256), 0, ctx->stream, P);
	else hipLaunchKernelGGL((k_template_intensity<SCORE, U8, false>), grid, dim3(256), 0, ctx->stream, P);
}

template <class T>
int bhip_launch_template_intensity(bhip_ctx* ctx, int score, DevImg<const T> img, DevImg<const T> tpl, DevImg<const T> mask, float* stats, DevImg<float> out) {
	const int W = img.width, H = img.height, batch = img.batch, tw = tpl.width, th = tpl.height;
	if (score < BHIP_TEMPLATE_SAD || score > BHIP_TEMPLATE_NCC || tw < 1 || th < 1 || tw > W || th > H || tw > BHIP_TEMPLATE_MAX_WIDTH || batch <= 0 ||
		(mask.data && (mask.width != tw || mask.height != th)) || (score == BHIP_TEMPLATE_NCC && !stats))
		return bhip_fail(ctx, BHIP_ERR_INVALID, "bhip_launch_template_intensity: outside the kernel's limits");
	const int w = W - tw + 1, h = H - th + 1;
	const bool shared = tpl.imageStride == 0;
	TplKernelParams P{img.data, img.imageStride, img.stride, W, H, tpl.data, tpl.imageStride, tpl.stride, tw, th, mask.data, mask.data ? mask.imageStride : 0,
					  mask.stride, stats, out.data, out.imageStride, out.stride};
	{
		ProfScope ps(ctx, "k_template_border", 0);
		hipLaunchKernelGGL(k_template_border, dim3((W + 63) / 64, (H + 3) / 4, batch), dim3(256), 0, ctx->stream, out.data, out.imageStride, out.stride, W, H, tw / 2,
						   tw / 2 + w, th / 2, th / 2 + h);
	}
	if (score == BHIP_TEMPLATE_NCC) {
		ProfScope ps(ctx, "k_template_stats", 0);
		hipLaunchKernelGGL(k_template_stats<T>, dim3(shared ? 1 : batch), dim3(64), 0, ctx->stream, tpl.data, tpl.imageStride, tpl.stride, tw, th, stats);
	}
	const dim3 grid((w + TPL_TW - 1) / TPL_TW, (h + TPL_TH - 1) / TPL_TH, batch);
	const double px = (double)W * H * batch, ops = (double)w * h * batch * tw * th;
	{
		static const char* const names[2][3] = {{"k_template_sad_f32", "k_template_sse_f32", "k_template_ncc_f32"}, {"k_template_sad_u8", "k_template_sse_u8", "k_template_ncc_u8"}};
		ProfScope ps(ctx, names[sizeof(T) == 1][score], (sizeof(T) + 4.0) * px, ops);
		if (score == BHIP_TEMPLATE_SAD) tplLaunch<BHIP_TEMPLATE_SAD, T>(ctx, P, grid, mask.data != nullptr);
		else if (score == BHIP_TEMPLATE_SSE) tplLaunch<BHIP_TEMPLATE_SSE, T>(ctx, P, grid, mask.data != nullptr);
		else tplLaunch<BHIP_TEMPLATE_NCC, T>(ctx, P, grid, mask.data != nullptr);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_template_intensity(bhip_ctx*, int, DevImg<const uint8_t>, DevImg<const uint8_t>, DevImg<const uint8_t>, float*, DevImg<float>);
template int bhip_launch_template_intensity(bhip_ctx*, int, DevImg<const float>, DevImg<const float>, DevImg<const float>, float*, DevImg<float>);
