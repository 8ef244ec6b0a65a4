// Image remap: ImageDistort<T,T> on single-band GrayU8 -> GrayU8 and GrayF32 -> GrayF32 with nearest-neighbour or bilinear interpolation.
//
// Reference (I: = main/boofcv-ip/src/main/java/boofcv/):
//   ImageDistortBasic_SB.applyAll / applyOnlyInside (+ mask)   I:alg/distort/ImageDistortBasic_SB.java:56-135
//   ImageDistortCache_SB.renderAll / applyOnlyInside (+ mask)  I:alg/distort/ImageDistortCache_SB.java:136-206
//   AssignPixelValue_SB.F32 / .I8                              I:alg/distort/AssignPixelValue_SB.java:31-59
//   ImplBilinearPixel_U8 / _F32 get, get_fast, get_border      I:alg/interpolate/impl/ImplBilinearPixel_U8.java:48-90, ImplBilinearPixel_F32.java:48-90
//   NearestNeighborPixel_U8 / _F32 get, get_border             I:alg/interpolate/impl/NearestNeighborPixel_U8.java:56-72, NearestNeighborPixel_F32.java:56-72
//   BorderIndex1D_Extend.getIndex, ImageBorder_S32.get, ImageBorderValue (value 0)   I:core/image/border/
//
// One kernel template k_distort<T, INTERP, COORD>: pixel type, interpolation and where the source coordinates come from (a map in memory, an
// affine model or a homography evaluated in the kernel).  The border rule, renderAll and the presence of a mask are workgroup-uniform
// run-time branches.
//
// Tile: a workgroup of 256 owns 64 columns x 16 rows of the crop of one destination image; a lane owns DIST_PX = 4 consecutive pixels of one
// row, 16 lanes side by side, so a wave covers 64 x 4 pixels.  The footprint in the source of a rotated or sheared tile is then about as
// compact as it can be (64 x 16 against 1024 x 1 for a row segment).  The four pixels of a lane start where the destination row's address is
// a multiple of 4 elements: whatever the crop, the base pointer and the stride are, the lanes inside the crop store one dword (GrayU8) or
// four dwords (GrayF32), and only the lanes cut by the crop's left or right edge store single elements.
//   map reads   the 4 entries of a lane are 32 consecutive bytes: two 16-byte loads when that address is 16-byte aligned, four 8-byte loads
//               when it is 8-byte aligned, scalars otherwise.
//   taps        a GrayU8 tap pair (xt, xt+1) is read as the two bytes it is, at any alignment, never as a dword around it: no read leaves
//               the source view.  The fast path is taken only for 0 <= sx <= sw-2 and 0 <= sy <= sh-2, positively stated, so that a NaN goes
//               to the border path, whose integer coordinates are clamped (EXTENDED) or tested (ZERO) before any read.
//   stores      renderAll = false: a lane with a skipped pixel stores the others one by one; a skipped pixel is never stored.
// LDS: none.
#include "common.h"

#define DIST_TW 64
#define DIST_TH 16
#define DIST_PX 4

enum { DIST_COORD_MAP = 0, DIST_COORD_AFFINE = 1, DIST_COORD_HOMOGRAPHY = 2 };

struct DistortParams {
	const void* src;
	long long sImageStride;
	int sStride, sw, sh;
	const float* map;            // DIST_COORD_MAP: [dh][dw] pairs (x, y); images mapImageStride floats apart (0: one map for the batch)
	long long mapImageStride;
	float c[9];                  // the model's coefficients
	int dw, x0, y0, x1, y1;      // destination width (the map's row length) and the crop
	int border, renderAll;
	void* dst;
	long long dImageStride;
	int dStride;
	uint8_t* mask;               // nullptr: no mask
	long long mImageStride;
	int mStride;
};

// Java's (int) of a float: NaN -> 0, saturating
__device__ __forceinline__ int distF2I(float v) {
	if (v >= 2147483648.0f) return 2147483647;
	if (v <= -2147483648.0f) return -2147483647 - 1;
	if (v != v) return 0;
	return (int)v;
}

// AffinePointOps_F32.transform / HomographyPointOps_F32.transform as include/boofhip.h defines them: every sum left to right
template <int COORD>
__device__ __forceinline__ void distModel(const float* c, int xi, int yi, float& sx, float& sy) {
	const float x = (float)xi, y = (float)yi;
	if constexpr (COORD == DIST_COORD_AFFINE) {
		sx = c[4] + c[0] * x + c[1] * y;
		sy = c[5] + c[2] * x + c[3] * y;
	} else {
		const float z = c[6] * x + c[7] * y + c[8];
		sx = (c[0] * x + c[1] * y + c[2]) / z;
		sy = (c[3] * x + c[4] * y + c[5]) / z;
	}
}

// ImageBorder_S32.get / ImageBorder_F32.get for any int coordinates: the pixel when inside, else the clamped pixel (EXTENDED) or 0 (ZERO)
template <class T>
__device__ __forceinline__ float distBorderGet(const T* img, int stride, int sw, int sh, int x, int y, int border) {
	if (border == BHIP_BORDER_EXTENDED) {
		x = min(max(x, 0), sw - 1);
		y = min(max(y, 0), sh - 1);
	} else if ((unsigned int)x >= (unsigned int)sw || (unsigned int)y >= (unsigned int)sh) {
		return 0.0f;
	}
	return (float)img[(long long)y * stride + x];
}

// the taps (x, y) and (x + 1, y) of a row, both inside the view: two adjacent elements at any alignment
__device__ __forceinline__ void distPair(const uint8_t* p, float& a, float& b) {
	unsigned short v;
	__builtin_memcpy(&v, p, 2);
	a = (float)(v & 255u);
	b = (float)(v >> 8);
}
__device__ __forceinline__ void distPair(const float* p, float& a, float& b) {
	a = p[0];
	b = p[1];
}

// InterpolatePixelS.get(sx, sy)
template <class T, int INTERP>
__device__ __forceinline__ float distGet(const T* img, int stride, int sw, int sh, float sx, float sy, int border) {
	if constexpr (INTERP == BHIP_INTERP_NEAREST_NEIGHBOR) {
		if (sx >= 0.0f && sy >= 0.0f && sx <= (float)(sw - 1) && sy <= (float)(sh - 1)) return (float)img[(long long)(int)sy * stride + (int)sx];
		return distBorderGet(img, stride, sw, sh, distF2I(floorf(sx)), distF2I(floorf(sy)), border);
	} else {
		float ax, ay, p00, p10, p11, p01;
		if (sx >= 0.0f && sy >= 0.0f && sx <= (float)(sw - 2) && sy <= (float)(sh - 2)) {   // get_fast
			const int xt = (int)sx, yt = (int)sy;
			ax = sx - (float)xt;
			ay = sy - (float)yt;
			const T* p = img + (long long)yt * stride + xt;
			distPair(p, p00, p10);
			distPair(p + stride, p01, p11);
		} else {                                                                          // get_border
			const float xf = floorf(sx), yf = floorf(sy);
			const int xt = distF2I(xf), yt = distF2I(yf);
			const int xt1 = (int)((unsigned int)xt + 1u), yt1 = (int)((unsigned int)yt + 1u);   // wraps outside the domain; still a tested coordinate
			ax = sx - xf;
			ay = sy - yf;
			p00 = distBorderGet(img, stride, sw, sh, xt, yt, border);
			p10 = distBorderGet(img, stride, sw, sh, xt1, yt, border);
			p11 = distBorderGet(img, stride, sw, sh, xt1, yt1, border);
			p01 = distBorderGet(img, stride, sw, sh, xt, yt1, border);
		}
		float val = (1.0f - ax) * (1.0f - ay) * p00;
		val += ax * (1.0f - ay) * p10;
		val += ax * ay * p11;
		val += (1.0f - ax) * ay * p01;
		return val;
	}
}

// AssignPixelValue_SB: F32 stores the float, I8 stores (byte)value
__device__ __forceinline__ float distAssign(float v, float*) { return v; }
__device__ __forceinline__ uint8_t distAssign(float v, uint8_t*) { return (uint8_t)(distF2I(v) & 255); }

// the elements p[0..3] of a lane whose bit is set in `on`: one vector store when all four are and p is aligned to it (a destination row always is, a mask row may be)
__device__ __forceinline__ void distStore4(uint8_t* p, const uint8_t* v, unsigned int on) {
	if (on == 15u && ((uintptr_t)p & 3) == 0) {
		*(unsigned int*)p = (unsigned int)v[0] | ((unsigned int)v[1] << 8) | ((unsigned int)v[2] << 16) | ((unsigned int)v[3] << 24);
	} else {
#pragma unroll
		for (int j = 0; j < DIST_PX; j++)
			if (on >> j & 1u) p[j] = v[j];
	}
}
__device__ __forceinline__ void distStore4(float* p, const float* v, unsigned int on) {
	if (on == 15u && ((uintptr_t)p & 15) == 0) {
		*(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
	} else {
#pragma unroll
		for (int j = 0; j < DIST_PX; j++)
			if (on >> j & 1u) p[j] = v[j];
	}
}

// map entries x .. x+3 of a row (m points at entry x); only called when all four are inside the map
__device__ __forceinline__ void distLoadMap4(const float* m, float* sx, float* sy) {
	const uintptr_t a = (uintptr_t)m;
	if ((a & 15) == 0) {
		const float4 u = ((const float4*)m)[0], v = ((const float4*)m)[1];
		sx[0] = u.x; sy[0] = u.y; sx[1] = u.z; sy[1] = u.w; sx[2] = v.x; sy[2] = v.y; sx[3] = v.z; sy[3] = v.w;
	} else if ((a & 7) == 0) {
#pragma unroll
		for (int j = 0; j < DIST_PX; j++) {
			const float2 u = ((const float2*)m)[j];
			sx[j] = u.x; sy[j] = u.y;
		}
	} else {
#pragma unroll
		for (int j = 0; j < DIST_PX; j++) {
			sx[j] = m[2 * j]; sy[j] = m[2 * j + 1];
		}
	}
}

template <class T, int INTERP, int COORD>
__global__ __launch_bounds__(256) void k_distort(DistortParams P) {
	const long long b = blockIdx.z;
	const int y = P.y0 + blockIdx.y * DIST_TH + (threadIdx.x >> 4);
	if (y >= P.y1) return;
	T* drow = (T*)P.dst + b * P.dImageStride + (long long)y * P.dStride;
	// the lane's first column: the row's address at xa is a multiple of 4 elements, xa <= x0 < xa + 4
	const int xa = P.x0 - (int)(((uintptr_t)(drow + P.x0) / sizeof(T)) & 3);
	const int x = xa + (blockIdx.x * (DIST_TW / DIST_PX) + (threadIdx.x & 15)) * DIST_PX;
	if (x >= P.x1) return;
	unsigned int in = 0;   // the lane's pixels inside the crop
#pragma unroll
	for (int j = 0; j < DIST_PX; j++)
		if (x + j >= P.x0 && x + j < P.x1) in |= 1u << j;

	float sx[DIST_PX], sy[DIST_PX];
	if constexpr (COORD == DIST_COORD_MAP) {
		const float* m = P.map + b * P.mapImageStride + 2 * ((long long)y * P.dw + x);
		if (in == 15u) {
			distLoadMap4(m, sx, sy);
		} else {
#pragma unroll
			for (int j = 0; j < DIST_PX; j++) {
				sx[j] = sy[j] = 0.0f;
				if (in >> j & 1u) { sx[j] = m[2 * j]; sy[j] = m[2 * j + 1]; }
			}
		}
	} else {
#pragma unroll
		for (int j = 0; j < DIST_PX; j++) distModel<COORD>(P.c, x + j, y, sx[j], sy[j]);
	}

	const T* img = (const T*)P.src + b * P.sImageStride;
	const float maxW = (float)(P.sw - 1), maxH = (float)(P.sh - 1);
	T val[DIST_PX];
	uint8_t inside[DIST_PX];
	unsigned int on = 0;   // the pixels to assign
#pragma unroll
	for (int j = 0; j < DIST_PX; j++) {
		const bool ins = sx[j] >= 0.0f && sx[j] <= maxW && sy[j] >= 0.0f && sy[j] <= maxH;
		inside[j] = ins ? 1 : 0;
		val[j] = 0;
		if ((in >> j & 1u) && (P.renderAll || ins)) {
			on |= 1u << j;
			val[j] = distAssign(distGet<T, INTERP>(img, P.sStride, P.sw, P.sh, sx[j], sy[j], P.border), (T*)nullptr);
		}
	}
	distStore4(drow + x, val, on);
	if (P.mask) distStore4(P.mask + b * P.mImageStride + (long long)y * P.mStride + x, inside, in);
}

// the map of a model: entry (x, y) of a dw x dh map = the model's (sx, sy); a lane writes the two entries of two neighbouring pixels
template <int COORD>
__global__ __launch_bounds__(256) void k_distort_build_map(DistortParams P, float* map, int dh) {
	const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 2, y = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (x >= P.dw || y >= dh) return;
	float* m = map + 2 * ((long long)y * P.dw + x);
	float sx0, sy0, sx1 = 0.0f, sy1 = 0.0f;
	distModel<COORD>(P.c, x, y, sx0, sy0);
	if (x + 1 < P.dw) distModel<COORD>(P.c, x + 1, y, sx1, sy1);
	if (x + 1 < P.dw && ((uintptr_t)m & 15) == 0) {
		*(float4*)m = make_float4(sx0, sy0, sx1, sy1);
	} else {
		m[0] = sx0; m[1] = sy0;
		if (x + 1 < P.dw) { m[2] = sx1; m[3] = sy1; }
	}
}

static int distCoeffCount(int model) { return model == BHIP_DISTORT_AFFINE ? 6 : model == BHIP_DISTORT_HOMOGRAPHY ? 9 : 0; }

int bhip_launch_distort_build_map(bhip_ctx* ctx, int model, const float* coeff, int dw, int dh, float* map) {
	DistortParams P{};
	for (int i = 0; i < distCoeffCount(model); i++) P.c[i] = coeff[i];
	P.dw = dw;
	const dim3 grid((dw + 127) / 128, (dh + 3) / 4);
	ProfScope ps(ctx, "k_distort_build_map", 8.0 * dw * dh);
	if (model == BHIP_DISTORT_AFFINE) hipLaunchKernelGGL(k_distort_build_map<DIST_COORD_AFFINE>, grid, dim3(256), 0, ctx->stream, P, map, dh);
	else hipLaunchKernelGGL(k_distort_build_map<DIST_COORD_HOMOGRAPHY>, grid, dim3(256), 0, ctx->stream, P, map, dh);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

template <class T, int INTERP>
static void distLaunch(int coord, dim3 grid, hipStream_t st, const DistortParams& P) {
	if (coord == DIST_COORD_MAP) hipLaunchKernelGGL((k_distort<T, INTERP, DIST_COORD_MAP>), grid, dim3(256), 0, st, P);
	else if (coord == DIST_COORD_AFFINE) hipLaunchKernelGGL((k_distort<T, INTERP, DIST_COORD_AFFINE>), grid, dim3(256), 0, st, P);
	else hipLaunchKernelGGL((k_distort<T, INTERP, DIST_COORD_HOMOGRAPHY>), grid, dim3(256), 0, st, P);
}

template <class T>
int bhip_launch_distort(bhip_ctx* ctx, DevImg<const T> src, const DistortCoords& co, const DistortCrop& crop, int interp, int border, int renderAll, DevImg<T> dst,
						DevImg<uint8_t> mask) {
	const int cw = crop.x1 - crop.x0, ch = crop.y1 - crop.y0;
	if (cw <= 0 || ch <= 0 || src.batch <= 0) return BHIP_OK;
	DistortParams P{};
	P.src = src.data; P.sImageStride = src.imageStride; P.sStride = src.stride; P.sw = src.width; P.sh = src.height;
	P.map = co.map; P.mapImageStride = co.mapImageStride;
	for (int i = 0; i < distCoeffCount(co.model); i++) P.c[i] = co.coeff[i];
	P.dw = dst.width; P.x0 = crop.x0; P.y0 = crop.y0; P.x1 = crop.x1; P.y1 = crop.y1;
	P.border = border; P.renderAll = renderAll;
	P.dst = dst.data; P.dImageStride = dst.imageStride; P.dStride = dst.stride;
	P.mask = mask.data; P.mImageStride = mask.imageStride; P.mStride = mask.stride;
	const int coord = co.model == BHIP_DISTORT_AFFINE ? DIST_COORD_AFFINE : co.model == BHIP_DISTORT_HOMOGRAPHY ? DIST_COORD_HOMOGRAPHY : DIST_COORD_MAP;
	// + DIST_PX - 1: a row's first lane may start up to three columns left of the crop
	const dim3 grid((cw + DIST_PX - 1 + DIST_TW - 1) / DIST_TW, (ch + DIST_TH - 1) / DIST_TH, src.batch);
	const double px = (double)cw * ch * src.batch;
	const double mapBytes = coord == DIST_COORD_MAP ? 8.0 * cw * ch * (co.mapImageStride ? src.batch : 1) : 0.0;
	static const char* const tags[2][3] = {{"k_distort_map_u8", "k_distort_affine_u8", "k_distort_homography_u8"},
										   {"k_distort_map_f32", "k_distort_affine_f32", "k_distort_homography_f32"}};
	ProfScope ps(ctx, tags[sizeof(T) == 4][coord], mapBytes + px * (2.0 * sizeof(T) + (mask.data ? 1.0 : 0.0)));
	if (interp == BHIP_INTERP_NEAREST_NEIGHBOR) distLaunch<T, BHIP_INTERP_NEAREST_NEIGHBOR>(coord, grid, ctx->stream, P);
	else distLaunch<T, BHIP_INTERP_BILINEAR>(coord, grid, ctx->stream, P);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_distort(bhip_ctx*, DevImg<const uint8_t>, const DistortCoords&, const DistortCrop&, int, int, int, DevImg<uint8_t>, DevImg<uint8_t>);
template int bhip_launch_distort(bhip_ctx*, DevImg<const float>, const DistortCoords&, const DistortCrop&, int, int, int, DevImg<float>, DevImg<uint8_t>);
