// ---------------------------------------------------------------------------------------------------------------
// EnhanceImageOps (I:alg/enhance/EnhanceImageOps.java) on device-resident batches, any row / image stride, any byte alignment:
//   equalize(histogram, transform)                    :65-77     k_equalize_table (the histogram is k_hist_u8 of threshold.hip)
//   applyTransform(GrayU8, transform, GrayU8)         :86-94     over impl/ImplEnhanceHistogram.java:42-53
//   equalizeLocal(GrayU8, radius, GrayU8, length, ..) :176-232   over impl/ImplEnhanceHistogram.java:111-417
//   sharpen4 / sharpen8 (GrayU8, GrayF32)             :307-371   over impl/ImplEnhanceFilter.java
// Only the width x height pixels of an output view are stored.
//
// equalizeLocal as one rule.  The reference dispatches three ways (inner + two row + two column strips; the whole-image histogram; the naive
// loop) and slides a 256-bin histogram; every branch gives, for every pixel and every image size,
//     w = 2r+1,  x0 = max(0, min(x-r, W-w)),  x1 = min(W, x0+w)   (the same in y)
//     out(x,y) = (byte)((#{pixels of [x0,x1) x [y0,y1) with a value <= in(x,y)} * (histogramLength-1)) / ((x1-x0)*(y1-y0)))
// i.e. the window is shifted, not cropped, to stay inside the image and the result is the rank of the centre pixel in it
// (tests/enhance_ref.py restates the five loops and checks this).  A value >= histogramLength is ranked like any other (the reference
// throws ArrayIndexOutOfBoundsException).  Two kernels compute the rank: a direct count out of an LDS tile and a sliding histogram.
// ---------------------------------------------------------------------------------------------------------------
#include "common.h"
#include <algorithm>

// ---- equalize: one workgroup per histogram.  transform[i] = (prefix[i] * (length-1)) / sum in Java's int arithmetic (a product beyond
// 2^31 wraps as it does there); a histogram whose sum is 0 gives zeros (the reference divides by zero and throws) ----
__global__ __launch_bounds__(256) void k_equalize_table(const int* hist, int length, int* transform) {   // transform may be hist
	__shared__ int s[256];
	const int t = threadIdx.x;
	s[t] = t < length ? hist[(long long)blockIdx.x * length + t] : 0;
	__syncthreads();
	for (int d = 1; d < 256; d <<= 1) {
		const int add = t >= d ? s[t - d] : 0;
		__syncthreads();
		s[t] += add;
		__syncthreads();
	}
	const int sum = s[255];
	if (t < length) transform[(long long)blockIdx.x * length + t] = sum == 0 ? 0 : (int)((unsigned)s[t] * (unsigned)(length - 1)) / sum;
}
int bhip_launch_equalize_table(bhip_ctx* ctx, const int* hist, int length, int batch, int* transform) {
	ProfScope prof(ctx, "k_equalize_table", 8.0 * length * batch);
	hipLaunchKernelGGL(k_equalize_table, dim3(batch), dim3(256), 0, ctx->stream, hist, length, transform);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---- applyTransform: 16 pixels of a row per lane (threshold.hip's lane shape), the table of the image in LDS.  A pixel >= length gives 0
// (the reference throws).  In place is allowed: a lane reads its bytes before it writes them ----
__global__ __launch_bounds__(256) void k_apply_transform(const uint8_t* in, long long inImageStride, int inStride, uint8_t* out, long long outImageStride, int outStride,
														 int width, int height, const int* __restrict__ table, long long tableStride, int length) {
	__shared__ uint8_t lut[256];
	lut[threadIdx.x] = (int)threadIdx.x < length ? (uint8_t)table[(long long)blockIdx.z * tableStride + threadIdx.x] : (uint8_t)0;
	__syncthreads();
	const int x = (blockIdx.x * 256 + threadIdx.x) * 16;
	if (x >= width) return;
	const int n = width - x;
	const uint8_t* pi = in + (long long)blockIdx.z * inImageStride + x;
	uint8_t* po = out + (long long)blockIdx.z * outImageStride + x;
	for (int y = blockIdx.y; y < height; y += gridDim.y) {
		const uint8_t* ri = pi + (long long)y * inStride;
		uint8_t* ro = po + (long long)y * outStride;
		if (n >= 16) {
			uint32_t wi[4], wo[4];
			__builtin_memcpy(wi, ri, 16);
#pragma unroll
			for (int j = 0; j < 4; j++)
				wo[j] = (uint32_t)lut[wi[j] & 0xff] | ((uint32_t)lut[(wi[j] >> 8) & 0xff] << 8) | ((uint32_t)lut[(wi[j] >> 16) & 0xff] << 16) | ((uint32_t)lut[wi[j] >> 24] << 24);
			__builtin_memcpy(ro, wo, 16);
		} else {
			for (int j = 0; j < n; j++) ro[j] = lut[ri[j]];
		}
	}
}
// tableStride: ints between the tables of two images, 0 = one table for the batch
int bhip_launch_apply_transform(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<uint8_t> out, const int* table, long long tableStride, int length) {
	ProfScope prof(ctx, "k_apply_transform", 2.0 * in.width * in.height * in.batch);
	dim3 grid((in.width + 4095) / 4096, std::min(in.height, 1024), in.batch);
	hipLaunchKernelGGL(k_apply_transform, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width, in.height,
					   table, tableStride, length);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// equalizeLocal, direct form.  A workgroup owns an EQ_TW x EQ_TH tile of the output.  The windows of its pixels lie in the columns
// [x0(first), x1(last)) and the rows [y0(first), y1(last)) -- x0 and x1 never decrease with x -- which it stages into LDS as bytes, row pitch
// a multiple of 4.  A lane then walks its pixel's window as aligned 32-bit words, four pixels per word: a SWAR compare leaves 0x80 in every
// byte <= the centre value, the words at the two ends of a window row are masked to the window, and a population count adds the word's hits
// to the lane's count (v_bcnt_u32_b32 adds in the same instruction), so no packed counter can overflow.  Tiles whose windows are nowhere
// shifted by the image edge (INNER) take x0 = x - r, y0 = y - r and area w * w without the clamps.
// ---------------------------------------------------------------------------------------------------------------
#define EQ_TW 64
#define EQ_TH 16
struct EqWin {
	int lo, hi;
};
// [lo, hi) of the window of coordinate c on an axis of n pixels: shifted to stay inside, cropped only when n < w
__device__ __host__ __forceinline__ EqWin eqWindow(int c, int r, int n) {
	const int w = 2 * r + 1;
	const int lo = std::max(0, std::min(c - r, n - w));
	return {lo, std::min(n, lo + w)};
}
// 0x80 in every byte of x that is <= the byte of y at its place (yl = y | 0x80808080)
__device__ __forceinline__ uint32_t leBytes(uint32_t x, uint32_t y, uint32_t yl) {
	const uint32_t t = yl - (x & 0x7f7f7f7fu);   // per byte, no borrow across bytes: bit 7 = (y & 0x7f) >= (x & 0x7f)
	return ((y & ~x) | (~(y ^ x) & t)) & 0x80808080u;
}
template <bool INNER>
__global__ __launch_bounds__(256) void k_equalize_local_direct(const uint8_t* __restrict__ in, long long inImageStride, int inStride, uint8_t* __restrict__ out,
															   long long outImageStride, int outStride, int width, int height, int r, int maxValue, int pitch,
															   int innerX0, int innerX1, int innerY0, int innerY1) {
	extern __shared__ __attribute__((aligned(16))) uint8_t eqTile[];
	const int tid = threadIdx.x;
	int bx = blockIdx.x, by = blockIdx.y;
	if (INNER) {   // the grid covers the inner tiles only
		bx += innerX0;
		by += innerY0;
	} else if (bx >= innerX0 && bx < innerX1 && by >= innerY0 && by < innerY1) {
		return;   // an inner tile: the other launch has it
	}
	const int tx0 = bx * EQ_TW, ty0 = by * EQ_TH;
	const int tx1 = std::min(tx0 + EQ_TW, width), ty1 = std::min(ty0 + EQ_TH, height);
	const int sx0 = eqWindow(tx0, r, width).lo, sx1 = eqWindow(tx1 - 1, r, width).hi;
	const int sy0 = eqWindow(ty0, r, height).lo, sy1 = eqWindow(ty1 - 1, r, height).hi;
	const int rows = sy1 - sy0, wordsPerRow = pitch >> 2;
	const uint8_t* src = in + (long long)blockIdx.z * inImageStride;
	// staging: a word of four columns per lane and step; global memory takes the unaligned 4-byte load, columns from sx1 on are zero and
	// are never counted (the masks of a window's last word)
	for (int i = tid; i < rows * wordsPerRow; i += 256) {
		const int ly = i / wordsPerRow, lx = (i - ly * wordsPerRow) * 4;
		const int gx = sx0 + lx;
		uint32_t w = 0;
		if (gx < sx1) {
			const uint8_t* p = src + (long long)(sy0 + ly) * inStride + gx;
			if (gx + 3 < sx1) __builtin_memcpy(&w, p, 4);
			else
				for (int j = 0; gx + j < sx1; j++) w |= (uint32_t)p[j] << (8 * j);
		}
		*reinterpret_cast<uint32_t*>(&eqTile[ly * pitch + lx]) = w;
	}
	__syncthreads();
	uint8_t* dst = out + (long long)blockIdx.z * outImageStride;
	const int lxp = tid & (EQ_TW - 1);
	const int x = tx0 + lxp;
	if (x >= width) return;
	int cx0, cx1;
	if (INNER) {
		cx0 = x - r - sx0;
		cx1 = cx0 + 2 * r + 1;
	} else {
		const EqWin wx = eqWindow(x, r, width);
		cx0 = wx.lo - sx0;
		cx1 = wx.hi - sx0;
	}
	// the window's words of a row: first .. last, the bytes before cx0 and from cx1 on masked away
	const int first = cx0 >> 2, last = (cx1 - 1) >> 2;
	const uint32_t headMask = 0x80808080u << (8 * (cx0 & 3));
	const uint32_t tailMask = 0x80808080u >> (8 * (3 - ((cx1 - 1) & 3)));
	const uint32_t firstMask = first == last ? headMask & tailMask : headMask;
	for (int y = ty0 + (tid >> 6); y < ty1; y += 256 / EQ_TW) {
		int cy0, cy1;
		if (INNER) {
			cy0 = y - r - sy0;
			cy1 = cy0 + 2 * r + 1;
		} else {
			const EqWin wy = eqWindow(y, r, height);
			cy0 = wy.lo - sy0;
			cy1 = wy.hi - sy0;
		}
		const uint32_t v = eqTile[(y - sy0) * pitch + (x - sx0)];
		const uint32_t v4 = v * 0x01010101u, vl = v4 | 0x80808080u;
		int cnt = 0;
		for (int ly = cy0; ly < cy1; ly++) {
			const uint32_t* row = reinterpret_cast<const uint32_t*>(&eqTile[ly * pitch]);
			cnt += __popc(leBytes(row[first], v4, vl) & firstMask);
			for (int k = first + 1; k < last; k++) cnt += __popc(leBytes(row[k], v4, vl));
			if (last > first) cnt += __popc(leBytes(row[last], v4, vl) & tailMask);
		}
		const int area = (cx1 - cx0) * (cy1 - cy0);
		dst[(long long)y * outStride + x] = (uint8_t)((cnt * maxValue) / area);
	}
}
// LDS bytes of the direct form's tile at this radius and image size; the form runs when they fit BHIP_EQLOCAL_DIRECT_LDS_MAX
static size_t eqDirectLds(int r, int width, int height, int* pitch) {
	const long long cols = std::min<long long>(width, EQ_TW + 2LL * r), rows = std::min<long long>(height, EQ_TH + 2LL * r);
	*pitch = (int)((cols + 3) & ~3LL);
	return (size_t)(*pitch * rows);
}
#define BHIP_EQLOCAL_DIRECT_LDS_MAX 65536
bool bhip_equalize_local_direct_fits(int radius, int width, int height) {
	int pitch;
	return eqDirectLds(radius, width, height, &pitch) <= BHIP_EQLOCAL_DIRECT_LDS_MAX;
}
int bhip_launch_equalize_local_direct(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<uint8_t> out, int r, int histogramLength) {
	int pitch;
	const size_t lds = eqDirectLds(r, in.width, in.height, &pitch);
	if (lds > BHIP_EQLOCAL_DIRECT_LDS_MAX) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "equalizeLocal: the direct form's tile does not fit LDS at this radius");
	const int ntx = (in.width + EQ_TW - 1) / EQ_TW, nty = (in.height + EQ_TH - 1) / EQ_TH;
	// inner tiles: full tiles whose first pixel's window starts inside the image and whose last pixel's window ends inside it
	const int ix0 = (r + EQ_TW - 1) / EQ_TW, ix1 = std::max(ix0, (in.width - r) / EQ_TW);
	const int iy0 = (r + EQ_TH - 1) / EQ_TH, iy1 = std::max(iy0, (in.height - r) / EQ_TH);
	const bool inner = ix1 > ix0 && iy1 > iy0;
	const double halo = (double)(EQ_TW + 2 * r) * (EQ_TH + 2 * r) / (EQ_TW * EQ_TH);
	ProfScope prof(ctx, "k_equalize_local_direct", (1.0 + halo) * in.width * in.height * in.batch, (double)(2 * r + 1) * (2 * r + 1) * in.width * in.height * in.batch);
	if (inner) {
		hipLaunchKernelGGL(k_equalize_local_direct<true>, dim3(ix1 - ix0, iy1 - iy0, in.batch), dim3(256), lds, ctx->stream, in.data, in.imageStride, in.stride, out.data,
						   out.imageStride, out.stride, in.width, in.height, r, histogramLength - 1, pitch, ix0, ix1, iy0, iy1);
		BHIP_HIP(ctx, hipGetLastError());
	}
	if (!inner || (ix1 - ix0) * (iy1 - iy0) < ntx * nty) {
		hipLaunchKernelGGL(k_equalize_local_direct<false>, dim3(ntx, nty, in.batch), dim3(256), lds, ctx->stream, in.data, in.imageStride, in.stride, out.data,
						   out.imageStride, out.stride, in.width, in.height, r, histogramLength - 1, pitch, inner ? ix0 : 0, inner ? ix1 : 0, inner ? iy0 : 0,
						   inner ? iy1 : 0);
		BHIP_HIP(ctx, hipGetLastError());
	}
	return BHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// equalizeLocal, sliding form.  A workgroup is one wave and owns EQ_RUN consecutive pixels of one row.  It builds the 256-bin histogram of
// the first pixel's window in LDS (lanes spread over the window's entries, LDS atomics), then moves right as the reference does: where the
// window moves, the lanes spread over its rows take the column that leaves out of the histogram and put the column that enters in.  A pixel
// is answered by a masked wave reduction: lane j sums the bins 4j .. 4j+3 that are <= the pixel's value.  Lane (i & 63) keeps the answer of
// pixel i, and 64 answers are stored at a time.  The window's rows are those of the row's y for the whole run.
// ---------------------------------------------------------------------------------------------------------------
#define EQ_RUN 128
__global__ __launch_bounds__(64) void k_equalize_local_sliding(const uint8_t* __restrict__ in, long long inImageStride, int inStride, uint8_t* __restrict__ out,
															   long long outImageStride, int outStride, int width, int height, int r, int maxValue) {
	__shared__ __attribute__((aligned(16))) int hist[256];
	const int lane = threadIdx.x;
	const int y = blockIdx.y;
	const int xa = blockIdx.x * EQ_RUN, xb = std::min(xa + EQ_RUN, width);
	const uint8_t* src = in + (long long)blockIdx.z * inImageStride;
	uint8_t* dst = out + (long long)blockIdx.z * outImageStride + (long long)y * outStride;
	const EqWin wy = eqWindow(y, r, height);
	const int wh = wy.hi - wy.lo;
	const uint8_t* top = src + (long long)wy.lo * inStride;
#pragma unroll
	for (int j = 0; j < 4; j++) hist[lane * 4 + j] = 0;
	__syncthreads();
	EqWin wx = eqWindow(xa, r, width);
	{
		const int ww = wx.hi - wx.lo, n = ww * wh;
		for (int i = lane; i < n; i += 64) {
			const int row = i / ww, col = i - row * ww;
			atomicAdd(&hist[top[(long long)row * inStride + wx.lo + col]], 1);
		}
	}
	__syncthreads();
	// the run's centre values, read once: lane l holds those of pixels xa + l and xa + 64 + l (EQ_RUN == 128)
	const uint8_t* centre = src + (long long)y * inStride;
	const int c0 = xa + lane < xb ? centre[xa + lane] : 0;
	const int c1 = xa + 64 + lane < xb ? centre[xa + 64 + lane] : 0;
	int keep = 0;
	for (int x = xa; x < xb; x++) {
		const EqWin nw = eqWindow(x, r, width);
		if (nw.lo != wx.lo) {   // one column to the right: wx.lo leaves, wx.hi enters (the same decision in every lane)
			for (int i = lane; i < wh; i += 64) {
				const uint8_t* p = top + (long long)i * inStride;
				atomicSub(&hist[p[wx.lo]], 1);
				atomicAdd(&hist[p[wx.hi]], 1);
			}
			wx = nw;
			__syncthreads();
		}
		const int k = x - xa;   // the same in every lane
		const int v = __builtin_amdgcn_readlane(k < 64 ? c0 : c1, k & 63);
		const int4 h = *reinterpret_cast<const int4*>(&hist[lane * 4]);
		const int b = lane * 4;
		int s = (b <= v ? h.x : 0) + (b + 1 <= v ? h.y : 0) + (b + 2 <= v ? h.z : 0) + (b + 3 <= v ? h.w : 0);
#pragma unroll
		for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
		__syncthreads();   // the bins are read before the next step changes them
		const int area = (wx.hi - wx.lo) * wh;
		if (lane == ((x - xa) & 63)) keep = (s * maxValue) / area;
		if (((x - xa) & 63) == 63 || x == xb - 1) {
			const int base = x - ((x - xa) & 63);
			if (base + lane <= x) dst[base + lane] = (uint8_t)keep;
		}
	}
}
int bhip_launch_equalize_local_sliding(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<uint8_t> out, int r, int histogramLength) {
	if (in.height > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "equalizeLocal: more than 65535 rows");
	ProfScope prof(ctx, "k_equalize_local_sliding", 2.0 * in.width * in.height * in.batch, 2.0 * (2 * r + 1) * in.width * in.height * in.batch);
	dim3 grid((in.width + EQ_RUN - 1) / EQ_RUN, in.height, in.batch);
	hipLaunchKernelGGL(k_equalize_local_sliding, grid, dim3(64), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width,
					   in.height, r, histogramLength - 1);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// sharpen4 / sharpen8.  The reference runs an inner loop over 1 <= x < W-1, 1 <= y < H-1, then sharpenBorder: for every x the top pixel, then
// the bottom pixel; then for every y in 1 .. H-2 the left pixel, then the right pixel.  A pixel keeps its LAST write, so its formula is
//     y in 1 .. H-2:   x == W-1: RIGHT    else x == 0: LEFT    else INNER
//     otherwise:       y == H-1: BOTTOM   else TOP                           (H == 1: every pixel is BOTTOM; W == 1: rows 1 .. H-2 are RIGHT)
// with g = safeGet (coordinates clamped into the image), the sums in the reference's order (it matters for float):
//   sharpen4  INNER   5*c - (((l + r) + u) + d)
//             TOP     4*c - ((g(x-1,0) + g(x+1,0)) + g(x,1))            BOTTOM  4*c - ((g(x-1,b) + g(x+1,b)) + g(x,b-1))
//             LEFT    4*c - ((g(1,y) + g(0,y-1)) + g(0,y+1))            RIGHT   4*c - ((g(c-1,y) + g(c,y-1)) + g(c,y+1))
//   sharpen8  every form is 9*c - (a11+a12+a13+a21+a23+a31+a32+a33) over the clamped 3x3 in raster order, so the owner does not matter
// then the clamp `if (a > 255) a = 255; else if (a < 0) a = 0` (a float NaN passes through).  No fused multiply-add: the library is built
// with -ffp-contract=off, and the products are rounded before the subtraction.
// ---------------------------------------------------------------------------------------------------------------
template <class T> struct SharpAcc;
template <> struct SharpAcc<uint8_t> { using type = int; };
template <> struct SharpAcc<float> { using type = float; };
template <class T, int RULE>
__device__ __forceinline__ typename SharpAcc<T>::type sharpenPixel(const T* __restrict__ img, int stride, int x, int y, int W, int H) {
	using A = typename SharpAcc<T>::type;
	auto g = [&](int gx, int gy) -> A {
		gx = gx < 0 ? 0 : gx >= W ? W - 1 : gx;
		gy = gy < 0 ? 0 : gy >= H ? H - 1 : gy;
		return (A)img[(long long)gy * stride + gx];
	};
	const A c = g(x, y);
	A a;
	if (RULE == 8) {
		a = (A)9 * c - (g(x - 1, y - 1) + g(x, y - 1) + g(x + 1, y - 1) + g(x - 1, y) + g(x + 1, y) + g(x - 1, y + 1) + g(x, y + 1) + g(x + 1, y + 1));
	} else if (y >= 1 && y <= H - 2) {
		if (x == W - 1) a = (A)4 * c - (g(x - 1, y) + g(x, y - 1) + g(x, y + 1));        // RIGHT
		else if (x == 0) a = (A)4 * c - (g(1, y) + g(0, y - 1) + g(0, y + 1));             // LEFT
		else a = (A)5 * c - (g(x - 1, y) + g(x + 1, y) + g(x, y - 1) + g(x, y + 1));       // INNER
	} else if (y == H - 1) {
		a = (A)4 * c - (g(x - 1, y) + g(x + 1, y) + g(x, y - 1));                          // BOTTOM
	} else {
		a = (A)4 * c - (g(x - 1, 0) + g(x + 1, 0) + g(x, 1));                              // TOP
	}
	if (a > (A)255) a = (A)255;
	else if (a < (A)0) a = (A)0;
	return a;
}
// a lane computes PX consecutive pixels of a row (4 for GrayU8: one 32-bit store; 1 for GrayF32)
template <class T, int RULE>
__global__ __launch_bounds__(256) void k_sharpen(const T* __restrict__ in, long long inImageStride, int inStride, T* __restrict__ out, long long outImageStride,
												 int outStride, int width, int height) {
	constexpr int PX = sizeof(T) == 1 ? 4 : 1;
	const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * PX;
	const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (x >= width || y >= height) return;
	const T* src = in + (long long)blockIdx.z * inImageStride;
	T* q = out + (long long)blockIdx.z * outImageStride + (long long)y * outStride + x;
	T res[PX];
#pragma unroll
	for (int j = 0; j < PX; j++) res[j] = x + j < width ? (T)sharpenPixel<T, RULE>(src, inStride, x + j, y, width, height) : (T)0;
	if (x + PX <= width) __builtin_memcpy(q, res, sizeof(res));
	else
		for (int j = 0; x + j < width; j++) q[j] = res[j];
}
template <class T>
int bhip_launch_sharpen(bhip_ctx* ctx, int rule, DevImg<const T> in, DevImg<T> out) {
	constexpr int PX = sizeof(T) == 1 ? 4 : 1;
	ProfScope prof(ctx, sizeof(T) == 1 ? "k_sharpen_u8" : "k_sharpen_f32", 2.0 * sizeof(T) * in.width * in.height * in.batch);
	dim3 grid((in.width + 64 * PX - 1) / (64 * PX), (in.height + 3) / 4, in.batch);
	if (rule == 4)
		hipLaunchKernelGGL((k_sharpen<T, 4>), grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width,
						   in.height);
	else
		hipLaunchKernelGGL((k_sharpen<T, 8>), grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width,
						   in.height);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_sharpen<uint8_t>(bhip_ctx*, int, DevImg<const uint8_t>, DevImg<uint8_t>);
template int bhip_launch_sharpen<float>(bhip_ctx*, int, DevImg<const float>, DevImg<float>);
