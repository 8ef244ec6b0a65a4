// K9: boofcv-ip image gradients (Sobel, Prewitt, three-tap) on GrayF32 and GrayU8, and the gradient intensity.  The float forms keep the
// reference's evaluation order with no FMA contraction; the integer forms are exact.
//
// Reference:
//   GradientSobel_UnrolledOuter.process_F32_sub   I:alg/filter/derivative/impl/GradientSobel_UnrolledOuter.java:210-
//   GradientThree_Standard.process                I:alg/filter/derivative/impl/GradientThree_Standard.java:40-62
//   border handling                               I:alg/filter/convolve/border/ConvolveJustBorder_General_SB.java:46-175,
//                                                 I:alg/filter/derivative/DerivativeHelperFunctions.java:140-175
// Bound: HBM (12P bytes for a float gradient).
#include "ip_dev.h"

// ---------------- gradients ----------------
struct GradParams {
	const float* in;
	float* dx;
	float* dy;
	long long inImageStride, outImageStride;   // floats between the images of a batch
	int inStride, outStride, width, height;
	int border;  // 0: frame untouched, 1: ImageBorderValue(0), 2: BorderType.EXTENDED (Sobel only)
};

__device__ __forceinline__ float at0(const GradParams& P, const float* img, int x, int y) {
	return (x >= 0 && x < P.width && y >= 0 && y < P.height) ? img[(long long)y * P.inStride + x] : 0.0f;
}

// One pixel of GradientSobel / GradientThree from its 3x3 neighbourhood a[row][col] (0 outside the image), reference expressions:
//   Sobel interior   GradientSobel_UnrolledOuter.process_F32_sub; frame with a border = generic border convolution with kernelDerivX/Y_F32
//                    (total = 0; total += get(x+j,y+i)*k in row-major kernel order)
//   three-tap        GradientThree_Standard.process inside; with a border the first/last column (row) of derivX (derivY) takes the generic
//                    form, rows {0,1,H-2,H-1} (columns for derivY) the unrolled 3-tap form
//   Prewitt (KIND 2) GradientPrewitt_Shared.process(GrayF32, ...) (I:alg/filter/derivative/impl/GradientPrewitt_Shared.java:104-137) inside; frame
//                    with a border = the same generic border convolution with GradientPrewitt.kernelDerivX/Y_F32 (GradientPrewitt.java:45-48,128-142)
// Returns false when the pixel is left untouched (frame pixel, no border policy).
// The generic border convolution of a frame pixel (ConvolveJustBorder_General_SB.convolve(Kernel2D_F32, ...)): total = 0, then
// total += get(x+j, y+i) * k in row-major kernel order, for both kernels
__device__ __forceinline__ void gradFrame3x3(const float a[3][3], int x, int y, int W, int H, int border, const float kx[9], const float ky[9], float& dx, float& dy) {
	float tx = 0, ty = 0;
	// border 2 = BorderType.EXTENDED (BorderIndex1D_Extend): an index outside the image is clamped, and the clamped pixel of a frame
	// pixel's neighbourhood is always one of the nine values at hand
	const int r0 = (border == 2 && y == 0) ? 1 : 0, r2 = (border == 2 && y == H - 1) ? 1 : 2;
	const int c0 = (border == 2 && x == 0) ? 1 : 0, c2 = (border == 2 && x == W - 1) ? 1 : 2;
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++) {
			const int ii = i == 0 ? r0 : i == 2 ? r2 : 1, jj = j == 0 ? c0 : j == 2 ? c2 : 1;
			const float v = (ii == 0 ? (jj == 0 ? a[0][0] : jj == 1 ? a[0][1] : a[0][2])
							 : ii == 1 ? (jj == 0 ? a[1][0] : jj == 1 ? a[1][1] : a[1][2])
									   : (jj == 0 ? a[2][0] : jj == 1 ? a[2][1] : a[2][2]));
			tx += v * kx[i * 3 + j];
			ty += v * ky[i * 3 + j];
		}
	dx = tx; dy = ty;
}
template <int KIND>
__device__ __forceinline__ bool gradOne(const float a[3][3], int x, int y, int W, int H, int border, float& dx, float& dy) {
	const bool interior = x >= 1 && x < W - 1 && y >= 1 && y < H - 1;
	if (KIND == 0) {
		if (interior) {
			const float v = (a[2][2] - a[0][0]) * 0.25f;
			const float w = (a[2][0] - a[0][2]) * 0.25f;
			dy = (a[2][1] - a[0][1]) * 0.5f + v + w;
			dx = (a[1][2] - a[1][0]) * 0.5f + v - w;
			return true;
		}
		if (!border) return false;
		const float kx[9] = {-0.25f, 0, 0.25f, -0.5f, 0, 0.5f, -0.25f, 0, 0.25f};
		const float ky[9] = {-0.25f, -0.5f, -0.25f, 0, 0, 0, 0.25f, 0.5f, 0.25f};
		gradFrame3x3(a, x, y, W, H, border, kx, ky, dx, dy);
		return true;
	}
	if (KIND == 2) {
		if (interior) {
			const float w = a[2][2] - a[0][0];
			const float v = a[2][0] - a[0][2];
			dy = a[2][1] + w + v - a[0][1];
			dx = a[1][2] + w - v - a[1][0];
			return true;
		}
		if (!border) return false;
		const float kx[9] = {-1.0f, 0, 1.0f, -1.0f, 0, 1.0f, -1.0f, 0, 1.0f};
		const float ky[9] = {-1.0f, -1.0f, -1.0f, 0, 0, 0, 1.0f, 1.0f, 1.0f};
		gradFrame3x3(a, x, y, W, H, border, kx, ky, dx, dy);
		return true;
	}
	if (!border) {
		if (!interior) return false;
		dx = (a[1][2] - a[1][0]) * 0.5f;
		dy = (a[2][1] - a[0][1]) * 0.5f;
		return true;
	}
	const float k0 = -0.5f, k1 = 0.0f, k2 = 0.5f;
	if (x == 0 || x == W - 1) {
		float t = 0;
		t += a[1][0] * k0; t += a[1][1] * k1; t += a[1][2] * k2;
		dx = t;
	} else if (y <= 1 || y >= H - 2) {
		float t = a[1][0] * k0; t += a[1][1] * k1; t += a[1][2] * k2;
		dx = t;
	} else {
		dx = (a[1][2] - a[1][0]) * 0.5f;
	}
	if (y == 0 || y == H - 1) {
		float t = 0;
		t += a[0][1] * k0; t += a[1][1] * k1; t += a[2][1] * k2;
		dy = t;
	} else if (x <= 1 || x >= W - 2) {
		float t = a[0][1] * k0; t += a[1][1] * k1; t += a[2][1] * k2;
		dy = t;
	} else {
		dy = (a[2][1] - a[0][1]) * 0.5f;
	}
	return true;
}

// General form: one pixel per thread, any alignment
template <int KIND>
__global__ __launch_bounds__(256) void k_grad(GradParams P) {
	const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
	if (x >= P.width) return;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	float a[3][3];
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++) a[i][j] = at0(P, img, x + j - 1, y + i - 1);
	float dx, dy;
	if (!gradOne<KIND>(a, x, y, P.width, P.height, P.border, dx, dy)) return;
	const long long o = (long long)blockIdx.z * P.outImageStride + (long long)y * P.outStride + x;
	P.dx[o] = dx;
	P.dy[o] = dy;
}

// Streaming form: a wave walks GR_ROWS rows of a 256-column strip; lane l owns columns 4l .. 4l+3 and keeps a three-row window in
// registers, so every input row is loaded once per strip (16 bytes per lane); the two columns beside a lane's four come from the
// neighbouring lanes, the strip's outermost two from single loads.  Outputs leave as 16-byte stores.  HBM: 4P read + 8P written.
#define GR_ROWS 8
struct GradRow { float v[6]; };   // columns x-1 .. x+4 of one row (0 outside the image)
__device__ __forceinline__ GradRow gradLoadRow(const GradParams& P, const float* img, int x, int y, int lane) {
	GradRow r;
	if (y < 0 || y >= P.height) {
#pragma unroll
		for (int i = 0; i < 6; i++) r.v[i] = 0.0f;
		return r;
	}
	const float* row = img + (long long)y * P.inStride;
	const float4 c = x < P.width ? loadRow4(row, x, P.width) : make_float4(0, 0, 0, 0);
	float left = __shfl_up(c.w, 1, 64), right = __shfl_down(c.x, 1, 64);
	if (lane == 0) left = (x - 1 >= 0 && x - 1 < P.width) ? row[x - 1] : 0.0f;
	if (lane == 63) right = (x + 4 < P.width) ? row[x + 4] : 0.0f;
	r.v[0] = left; r.v[1] = c.x; r.v[2] = c.y; r.v[3] = c.z; r.v[4] = c.w; r.v[5] = right;
	return r;
}
template <int KIND>
__global__ __launch_bounds__(256) void k_grad_stream(GradParams P) {
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x = blockIdx.x * 256 + 4 * lane;
	const int y0 = (blockIdx.y * 4 + wave) * GR_ROWS;
	if (y0 >= P.height) return;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	float* dxImg = P.dx + (long long)blockIdx.z * P.outImageStride;
	float* dyImg = P.dy + (long long)blockIdx.z * P.outImageStride;
	GradRow r0 = gradLoadRow(P, img, x, y0 - 1, lane), r1 = gradLoadRow(P, img, x, y0, lane), r2 = gradLoadRow(P, img, x, y0 + 1, lane);
	const int yEnd = min(y0 + GR_ROWS, P.height);
	for (int y = y0; y < yEnd; y++) {
		// row y+2 (the bottom row of the NEXT output) is requested before this output is computed: one row of loads always in flight
		GradRow r3 = r2;
		if (y + 1 < yEnd) r3 = gradLoadRow(P, img, x, y + 2, lane);
		if (x < P.width) {
			float dx[4], dy[4];
			bool wr[4];
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const float a[3][3] = {{r0.v[j], r0.v[j + 1], r0.v[j + 2]}, {r1.v[j], r1.v[j + 1], r1.v[j + 2]}, {r2.v[j], r2.v[j + 1], r2.v[j + 2]}};
				wr[j] = gradOne<KIND>(a, x + j, y, P.width, P.height, P.border, dx[j], dy[j]);
			}
			const long long o = (long long)y * P.outStride + x;
			if (x + 3 < P.width && wr[0] && wr[1] && wr[2] && wr[3]) {
				*reinterpret_cast<float4*>(dxImg + o) = make_float4(dx[0], dx[1], dx[2], dx[3]);
				*reinterpret_cast<float4*>(dyImg + o) = make_float4(dy[0], dy[1], dy[2], dy[3]);
			} else {
#pragma unroll
				for (int j = 0; j < 4; j++)
					if (x + j < P.width && wr[j]) { dxImg[o + j] = dx[j]; dyImg[o + j] = dy[j]; }
			}
		}
		r0 = r1; r1 = r2; r2 = r3;
	}
}

int bhip_launch_gradient(bhip_ctx* ctx, int kind, DevImg<const float> in, DevImg<float> dx, DevImg<float> dy, int border) {
	const int width = in.width, height = in.height, batch = in.batch;
	if (width <= 0 || height <= 0 || batch <= 0) return BHIP_OK;
	if (!sameLayout(dx, dy)) return bhip_fail(ctx, BHIP_ERR_INVALID, "dx and dy must share one layout");
	GradParams P{in.data, dx.data, dy.data, in.imageStride, dx.imageStride, in.stride, dx.stride, width, height, border};
	ProfScope prof(ctx, kind == 0 ? "k_sobel" : kind == 2 ? "k_prewitt" : "k_three", 12.0 * width * height * batch);
	const bool stream = vec4(in) && vec4(dx) && aligned16(dy.data);
	if (stream) {
		dim3 grid((width + 255) / 256, (height + 4 * GR_ROWS - 1) / (4 * GR_ROWS), batch);
		if (kind == 0) hipLaunchKernelGGL(k_grad_stream<0>, grid, dim3(256), 0, ctx->stream, P);
		else if (kind == 2) hipLaunchKernelGGL(k_grad_stream<2>, grid, dim3(256), 0, ctx->stream, P);
		else hipLaunchKernelGGL(k_grad_stream<1>, grid, dim3(256), 0, ctx->stream, P);
	} else {
		dim3 grid((width + 255) / 256, height, batch);
		if (kind == 0) hipLaunchKernelGGL(k_grad<0>, grid, dim3(256), 0, ctx->stream, P);
		else if (kind == 2) hipLaunchKernelGGL(k_grad<2>, grid, dim3(256), 0, ctx->stream, P);
		else hipLaunchKernelGGL(k_grad<1>, grid, dim3(256), 0, ctx->stream, P);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// GradientToEdgeFeatures.intensityE / intensityAbs (F:alg/feature/detect/edge/impl/ImplGradientToEdgeFeatures.java:40-85) and the squared
// magnitude dx*dx + dy*dy (no reference function of its own: the |grad|^2 of BASELINE config 5; same products and sum as intensityE,
// without the square root).  Element-wise, 8P read + 4P written.
__global__ __launch_bounds__(256) void k_grad_intensity(const float* __restrict__ dx, const float* __restrict__ dy, long long dImageStride, int dStride,
														 float* __restrict__ out, long long oImageStride, int oStride, int width, int height, int kind) {
	const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
	if (x >= width) return;
	const long long i = (long long)blockIdx.z * dImageStride + (long long)y * dStride + x;
	const float a = dx[i], b = dy[i];
	float r;
	if (kind == 0) r = sqrtf(a * a + b * b);           // (float)Math.sqrt((double)f): correctly rounded, as sqrtf
	else if (kind == 1) r = fabsf(a) + fabsf(b);
	else r = a * a + b * b;
	out[(long long)blockIdx.z * oImageStride + (long long)y * oStride + x] = r;
}
int bhip_launch_grad_intensity(bhip_ctx* ctx, int kind, DevImg<const float> dx, DevImg<const float> dy, DevImg<float> out) {
	const int width = dx.width, height = dx.height, batch = dx.batch;
	if (kind < 0 || kind > 2) return bhip_fail(ctx, BHIP_ERR_INVALID, "unknown gradient intensity");
	if (width <= 0 || height <= 0 || batch <= 0) return BHIP_OK;
	if (!sameLayout(dx, dy)) return bhip_fail(ctx, BHIP_ERR_INVALID, "dx and dy must share one layout");
	ProfScope prof(ctx, "k_grad_intensity", 12.0 * width * height * batch);
	hipLaunchKernelGGL(k_grad_intensity, dim3((width + 255) / 256, height, batch), dim3(256), 0, ctx->stream, dx.data, dy.data, dx.imageStride, dx.stride, out.data,
					   out.imageStride, out.stride, width, height, kind);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------- integer gradient + corner path: GrayU8 -> GrayS16 gradients, S16 / weighted corner intensity ----------------
// GradientSobel_Outer.process_sub(GrayU8, GrayS16, GrayS16)     I:alg/filter/derivative/impl/GradientSobel_Outer.java:76-
//   border: ConvolveJustBorder_General_SB.convolve(kernelDerivX/Y_I32, ImageBorderValue(0))   I:alg/filter/derivative/GradientSobel.java:73-74,110-124
// GradientThree_Standard.process(GrayU8, GrayS16, GrayS16)      I:alg/filter/derivative/impl/GradientThree_Standard.java:67-88
//   border: DerivativeHelperFunctions.processBorderHorizontal/Vertical with kernelDeriv_I32
// The arithmetic is integer, so the interior expression and every border form give the same value: the 3x3 (3-tap) formula on the image
// padded with 0.  With border 1 every pixel is written, with border 0 only the interior (frame untouched).  Results fit in a short.
// Border 2 (Sobel only) is BorderType.EXTENDED -- ImageBorder1D_S32 with BorderIndex1D_Extend (I:core/image/border/BorderIndex1D_Extend.java):
// the same nine-tap sum on the index-clamped image; every pixel is written.
struct GradU8Params {
	const uint8_t* in;
	int16_t* dx;
	int16_t* dy;
	long long inImageStride, outImageStride;   // elements between the images of a batch
	int inStride, outStride, width, height;
	int border;
};
struct GradRowU8 { int v[6]; };   // columns x-1 .. x+4 of one row (0 outside the image)
__device__ __forceinline__ GradRowU8 gradU8LoadRow(const GradU8Params& P, const uint8_t* img, int x, int y, int lane) {
	GradRowU8 r;
	const bool ext = P.border == 2;   // outside pixels read the nearest pixel of the image instead of 0
	if (y < 0 || y >= P.height) {
		if (!ext) {
#pragma unroll
			for (int i = 0; i < 6; i++) r.v[i] = 0;
			return r;
		}
		y = y < 0 ? 0 : P.height - 1;
	}
	const uint8_t* row = img + (long long)y * P.inStride;
	const int last = P.width - 1;
	int c[4];
	if (x + 3 < P.width && (reinterpret_cast<uintptr_t>(row + x) & 3) == 0) {
		const unsigned w = *reinterpret_cast<const unsigned*>(row + x);
		c[0] = w & 255; c[1] = (w >> 8) & 255; c[2] = (w >> 16) & 255; c[3] = w >> 24;
	} else {
#pragma unroll
		for (int j = 0; j < 4; j++) c[j] = x + j < P.width ? row[x + j] : ext ? row[last] : 0;
	}
	int left = __shfl_up(c[3], 1, 64), right = __shfl_down(c[0], 1, 64);
	if (lane == 0) left = x - 1 < 0 ? (ext ? row[0] : 0) : x - 1 < P.width ? row[x - 1] : ext ? row[last] : 0;
	if (lane == 63) right = x + 4 < P.width ? row[x + 4] : ext ? row[last] : 0;
	r.v[0] = left; r.v[1] = c[0]; r.v[2] = c[1]; r.v[3] = c[2]; r.v[4] = c[3]; r.v[5] = right;
	return r;
}
// A wave walks GR_ROWS rows of a 256-column strip, lane l owns columns 4l .. 4l+3 and keeps three rows in registers (as k_grad_stream).
// HBM: 1P read + 4P written.
template <int KIND>
__global__ __launch_bounds__(256) void k_grad_u8(GradU8Params P) {
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x = blockIdx.x * 256 + 4 * lane;
	const int y0 = (blockIdx.y * 4 + wave) * GR_ROWS;
	if (y0 >= P.height) return;
	const uint8_t* img = P.in + (long long)blockIdx.z * P.inImageStride;
	int16_t* dxImg = P.dx + (long long)blockIdx.z * P.outImageStride;
	int16_t* dyImg = P.dy + (long long)blockIdx.z * P.outImageStride;
	GradRowU8 r0 = gradU8LoadRow(P, img, x, y0 - 1, lane), r1 = gradU8LoadRow(P, img, x, y0, lane), r2 = gradU8LoadRow(P, img, x, y0 + 1, lane);
	const int yEnd = min(y0 + GR_ROWS, P.height);
	for (int y = y0; y < yEnd; y++) {
		GradRowU8 r3 = r2;
		if (y + 1 < yEnd) r3 = gradU8LoadRow(P, img, x, y + 2, lane);
		if (x < P.width) {
			int16_t dx[4], dy[4];
			bool wr[4];
			const bool rowIn = y >= 1 && y < P.height - 1;
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int a00 = r0.v[j], a01 = r0.v[j + 1], a02 = r0.v[j + 2];
				const int a10 = r1.v[j], a12 = r1.v[j + 2];
				const int a20 = r2.v[j], a21 = r2.v[j + 1], a22 = r2.v[j + 2];
				if (KIND == 0) {
					const int v = a22 - a00, w = a20 - a02;
					dy[j] = (int16_t)((a21 - a01) * 2 + v + w);
					dx[j] = (int16_t)((a12 - a10) * 2 + v - w);
				} else if (KIND == 2) {
					// GradientPrewitt_Shared.process(GrayU8, ...) (impl/GradientPrewitt_Shared.java:34-67); on the frame the int sums of the generic
					// border convolution with GradientPrewitt.kernelDerivX/Y_I32 are the same expression over the padded pixels
					const int w = a22 - a00, v = a20 - a02;
					dy[j] = (int16_t)(a21 + w + v - a01);
					dx[j] = (int16_t)(a12 + w - v - a10);
				} else {
					dx[j] = (int16_t)(a12 - a10);
					dy[j] = (int16_t)(a21 - a01);
				}
				wr[j] = P.border || (rowIn && x + j >= 1 && x + j < P.width - 1);
			}
			int16_t* ox = dxImg + (long long)y * P.outStride + x;
			int16_t* oy = dyImg + (long long)y * P.outStride + x;
			if (x + 3 < P.width && wr[0] && wr[1] && wr[2] && wr[3] && (reinterpret_cast<uintptr_t>(ox) & 7) == 0 &&
				(reinterpret_cast<uintptr_t>(oy) & 7) == 0) {
				short4 sx, sy;
				sx.x = dx[0]; sx.y = dx[1]; sx.z = dx[2]; sx.w = dx[3];
				sy.x = dy[0]; sy.y = dy[1]; sy.z = dy[2]; sy.w = dy[3];
				*reinterpret_cast<short4*>(ox) = sx;
				*reinterpret_cast<short4*>(oy) = sy;
			} else {
#pragma unroll
				for (int j = 0; j < 4; j++)
					if (x + j < P.width && wr[j]) { ox[j] = dx[j]; oy[j] = dy[j]; }
			}
		}
		r0 = r1; r1 = r2; r2 = r3;
	}
}

int bhip_launch_gradient(bhip_ctx* ctx, int kind, DevImg<const uint8_t> in, DevImg<int16_t> dx, DevImg<int16_t> dy, int border) {
	const int width = in.width, height = in.height, batch = in.batch;
	if (width <= 0 || height <= 0 || batch <= 0) return BHIP_OK;
	if (!sameLayout(dx, dy)) return bhip_fail(ctx, BHIP_ERR_INVALID, "dx and dy must share one layout");
	GradU8Params P{in.data, dx.data, dy.data, in.imageStride, dx.imageStride, in.stride, dx.stride, width, height, border};
	ProfScope prof(ctx, kind == 0 ? "k_sobel_u8" : kind == 2 ? "k_prewitt_u8" : "k_three_u8", 5.0 * width * height * batch);
	dim3 grid((width + 255) / 256, (height + 4 * GR_ROWS - 1) / (4 * GR_ROWS), batch);
	if (kind == 0) hipLaunchKernelGGL(k_grad_u8<0>, grid, dim3(256), 0, ctx->stream, P);
	else if (kind == 2) hipLaunchKernelGGL(k_grad_u8<2>, grid, dim3(256), 0, ctx->stream, P);
	else hipLaunchKernelGGL(k_grad_u8<1>, grid, dim3(256), 0, ctx->stream, P);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
