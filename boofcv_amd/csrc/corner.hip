// Gradient corner intensity (Shi-Tomasi / Harris): box windows on F32 and S16 derivatives, Gaussian-weighted windows on both.
#include "ip_dev.h"

// ---------------- gradient corner intensity (Shi-Tomasi / Harris on box-window sums of the gradient products) ----------------
// GradientCornerIntensity.process = ImplSsdCornerBox.process   F:alg/feature/detect/intensity/impl/ImplSsdCornerBox.java:36-51
//   horizontal() / vertical()                                  F:alg/feature/detect/intensity/impl/ImplSsdCorner_F32.java:62-127, 133-196
//   scores                                                     F:.../impl/ShiTomasiCorner_F32.java:33-42, HarrisCorner_F32.java:45-50
// The reference's window sums are running float sums (subtract the sample leaving the window, add the one entering), so every value
// depends on the history of its whole row (horizontal pass) or column (vertical pass).  The chains are kept exactly: one thread walks
// one row, then one thread walks one column; parallelism is across rows / columns (and images).  Bound: the horizontal pass is a
// latency chain over W per row (each lane streams its own row through L1); the vertical pass is coalesced and HBM bound (12P read, 4P write).
struct CornerParams {
	const float* dx; const float* dy;
	long long dImageStride, hImageStride, iImageStride;   // floats between the images of a batch (blockIdx.y)
	int dStride, width, height, radius;
	float* hXX; float* hXY; float* hYY;   // dense width x height planes
	float* intensity; int iStride;
	int kind; float kappa;
};

__global__ __launch_bounds__(64) void k_corner_rows(CornerParams P) {
	const int row = blockIdx.x * blockDim.x + threadIdx.x;
	if (row >= P.height) return;
	const int W = P.width, r = P.radius, ww = 2 * r + 1;
	const float* __restrict__ X = P.dx + (long long)blockIdx.y * P.dImageStride + (long long)row * P.dStride;
	const float* __restrict__ Y = P.dy + (long long)blockIdx.y * P.dImageStride + (long long)row * P.dStride;
	const long long ho = (long long)blockIdx.y * P.hImageStride + (long long)row * W;
	float* oXX = P.hXX + ho; float* oXY = P.hXY + ho; float* oYY = P.hYY + ho;
	float tXX = 0, tXY = 0, tYY = 0;
	for (int i = 0; i < ww; i++) {
		const float dx = X[i], dy = Y[i];
		tXX += dx * dx; tXY += dx * dy; tYY += dy * dy;
	}
	oXX[r] = tXX; oXY[r] = tXY; oYY[r] = tYY;
	int i = ww;
	// eight steps at a time: the 32 loads of a batch are independent and issued together, the chain arithmetic keeps its order
	for (; i + 8 <= W; i += 8) {
		float ax[8], ay[8], bx[8], by[8], rXX[8], rXY[8], rYY[8];
#pragma unroll
		for (int k = 0; k < 8; k++) { ax[k] = X[i - ww + k]; ay[k] = Y[i - ww + k]; bx[k] = X[i + k]; by[k] = Y[i + k]; }
#pragma unroll
		for (int k = 0; k < 8; k++) {
			tXX -= ax[k] * ax[k]; tXY -= ax[k] * ay[k]; tYY -= ay[k] * ay[k];
			tXX += bx[k] * bx[k]; tXY += bx[k] * by[k]; tYY += by[k] * by[k];
			rXX[k] = tXX; rXY[k] = tXY; rYY[k] = tYY;
		}
#pragma unroll
		for (int k = 0; k < 8; k++) { oXX[i - r + k] = rXX[k]; oXY[i - r + k] = rXY[k]; oYY[i - r + k] = rYY[k]; }
	}
	for (; i < W; i++) {
		float dx = X[i - ww], dy = Y[i - ww];
		tXX -= dx * dx; tXY -= dx * dy; tYY -= dy * dy;
		dx = X[i]; dy = Y[i];
		tXX += dx * dx; tXY += dx * dy; tYY += dy * dy;
		oXX[i - r] = tXX; oXY[i - r] = tXY; oYY[i - r] = tYY;
	}
}

__device__ __forceinline__ float cornerScore(int kind, float kappa, float xx, float xy, float yy) {
	if (kind == 0) {
		const float left = (xx + yy) * 0.5f;
		const float b = (xx - yy) * 0.5f;
		const float right = sqrtf(b * b + xy * xy);   // (float)Math.sqrt((double)f) == correctly rounded float sqrt
		return left - right;
	}
	const float trace = xx + yy;
	return (xx * yy - xy * xy) - kappa * trace * trace;
}

__global__ __launch_bounds__(256) void k_corner_cols(CornerParams P) {
	const int W = P.width, H = P.height, r = P.radius, kw = 2 * r + 1;
	const int x = r + blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= W - r) return;
	const float* __restrict__ hXX = P.hXX + (long long)blockIdx.y * P.hImageStride;
	const float* __restrict__ hXY = P.hXY + (long long)blockIdx.y * P.hImageStride;
	const float* __restrict__ hYY = P.hYY + (long long)blockIdx.y * P.hImageStride;
	float* __restrict__ inten = P.intensity + (long long)blockIdx.y * P.iImageStride;
	float tXX = 0, tXY = 0, tYY = 0;
	for (int k = 0; k < kw; k++) {
		const long long s = (long long)k * W + x;
		tXX += hXX[s]; tXY += hXY[s]; tYY += hYY[s];
	}
	inten[(long long)r * P.iStride + x] = cornerScore(P.kind, P.kappa, tXX, tXY, tYY);
	int y = r + 1;
	for (; y + 8 <= H - r; y += 8) {
		float a[3][8], b[3][8];
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const long long in = (long long)(y + k + r) * W + x, out = in - (long long)kw * W;
			a[0][k] = hXX[out]; a[1][k] = hXY[out]; a[2][k] = hYY[out];
			b[0][k] = hXX[in]; b[1][k] = hXY[in]; b[2][k] = hYY[in];
		}
#pragma unroll
		for (int k = 0; k < 8; k++) {
			tXX = tXX - a[0][k]; tXX += b[0][k];
			tXY = tXY - a[1][k]; tXY += b[1][k];
			tYY = tYY - a[2][k]; tYY += b[2][k];
			inten[(long long)(y + k) * P.iStride + x] = cornerScore(P.kind, P.kappa, tXX, tXY, tYY);
		}
	}
	for (; y < H - r; y++) {
		const long long in = (long long)(y + r) * W + x, out = in - (long long)kw * W;
		tXX = tXX - hXX[out]; tXX += hXX[in];
		tXY = tXY - hXY[out]; tXY += hXY[in];
		tYY = tYY - hYY[out]; tYY += hYY[in];
		inten[(long long)y * P.iStride + x] = cornerScore(P.kind, P.kappa, tXX, tXY, tYY);
	}
}

// intensity must be zero along its border of `radius` pixels: the caller clears the whole image first.  scratch: the row sums XX, XY, YY
// as three dense width x height planes per image.
int bhip_launch_corner_intensity(bhip_ctx* ctx, int kind, int radius, float kappa, DevImg<const float> dx, DevImg<const float> dy, DevImg<float> intensity,
								 float* scratch) {
	const int width = dx.width, height = dx.height, batch = dx.batch;
	if (kind != 0 && kind != 1) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "corner score not supported");
	if (radius < 0 || 2 * radius + 1 > width || 2 * radius + 1 > height) return bhip_fail(ctx, BHIP_ERR_INVALID, "window larger than the image");
	if (batch <= 0) return BHIP_OK;
	if (!sameLayout(dx, dy)) return bhip_fail(ctx, BHIP_ERR_INVALID, "dx and dy must share one layout");
	const long long px = (long long)width * height;
	CornerParams P{dx.data, dy.data, dx.imageStride, px * 3, intensity.imageStride, dx.stride, width, height, radius, scratch, scratch + px, scratch + 2 * px,
				   intensity.data, intensity.stride, kind, kappa};
	{
		ProfScope prof(ctx, "k_corner_rows", 4.0 * width * height * 5 * batch);
		hipLaunchKernelGGL(k_corner_rows, dim3((height + 63) / 64, batch), dim3(64), 0, ctx->stream, P);
	}
	{
		ProfScope prof(ctx, "k_corner_cols", 4.0 * width * height * 4 * batch);
		hipLaunchKernelGGL(k_corner_cols, dim3((width - 2 * radius + 255) / 256, batch), dim3(256), 0, ctx->stream, P);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---- corner scores on int32 window sums ----
// ShiTomasiCorner_S32.compute   F:alg/feature/detect/intensity/impl/ShiTomasiCorner_S32.java:34-42 (int adds wrap, then double, Math.sqrt)
// HarrisCorner_S32.compute      F:alg/feature/detect/intensity/impl/HarrisCorner_S32.java:45-51 (each int to float, then the F32 expression)
// The sums arrive as uint32_t: Java's int arithmetic wraps, C++ signed overflow is undefined.
__device__ __forceinline__ float cornerScoreS32(int kind, float kappa, uint32_t xx, uint32_t xy, uint32_t yy) {
	if (kind == 0) {
		const double left = (double)(int32_t)(xx + yy) * 0.5;
		const double b = (double)(int32_t)(xx - yy) * 0.5;
		const double sxy = (double)(int32_t)xy;
		const double right = sqrt(b * b + sxy * sxy);   // correctly rounded f64 square root, as Math.sqrt
		return (float)(left - right);
	}
	const float fxx = (float)(int32_t)xx, fyy = (float)(int32_t)yy, fxy = (float)(int32_t)xy;
	const float trace = fxx + fyy;
	return (fxx * fyy - fxy * fxy) - kappa * trace * trace;
}

// ---- unweighted S16 corner intensity, fused ----
// GradientCornerIntensity.process = ImplSsdCornerBox.process   F:alg/feature/detect/intensity/impl/ImplSsdCornerBox.java:36-54
//   horizontal() / vertical()                                  F:alg/feature/detect/intensity/impl/ImplSsdCorner_S16.java:63-198
// Window sums of the int products are int32 with wrap-around, so they do not depend on the summation order: one pass stages dx,dy of a
// (CB_TX + 2r) x (CB_TY + 2r) block in LDS (packed 16+16 bits), forms the horizontal window sums of the three products for the block's
// columns, then each lane walks its column down CB_TY / 4 rows with a running vertical sum and writes the score.  Pixels within `radius` of the
// image edge get 0 (ImplSsdCornerBox fills the border), so every intensity pixel is written exactly once and nothing else is.
// HBM: 4P read (+ halo, mostly served by L2) + 4P written.
#define CB_TX 64
#define CB_TY 32
struct CornerS16Params {
	const int16_t* dx; const int16_t* dy;
	long long dImageStride, iImageStride;
	int dStride, width, height, radius;
	float* intensity; int iStride;
	int kind; float kappa;
};
static size_t cornerBoxLds(int r) { return (size_t)(CB_TX + 2 * r) * (CB_TY + 2 * r) * 4 + (size_t)3 * CB_TX * (CB_TY + 2 * r) * 4; }

__global__ __launch_bounds__(256) void k_corner_box_s16(CornerS16Params P) {
	extern __shared__ uint32_t cbLds[];
	const int r = P.radius, RW = CB_TX + 2 * r, RH = CB_TY + 2 * r, W = P.width, H = P.height;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x0 = blockIdx.x * CB_TX, y0 = blockIdx.y * CB_TY;
	uint32_t* d = cbLds;                       // [RH][RW]: dx in the low half, dy in the high half
	uint32_t* hXX = d + RW * RH;               // [RH][CB_TX] horizontal window sums
	uint32_t* hXY = hXX + CB_TX * RH;
	uint32_t* hYY = hXY + CB_TX * RH;
	const long long img = (long long)blockIdx.z * P.dImageStride;
	for (int ry = wave; ry < RH; ry += 4) {
		const int gy = y0 - r + ry;
		const bool rowIn = gy >= 0 && gy < H;
		for (int rx = lane; rx < RW; rx += 64) {
			const int gx = x0 - r + rx;
			uint32_t v = 0;
			if (rowIn && gx >= 0 && gx < W) {
				const long long o = img + (long long)gy * P.dStride + gx;
				v = (uint32_t)(uint16_t)P.dx[o] | ((uint32_t)(uint16_t)P.dy[o] << 16);
			}
			d[ry * RW + rx] = v;
		}
	}
	__syncthreads();
	const int kw = 2 * r + 1;
	for (int ry = wave; ry < RH; ry += 4) {
		uint32_t sXX = 0, sXY = 0, sYY = 0;
		const uint32_t* s = d + ry * RW + lane;
		for (int k = 0; k < kw; k++) {
			const uint32_t v = s[k];
			const int32_t ix = (int16_t)(v & 0xffff), iy = (int16_t)(v >> 16);
			sXX += (uint32_t)(ix * ix); sXY += (uint32_t)(ix * iy); sYY += (uint32_t)(iy * iy);   // |product| <= 2^30
		}
		hXX[ry * CB_TX + lane] = sXX; hXY[ry * CB_TX + lane] = sXY; hYY[ry * CB_TX + lane] = sYY;
	}
	__syncthreads();
	const int gx = x0 + lane;
	if (gx >= W) return;
	const bool colIn = gx >= r && gx < W - r;
	const int oy0 = wave * (CB_TY / 4);
	uint32_t tXX = 0, tXY = 0, tYY = 0;
	for (int k = 0; k < kw; k++) {
		const int i = (oy0 + k) * CB_TX + lane;
		tXX += hXX[i]; tXY += hXY[i]; tYY += hYY[i];
	}
	float* out = P.intensity + (long long)blockIdx.z * P.iImageStride + gx;
	for (int oy = oy0; oy < oy0 + CB_TY / 4; oy++) {
		const int gy = y0 + oy;
		if (gy >= H) break;
		if (oy > oy0) {
			const int iOut = (oy - 1) * CB_TX + lane, iIn = (oy + 2 * r) * CB_TX + lane;
			tXX += hXX[iIn] - hXX[iOut]; tXY += hXY[iIn] - hXY[iOut]; tYY += hYY[iIn] - hYY[iOut];
		}
		const bool in = colIn && gy >= r && gy < H - r;
		out[(long long)gy * P.iStride] = in ? cornerScoreS32(P.kind, P.kappa, tXX, tXY, tYY) : 0.0f;
	}
}

// Radii whose block does not fit the LDS: ImplSsdCorner_S16's two passes over int32 planes (dense width x height per image).  Running sums
// with wrap-around equal the direct sums.  The caller clears the intensity border.
__global__ __launch_bounds__(64) void k_corner_rows_s16(CornerS16Params P, uint32_t* hXX, uint32_t* hXY, uint32_t* hYY, long long hImageStride) {
	const int row = blockIdx.x * blockDim.x + threadIdx.x;
	if (row >= P.height) return;
	const int W = P.width, r = P.radius, ww = 2 * r + 1;
	const int16_t* X = P.dx + (long long)blockIdx.y * P.dImageStride + (long long)row * P.dStride;
	const int16_t* Y = P.dy + (long long)blockIdx.y * P.dImageStride + (long long)row * P.dStride;
	const long long ho = (long long)blockIdx.y * hImageStride + (long long)row * W;
	uint32_t tXX = 0, tXY = 0, tYY = 0;
	for (int i = 0; i < W; i++) {
		int32_t dx = X[i], dy = Y[i];
		tXX += (uint32_t)(dx * dx); tXY += (uint32_t)(dx * dy); tYY += (uint32_t)(dy * dy);
		if (i >= ww) {
			dx = X[i - ww]; dy = Y[i - ww];
			tXX -= (uint32_t)(dx * dx); tXY -= (uint32_t)(dx * dy); tYY -= (uint32_t)(dy * dy);
		}
		if (i >= ww - 1) { hXX[ho + i - r] = tXX; hXY[ho + i - r] = tXY; hYY[ho + i - r] = tYY; }
	}
}
__global__ __launch_bounds__(256) void k_corner_cols_s16(CornerS16Params P, const uint32_t* hXX, const uint32_t* hXY, const uint32_t* hYY, long long hImageStride) {
	const int W = P.width, H = P.height, r = P.radius, kw = 2 * r + 1;
	const int x = r + blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= W - r) return;
	const long long h0 = (long long)blockIdx.y * hImageStride + x;
	float* inten = P.intensity + (long long)blockIdx.y * P.iImageStride + x;
	uint32_t tXX = 0, tXY = 0, tYY = 0;
	for (int y = 0; y < H; y++) {
		const long long s = h0 + (long long)y * W;
		tXX += hXX[s]; tXY += hXY[s]; tYY += hYY[s];
		if (y >= kw) {
			const long long o = s - (long long)kw * W;
			tXX -= hXX[o]; tXY -= hXY[o]; tYY -= hYY[o];
		}
		if (y >= kw - 1) inten[(long long)(y - r) * P.iStride] = cornerScoreS32(P.kind, P.kappa, tXX, tXY, tYY);
	}
}

// scratch: 3 * width * height * 4 bytes per image, used only when the radius is beyond the fused block (bhip_corner_box_s16_scratch)
size_t bhip_corner_box_s16_scratch(int radius, int width, int height, int batch) {
	return cornerBoxLds(radius) <= 65536 ? 0 : (size_t)3 * width * height * 4 * batch;
}
int bhip_launch_corner_box_s16(bhip_ctx* ctx, int kind, int radius, float kappa, DevImg<const int16_t> dx, DevImg<const int16_t> dy, DevImg<float> intensity,
							   void* scratch) {
	const int width = dx.width, height = dx.height, batch = dx.batch;
	if (kind != 0 && kind != 1) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "corner score not supported");
	if (radius < 0 || 2 * radius + 1 > width || 2 * radius + 1 > height) return bhip_fail(ctx, BHIP_ERR_INVALID, "window larger than the image");
	if (batch <= 0) return BHIP_OK;
	if (!sameLayout(dx, dy)) return bhip_fail(ctx, BHIP_ERR_INVALID, "dx and dy must share one layout");
	CornerS16Params P{dx.data, dy.data, dx.imageStride, intensity.imageStride, dx.stride, width, height, radius, intensity.data, intensity.stride, kind, kappa};
	const size_t lds = cornerBoxLds(radius);
	if (lds <= 65536) {
		const int bx = (width + CB_TX - 1) / CB_TX, by = (height + CB_TY - 1) / CB_TY;
		// bytes: every block reads its dx,dy halo block (4 B/px), every pixel is written once (4 B/px)
		const double in = 4.0 * bx * by * (CB_TX + 2.0 * radius) * (CB_TY + 2.0 * radius);
		ProfScope prof(ctx, "k_corner_box_s16", (in + 4.0 * width * height) * batch);
		hipLaunchKernelGGL(k_corner_box_s16, dim3(bx, by, batch), dim3(256), lds, ctx->stream, P);
		BHIP_HIP(ctx, hipGetLastError());
		return BHIP_OK;
	}
	if (!scratch) return bhip_fail(ctx, BHIP_ERR_INVALID, "no scratch for the two-pass corner form");
	const long long px = (long long)width * height;
	uint32_t* h = static_cast<uint32_t*>(scratch);
	for (int b = 0; b < batch; b++)
		BHIP_HIP(ctx, hipMemset2DAsync(intensity.data + (long long)b * intensity.imageStride, (size_t)intensity.stride * 4, 0, (size_t)width * 4, (size_t)height,
									   ctx->stream));
	{
		ProfScope prof(ctx, "k_corner_rows_s16", (4.0 + 12.0) * px * batch);
		hipLaunchKernelGGL(k_corner_rows_s16, dim3((height + 63) / 64, batch), dim3(64), 0, ctx->stream, P, h, h + px, h + 2 * px, px * 3);
	}
	{
		ProfScope prof(ctx, "k_corner_cols_s16", 16.0 * px * batch);
		hipLaunchKernelGGL(k_corner_cols_s16, dim3((width - 2 * radius + 255) / 256, batch), dim3(256), 0, ctx->stream, P, h, h + px, h + 2 * px, px * 3);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---- Gaussian-weighted corner intensity, fused (F32 and S16 derivatives) ----
// ImplSsdCornerWeighted_F32.process   F:alg/feature/detect/intensity/impl/ImplSsdCornerWeighted_F32.java:46-104
// ImplSsdCornerWeighted_S16.process   F:alg/feature/detect/intensity/impl/ImplSsdCornerWeighted_S16.java:50-108
//   products, then ConvolveImageNormalized.horizontal then vertical on each of XX, XY, YY, then the score on every pixel (getIgnoreBorder() 0)
//   F32: ConvolveImageNormalized.java:48-93 -- the arithmetic of bhip_conv_norm_h/v (convOne, setNormalizedMode), per axis
//   S32: ConvolveImageNormalized.java:768-800 -- interior (total + divisor/2) / divisor with divisor = kernel.computeSum()
//        (noborder/ConvolveImageUnrolled_SB_S32_S32_Div), border and naive forms (total + weight/2) / weight with the clipped weight
//        (normalized/ConvolveNormalized_JustBorder_SB.java:1147-1250, ConvolveNormalizedNaive_SB.java:504-560): one formula, the clipped
//        weight equals the divisor inside.  int adds and multiplies wrap; / truncates toward zero.
// One block: a CW_TX x CW_TY tile.  The products of the (tile + 2r)^2 block go to LDS, the horizontal pass writes CW_TX x (CW_TY + 2r) values
// to LDS, the vertical pass and the score run from there.  Only the intensity is written.  HBM: 8P (F32) / 4P (S16) read + halo, 4P written.
#define CW_TX 32
#define CW_TY 16
#define CW_MAX_RADIUS 15
struct CornerWParams {
	const void* dx; const void* dy;
	long long dImageStride, iImageStride;
	int dStride, width, height, radius;
	float* intensity; int iStride;
	int kind; float kappa;
	int ks[2 * CW_MAX_RADIUS + 1];   // S32 kernel
};
template <class T>
static size_t cornerWeightedLds(int r) {
	return (size_t)3 * sizeof(T) * ((size_t)(CW_TX + 2 * r) * (CW_TY + 2 * r) + (size_t)CW_TX * (CW_TY + 2 * r)) + (size_t)2 * (2 * r + 1) * 4;
}

// one normalised S32 output from taps s[k*step], k in [0, kw), centred (offset r) on `pos` of an axis of `extent` pixels
__device__ __forceinline__ int32_t convNormS32(const int32_t* s, int step, int pos, int extent, int kw, int r, const int32_t* kc) {
	const int k0 = max(0, r - pos);
	const int k1 = min(kw, extent - pos + r);
	uint32_t total = 0;
	int32_t weight = 0;
	for (int k = k0; k < k1; k++) {
		const int32_t w = kc[k];
		weight += w;
		total += (uint32_t)s[k * step] * (uint32_t)w;
	}
	return (int32_t)(total + (uint32_t)(weight / 2)) / weight;
}

template <bool S16>
__global__ __launch_bounds__(256) void k_corner_weighted(CornerWParams Q, ConvParams Ph, ConvParams Pv) {
	typedef typename std::conditional<S16, int32_t, float>::type T;
	extern __shared__ uint32_t cwLds[];
	const int r = Q.radius, kw = 2 * r + 1, RW = CW_TX + 2 * r, RH = CW_TY + 2 * r, W = Q.width, H = Q.height;
	const int tx = threadIdx.x & (CW_TX - 1), ty = threadIdx.x / CW_TX;   // 32 x 8
	const int x0 = blockIdx.x * CW_TX, y0 = blockIdx.y * CW_TY;
	T* pXX = reinterpret_cast<T*>(cwLds);   // [RH][RW] products
	T* pXY = pXX + RW * RH;
	T* pYY = pXY + RW * RH;
	T* hXX = pYY + RW * RH;                 // [RH][CW_TX] horizontal pass
	T* hXY = hXX + CW_TX * RH;
	T* hYY = hXY + CW_TX * RH;
	float* kh = reinterpret_cast<float*>(hYY + CW_TX * RH);   // F32 horizontal / vertical kernels
	float* kv = kh + kw;
	int32_t* ks = reinterpret_cast<int32_t*>(kh);            // S32 kernel
	if (threadIdx.x < kw) {
		if constexpr (S16) ks[threadIdx.x] = Q.ks[threadIdx.x];
		else { kh[threadIdx.x] = Ph.k[threadIdx.x]; kv[threadIdx.x] = Pv.k[threadIdx.x]; }
	}
	const long long img = (long long)blockIdx.z * Q.dImageStride;
	for (int ry = ty; ry < RH; ry += 8) {
		const int gy = y0 - r + ry;
		const bool rowIn = gy >= 0 && gy < H;
		for (int rx = tx; rx < RW; rx += CW_TX) {
			const int gx = x0 - r + rx;
			T xx = 0, xy = 0, yy = 0;
			if (rowIn && gx >= 0 && gx < W) {
				const long long o = img + (long long)gy * Q.dStride + gx;
				if constexpr (S16) {
					const int32_t a = static_cast<const int16_t*>(Q.dx)[o], b = static_cast<const int16_t*>(Q.dy)[o];
					xx = a * a; xy = a * b; yy = b * b;   // |product| <= 2^30: no wrap
				} else {
					const float a = static_cast<const float*>(Q.dx)[o], b = static_cast<const float*>(Q.dy)[o];
					xx = a * a; xy = a * b; yy = b * b;
				}
			}
			const int i = ry * RW + rx;
			pXX[i] = xx; pXY[i] = xy; pYY[i] = yy;
		}
	}
	__syncthreads();
	// horizontal pass: rows of the block inside the image, the tile's columns; tap 0 of column c is block column c (image column gx - r)
	const int gx = x0 + tx;
	for (int ry = ty; ry < RH; ry += 8) {
		const int gy = y0 - r + ry;
		if (gy < 0 || gy >= H || gx >= W) continue;
		const int i = ry * RW + tx, o = ry * CW_TX + tx;
		if constexpr (S16) {
			hXX[o] = convNormS32(reinterpret_cast<const int32_t*>(pXX) + i, 1, gx, W, kw, r, ks);
			hXY[o] = convNormS32(reinterpret_cast<const int32_t*>(pXY) + i, 1, gx, W, kw, r, ks);
			hYY[o] = convNormS32(reinterpret_cast<const int32_t*>(pYY) + i, 1, gx, W, kw, r, ks);
		} else {
			float v;
			convOne<0>(Ph, reinterpret_cast<const float*>(pXX) + i, 1, gx, W, v, kh); hXX[o] = v;
			convOne<0>(Ph, reinterpret_cast<const float*>(pXY) + i, 1, gx, W, v, kh); hXY[o] = v;
			convOne<0>(Ph, reinterpret_cast<const float*>(pYY) + i, 1, gx, W, v, kh); hYY[o] = v;
		}
	}
	__syncthreads();
	if (gx >= W) return;
	float* out = Q.intensity + (long long)blockIdx.z * Q.iImageStride + gx;
	for (int oy = ty; oy < CW_TY; oy += 8) {
		const int gy = y0 + oy;
		if (gy >= H) break;
		const int i = oy * CW_TX + tx;   // tap 0 of row oy is block row oy (image row gy - r)
		float score;
		if constexpr (S16) {
			const int32_t xx = convNormS32(reinterpret_cast<const int32_t*>(hXX) + i, CW_TX, gy, H, kw, r, ks);
			const int32_t xy = convNormS32(reinterpret_cast<const int32_t*>(hXY) + i, CW_TX, gy, H, kw, r, ks);
			const int32_t yy = convNormS32(reinterpret_cast<const int32_t*>(hYY) + i, CW_TX, gy, H, kw, r, ks);
			score = cornerScoreS32(Q.kind, Q.kappa, (uint32_t)xx, (uint32_t)xy, (uint32_t)yy);
		} else {
			float xx, xy, yy;
			convOne<0>(Pv, reinterpret_cast<const float*>(hXX) + i, CW_TX, gy, H, xx, kv);
			convOne<0>(Pv, reinterpret_cast<const float*>(hXY) + i, CW_TX, gy, H, xy, kv);
			convOne<0>(Pv, reinterpret_cast<const float*>(hYY) + i, CW_TX, gy, H, yy, kv);
			score = cornerScore(Q.kind, Q.kappa, xx, xy, yy);
		}
		out[(long long)gy * Q.iStride] = score;
	}
}

int bhip_corner_weighted_max_radius() { return CW_MAX_RADIUS; }

// T: the derivatives are int16_t (ImplSsdCornerWeighted_S16) or float (ImplSsdCornerWeighted_F32).  radius must be 1 .. CW_MAX_RADIUS.
template <class T>
static int launchCornerWeighted(bhip_ctx* ctx, int kind, int radius, float kappa, DevImg<const T> dx, DevImg<const T> dy, DevImg<float> intensity) {
	constexpr bool s16 = std::is_same_v<T, int16_t>;
	const int width = dx.width, height = dx.height, batch = dx.batch;
	if (kind != 0 && kind != 1) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "corner score not supported");
	if (radius <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Radius must be > 0");
	if (radius > CW_MAX_RADIUS) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "weighted corner radius above the supported limit");
	if (width <= 0 || height <= 0 || batch <= 0) return BHIP_OK;
	if (!sameLayout(dx, dy)) return bhip_fail(ctx, BHIP_ERR_INVALID, "dx and dy must share one layout");
	CornerWParams Q{};
	Q.dx = dx.data; Q.dy = dy.data; Q.dImageStride = dx.imageStride; Q.iImageStride = intensity.imageStride; Q.dStride = dx.stride; Q.width = width; Q.height = height;
	Q.radius = radius; Q.intensity = intensity.data; Q.iStride = intensity.stride; Q.kind = kind; Q.kappa = kappa;
	const int kw = 2 * radius + 1;
	ConvParams Ph{}, Pv{};
	if (s16) {
		std::vector<int32_t> k = bhip_gaussian1d_s32(radius);
		for (int i = 0; i < kw; i++) Q.ks[i] = k[i];
	} else {
		// FactoryKernelGaussian.gaussian(Kernel1D_F32.class, -1, radius), each axis normalised as ConvolveImageNormalized does
		std::vector<float> k = bhip_gaussian1d_f32(-1, radius);
		for (ConvParams* P : {&Ph, &Pv}) {
			P->kw = kw; P->koff = radius;
			for (int i = 0; i < kw; i++) P->k[i] = k[i];
			P->unrolled = kw <= 11 ? 1 : 0;   // ConvolveImageUnrolled widths 3..11 (first tap assigns)
		}
		setNormalizedMode(Ph, width);
		setNormalizedMode(Pv, height);
	}
	const int bx = (width + CW_TX - 1) / CW_TX, by = (height + CW_TY - 1) / CW_TY;
	const size_t lds = s16 ? cornerWeightedLds<int32_t>(radius) : cornerWeightedLds<float>(radius);
	// bytes: every block reads its dx,dy halo block (8 B/px F32, 4 B/px S16), every pixel is written once
	const double in = (s16 ? 4.0 : 8.0) * bx * by * (CW_TX + 2.0 * radius) * (CW_TY + 2.0 * radius);
	ProfScope prof(ctx, s16 ? "k_corner_weighted_s16" : "k_corner_weighted_f32", (in + 4.0 * width * height) * batch);
	if (s16) hipLaunchKernelGGL(k_corner_weighted<true>, dim3(bx, by, batch), dim3(256), lds, ctx->stream, Q, Ph, Pv);
	else hipLaunchKernelGGL(k_corner_weighted<false>, dim3(bx, by, batch), dim3(256), lds, ctx->stream, Q, Ph, Pv);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
int bhip_launch_corner_weighted(bhip_ctx* ctx, int kind, int radius, float kappa, DevImg<const float> dx, DevImg<const float> dy, DevImg<float> intensity) {
	return launchCornerWeighted(ctx, kind, radius, kappa, dx, dy, intensity);
}
int bhip_launch_corner_weighted(bhip_ctx* ctx, int kind, int radius, float kappa, DevImg<const int16_t> dx, DevImg<const int16_t> dy, DevImg<float> intensity) {
	return launchCornerWeighted(ctx, kind, radius, kappa, dx, dy, intensity);
}
