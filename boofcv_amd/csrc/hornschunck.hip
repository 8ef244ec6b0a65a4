// Horn-Schunck dense optical flow: HornSchunck_F32 / HornSchunck_U8 behind FactoryDenseOpticalFlow.hornSchunck.
//   F:alg/flow/HornSchunck.java:92-191, HornSchunck_F32.java:36-175, HornSchunck_U8.java:38-177, F:factory/flow/FactoryDenseOpticalFlow.java:122-138
//
// Derivatives (k_hs_deriv), with w = width-1, h = height-1; A = image1, B = image2, every sum left to right, nothing contracted:
//   derivX   x < w, y < h: 0.25f*(d0+d1+d2+d3), the x forward differences of A row y, A row y+1, B row y, B row y+1; y == h: 0.5f*(d0+d1) of A, B;
//            x == w: 0
//   derivY   x < w, y < h: 0.25f*(d0+d1+d2+d3), the y forward differences of A column x, A column x+1, B column x, B column x+1; x == w, y < h:
//            0.5f*(d0+d1) of A, B; y == h: 0
//   derivT   0.25f*(d0+d1+d2+d3), dk = B - A at (x,y), (x+1,y), (x,y+1), (x+1,y+1), coordinates clamped to the image (computeDerivT's inner loop
//            and borderDerivT are this one rule)
// GrayU8: the same taps in int, (..)/4 and (..)/2 truncating toward zero; the GrayS16 value is stored as float (exact).  borderDerivT of
// HornSchunck_U8 goes through float and (short): the sum of four differences and its quarter are exact in float and the cast truncates, which is
// the integer form.
//
// Iteration (k_hs_iterate).  findFlow is a Jacobi iteration: borderAverageFlow / innerAverageFlow write averageFlow from the flow of the last
// iteration, then every pixel is updated from averageFlow alone.  With getExtend's clamp the border and the inner routine are one expression:
//   u = 0.1666667f*(f0+f1+f2+f3) + 0.08333333f*(f4+f5+f6+f7)   (x and y alike; left, right, up, down, up-left, up-right, down-left, down-right)
//   r = (dx*u + dy*v + dt)/(alpha2 + dx*dx + dy*dy);  flow = (u - dx*r, v - dy*r)
// so a pixel after iteration k depends on its 3x3 neighbourhood after iteration k-1 and on nothing else.  A workgroup owns an HS_TW x HS_TH tile
// and runs n <= HS_K iterations on it out of LDS: it stages the tile with a halo of n pixels -- where the halo leaves the image there is none:
// the clamped neighbours of a border pixel are cells of the region -- and every iteration recomputes every staged pixel from one LDS plane
// into the other.  A cell on an edge of the region that is not an edge of the image reads itself in place of the neighbour it lacks, so after
// iteration i the cells closer than i to such an edge are wrong, and the others are what the whole-image iteration gives: they read only
// cells that were right one iteration before.  The tile proper is n cells away, so it is exact after n iterations, whatever n is -- the fusion
// depth does not change a bit of the result.
//
// Layout: the region is HS_RW x HS_RH = 128 x 64 cells of (x, y) float pairs, two planes, 128 KiB of LDS; 1024 lanes, lane t owns column
// t % 128 and the HS_P = 8 rows from 8 * (t / 128) on and keeps dx, dy, dt and alpha2 + dx*dx + dy*dy of those eight pixels in registers for
// the launch.  A wave is 64 consecutive cells of a row: its ds_read_b64 of a row (and of the row shifted by one cell) covers every bank once per
// 32-lane half.  Walking down its column a lane carries the two rows above in registers and reads three cells per pixel instead of eight.
// One barrier per iteration; the row tests are uniform over a wave.  Resource figures: DESIGN.md, "Horn-Schunck dense optical flow".
#include "common.h"

#define HS_K BHIP_FLOW_HS_MAX_FUSED
#define HS_TW BHIP_HS_TILE_W
#define HS_TH BHIP_HS_TILE_H
#define HS_RW (HS_TW + 2 * HS_K)
#define HS_RH (HS_TH + 2 * HS_K)
#define HS_P 8
#define HS_THREADS (HS_RW * HS_RH / HS_P)
static_assert(HS_RW == 128 && HS_RH % HS_P == 0 && HS_THREADS == 1024, "the lane mapping below is written for a 128-wide region and 1024 lanes");

// ---- derivatives ----
template <class T> struct HsArith;
template <> struct HsArith<float> {
	using V = float;
	static __device__ __forceinline__ float quarter(float s) { return 0.25f * s; }
	static __device__ __forceinline__ float half(float s) { return 0.5f * s; }
};
template <> struct HsArith<uint8_t> {
	using V = int;
	static __device__ __forceinline__ float quarter(int s) { return (float)(s / 4); }
	static __device__ __forceinline__ float half(int s) { return (float)(s / 2); }
};

// deriv: dense [batch][3][H][W] floats -- derivX, derivY, derivT
template <class T>
__global__ __launch_bounds__(256) void k_hs_deriv(const T* __restrict__ a, long long aImageStride, int aStride, const T* __restrict__ b, long long bImageStride,
													int bStride, int W, int H, float* __restrict__ deriv) {
	using A = HsArith<T>;
	using V = typename A::V;
	const int x = blockIdx.x * 256 + threadIdx.x;
	if (x >= W) return;
	const int w = W - 1, h = H - 1, x1 = min(x + 1, w);
	a += (long long)blockIdx.z * aImageStride;
	b += (long long)blockIdx.z * bImageStride;
	const long long plane = (long long)W * H;
	deriv += (long long)blockIdx.z * 3 * plane;
	for (int y = blockIdx.y; y < H; y += gridDim.y) {
		const int y1 = min(y + 1, h);
		const T *a0 = a + (long long)y * aStride, *a1 = a + (long long)y1 * aStride, *b0 = b + (long long)y * bStride, *b1 = b + (long long)y1 * bStride;
		const V A00 = a0[x], A10 = a0[x1], A01 = a1[x], A11 = a1[x1], B00 = b0[x], B10 = b0[x1], B01 = b1[x], B11 = b1[x1];
		float gx = 0, gy = 0;
		if (x < w) gx = y < h ? A::quarter((A10 - A00) + (A11 - A01) + (B10 - B00) + (B11 - B01)) : A::half((A10 - A00) + (B10 - B00));
		if (y < h) gy = x < w ? A::quarter((A01 - A00) + (A11 - A10) + (B01 - B00) + (B11 - B10)) : A::half((A01 - A00) + (B01 - B00));
		const float gt = A::quarter((B00 - A00) + (B10 - A10) + (B01 - A01) + (B11 - A11));
		const long long i = (long long)y * W + x;
		deriv[i] = gx;
		deriv[plane + i] = gy;
		deriv[2 * plane + i] = gt;
	}
}

template <class T>
int bhip_launch_hs_derivatives(bhip_ctx* ctx, DevImg<const T> src, DevImg<const T> dst, float* deriv) {
	const double px = (double)src.width * src.height * src.batch;
	ProfScope prof(ctx, sizeof(T) == 1 ? "k_hs_deriv_u8" : "k_hs_deriv", px * (2.0 * sizeof(T) + 12.0));
	dim3 grid((src.width + 255) / 256, std::min(src.height, 65535), src.batch);
	hipLaunchKernelGGL(k_hs_deriv<T>, grid, dim3(256), 0, ctx->stream, src.data, src.imageStride, src.stride, dst.data, dst.imageStride, dst.stride, src.width, src.height,
					   deriv);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_hs_derivatives<float>(bhip_ctx*, DevImg<const float>, DevImg<const float>, float*);
template int bhip_launch_hs_derivatives<uint8_t>(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, float*);

// ---- iteration ----
// in: the flow before, dense [batch][H][W] (x, y) pairs, or nullptr = the zero flow; out: pixel (x, y) at out + b*outImageStride + y*outStride + 2*x
__global__ __launch_bounds__(HS_THREADS) void k_hs_iterate(const float* __restrict__ deriv, const float2* __restrict__ in, float* __restrict__ out, long long outImageStride,
															 int outStride, int W, int H, float alpha2, int n) {
	__shared__ float2 planes[2][HS_RH * HS_RW];
	const int tid = threadIdx.x, lx = tid & (HS_RW - 1), r0 = (tid >> 7) * HS_P;
	const int x0 = blockIdx.x * HS_TW - n, y0 = blockIdx.y * HS_TH - n;   // image position of region cell (0, 0)
	// the staged cells: the tile and its halo, inside the image
	const int cx0 = max(0, -x0), cx1 = min(HS_TW + 2 * n - 1, W - 1 - x0), cy0 = max(0, -y0), cy1 = min(HS_TH + 2 * n - 1, H - 1 - y0);
	const bool colOn = lx >= cx0 && lx <= cx1;
	const long long plane = (long long)W * H;
	deriv += (long long)blockIdx.z * 3 * plane;
	if (in) in += (long long)blockIdx.z * plane;
	const int gx = x0 + lx;
	float dx[HS_P], dy[HS_P], dt[HS_P], den[HS_P];
#pragma unroll
	for (int j = 0; j < HS_P; j++) {
		const int row = r0 + j;
		dx[j] = 0; dy[j] = 0; dt[j] = 0;
		if (colOn && row >= cy0 && row <= cy1) {
			const long long i = (long long)(y0 + row) * W + gx;
			dx[j] = deriv[i];
			dy[j] = deriv[plane + i];
			dt[j] = deriv[2 * plane + i];
			planes[0][row * HS_RW + lx] = in ? in[i] : make_float2(0.0f, 0.0f);
		}
		den[j] = alpha2 + dx[j] * dx[j] + dy[j] * dy[j];
	}
	__syncthreads();
	const int xl = min(max(lx - 1, cx0), cx1), xr = min(max(lx + 1, cx0), cx1);   // getExtend; on an inner edge of the region: the cell itself
	const bool rowsOn = colOn && r0 <= cy1 && r0 + HS_P - 1 >= cy0;
	for (int it = 0; it < n; it++) {
		const float2* s = planes[it & 1];
		float2* d = planes[(it & 1) ^ 1];
		if (rowsOn) {
			const int ra = min(max(r0 - 1, cy0), cy1) * HS_RW, rb = min(max(r0, cy0), cy1) * HS_RW;
			float2 a0 = s[ra + xl], a1 = s[ra + lx], a2 = s[ra + xr];   // the row above
			float2 b0 = s[rb + xl], b1 = s[rb + lx], b2 = s[rb + xr];   // the pixel's row
#pragma unroll
			for (int j = 0; j < HS_P; j++) {
				const int row = r0 + j, rc = min(max(row + 1, cy0), cy1) * HS_RW;
				const float2 c0 = s[rc + xl], c1 = s[rc + lx], c2 = s[rc + xr];   // the row below
				if (row >= cy0 && row <= cy1) {
					const float u = 0.1666667f * (b0.x + b2.x + a1.x + c1.x) + 0.08333333f * (a0.x + a2.x + c0.x + c2.x);
					const float v = 0.1666667f * (b0.y + b2.y + a1.y + c1.y) + 0.08333333f * (a0.y + a2.y + c0.y + c2.y);
					const float r = (dx[j] * u + dy[j] * v + dt[j]) / den[j];
					d[row * HS_RW + lx] = make_float2(u - dx[j] * r, v - dy[j] * r);
				}
				a0 = b0; a1 = b1; a2 = b2;
				b0 = c0; b1 = c1; b2 = c2;
			}
		}
		__syncthreads();
	}
	// the tile proper, each lane the cells it wrote itself
	if (!colOn || lx < n || lx >= n + HS_TW) return;
	const float2* s = planes[n & 1];
	out += (long long)blockIdx.z * outImageStride + 2 * (long long)gx;
#pragma unroll
	for (int j = 0; j < HS_P; j++) {
		const int row = r0 + j;
		if (row < max(cy0, n) || row > min(cy1, n + HS_TH - 1)) continue;
		const float2 f = s[row * HS_RW + lx];
		float* o = out + (long long)(y0 + row) * outStride;
		o[0] = f.x;
		o[1] = f.y;
	}
}

int bhip_launch_hs_iterate(bhip_ctx* ctx, const float* deriv, const float* in, DevImg<float> out, float alpha2, int n) {
	if (n < 0 || n > HS_K) return bhip_fail(ctx, BHIP_ERR_INVALID, "Horn-Schunck: iterations per launch");
	const double px = (double)out.width * out.height * out.batch;
	const double halo = (double)(HS_TW + 2 * n) * (HS_TH + 2 * n) / (HS_TW * HS_TH);
	ProfScope prof(ctx, "k_hs_iterate", px * (halo * (12.0 + (in ? 8.0 : 0.0)) + 8.0), px * halo * n * 36.0);
	dim3 grid((out.width + HS_TW - 1) / HS_TW, (out.height + HS_TH - 1) / HS_TH, out.batch);
	hipLaunchKernelGGL(k_hs_iterate, grid, dim3(HS_THREADS), 0, ctx->stream, deriv, reinterpret_cast<const float2*>(in), out.data, out.imageStride, out.stride, out.width,
					   out.height, alpha2, n);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
