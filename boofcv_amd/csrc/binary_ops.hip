// ---------------------------------------------------------------------------------------------------------------
// BinaryImageOps on GrayU8 0/1 images (I:alg/filter/binary/BinaryImageOps.java), batched, any row / image stride, any byte alignment:
//   logicAnd / logicOr / logicXor / invert                    :69-145  over impl/ImplBinaryImageOps.java:30-93
//   erode4 / dilate4 / erode8 / dilate8 (numTimes)            :158-361 over impl/ImplBinaryInnerOps.java and impl/ImplBinaryBorderOps.java
//   edge4 / edge8 (outsideZero), removePointNoise             :258-411 over the same two files
//   relabel, labelToBinary                                    :509-557 over impl/ImplBinaryImageOps.java:95-149
// The labelled image of BinaryImageOps.contour is in label.hip.  Not provided: thin (BinaryThinning), the contour point lists,
// labelToClusters / clusterToBinary, image types other than GrayU8 / GrayS32.
//
// Only the width x height pixels of an output view are stored.  Parity with the reference holds for images of 0 and 1; other byte values
// give an unspecified result inside the view (the reference sums raw signed bytes in its inner loops and unsigned get() values on the
// frame; here every byte is unsigned).
//
// The neighbourhood rule of a pixel.  The reference runs an inner loop over 1 <= x < width-1, 1 <= y < height-1 and then border loops: for
// every x the top pixel, then the bottom pixel; then for every y the left pixel, then the right pixel.  A frame pixel therefore keeps what
// the LAST of those writes gave it: the right-column form where x == width-1, else the left-column form where x == 0, else the bottom-row
// form where y == height-1, else the top-row form.  (Width or height 1 and 2 have no inner pixels and fall out of the same order.)  Each
// border form sums the operation's 3x3 cells WITHOUT the row or column on its own outward side, reads every other cell outside the image as
// the operation's outside value (ImageBorderValue), and compares with the number of cells it summed.  So a pixel is: a mask of 3x3 cells =
// the operation's cells minus one outward line, a sum over it with the outside value, and the operation's test.  For erode4 this is not
// "pad with a constant": a top-row pixel ignores the cell above it but a corner still reads one cell outside, which is 0.
// ---------------------------------------------------------------------------------------------------------------
#include "common.h"
#include <algorithm>

// ---- streaming forms: 16 pixels of a row per lane as four 32-bit words (threshold.hip's lane shape), single bytes at the right edge ----
// 0x01 in every byte of w that is zero
__device__ __forceinline__ uint32_t zeroBytes(uint32_t w) {
	return (~(((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w | 0x7f7f7f7fu)) >> 7;
}
__device__ __forceinline__ uint32_t oneBytes(uint32_t w) { return zeroBytes(w ^ 0x01010101u); }   // 0x01 where the byte is 1
#define LOGIC_INVERT 3   // after BHIP_LOGIC_AND / _OR / _XOR: the one-input form
// ImplBinaryImageOps: and = (a == 1 && a == b), or = (a == 1 || b == 1), xor = (a != b), invert = (a == 0)
__device__ __forceinline__ uint32_t logicWord(int op, uint32_t a, uint32_t b) {
	switch (op) {
	case BHIP_LOGIC_AND: return oneBytes(a) & oneBytes(b);
	case BHIP_LOGIC_OR: return oneBytes(a) | oneBytes(b);
	case BHIP_LOGIC_XOR: return zeroBytes(a ^ b) ^ 0x01010101u;
	default: return zeroBytes(a);   // LOGIC_INVERT
	}
}
// in-place is allowed: a lane reads its 16 bytes of a row before it writes them, and no other lane touches them
__global__ __launch_bounds__(256) void k_binary_logic(int op, const uint8_t* a, long long aImageStride, int aStride, const uint8_t* b, long long bImageStride, int bStride,
													  uint8_t* out, long long outImageStride, int outStride, int width, int height) {
	const int x = (blockIdx.x * 256 + threadIdx.x) * 16;
	if (x >= width) return;
	const int n = width - x;
	const uint8_t* pa = a + (long long)blockIdx.z * aImageStride + x;
	const uint8_t* pb = b + (long long)blockIdx.z * bImageStride + x;
	uint8_t* po = out + (long long)blockIdx.z * outImageStride + x;
	for (int y = blockIdx.y; y < height; y += gridDim.y) {
		const uint8_t* ra = pa + (long long)y * aStride;
		const uint8_t* rb = pb + (long long)y * bStride;
		uint8_t* ro = po + (long long)y * outStride;
		if (n >= 16) {
			uint32_t wa[4], wb[4], wo[4];
			__builtin_memcpy(wa, ra, 16);
			__builtin_memcpy(wb, rb, 16);
#pragma unroll
			for (int j = 0; j < 4; j++) wo[j] = logicWord(op, wa[j], wb[j]);
			__builtin_memcpy(ro, wo, 16);
		} else {
			for (int j = 0; j < n; j++) ro[j] = (uint8_t)(logicWord(op, ra[j], rb[j]) & 1u);
		}
	}
}
// op: BHIP_LOGIC_*; b == nullptr: invert(a)
int bhip_launch_binary_logic(bhip_ctx* ctx, int op, DevImg<const uint8_t> a, const DevImg<const uint8_t>* b, DevImg<uint8_t> out) {
	ProfScope prof(ctx, b ? "k_binary_logic" : "k_binary_invert", (b ? 3.0 : 2.0) * a.width * a.height * a.batch);
	const DevImg<const uint8_t> bb = b ? *b : a;
	dim3 grid((a.width + 4095) / 4096, std::min(a.height, 1024), a.batch);
	hipLaunchKernelGGL(k_binary_logic, grid, dim3(256), 0, ctx->stream, b ? op : LOGIC_INVERT, a.data, a.imageStride, a.stride, bb.data, bb.imageStride, bb.stride,
					   out.data, out.imageStride, out.stride, a.width, a.height);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Neighbourhood operations.  A workgroup owns a BM_W x BM_H tile of the output and applies n <= BHIP_MORPH_FUSED_MAX iterations inside LDS:
// it stages the tile with an n-pixel halo, and iteration i recomputes the tile with an (n - i)-pixel halo from the previous buffer into the
// other one.  Cells outside the image hold the operation's outside value in BOTH buffers from the start and are never recomputed, so they
// are that constant at every iteration, as in n separate passes.  LDS: 2 x (BM_H + 2K) x (BM_W + 2K) bytes = 5760 at K = 4.
// ---------------------------------------------------------------------------------------------------------------
#define BM_W 64
#define BM_H 32
#define BM_K BHIP_MORPH_FUSED_MAX
#define BM_PITCH (BM_W + 2 * BM_K)
#define BM_ROWS (BM_H + 2 * BM_K)
enum { MORPH_ALL = 0, MORPH_ANY = 1, MORPH_EDGE = 2, MORPH_NOISE = 3 };
struct MorphRule {
	int mask;        // 3x3 cells summed by the inner form: bit (dy+1)*3 + (dx+1)
	int kind;        // MORPH_*
	int outside;     // value of a cell outside the image
	int frameCopy;   // edge with outsideZero: the frame is a copy of the input (edge_outside0)
};
// one pixel (gx, gy) of the image from the 3x3 cells around t[0] (row pitch BM_PITCH)
__device__ __forceinline__ int morphPixel(const MorphRule& r, const uint8_t* t, int gx, int gy, int width, int height) {
	int m = r.mask;
	bool frame = true;
	if (gx == width - 1) m &= ~0x124;        // right column: without dx = +1
	else if (gx == 0) m &= ~0x049;           // left column: without dx = -1
	else if (gy == height - 1) m &= ~0x1c0;  // bottom row: without dy = +1
	else if (gy == 0) m &= ~0x007;           // top row: without dy = -1
	else frame = false;
	const int c = t[0];
	if (frame && r.frameCopy) return c;
	int sum = 0;
	if (!frame) {   // the mask is the kernel argument: which cells are read is decided once for the wave
#pragma unroll
		for (int b = 0; b < 9; b++)
			if ((r.mask >> b) & 1) sum += t[(b / 3 - 1) * BM_PITCH + (b % 3 - 1)];
	} else {
#pragma unroll
		for (int b = 0; b < 9; b++)
			if ((m >> b) & 1) sum += t[(b / 3 - 1) * BM_PITCH + (b % 3 - 1)];
	}
	const int cnt = __popc(m);
	switch (r.kind) {
	case MORPH_ALL: return sum == cnt ? 1 : 0;
	case MORPH_ANY: return sum > 0 ? 1 : 0;
	case MORPH_EDGE: return sum == cnt ? 0 : c;
	default: return sum < 2 ? 0 : (!frame && sum > 6) ? 1 : c;   // removePointNoise: the frame forms have no "> 6" branch
	}
}
__global__ __launch_bounds__(256) void k_binary_morph(const uint8_t* __restrict__ in, long long inImageStride, int inStride, uint8_t* __restrict__ out,
													  long long outImageStride, int outStride, int width, int height, MorphRule r, int n) {
	__shared__ __attribute__((aligned(16))) uint8_t buf[2][BM_ROWS * BM_PITCH];
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * BM_W - n, y0 = blockIdx.y * BM_H - n;   // image position of LDS cell (0, 0)
	const int cols = BM_W + 2 * n, rows = BM_H + 2 * n;
	const uint8_t* src = in + (long long)blockIdx.z * inImageStride;
	// staging: four cells of a row per lane and step, walked over the constant pitch (a multiple of 4, so LDS words are aligned; global
	// memory takes the unaligned 4-byte load).  Cells between `cols` and the pitch are filled too and never read.
	const uint32_t outside4 = 0x01010101u * (uint32_t)r.outside;
	for (int i = tid; i < rows * (BM_PITCH / 4); i += 256) {
		const int ly = i / (BM_PITCH / 4), lx = (i - ly * (BM_PITCH / 4)) * 4;
		const int gx = x0 + lx, gy = y0 + ly;
		uint32_t w = outside4;
		bool allInside = false;
		if (gy >= 0 && gy < height && gx + 3 >= 0 && gx < width) {
			const uint8_t* p = src + (long long)gy * inStride + gx;
			if (gx >= 0 && gx + 3 < width) {
				__builtin_memcpy(&w, p, 4);
				allInside = true;
			} else {
#pragma unroll
				for (int j = 0; j < 4; j++)
					if (gx + j >= 0 && gx + j < width) w = (w & ~(0xffu << (8 * j))) | ((uint32_t)p[j] << (8 * j));
			}
		}
		*reinterpret_cast<uint32_t*>(&buf[0][ly * BM_PITCH + lx]) = w;
		if (!allInside) *reinterpret_cast<uint32_t*>(&buf[1][ly * BM_PITCH + lx]) = w;   // its cells inside the image are recomputed before they are read
	}
	__syncthreads();
	int cur = 0;
	for (int it = 1; it <= n; it++) {
		for (int i = it * BM_PITCH + tid; i < (rows - it) * BM_PITCH; i += 256) {
			const int ly = i / BM_PITCH, lx = i - ly * BM_PITCH;
			if (lx < it || lx >= cols - it) continue;
			const int gx = x0 + lx, gy = y0 + ly;
			if (gx < 0 || gx >= width || gy < 0 || gy >= height) continue;
			buf[cur ^ 1][ly * BM_PITCH + lx] = (uint8_t)morphPixel(r, &buf[cur][ly * BM_PITCH + lx], gx, gy, width, height);
		}
		__syncthreads();
		cur ^= 1;
	}
	uint8_t* dst = out + (long long)blockIdx.z * outImageStride;
	for (int i = tid; i < BM_W / 4 * BM_H; i += 256) {   // four pixels of a row per lane
		const int ly = i / (BM_W / 4), lx = (i - ly * (BM_W / 4)) * 4;
		const int gx = x0 + n + lx, gy = y0 + n + ly;
		if (gx >= width || gy >= height) continue;
		const uint8_t* t = &buf[cur][(ly + n) * BM_PITCH + lx + n];
		uint8_t* q = dst + (long long)gy * outStride + gx;
		if (gx + 3 < width) {
			const uint32_t w = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
			__builtin_memcpy(q, &w, 4);
		} else
			for (int j = 0; gx + j < width; j++) q[j] = t[j];
	}
}
static int morphRule(int op, int outsideZero, MorphRule& r) {
	switch (op) {
	case BHIP_MORPH_ERODE4: r = {0x0ba, MORPH_ALL, 0, 0}; return BHIP_OK;
	case BHIP_MORPH_DILATE4: r = {0x0ba, MORPH_ANY, 0, 0}; return BHIP_OK;
	case BHIP_MORPH_ERODE8: r = {0x1ff, MORPH_ALL, 1, 0}; return BHIP_OK;
	case BHIP_MORPH_DILATE8: r = {0x1ff, MORPH_ANY, 0, 0}; return BHIP_OK;
	case BHIP_MORPH_EDGE4: r = {0x0aa, MORPH_EDGE, 1, outsideZero ? 1 : 0}; return BHIP_OK;
	case BHIP_MORPH_EDGE8: r = {0x1ef, MORPH_EDGE, 1, outsideZero ? 1 : 0}; return BHIP_OK;
	case BHIP_MORPH_REMOVE_POINT_NOISE: r = {0x1ef, MORPH_NOISE, 0, 0}; return BHIP_OK;
	}
	return BHIP_ERR_INVALID;
}
// n iterations of `op` (BHIP_MORPH_*), 1 <= n <= BHIP_MORPH_FUSED_MAX, in one launch; in and out must not overlap
int bhip_launch_binary_morph(bhip_ctx* ctx, int op, int outsideZero, int n, DevImg<const uint8_t> in, DevImg<uint8_t> out) {
	MorphRule r;
	if (morphRule(op, outsideZero, r) != BHIP_OK || n < 1 || n > BM_K) return bhip_fail(ctx, BHIP_ERR_INVALID, "binary neighbourhood operation");
	const double halo = (double)(BM_W + 2 * n) * (BM_H + 2 * n) / (BM_W * BM_H);
	ProfScope prof(ctx, "k_binary_morph", (1.0 + halo) * in.width * in.height * in.batch);
	dim3 grid((in.width + BM_W - 1) / BM_W, (in.height + BM_H - 1) / BM_H, in.batch);
	hipLaunchKernelGGL(k_binary_morph, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width, in.height,
					   r, n);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Label utilities.  relabel: labels[] indexed by the pixel; a pixel outside [0, numLabels) stays as it is (the reference throws there).
// labelToBinary: pixel != 0, or selected[pixel] (a pixel outside [0, numSelected) gives 0).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_relabel(int32_t* img, long long imageStride, int stride, int width, int height, const int* __restrict__ labels, int numLabels) {
	const int x = blockIdx.x * 256 + threadIdx.x;
	if (x >= width) return;
	int32_t* p = img + (long long)blockIdx.z * imageStride + x;
	for (int y = blockIdx.y; y < height; y += gridDim.y) {
		const int v = p[(long long)y * stride];
		if (v >= 0 && v < numLabels) p[(long long)y * stride] = labels[v];
	}
}
int bhip_launch_relabel(bhip_ctx* ctx, DevImg<int32_t> img, const int* devLabels, int numLabels) {
	ProfScope prof(ctx, "k_relabel", 8.0 * img.width * img.height * img.batch);
	dim3 grid((img.width + 255) / 256, std::min(img.height, 1024), img.batch);
	hipLaunchKernelGGL(k_relabel, grid, dim3(256), 0, ctx->stream, img.data, img.imageStride, img.stride, img.width, img.height, devLabels, numLabels);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
__global__ __launch_bounds__(256) void k_label_to_binary(const int32_t* __restrict__ in, long long inImageStride, int inStride, uint8_t* __restrict__ out,
														 long long outImageStride, int outStride, int width, int height, const uint8_t* __restrict__ selected,
														 int numSelected) {
	const int x = blockIdx.x * 256 + threadIdx.x;
	if (x >= width) return;
	const int32_t* p = in + (long long)blockIdx.z * inImageStride + x;
	uint8_t* q = out + (long long)blockIdx.z * outImageStride + x;
	for (int y = blockIdx.y; y < height; y += gridDim.y) {
		const int v = p[(long long)y * inStride];
		q[(long long)y * outStride] = selected ? (uint8_t)(v >= 0 && v < numSelected && selected[v] ? 1 : 0) : (uint8_t)(v != 0 ? 1 : 0);
	}
}
int bhip_launch_label_to_binary(bhip_ctx* ctx, DevImg<const int32_t> in, DevImg<uint8_t> out, const uint8_t* devSelected, int numSelected) {
	ProfScope prof(ctx, "k_label_to_binary", 5.0 * in.width * in.height * in.batch);
	dim3 grid((in.width + 255) / 256, std::min(in.height, 1024), in.batch);
	hipLaunchKernelGGL(k_label_to_binary, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width, in.height,
					   devSelected, numSelected);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
