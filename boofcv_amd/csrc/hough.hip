// ---------------------------------------------------------------------------------------------------------------
// Hough line detection on batches of device frames (F:alg/feature/detect/line/*.java, single-threaded forms):
//   binary polar vote     HoughTransformBinary.computeParameters :124-135 with HoughParametersPolar.parameterize(x,y,transform) :97-114
//   gradient foot vote    HoughTransformGradient.transform / parameterize / addParameters :184-213,238-252 with
//                         HoughParametersFootOfNorm.parameterize :76-85
//   relaxed block NMS     NonMaxBlock.process (F:alg/feature/detect/extract/NonMaxBlock.java:69-94) with NonMaxBlockSearchRelaxed.Max
//                         (NonMaxBlockSearchRelaxed.java:69-98, checkLocalMax :227-251)
//   mean-shift refinement MeanShiftPeak.search (F:alg/feature/detect/peak/MeanShiftPeak.java:103-160) on a GrayF32 with bilinear
//                         interpolation and the ZERO border (I:alg/interpolate/impl/ImplBilinearPixel_F32.java:48-90, BilinearPixelS.java:61-63)
//
// Binary vote.  Counts do not depend on the order of the pixels, so they are int32 atomics; the GrayF32 transform is their conversion
// (exact up to 2^24, which is what the entry point admits).  A workgroup owns HV_CHUNK * HV_ROUNDS consecutive pixels (raster index) and a slab
// of angle rows of the transform that fits LDS: HV_CHUNK pixels at a time it lists the foreground pixels, spreads (pixel, angle) pairs over
// its threads and counts in LDS; at the end it adds the non-zero cells to the global counts.  A transform row too long for an LDS slab is counted in global memory directly.
// The Java linear index i*stride + col is kept as it is: col == numBinsRange lands in the next row's first cell, col == -1 in the previous
// row's last one; an index outside the transform is dropped (Java throws ArrayIndexOutOfBoundsException there).
//
// Gradient vote.  A transform cell is the float sum of its contributions in the order the reference adds them: edge pixels in raster
// order, and the four cells of a pixel in the order (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1).  No float atomics: the edge pixels are
// ranked in raster order (a bitmap of the binary image and the popcount prefix of its words), pixel k writes its four (cell, weight) records
// to slots 4k .. 4k+3, a stable radix sort by cell (rocprim, the image in the key) gathers each cell's records in slot order, and the
// first record of each run sums the run with one lane.  `cap` edge pixels per image vote; the count that is returned may exceed it.
//
// Relaxed NMS.  With the relaxed rule a pixel is reported iff it is >= the threshold, != Float.MAX_VALUE and no pixel of its clipped
// (2r+1)^2 window is greater: its (r+1)^2 block lies inside that window, so such a pixel equals the block's running peak value and is in
// the block's list of equal maxima, and a pixel that fails has a greater one in its window or is below the peak.  All such pixels of a
// block are reported in raster order, the blocks in raster order: bit ((by*nbx+bx)*step + yInBlock)*step + xInBlock of a bitmap, ranked by
// the popcount prefix as for the strict rule.
// ---------------------------------------------------------------------------------------------------------------
#include "common.h"
#include <cfloat>
#include <rocprim/device/device_radix_sort.hpp>

// Java's (int) of a float: NaN -> 0, saturating
__device__ __forceinline__ int javaF2I(float v) {
	if (v != v) return 0;
	if (v >= 2147483648.0f) return 2147483647;
	if (v <= -2147483648.0f) return (-2147483647 - 1);
	return (int)v;
}
__device__ __forceinline__ int javaD2I(double v) {
	if (v != v) return 0;
	if (v >= 2147483648.0) return 2147483647;
	if (v <= -2147483648.0) return (-2147483647 - 1);
	return (int)v;
}

// ---------------- binary polar vote ----------------
#define HV_CHUNK 4096          // pixels listed at a time
#define HV_ROUNDS 16           // lists per workgroup: it owns HV_CHUNK * HV_ROUNDS consecutive pixels and clears / flushes its slab once
#define HV_LDS_CELLS 12288     // int32 cells of an LDS slab (48 KiB)
struct HoughBinaryParams {
	const uint8_t* bin;
	long long imageStride;
	int stride, width, height;
	const float* cosT;
	const float* sinT;
	int numBinsAngle, numBinsRange, slabRows, useLds;
	int originX, originY, w2;
	float rMax;
	int* counts;   // [batch][numBinsAngle * numBinsRange]
};
__global__ __launch_bounds__(256) void k_hough_binary_polar(HoughBinaryParams P) {
	extern __shared__ int slab[];
	__shared__ unsigned short px[HV_CHUNK];
	__shared__ int npx;
	const int tid = threadIdx.x;
	const int A = P.numBinsAngle, R = P.numBinsRange;
	const int a0 = blockIdx.y * P.slabRows, rows = min(P.slabRows, A - a0);
	const int slabCells = P.useLds ? rows * R : 0;
	const long long cells = (long long)A * R;
	const long long slabLo = (long long)a0 * R;
	const int total = P.width * P.height;   // <= 2^24
	const uint8_t* img = P.bin + (long long)blockIdx.z * P.imageStride;
	int* counts = P.counts + (long long)blockIdx.z * cells;
	for (int i = tid; i < slabCells; i += 256) slab[i] = 0;
	for (int round = 0; round < HV_ROUNDS; round++) {
		const int base = (blockIdx.x * HV_ROUNDS + round) * HV_CHUNK;
		if (base >= total) break;   // the same for every thread
		if (tid == 0) npx = 0;
		__syncthreads();
		for (int i = tid; i < HV_CHUNK; i += 256) {
			const int idx = base + i;
			if (idx >= total) break;
			const int y = idx / P.width, x = idx - y * P.width;
			if (img[(long long)y * P.stride + x] != 0) px[atomicAdd(&npx, 1)] = (unsigned short)i;
		}
		__syncthreads();
		const int n = npx;
		for (long long it = tid; it < (long long)n * rows; it += 256) {
			const int p = (int)(it / rows), a = a0 + (int)(it - (long long)p * rows);
			const int idx = base + px[p];
			const int yy = idx / P.width;
			const int x = idx - yy * P.width - P.originX, y = yy - P.originY;
			// double p = x*c[i] + y*s[i] (a float sum, widened); col = (int)Math.floor(p * w2 / r_max) + w2
			const float pf = (float)x * P.cosT[a] + (float)y * P.sinT[a];
			const int col = (int)((unsigned)javaD2I(floor((double)pf * (double)P.w2 / (double)P.rMax)) + (unsigned)P.w2);
			const long long index = (long long)a * R + col;
			if (index < 0 || index >= cells) continue;
			if (index >= slabLo && index < slabLo + slabCells) atomicAdd(&slab[index - slabLo], 1);
			else atomicAdd(&counts[index], 1);
		}
		__syncthreads();   // the list is rebuilt in the next round
	}
	__syncthreads();
	for (int i = tid; i < slabCells; i += 256) {
		const int v = slab[i];
		if (v) atomicAdd(&counts[slabLo + i], v);
	}
}
__global__ __launch_bounds__(256) void k_hough_counts_to_f32(const int* __restrict__ counts, int width, int height, float* __restrict__ out, long long outImageStride,
															  int outStride) {
	const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
	if (x >= width) return;
	out[(long long)blockIdx.z * outImageStride + (long long)y * outStride + x] = (float)counts[((long long)blockIdx.z * height + y) * width + x];
}

// counts: batch * numBinsAngle * numBinsRange ints of scratch; transform: numBinsRange wide, numBinsAngle high.  width * height <= 2^24,
// batch and numBinsAngle <= 65535 (checked by the caller)
int bhip_launch_hough_binary_polar(bhip_ctx* ctx, DevImg<const uint8_t> bin, const float* devCos, const float* devSin, int numBinsAngle, int numBinsRange, float rMax,
								   DevImg<float> transform, int* counts) {
	const int W = bin.width, H = bin.height, B = bin.batch;
	const size_t cells = (size_t)numBinsAngle * numBinsRange;
	BHIP_HIP(ctx, hipMemsetAsync(counts, 0, cells * B * sizeof(int), ctx->stream));
	HoughBinaryParams P{bin.data, bin.imageStride, bin.stride, W, H, devCos, devSin, numBinsAngle, numBinsRange, 0, 0, W / 2, H / 2, numBinsRange / 2, rMax, counts};
	P.useLds = numBinsRange <= HV_LDS_CELLS;
	P.slabRows = P.useLds ? std::min(numBinsAngle, HV_LDS_CELLS / numBinsRange) : numBinsAngle;
	const int slabs = (numBinsAngle + P.slabRows - 1) / P.slabRows;
	const int chunks = (W * H + HV_CHUNK * HV_ROUNDS - 1) / (HV_CHUNK * HV_ROUNDS);
	{
		ProfScope ps(ctx, "k_hough_binary_polar", (double)W * H * B * slabs + 8.0 * cells * B);
		hipLaunchKernelGGL(k_hough_binary_polar, dim3(chunks, slabs, B), dim3(256), P.useLds ? (size_t)P.slabRows * numBinsRange * sizeof(int) : 0, ctx->stream, P);
		hipLaunchKernelGGL(k_hough_counts_to_f32, dim3((numBinsRange + 255) / 256, numBinsAngle, B), dim3(256), 0, ctx->stream, counts, numBinsRange, numBinsAngle,
						   transform.data, transform.imageStride, transform.stride);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------- gradient vote ----------------
// The parameterisation of one edge pixel: (x, y) in the image, its derivatives as floats -> the point in transform space.  A template
// argument of the record kernel, so that another HoughTransformParameters drops in.
struct FootOfNorm {
	int originX, originY;
	__device__ __forceinline__ void parameterize(int x, int y, float derivX, float derivY, float& px, float& py) const {
		x -= originX;
		y -= originY;
		const float v = ((float)x * derivX + (float)y * derivY) / (derivX * derivX + derivY * derivY);
		px = v * derivX + (float)originX;
		py = v * derivY + (float)originY;
	}
};

// bit p of image b's bitmap: binary pixel p (raster index) is non-zero.  Every word is written.
__global__ __launch_bounds__(256) void k_hough_edge_bitmap(const uint8_t* __restrict__ bin, long long imageStride, int stride, int width, long long cells,
															unsigned int* __restrict__ bitmap, int words) {
	const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
	bool on = false;
	if (idx < cells) {
		const int y = (int)(idx / width), x = (int)(idx - (long long)y * width);
		on = bin[(long long)blockIdx.z * imageStride + (long long)y * stride + x] != 0;
	}
	const unsigned long long m = __ballot(on);
	const int lane = threadIdx.x & 63;
	const long long word = idx >> 5;
	if (word < words) {
		if (lane == 0) bitmap[(long long)blockIdx.z * words + word] = (unsigned int)m;
		if (lane == 32) bitmap[(long long)blockIdx.z * words + word] = (unsigned int)(m >> 32);
	}
}
template <class T, class Param>
__global__ __launch_bounds__(256) void k_hough_gradient_records(Param param, const T* __restrict__ dx, const T* __restrict__ dy, long long dImageStride, int dStride,
																 int width, int height, const unsigned int* __restrict__ bitmap,
																 const unsigned int* __restrict__ prefix, int words, int cap, unsigned int invalid,
																 unsigned int* __restrict__ keys, float* __restrict__ vals) {
	const long long cells = (long long)width * height;
	const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
	if (idx >= cells) return;
	const long long word = idx >> 5;
	const unsigned int bits = bitmap[(long long)blockIdx.z * words + word];
	const int bit = (int)(idx & 31);
	if (!((bits >> bit) & 1u)) return;
	const unsigned int rank = prefix[(long long)blockIdx.z * words + word] + __popc(bits & ((1u << bit) - 1u));
	if (rank >= (unsigned)cap) return;
	const int y = (int)(idx / width), x = (int)(idx - (long long)y * width);
	const long long di = (long long)blockIdx.z * dImageStride + (long long)y * dStride + x;
	float px, py;
	param.parameterize(x, y, (float)dx[di], (float)dy[di], px, py);
	const int x0 = javaF2I(px), y0 = javaF2I(py);
	const float wx = px - (float)x0, wy = py - (float)y0;
	const int x1 = (int)((unsigned)x0 + 1u), y1 = (int)((unsigned)y0 + 1u);   // Java's wrapping x0+1
	const int cx[4] = {x0, x1, x0, x1}, cy[4] = {y0, y0, y1, y1};
	const float w[4] = {(1.0f - wx) * (1.0f - wy), wx * (1.0f - wy), (1.0f - wx) * wy, wx * wy};
	const long long slot = ((long long)blockIdx.z * cap + rank) * 4;
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const bool in = cx[j] >= 0 && cx[j] < width && cy[j] >= 0 && cy[j] < height;   // GrayF32.isInBounds
		keys[slot + j] = in ? (unsigned int)(blockIdx.z * cells + (long long)cy[j] * width + cx[j]) : invalid;
		vals[slot + j] = w[j];
	}
}
// the first record of a run of equal keys sums the run in slot order, from 0 as the cleared transform does
__global__ __launch_bounds__(256) void k_hough_gradient_sum(const unsigned int* __restrict__ keys, const float* __restrict__ vals, long long n, unsigned int invalid,
															 int width, long long cells, float* __restrict__ out, long long outImageStride, int outStride) {
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const unsigned int key = keys[i];
	if (key == invalid || (i > 0 && keys[i - 1] == key)) return;
	float sum = 0.0f;
	for (long long j = i; j < n && keys[j] == key; j++) sum += vals[j];
	const long long img = key / cells, cell = key - img * cells;
	const int y = (int)(cell / width), x = (int)(cell - (long long)y * width);
	out[img * outImageStride + (long long)y * outStride + x] = sum;
}
__global__ __launch_bounds__(256) void k_hough_fill_f32(float* __restrict__ out, long long outImageStride, int outStride, int width, float value) {
	const int x = blockIdx.x * 256 + threadIdx.x;
	if (x < width) out[(long long)blockIdx.z * outImageStride + (long long)blockIdx.y * outStride + x] = value;
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct HoughGradientLayout {
	size_t bitmap, prefix, keysA, keysB, valsA, valsB, temp, tempBytes, total;
	int words;
	unsigned int invalid;
	int endBit;
};
// images * width * height must be below 2^32 - 1 (the image is part of the sort key)
static hipError_t houghGradientLayout(int width, int height, int images, int cap, HoughGradientLayout& L) {
	const long long cells = (long long)width * height;
	L.words = (int)((cells + 63) / 64) * 2;
	const size_t records = (size_t)images * cap * 4;
	L.invalid = (unsigned int)((long long)images * cells);
	L.endBit = 1;
	while (L.endBit < 32 && (L.invalid >> L.endBit)) L.endBit++;
	L.tempBytes = 0;
	const hipError_t e = rocprim::radix_sort_pairs(nullptr, L.tempBytes, (unsigned int*)nullptr, (unsigned int*)nullptr, (float*)nullptr, (float*)nullptr, records, 0,
												   (unsigned int)L.endBit, (hipStream_t) nullptr);
	size_t o = 0;
	L.bitmap = o; o += align256((size_t)images * L.words * 4);
	L.prefix = o; o += align256((size_t)images * L.words * 4);
	L.keysA = o; o += align256(records * 4);
	L.keysB = o; o += align256(records * 4);
	L.valsA = o; o += align256(records * 4);
	L.valsB = o; o += align256(records * 4);
	L.temp = o; o += align256(std::max<size_t>(L.tempBytes, 16));
	L.total = o;
	return e;
}
size_t bhip_hough_gradient_scratch(int width, int height, int images, int cap) {
	HoughGradientLayout L;
	if (houghGradientLayout(width, height, images, cap, L) != hipSuccess) return 0;
	return L.total;
}

// HoughTransformGradient.transform(derivX, derivY, binary) with HoughParametersFootOfNorm for the images of the views (at most 65535, and
// images * width * height < 2^32 - 1); scratch: bhip_hough_gradient_scratch(width, height, images, cap) bytes; devN[b]: edge pixels of image b
template <class T>
int bhip_launch_hough_gradient_foot(bhip_ctx* ctx, DevImg<const T> dx, DevImg<const T> dy, DevImg<const uint8_t> bin, DevImg<float> transform, int cap, int* devN,
									void* scratch) {
	const int W = bin.width, H = bin.height, B = bin.batch;
	if (dx.stride != dy.stride || dx.imageStride != dy.imageStride) return bhip_fail(ctx, BHIP_ERR_INVALID, "derivX and derivY must share one layout");
	const long long cells = (long long)W * H;
	HoughGradientLayout L;
	BHIP_HIP(ctx, houghGradientLayout(W, H, B, cap, L));
	char* s = (char*)scratch;
	unsigned int* bitmap = (unsigned int*)(s + L.bitmap);
	unsigned int* prefix = (unsigned int*)(s + L.prefix);
	unsigned int *keysA = (unsigned int*)(s + L.keysA), *keysB = (unsigned int*)(s + L.keysB);
	float *valsA = (float*)(s + L.valsA), *valsB = (float*)(s + L.valsB);
	const size_t records = (size_t)B * cap * 4;
	const unsigned int pixelBlocks = (unsigned int)((cells + 255) / 256);
	{
		ProfScope ps(ctx, "k_hough_gradient_rank", 1.0 * cells * B);
		hipLaunchKernelGGL(k_hough_edge_bitmap, dim3(pixelBlocks, 1, B), dim3(256), 0, ctx->stream, bin.data, bin.imageStride, bin.stride, W, cells, bitmap, L.words);
	}
	BHIP_HIP(ctx, hipGetLastError());
	BHIP_TRY(bhip_launch_word_prefix(ctx, bitmap, L.words, B, prefix, devN));
	{
		ProfScope ps(ctx, "k_hough_gradient_records", (2.0 * sizeof(T)) * cells * B);
		hipLaunchKernelGGL(k_hough_fill_f32, dim3((W + 255) / 256, H, B), dim3(256), 0, ctx->stream, transform.data, transform.imageStride, transform.stride, W, 0.0f);
		if (records > 0) {
			BHIP_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)keysA, (int)L.invalid, records, ctx->stream));
			hipLaunchKernelGGL((k_hough_gradient_records<T, FootOfNorm>), dim3(pixelBlocks, 1, B), dim3(256), 0, ctx->stream, FootOfNorm{W / 2, H / 2}, dx.data, dy.data,
							   dx.imageStride, dx.stride, W, H, bitmap, prefix, L.words, cap, L.invalid, keysA, valsA);
		}
	}
	BHIP_HIP(ctx, hipGetLastError());
	if (records == 0) return BHIP_OK;
	{
		ProfScope ps(ctx, "hough_gradient_sort", 16.0 * records);
		size_t tempBytes = L.tempBytes;
		BHIP_HIP(ctx, rocprim::radix_sort_pairs(s + L.temp, tempBytes, keysA, keysB, valsA, valsB, records, 0, (unsigned int)L.endBit, ctx->stream));
	}
	{
		ProfScope ps(ctx, "k_hough_gradient_sum", 8.0 * records);
		hipLaunchKernelGGL(k_hough_gradient_sum, dim3((unsigned int)((records + 255) / 256)), dim3(256), 0, ctx->stream, keysB, valsB, (long long)records, L.invalid, W,
						   cells, transform.data, transform.imageStride, transform.stride);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_hough_gradient_foot<float>(bhip_ctx*, DevImg<const float>, DevImg<const float>, DevImg<const uint8_t>, DevImg<float>, int, int*, void*);
template int bhip_launch_hough_gradient_foot<int16_t>(bhip_ctx*, DevImg<const int16_t>, DevImg<const int16_t>, DevImg<const uint8_t>, DevImg<float>, int, int*, void*);

// ---------------- relaxed block NMS ----------------
struct RelaxedParams {
	const float* img;
	long long imageStride;
	int stride, w, h, radius, border, nbx, words;
	float threshold;
	unsigned int* bitmap;   // [batch][words]
};
__global__ __launch_bounds__(256) void k_nonmax_relaxed(RelaxedParams P) {
	const int b = P.border, w = P.w, h = P.h, r = P.radius;
	const int x = b + blockIdx.x * 64 + (threadIdx.x & 63), y = b + blockIdx.y * 4 + (threadIdx.x >> 6);
	if (x >= w - b || y >= h - b) return;
	const float* img = P.img + (long long)blockIdx.z * P.imageStride;
	const float v = img[(long long)y * P.stride + x];
	if (!(v >= P.threshold) || v == FLT_MAX) return;
	const int x0 = max(x - r, 0), x1 = min(x + r, w - 1), y0 = max(y - r, 0), y1 = min(y + r, h - 1);
	bool peak = true;
	for (int j = y0; j <= y1; j++) {
		const float* row = img + (long long)j * P.stride;
		for (int i = x0; i <= x1; i++)
			if (row[i] > v) peak = false;
	}
	if (!peak) return;
	const int step = r + 1;
	const int bx = (x - b) / step, by = (y - b) / step;
	const unsigned int ord = (((unsigned)by * (unsigned)P.nbx + (unsigned)bx) * (unsigned)step + (unsigned)(y - b - by * step)) * (unsigned)step + (unsigned)(x - b - bx * step);
	atomicOr(&P.bitmap[(long long)blockIdx.z * P.words + (ord >> 5)], 1u << (ord & 31));
}
// bitmap: batch * words zeroed words, words > nbx * nby * (radius+1)^2 / 32; the region inside the border must not be empty
int bhip_launch_nonmax_relaxed(bhip_ctx* ctx, DevImg<const float> img, int radius, float threshold, int border, unsigned int* bitmap, int words, int nbx) {
	const int rw = img.width - 2 * border, rh = img.height - 2 * border;
	RelaxedParams P{img.data, img.imageStride, img.stride, img.width, img.height, radius, border, nbx, words, threshold, bitmap};
	{
		ProfScope ps(ctx, "k_nonmax_relaxed", 4.0 * img.width * img.height * img.batch);
		hipLaunchKernelGGL(k_nonmax_relaxed, dim3((rw + 63) / 64, (rh + 3) / 4, img.batch), dim3(256), 0, ctx->stream, P);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
__global__ __launch_bounds__(256) void k_relaxed_to_xy(const unsigned int* __restrict__ bitmap, const unsigned int* __restrict__ prefix, int words, int nbx, int step,
													   int border, int16_t* __restrict__ xy, int cap) {
	const int word = blockIdx.x * blockDim.x + threadIdx.x;
	if (word >= words) return;
	const long long img = blockIdx.y;
	unsigned int bits = bitmap[img * words + word];
	unsigned int rank = prefix[img * words + word];
	const unsigned int area = (unsigned)step * (unsigned)step;
	while (bits) {
		const int bit = __ffs(bits) - 1;
		bits &= bits - 1;
		const unsigned int ord = (unsigned)word * 32u + (unsigned)bit;
		const unsigned int block = ord / area, pos = ord - block * area;
		const int by = (int)(block / (unsigned)nbx), bx = (int)(block - (unsigned)by * (unsigned)nbx);
		if ((int)rank < cap) {
			xy[(img * cap + rank) * 2] = (int16_t)(border + bx * step + (int)(pos % (unsigned)step));
			xy[(img * cap + rank) * 2 + 1] = (int16_t)(border + by * step + (int)(pos / (unsigned)step));
		}
		rank++;
	}
}
int bhip_launch_relaxed_to_xy(bhip_ctx* ctx, const unsigned int* bitmap, const unsigned int* wordPrefix, int words, int nbx, int batch, int radius, int border,
							  int16_t* xy, int cap) {
	if (batch <= 0 || words <= 0 || cap <= 0) return BHIP_OK;
	{
		ProfScope ps(ctx, "k_relaxed_to_xy");
		hipLaunchKernelGGL(k_relaxed_to_xy, dim3((words + 255) / 256, batch), dim3(256), 0, ctx->stream, bitmap, wordPrefix, words, nbx, radius + 1, border, xy, cap);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------- mean-shift refinement of peaks ----------------
struct MeanShiftParams {
	const float* img;
	long long imageStride;
	int stride, w, h;
	const int16_t* xy;   // [batch][cap][2]
	const int* n;        // [batch]; nullptr: cap peaks in every image
	int cap, radius, maxIterations;
	float convergenceTol;
	const float* weights;   // (2*radius+1)^2, row-major
	float* peak;            // [batch][cap][2]
	float* intensity;       // [batch][cap]
};
// a pixel for the interpolation: the reference reads it unchecked inside the fast bounds; the guard only matters for NaN coordinates, where
// every product is NaN whatever is read
__device__ __forceinline__ float msPixel(const MeanShiftParams& P, const float* img, int x, int y) {
	return (x >= 0 && x < P.w && y >= 0 && y < P.h) ? img[(long long)y * P.stride + x] : 0.0f;
}
__device__ __forceinline__ float msGetFast(const MeanShiftParams& P, const float* img, float x, float y) {
	const int xt = javaF2I(x), yt = javaF2I(y);
	const float ax = x - (float)xt, ay = y - (float)yt;
	float val = (1.0f - ax) * (1.0f - ay) * msPixel(P, img, xt, yt);
	val += ax * (1.0f - ay) * msPixel(P, img, xt + 1, yt);
	val += ax * ay * msPixel(P, img, xt + 1, yt + 1);
	val += (1.0f - ax) * ay * msPixel(P, img, xt, yt + 1);
	return val;
}
// get_border with ImageBorderValue(0): floor instead of truncation, 0 outside
__device__ __forceinline__ float msGetBorder(const MeanShiftParams& P, const float* img, float x, float y) {
	const float xf = floorf(x), yf = floorf(y);
	const int xt = javaF2I(xf), yt = javaF2I(yf);
	const float ax = x - xf, ay = y - yf;
	const int xt1 = (int)((unsigned)xt + 1u), yt1 = (int)((unsigned)yt + 1u);
	float val = (1.0f - ax) * (1.0f - ay) * msPixel(P, img, xt, yt);
	val += ax * (1.0f - ay) * msPixel(P, img, xt1, yt);
	val += ax * ay * msPixel(P, img, xt1, yt1);
	val += (1.0f - ax) * ay * msPixel(P, img, xt, yt1);
	return val;
}
__device__ __forceinline__ bool msFastBounds(const MeanShiftParams& P, float x, float y) { return !(x < 0 || y < 0 || x > (float)(P.w - 2) || y > (float)(P.h - 2)); }
__global__ __launch_bounds__(64) void k_mean_shift_peak(MeanShiftParams P) {
	const int i = blockIdx.x * 64 + threadIdx.x;
	const long long b = blockIdx.y;
	const int n = P.n ? min(max(P.n[b], 0), P.cap) : P.cap;
	if (i >= n) return;
	const float* img = P.img + b * P.imageStride;
	const int ix = P.xy[(b * P.cap + i) * 2], iy = P.xy[(b * P.cap + i) * 2 + 1];
	float peakX = (float)ix, peakY = (float)iy;
	P.intensity[b * P.cap + i] = msPixel(P, img, ix, iy);
	if (P.radius > 0) {
		const int width = 2 * P.radius + 1;
		const float offset = (float)(-P.radius);
		for (int it = 0; it < P.maxIterations; it++) {
			float total = 0, sumX = 0, sumY = 0;
			int k = 0;
			const bool fast = msFastBounds(P, peakX + offset, peakY + offset) && msFastBounds(P, peakX - offset, peakY - offset);
			for (int yy = 0; yy < width; yy++) {
				const float y = offset + (float)yy;
				for (int xx = 0; xx < width; xx++) {
					const float x = offset + (float)xx;
					const float w = P.weights[k++];
					const float px = peakX + x, py = peakY + y;
					const float value = fast || msFastBounds(P, px, py) ? msGetFast(P, img, px, py) : msGetBorder(P, img, px, py);
					const float weight = w * value;
					total += weight;
					sumX += weight * x;
					sumY += weight * y;
				}
			}
			if (total == 0) break;
			const float cx = peakX + sumX / total, cy = peakY + sumY / total;
			const float dx = cx - peakX, dy = cy - peakY;
			peakX = cx;
			peakY = cy;
			if (fabsf(dx) < P.convergenceTol && fabsf(dy) < P.convergenceTol) break;
		}
	}
	P.peak[(b * P.cap + i) * 2] = peakX;
	P.peak[(b * P.cap + i) * 2 + 1] = peakY;
}
// weights: device table of (2*radius+1)^2 floats (unused when radius <= 0); n == nullptr: every image has cap peaks
int bhip_launch_mean_shift_peak(bhip_ctx* ctx, DevImg<const float> img, const int16_t* xy, const int* n, int cap, int radius, int maxIterations, float convergenceTol,
								const float* weights, float* peak, float* intensity) {
	if (img.batch <= 0 || cap <= 0) return BHIP_OK;
	MeanShiftParams P{img.data, img.imageStride, img.stride, img.width, img.height, xy, n, cap, radius, maxIterations, convergenceTol, weights, peak, intensity};
	{
		ProfScope ps(ctx, "k_mean_shift_peak");
		hipLaunchKernelGGL(k_mean_shift_peak, dim3((cap + 63) / 64, img.batch), dim3(64), 0, ctx->stream, P);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
