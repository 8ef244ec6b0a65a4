// FAST-9..12 corner detector on GrayU8 / GrayF32 frames: classification, score, ordered corner lists, early stop.
//
// Reference:
//   DiscretizedCircle.imageOffsets(3, stride)          I:misc/DiscretizedCircle.java:39-77  (the 16 ring offsets: DX / DY of k_fast)
//   ImplFastCorner{9,10,11,12}_{U8,F32}.checkPixel     F:alg/feature/detect/intensity/impl/  (generated decision trees)
//   ImplFastHelper_U8 / _F32 scoreLower, scoreUpper    F:alg/feature/detect/intensity/impl/ImplFastHelper_U8.java:47-81, ImplFastHelper_F32.java:47-81
//   FastCornerDetector.process                         F:alg/feature/detect/intensity/FastCornerDetector.java:123-189
//
// The decision trees are a read-saving search order for one predicate, which is what runs here: with lower = centre - tol and
// upper = centre + tol a pixel is a bright corner (+1) when minContinuous cyclically contiguous ring pixels are all > upper, a dark
// corner (-1) when they are all < lower (both cannot hold for minContinuous >= 9 and tol >= 0).  The score sums the ring pixels beyond
// the bound and subtracts centre * count; the F32 helper keeps that sum in an `int` (total += v truncates toward zero after every
// addition), so the sign of an F32 score does not tell the polarity and the class travels in bitmaps of its own.
//
// Three launches per batch, no host synchronisation:
//   k_fast        one pass over the frame: LDS tile + 3-pixel halo, class and score per pixel, float intensity (optional) and one
//                 bit per pixel in a "dark" and a "bright" bitmap whose rows are padded to whole words (a wave's ballot is the word);
//   k_fast_rows   corners per row (popcounts), their running totals and the row at which FastCornerDetector stops: the first interior
//                 row after which low.size + high.size >= (int)(maxFeaturesFraction * width * height); that row is kept whole;
//   k_fast_lists  raster-ordered (x,y) lists from the bitmaps: a corner's position is its row's running total + its rank in the row
//                 (popcounts, no atomics -- the order is part of the result); rows past the stop row emit nothing.
//
// Deviations from the reference (include/boofhip.h): a negative pixelTol is refused; the intensity image is written as a whole: 0 in the
// 3-pixel border and in the rows past the stop row (k_fast_lists zeroes those), where the reference leaves what an earlier frame put
// there.  That is what the reference produces with a freshly constructed detector.
#include "common.h"

#define FAST_TW 64   // tile width = one wave per row, so that a ballot is two bitmap words
#define FAST_TH 32   // tile rows (8 per wave); the 6 halo rows are 19 % of the rows staged

template <class T> struct FastPx;
template <> struct FastPx<uint8_t> { using V = FastTol<uint8_t>::type; static constexpr int PITCH = 76; };   // 64 + 6 pixels + up to 3 bytes of misalignment, whole dwords
template <> struct FastPx<float> { using V = FastTol<float>::type; static constexpr int PITCH = FAST_TW + 6; };

template <class T>
struct FastParams {
	const T* img;
	long long imageStride;
	int stride, w, h;
	float* inten;                // nullptr: process(image), no intensity image
	long long iImageStride;
	int iStride;
	typename FastPx<T>::V tol;
	int minContinuous;
	unsigned int* bmLow;         // [batch][h][rowWords]
	unsigned int* bmHigh;
	int rowWords;
};

// Java's (int) of a float: NaN -> 0, saturating
__device__ __forceinline__ int javaFloatToInt(float f) {
	if (f != f) return 0;
	if (f >= 2147483648.0f) return 2147483647;
	if (f <= -2147483648.0f) return -2147483647 - 1;
	return (int)f;
}

// One more ring pixel into a class mask: m = (m << 1) | beyond.  The masks therefore hold ring pixel k at bit 15 - k (a cyclic run is a cyclic
// run in either direction).  For the integer pixels the compare is the sign bit of a difference, shifted in by one funnel shift: the kernel
// is bound by its vector ALU work (16 x 2 class bits per pixel), so each bit costs two operations instead of compare + select + or.
__device__ __forceinline__ unsigned int pushBelow(unsigned int m, int a, int b) { return __funnelshift_l((unsigned int)(a - b), m, 1); }   // a < b; |a - b| < 2^31
__device__ __forceinline__ unsigned int pushBelow(unsigned int m, float a, float b) { return (m << 1) | (unsigned int)(a < b); }

// bit i of the result: ring pixels i .. i+n-1 (cyclic) are all set in the 16-bit mask m; 9 <= n <= 12
__device__ __forceinline__ unsigned int fastRuns(unsigned int m, int n) {
	unsigned int d = m | (m << 16);
	d &= d >> 1;
	d &= d >> 2;
	d &= d >> 4;          // runs of 8
	d &= d >> (n - 8);
	return d & 0xFFFFu;
}

template <class T>
__global__ __launch_bounds__(256) void k_fast(FastParams<T> P) {
	using V = typename FastPx<T>::V;
	constexpr int PITCH = FastPx<T>::PITCH;
	constexpr int DX[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
	constexpr int DY[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
	__shared__ __attribute__((aligned(16))) T tile[(FAST_TH + 6) * PITCH];
	const int w = P.w, h = P.h;
	const int x0 = blockIdx.x * FAST_TW, y0 = blockIdx.y * FAST_TH;
	const T* img = P.img + (long long)blockIdx.z * P.imageStride;
	// the part of the frame this tile reads: never a pixel outside the view
	const int xs = max(x0 - 3, 0), xe = min(x0 + FAST_TW + 3, w);
	const int ys = max(y0 - 3, 0), ye = min(y0 + FAST_TH + 3, h);
	const int len = xe - xs, rows = ye - ys;
	if constexpr (sizeof(T) == 1) {
		// A row segment starts at any byte address (sub-images have odd startIndex / stride).  It is staged as the aligned dwords that
		// cover it, at the same misalignment in LDS: a dword inside the segment is one load, the head and tail dwords are put together
		// from the bytes that belong to the segment.  Pixel x of tile row r is tile[r * PITCH + mis(r) + x - xs].
		constexpr int SLOTS = PITCH / 4;
		for (int s = threadIdx.x; s < rows * SLOTS; s += 256) {
			const int r = s / SLOTS, k = s - r * SLOTS;
			const uint8_t* a = img + (long long)(ys + r) * P.stride + xs;
			const int o = 4 * k - (int)((uintptr_t)a & 3);   // the slot's first byte, relative to the segment
			if (o >= len) continue;
			unsigned int v = 0;
			if (o >= 0 && o + 4 <= len) {
				v = *(const unsigned int*)(a + o);
			} else {
#pragma unroll
				for (int j = 0; j < 4; j++)
					if (o + j >= 0 && o + j < len) v |= (unsigned int)a[o + j] << (8 * j);
			}
			*(unsigned int*)&tile[r * PITCH + 4 * k] = v;
		}
	} else {
		for (int s = threadIdx.x; s < rows * len; s += 256) {
			const int r = s / len, c = s - r * len;
			tile[r * PITCH + c] = img[(long long)(ys + r) * P.stride + xs + c];
		}
	}
	__syncthreads();
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int x = x0 + lane;
	const int need = P.minContinuous >> 2;   // a run of n ring pixels holds at least n/4 of the four compass pixels
	// tile index of pixel (0, yy) (wave-uniform)
	auto rowBase = [&](int yy) -> int {
		int b = (yy - ys) * PITCH - xs;
		if constexpr (sizeof(T) == 1) b += (int)((uintptr_t)(img + (long long)yy * P.stride + xs) & 3);
		return b;
	};
	for (int i = 0; i < FAST_TH / 4; i++) {
		const int y = y0 + i * 4 + wave;
		if (y >= h) break;   // wave-uniform
		int cls = 0;
		float score = 0.0f;
		if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) {
			const T* rp[7];   // rp[d][i]: pixel (x - 3 + i, y - 3 + d); non-negative constant offsets fold into the LDS instructions
#pragma unroll
			for (int d = 0; d < 7; d++) rp[d] = tile + rowBase(y + d - 3) + (x - 3);
			const V c = (V)rp[3][3];
			const V lower = c - P.tol, upper = c + P.tol;
			V p[16];
			unsigned int cb = 0, cd = 0;   // the four compass pixels
#pragma unroll
			for (int k = 0; k < 16; k += 4) {
				p[k] = (V)rp[DY[k] + 3][DX[k] + 3];
				cb = pushBelow(cb, upper, p[k]);
				cd = pushBelow(cd, p[k], lower);
			}
			if (__popc(cb) >= need || __popc(cd) >= need) {
				unsigned int mb = 0, md = 0;
#pragma unroll
				for (int k = 0; k < 16; k++) {
					if (k & 3) p[k] = (V)rp[DY[k] + 3][DX[k] + 3];
					mb = pushBelow(mb, upper, p[k]);
					md = pushBelow(md, p[k], lower);
				}
				cls = fastRuns(mb, P.minContinuous) ? 1 : fastRuns(md, P.minContinuous) ? -1 : 0;
				if (cls != 0 && P.inten) {
					const unsigned int m = cls > 0 ? mb : md;   // ring pixel k at bit 15 - k
					const int count = __popc(m);
					if constexpr (sizeof(T) == 1) {
						int total = 0;
#pragma unroll
						for (int k = 0; k < 16; k++) total += __mul24((int)((m >> (15 - k)) & 1), p[k]);
						score = (float)(total - c * count);
					} else {
						int total = 0;   // the F32 helper's `int total; total += v;`, in ring order
#pragma unroll
						for (int k = 0; k < 16; k++)
							if ((m >> (15 - k)) & 1) total = javaFloatToInt((float)total + p[k]);
						score = (float)total - c * (float)count;
					}
				}
			}
		}
		const unsigned long long bd = __ballot(cls < 0), bb = __ballot(cls > 0);
		if (lane == 0) {
			const long long row = ((long long)blockIdx.z * h + y) * P.rowWords + (x0 >> 5);
			P.bmLow[row] = (unsigned int)bd;
			P.bmHigh[row] = (unsigned int)bb;
			if ((x0 >> 5) + 1 < P.rowWords) {
				P.bmLow[row + 1] = (unsigned int)(bd >> 32);
				P.bmHigh[row + 1] = (unsigned int)(bb >> 32);
			}
		}
		if (P.inten && x < w) P.inten[(long long)blockIdx.z * P.iImageStride + (long long)y * P.iStride + x] = score;
	}
}

// One workgroup per image.  rowLow / rowHigh [batch][h]: corners of each polarity in rows 0 .. y (inclusive running totals);
// stop[batch]: the last row FastCornerDetector processes; nLow / nHigh[batch]: the list lengths
__global__ __launch_bounds__(1024) void k_fast_rows(const unsigned int* __restrict__ bmLow, const unsigned int* __restrict__ bmHigh, int rowWords, int h,
													 int maxFeatures, int* rowLow, int* rowHigh, int* __restrict__ stop, int* __restrict__ nLow,
													 int* __restrict__ nHigh) {
	__shared__ int waveLow[16], waveHigh[16];
	__shared__ int carryLow, carryHigh, stopRow;
	const int img = blockIdx.x;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int* rl = rowLow + (long long)img * h;
	int* rh = rowHigh + (long long)img * h;
	for (int y = wave; y < h; y += 16) {
		const long long row = ((long long)img * h + y) * rowWords;
		int cl = 0, ch = 0;
		for (int k = lane; k < rowWords; k += 64) {
			cl += __popc(bmLow[row + k]);
			ch += __popc(bmHigh[row + k]);
		}
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			cl += __shfl_xor(cl, o, 64);
			ch += __shfl_xor(ch, o, 64);
		}
		if (lane == 0) { rl[y] = cl; rh[y] = ch; }
	}
	if (threadIdx.x == 0) { carryLow = 0; carryHigh = 0; stopRow = max(h - 4, 0); }
	__syncthreads();
	for (int base = 0; base < h; base += 1024) {
		const int y = base + threadIdx.x;
		int sl = y < h ? rl[y] : 0, sh = y < h ? rh[y] : 0;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const int tl = __shfl_up(sl, o, 64), th = __shfl_up(sh, o, 64);
			if (lane >= o) { sl += tl; sh += th; }
		}
		if (lane == 63) { waveLow[wave] = sl; waveHigh[wave] = sh; }
		__syncthreads();
		int ol = carryLow, oh = carryHigh;
		for (int k = 0; k < wave; k++) { ol += waveLow[k]; oh += waveHigh[k]; }
		sl += ol;
		sh += oh;
		if (y < h) {
			rl[y] = sl;
			rh[y] = sh;
			// FastCornerDetector.java:152-154, after each interior row
			if (y >= 3 && y < h - 3 && sl + sh >= maxFeatures) atomicMin(&stopRow, y);
		}
		__syncthreads();
		if (threadIdx.x == 1023) { carryLow = sl; carryHigh = sh; }
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		const int s = stopRow;
		stop[img] = s;
		nLow[img] = rl[s];
		nHigh[img] = rh[s];
	}
}

// one wave per (row, polarity): the row's corners in x order at the row's running total; a row past the stop row clears its intensity
__global__ __launch_bounds__(256) void k_fast_lists(const unsigned int* __restrict__ bmLow, const unsigned int* __restrict__ bmHigh, int rowWords, int w, int h,
													 const int* __restrict__ rowLow, const int* __restrict__ rowHigh, const int* __restrict__ stop,
													 int16_t* __restrict__ xyLow, int16_t* __restrict__ xyHigh, int cap, float* __restrict__ inten,
													 long long iImageStride, int iStride) {
	const int lane = threadIdx.x & 63;
	const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
	const int high = blockIdx.y;
	const long long img = blockIdx.z;
	if (y >= h) return;
	if (y > stop[img]) {
		if (!high && inten && y < h - 3)
			for (int x = 3 + lane; x < w - 3; x += 64) inten[img * iImageStride + (long long)y * iStride + x] = 0.0f;
		return;
	}
	const int* inc = (high ? rowHigh : rowLow) + img * h;
	int base = y > 0 ? inc[y - 1] : 0;
	if (inc[y] == base) return;
	const unsigned int* bm = (high ? bmHigh : bmLow) + (img * h + y) * rowWords;
	int16_t* xy = (high ? xyHigh : xyLow) + img * cap * 2;
	for (int k0 = 0; k0 < rowWords; k0 += 64) {
		const int k = k0 + lane;
		unsigned int bits = k < rowWords ? bm[k] : 0u;
		const int c = __popc(bits);
		int s = c;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const int t = __shfl_up(s, o, 64);
			if (lane >= o) s += t;
		}
		int rank = base + s - c;
		while (bits) {
			const int bit = __ffs(bits) - 1;
			bits &= bits - 1;
			if (rank < cap) {
				xy[2 * (long long)rank] = (int16_t)(k * 32 + bit);
				xy[2 * (long long)rank + 1] = (int16_t)y;
			}
			rank++;
		}
		base += __shfl(s, 63, 64);
	}
}

static inline int fastRowWords(int width) { return (width + 31) / 32; }

// device scratch of one bhip_launch_fast call: two bitmaps, two row tables, the stop rows
size_t bhip_fast_scratch(int width, int height, int batch) {
	return ((size_t)2 * fastRowWords(width) * height + 2 * (size_t)height + 1) * 4 * batch;
}

template <class T>
int bhip_launch_fast(bhip_ctx* ctx, DevImg<const T> img, typename FastTol<T>::type tol, int minContinuous, int maxFeatures, DevImg<float> inten, void* scratch,
					 int16_t* xyLow, int* nLow, int16_t* xyHigh, int* nHigh, int cap) {
	const int w = img.width, h = img.height, batch = img.batch;
	if (batch <= 0 || w <= 0 || h <= 0) return BHIP_OK;
	if constexpr (sizeof(T) == 1) tol = tol < 256 ? tol : 256;   // no two GrayU8 pixels differ by more: the same (empty) result, and centre + tol cannot overflow
	const int rowWords = fastRowWords(w);
	const size_t bmWords = (size_t)rowWords * h * batch;
	unsigned int* bmLow = (unsigned int*)scratch;
	unsigned int* bmHigh = bmLow + bmWords;
	int* rowLow = (int*)(bmHigh + bmWords);
	int* rowHigh = rowLow + (size_t)h * batch;
	int* stop = rowHigh + (size_t)h * batch;
	FastParams<T> P{img.data, img.imageStride, img.stride, w, h, inten.data, inten.imageStride, inten.stride, tol, minContinuous, bmLow, bmHigh, rowWords};
	const double px = (double)w * h * batch;
	{
		ProfScope ps(ctx, sizeof(T) == 1 ? "k_fast_u8" : "k_fast_f32", (sizeof(T) + (inten.data ? 4.0 : 0.0) + 0.25) * px);
		hipLaunchKernelGGL(k_fast<T>, dim3((w + FAST_TW - 1) / FAST_TW, (h + FAST_TH - 1) / FAST_TH, batch), dim3(256), 0, ctx->stream, P);
	}
	{
		ProfScope ps(ctx, "k_fast_rows", 0.25 * px + 16.0 * h * batch);   // both bitmaps read, the row tables written and read
		hipLaunchKernelGGL(k_fast_rows, dim3(batch), dim3(1024), 0, ctx->stream, bmLow, bmHigh, rowWords, h, maxFeatures, rowLow, rowHigh, stop, nLow, nHigh);
	}
	{
		ProfScope ps(ctx, "k_fast_lists", 0.25 * px + 16.0 * h * batch);   // at most: bitmaps and row tables read (+ 4 B per corner, + the cleared rows)
		hipLaunchKernelGGL(k_fast_lists, dim3((h + 3) / 4, 2, batch), dim3(256), 0, ctx->stream, bmLow, bmHigh, rowWords, w, h, rowLow, rowHigh, stop, xyLow, xyHigh,
						   cap, inten.data, inten.imageStride, inten.stride);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_fast(bhip_ctx*, DevImg<const uint8_t>, int, int, int, DevImg<float>, void*, int16_t*, int*, int16_t*, int*, int);
template int bhip_launch_fast(bhip_ctx*, DevImg<const float>, float, int, int, DevImg<float>, void*, int16_t*, int*, int16_t*, int*, int);
