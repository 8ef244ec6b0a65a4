// Dense descriptors: a descriptor at every grid position of a frame.  FactoryDescribeImageDense.hog (both variants) and .sift.  All fp32 / fp64
// with the reference's types and evaluation order and no FMA contraction (build.py: -ffp-contract=off for every unit); every sum is taken in
// the reference's order by one lane, no atomics: two runs give the same bits.
//
// Reference:
//   DescribeDenseHogFastAlg.process / computeCellHistograms / computeDescriptor   F:alg/feature/dense/DescribeDenseHogFastAlg.java:80-215
//   DescribeDenseHogAlg.computePixelFeatures / process / computeCellHistogram / addToHistogram
//                                                                               F:alg/feature/dense/DescribeDenseHogAlg.java:179-339
//   DescribeDenseSiftAlg.process / precomputeAngles / computeDescriptor          F:alg/feature/dense/DescribeDenseSiftAlg.java:120-198
//   DescribeSiftCommon.trilinearInterpolation / normalizeDescriptor, UtilFeature.normalizeL2
//                                                                               F:alg/feature/describe/DescribeSiftCommon.java:84-131, F:alg/descriptor/UtilFeature.java:101-114
//   GradientThree, EXTENDED border: GrayF32 (a - b) * 0.5f; GrayU8 -> GrayS16 b - a (kernel -1 0 1, no divisor)
//                                                                               I:alg/filter/derivative/GradientThree.java:53-54,86-101, impl/GradientThree_Standard.java:40-89
// UtilAngle.atanSafe / domain2PI / dist are georegression's (not in the reference tree): restated from their contract, unpinned.
//
// Fast HOG, two launches.  k_dense_hog_cells: cells do not overlap, so a pixel's angle and magnitude are computed once, by the workgroup that
// owns a run of cells of one cell row: the lanes stage (index0, magnitude*(1-weight1), magnitude*weight1) of the run's pixels in LDS, then one
// lane per (cell, bin) walks its cell in raster order.  k_dense_hog_blocks: a workgroup gathers several blocks' cell histograms into LDS as
// doubles, one lane per descriptor takes each L2 sum in index order, all lanes scale, clip and write (the records of consecutive blocks are
// contiguous in the output).
// Standard HOG and dense SIFT: the windows overlap (9 blocks per pixel at the default step; 7 windows per pixel at period 6), so a per-pixel
// pre-pass stores what every window needs of a pixel -- the one atan / atan2 of the pixel among it -- in context scratch, and one workgroup
// per descriptor stages its window from there into LDS; one lane per descriptor element walks, in the reference's visiting order, the samples
// that can reach it.
#include "common.h"
#include "sift_dev.h"
#include <algorithm>

namespace {

constexpr int kDenseStage = 1024;   // pixels a standard-HOG workgroup stages at a time (whole cells; one cell of 32 x 32 at the most)

template <class T>
__device__ __forceinline__ float denseLoad(const T* p) { return (float)*p; }   // GrayU8: & 0xFF to float, exact

// GradientThree on clamped reads (EXTENDED).  S16: the GrayU8 -> GrayS16 gradient, read through getF
template <class T, bool S16>
__device__ __forceinline__ void denseGradient(const T* __restrict__ img, int S, int W, int H, int x, int y, float& dx, float& dy) {
	const int xl = max(x - 1, 0), xr = min(x + 1, W - 1), yt = max(y - 1, 0), yb = min(y + 1, H - 1);
	const T* row = img + (long long)y * S;
	if (S16) {
		dx = (float)((int)row[xr] - (int)row[xl]);
		dy = (float)((int)img[(long long)yb * S + x] - (int)img[(long long)yt * S + x]);
	} else {
		dx = (denseLoad(row + xr) - denseLoad(row + xl)) * 0.5f;
		dy = (denseLoad(img + (long long)yb * S + x) - denseLoad(img + (long long)yt * S + x)) * 0.5f;
	}
}

// UtilAngle.atanSafe(y, x) (float): x == 0 -> +-pi/2 by y >= 0, else (float)Math.atan(y / x) with the quotient in float
__device__ __forceinline__ float denseAtanSafe(float y, float x) {
	const float F_PId2 = (float)M_PI_2;
	if (x == 0.0f) return y >= 0.0f ? F_PId2 : -F_PId2;
	return (float)atan((double)(y / x));
}
// angle / angleBinSize of both HOG variants: angle from 0 to pi
__device__ __forceinline__ float hogFindex(float dx, float dy, float angleBinSize) {
	const float angle = denseAtanSafe(dy, dx) + (float)M_PI_2;
	return angle / angleBinSize;
}
// index0 = (int)findex0 % bins, weight1 = findex0 - (int)findex0.  A pixel that is not finite has no defined bin in the reference (it would
// index out of range); it goes to bin 0 here
__device__ __forceinline__ int hogIndex0(float findex0, int bins, float& weight1) {
	int index0 = (int)findex0;
	weight1 = findex0 - index0;
	index0 %= bins;
	return index0 < 0 ? 0 : index0;
}

__global__ void k_dense_count(int* __restrict__ count, int batch, int total) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b < batch) count[b] = total;
}

// grid (runs of cpw cells, cell rows, frames).  Dynamic LDS: [first float n | second float n | index0 int n], n = cpw * ppc^2
template <class T>
__global__ __launch_bounds__(256) void k_dense_hog_cells(const T* __restrict__ in, long long imageStride, int S, int W, int H, int bins, int ppc, int cellRows,
														   int cellCols, int cpw, float angleBinSize, float* __restrict__ cells) {
	extern __shared__ float sCell[];
	const int n = cpw * ppc * ppc;
	float *sFirst = sCell, *sSecond = sCell + n;
	int* sIndex = (int*)(sCell + 2 * n);
	const int t = threadIdx.x, c0 = blockIdx.x * cpw, row = blockIdx.y, b = blockIdx.z;
	const int nc = min(cpw, cellCols - c0), tw = nc * ppc, npx = tw * ppc;
	const T* img = in + (long long)b * imageStride;
	for (int p = t; p < npx; p += 256) {
		const int ly = p / tw, lx = p - ly * tw;
		float pixelDX, pixelDY;
		denseGradient<T, false>(img, S, W, H, c0 * ppc + lx, row * ppc + ly, pixelDX, pixelDY);
		const float magnitude = (float)sqrt((double)(pixelDX * pixelDX + pixelDY * pixelDY));
		float weight1;
		sIndex[p] = hogIndex0(hogFindex(pixelDX, pixelDY, angleBinSize), bins, weight1);
		sFirst[p] = magnitude * (1.0f - weight1);
		sSecond[p] = magnitude * weight1;
	}
	__syncthreads();
	for (int e = t; e < nc * bins; e += 256) {
		const int c = e / bins, bin = e - c * bins;
		float acc = 0;
		for (int k = 0; k < ppc; k++) {
			const int base = k * tw + c * ppc;
			for (int l = 0; l < ppc; l++) {
				const int index0 = sIndex[base + l], index1 = index0 + 1 == bins ? 0 : index0 + 1;
				if (index0 == bin) acc += sFirst[base + l];
				if (index1 == bin) acc += sSecond[base + l];
			}
		}
		cells[(((long long)b * cellRows + row) * cellCols + c0 + c) * bins + bin] = acc;
	}
}

// normalizeDescriptor on nd descriptors of `pitch` doubles each in LDS: one lane per descriptor sums in index order
__device__ void denseNormalizeMany(double* sD, double* sNorm, int nd, int dof, int pitch, double maxValue, int t, int nt) {
	for (int pass = 0; pass < 2; pass++) {
		__syncthreads();
		for (int d = t; d < nd; d += nt) {
			double norm = 0;
			for (int i = 0; i < dof; i++) {
				const double v = sD[d * pitch + i];
				norm += v * v;
			}
			sNorm[d] = norm;
		}
		__syncthreads();
		for (int idx = t; idx < nd * dof; idx += nt) {
			const int d = idx / dof, e = idx - d * dof;
			const double norm = sNorm[d];
			double v = sD[d * pitch + e];
			if (norm != 0) v = v / sqrt(norm);
			if (pass == 0 && v > maxValue) v = maxValue;
			sD[d * pitch + e] = v;
		}
	}
	__syncthreads();
}

// grid (groups of dpw blocks, frames).  Dynamic LDS: [descriptors double dpw * pitch | norms double dpw]
__global__ __launch_bounds__(256) void k_dense_hog_blocks(const float* __restrict__ cells, DenseHogParams P, int total, int dpw, int pitch, DenseOut out) {
	extern __shared__ double sBlock[];
	double* sNorm = sBlock + (size_t)dpw * pitch;
	const int t = threadIdx.x, b = blockIdx.y, k0 = blockIdx.x * dpw;
	const int nd = min(dpw, min(total, out.cap) - k0);
	if (nd <= 0) return;
	const int bins = P.orientationBins, dof = P.dof;
	const float* frame = cells + (long long)b * P.cellRows * P.cellCols * bins;
	for (int idx = t; idx < nd * dof; idx += 256) {
		const int d = idx / dof, e = idx - d * dof, k = k0 + d;
		const int by = k / P.numX, bx = k - by * P.numX;
		const int cell = e / bins, bin = e - cell * bins;
		const int i = cell / P.cellsPerBlockX, j = cell - i * P.cellsPerBlockX;
		sBlock[d * pitch + e] = frame[((long long)(by * P.stepBlock + i) * P.cellCols + bx * P.stepBlock + j) * bins + bin];
	}
	denseNormalizeMany(sBlock, sNorm, nd, dof, pitch, 0.2, t, 256);
	double* dst = out.desc + ((long long)b * out.cap + k0) * dof;
	for (int idx = t; idx < nd * dof; idx += 256) {
		const int d = idx / dof, e = idx - d * dof;
		dst[idx] = sBlock[d * pitch + e];
	}
	for (int d = t; d < nd; d += 256) {
		const int k = k0 + d, by = k / P.numX, bx = k - by * P.numX;
		int32_t* xy = out.xy + ((long long)b * out.cap + k) * 2;
		xy[0] = bx * P.stepBlock * P.pixelsPerCell;
		xy[1] = by * P.stepBlock * P.pixelsPerCell;
	}
}

template <class T>
__global__ __launch_bounds__(256) void k_dense_hog_pixels(const T* __restrict__ in, long long imageStride, int S, int W, int H, float angleBinSize,
															float* __restrict__ findex, float* __restrict__ sumsq) {
	const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
	if (x >= W) return;
	float dx, dy;
	denseGradient<T, false>(in + (long long)b * imageStride, S, W, H, x, y, dx, dy);
	const long long o = ((long long)b * H + y) * W + x;
	findex[o] = hogFindex(dx, dy, angleBinSize);
	sumsq[o] = dx * dx + dy * dy;
}

// normalizeDescriptor on the workgroup's one descriptor in LDS, then the record: L2, clip, L2; the sums in index order on one lane
template <int NT>
__device__ void denseNormalizeStore(double* sDesc, double* sNorm, int dof, double maxValue, double* __restrict__ dst, int t) {
	for (int pass = 0; pass < 2; pass++) {
		__syncthreads();
		if (t == 0) {
			double norm = 0;
			for (int i = 0; i < dof; i++) {
				const double v = sDesc[i];
				norm += v * v;
			}
			sNorm[0] = norm;
		}
		__syncthreads();
		const double norm = sNorm[0];
		const double root = sqrt(norm);
		for (int e = t; e < dof; e += NT) {
			double v = sDesc[e];
			if (norm != 0) v = v / root;
			if (pass == 0 && v > maxValue) v = maxValue;
			sDesc[e] = v;
		}
	}
	__syncthreads();
	for (int e = t; e < dof; e += NT) dst[e] = sDesc[e];
}

// grid (descriptors, frames), 128 lanes.  Dynamic LDS: [descriptor double dof | norm double 1 | spatial weights double 3 * 32 | magnitude double
// kDenseStage | oriWeight1 float kDenseStage | index0 int kDenseStage].  The cells of the block are staged in row-major order, as many whole
// cells at a time as fit; element (ty, tx, bin) takes, of every staged cell next to its own, the pixels in raster order
__global__ __launch_bounds__(128) void k_dense_hog_std(const float* __restrict__ findex, const float* __restrict__ sumsq, const double* __restrict__ weights, int W, int H,
														 DenseHogParams P, int total, int cellsPerStage, DenseOut out) {
	extern __shared__ double sStd[];
	const int bins = P.orientationBins, ppc = P.pixelsPerCell, cbx = P.cellsPerBlockX, cby = P.cellsPerBlockY, dof = P.dof;
	double* sDesc = sStd;
	double* sNorm = sDesc + dof;
	double* sSpatial = sNorm + 1;   // [3][32]: spatialWeight0 / 1 / 2 of a pixel offset inside its cell
	double* sMag = sSpatial + 96;
	float* sOri = (float*)(sMag + kDenseStage);
	int* sIndex = (int*)(sOri + kDenseStage);
	const int t = threadIdx.x, b = blockIdx.y, cellPixels = ppc * ppc, nCells = cbx * cby;
	if (t < ppc) {
		double w0, w1, w2;
		if (t <= ppc / 2) {
			w1 = (t + ppc / 2.0) / ppc;
			w0 = 1.0 - w1;
			w2 = 0;
		} else {
			w0 = 0;
			w2 = (t - ppc / 2.0) / ppc;
			w1 = 1.0 - w2;
		}
		sSpatial[t] = w0;
		sSpatial[32 + t] = w1;
		sSpatial[64 + t] = w2;
	}
	const int stepPixels = ppc * P.stepBlock, n = min(total, out.cap);
	const float* fi = findex + (long long)b * W * H;
	const float* ss = sumsq + (long long)b * W * H;
	for (int k = blockIdx.x; k < n; k += gridDim.x) {
		const int by = k / P.numX, bx = k - by * P.numX;
		const int x = bx * stepPixels, y = by * stepPixels;
		__syncthreads();   // the record before has been read out of LDS (and the spatial weights are there)
		for (int e = t; e < dof; e += 128) sDesc[e] = 0.0;
		for (int cell0 = 0; cell0 < nCells; cell0 += cellsPerStage) {
			const int nc = min(cellsPerStage, nCells - cell0);
			__syncthreads();   // the stage before has been walked
			for (int p = t; p < nc * cellPixels; p += 128) {
				const int c = p / cellPixels, r = p - c * cellPixels, i = r / ppc, j = r - i * ppc;
				const int cell = cell0 + c, cellY = cell / cbx, cellX = cell - cellY * cbx;
				const long long g = (long long)(y + cellY * ppc + i) * W + x + cellX * ppc + j;
				const int indexBlock = (cellY * ppc + i) * ppc * cbx + cellX * ppc + j;
				float oriWeight1;
				sIndex[p] = hogIndex0(fi[g], bins, oriWeight1);
				sOri[p] = oriWeight1;
				sMag[p] = sqrt((double)ss[g]) * weights[indexBlock];
			}
			__syncthreads();
			for (int e = t; e < dof; e += 128) {
				const int tcell = e / bins, bin = e - tcell * bins, ty = tcell / cbx, tx = tcell - ty * cbx;
				double acc = sDesc[e];
				for (int c = 0; c < nc; c++) {
					const int cell = cell0 + c, sy = cell / cbx, sx = cell - sy * cbx;
					const int a = tx - sx, d = ty - sy;   // addToHistogram(cellX + a, cellY + d, ...) reaches this element
					if (a < -1 || a > 1 || d < -1 || d > 1) continue;
					const double* spatialX = sSpatial + 32 * (a + 1);
					const double* spatialY = sSpatial + 32 * (d + 1);
					for (int i = 0; i < ppc; i++) {
						const double spatialWeightY = spatialY[i];
						if (spatialWeightY == 0) continue;   // the reference adds +0.0
						for (int j = 0; j < ppc; j++) {
							const double spatialWeightX = spatialX[j];
							if (spatialWeightX == 0) continue;
							const int p = c * cellPixels + i * ppc + j;
							const int index0 = sIndex[p], index1 = index0 + 1 == bins ? 0 : index0 + 1;
							const double oriWeight1 = sOri[p], magnitude = sMag[p];
							if (index0 == bin) acc += (1.0 - oriWeight1) * magnitude * spatialWeightX * spatialWeightY;
							if (index1 == bin) acc += oriWeight1 * magnitude * spatialWeightX * spatialWeightY;
						}
					}
				}
				sDesc[e] = acc;
			}
		}
		const long long o = (long long)b * out.cap + k;
		denseNormalizeStore<128>(sDesc, sNorm, dof, 0.2, out.desc + o * dof, t);
		if (t == 0) {
			out.xy[o * 2] = x;
			out.xy[o * 2 + 1] = y;
		}
	}
}

template <class T, bool S16>
__global__ __launch_bounds__(256) void k_dense_sift_pixels(const T* __restrict__ in, long long imageStride, int S, int W, int H, double* __restrict__ angle,
															 float* __restrict__ magnitude) {
	const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
	if (x >= W) return;
	float spacialDX, spacialDY;
	denseGradient<T, S16>(in + (long long)b * imageStride, S, W, H, x, y, spacialDX, spacialDY);
	const long long o = ((long long)b * H + y) * W + x;
	angle[o] = siftDomain2PI(siftAtan2((double)spacialDY, (double)spacialDX));
	magnitude[o] = (float)sqrt((double)(spacialDX * spacialDX + spacialDY * spacialDY));
}

// grid (descriptors, frames), 128 lanes.  FAST: the default grid (4, 4, 8) with its sizes as constants.  Dynamic LDS: [angle double ns | descriptor
// double dof | norm double 1 | weight float ns].  trilinearInterpolation turned inside out, as k_sift_describe does
template <bool FAST>
__global__ __launch_bounds__(128) void k_dense_sift(const double* __restrict__ angle, const float* __restrict__ magnitude, const float* __restrict__ gaussianWeight,
													  const double* __restrict__ binAngle, int W, int H, DenseSiftParams P, int total, DenseOut out) {
	extern __shared__ double sSift[];
	const int ws = FAST ? 4 : P.widthSubregion, wg = FAST ? 4 : P.widthGrid, nb = FAST ? 8 : P.numHistogramBins;
	const int sw = ws * wg, ns = sw * sw, dof = wg * wg * nb, radius = sw / 2;
	double* sAngle = sSift;
	double* sDesc = sSift + ns;
	double* sNorm = sDesc + dof;
	float* sW = (float*)(sNorm + 1);
	const int t = threadIdx.x, b = blockIdx.y, n = min(total, out.cap);
	const float fws = (float)ws;
	const double bw = P.histogramBinWidth;
	const double* ang = angle + (long long)b * W * H;
	const float* mag = magnitude + (long long)b * W * H;
	for (int k = blockIdx.x; k < n; k += gridDim.x) {
		const int gi = k / P.numX, gj = k - gi * P.numX;
		// (the host has checked that the products stay inside int, as they must in the reference)
		const int cy = P.spanY * gi / (P.numY - 1) + P.y0, cx = P.spanX * gj / (P.numX - 1) + P.x0;
		__syncthreads();   // the record before has been read out of LDS
		for (int smp = t; smp < ns; smp += 128) {
			const int i = smp / sw, j = smp - i * sw;
			const long long g = (long long)(cy - radius + i) * W + (cx - radius + j);
			sW[smp] = gaussianWeight[smp] * mag[g];
			sAngle[smp] = ang[g];
		}
		__syncthreads();
		for (int e = t; e < dof; e += 128) {
			const int kb = e % nb, ij = e / nb, j = ij % wg, i = ij / wg;
			const double angleBin = binAngle[kb];
			// a sample at or beyond widthSubregion * (i +- 1) has |sub - i| >= 1 (the float quotient is monotonic and exact there)
			const int sy0 = max(ws * (i - 1), 0), sy1 = min(ws * (i + 1), sw - 1);
			const int sx0 = max(ws * (j - 1), 0), sx1 = min(ws * (j + 1), sw - 1);
			double acc = 0;
			for (int sy = sy0; sy <= sy1; sy++) {
				const float subY = sy / fws;
				const double weightGridY = 1.0 - fabsf(subY - i);
				if (weightGridY <= 0) continue;
				for (int sx = sx0; sx <= sx1; sx++) {
					const float subX = sx / fws;
					const double weightGridX = 1.0 - fabsf(subX - j);
					if (weightGridX <= 0) continue;
					const double weightHistogram = 1.0 - siftAngleDist(sAngle[sy * sw + sx], angleBin) / bw;
					if (weightHistogram <= 0) continue;
					acc += sW[sy * sw + sx] * weightGridX * weightGridY * weightHistogram;
				}
			}
			sDesc[e] = acc;
		}
		const long long o = (long long)b * out.cap + k;
		denseNormalizeStore<128>(sDesc, sNorm, dof, P.maxDescriptorElementValue, out.desc + o * dof, t);
		if (t == 0) {
			out.xy[o * 2] = cx;
			out.xy[o * 2 + 1] = cy;
		}
	}
}

// rows in grid.y, frames in grid.z
bool denseGridOk(int rows, int batch) { return rows <= 65535 && batch <= 65535; }

}   // namespace

int bhip_launch_dense_count(bhip_ctx* ctx, int* count, int batch, int total) {
	if (batch <= 0) return BHIP_OK;
	ProfScope prof(ctx, "k_dense_count");
	hipLaunchKernelGGL(k_dense_count, dim3((batch + 255) / 256), dim3(256), 0, ctx->stream, count, batch, total);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

template <class T>
int bhip_launch_dense_hog_cells(bhip_ctx* ctx, DevImg<const T> in, const DenseHogParams& P, float* cells) {
	if (P.cellRows <= 0 || P.cellCols <= 0 || in.batch <= 0) return BHIP_OK;
	if (!denseGridOk(P.cellRows, in.batch)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "dense HOG on the GPU: at most 65535 cell rows and 65535 frames per call");
	const int ppc = P.pixelsPerCell;
	const int cpw = std::max(1, std::min(2048 / (ppc * ppc), P.cellCols));   // a run of at most 2048 pixels, 24 KiB of LDS: 32 cells of 8 x 8, 2 of 32 x 32
	const size_t lds = (size_t)cpw * ppc * ppc * 12;
	const float angleBinSize = (float)M_PI / P.orientationBins;   // GrlConstants.F_PI / orientationBins: float by int
	ProfScope prof(ctx, "k_dense_hog_cells");
	hipLaunchKernelGGL(k_dense_hog_cells<T>, dim3((P.cellCols + cpw - 1) / cpw, P.cellRows, in.batch), dim3(256), lds, ctx->stream, in.data, in.imageStride, in.stride,
					   in.width, in.height, P.orientationBins, ppc, P.cellRows, P.cellCols, cpw, angleBinSize, cells);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_dense_hog_cells<float>(bhip_ctx*, DevImg<const float>, const DenseHogParams&, float*);
template int bhip_launch_dense_hog_cells<uint8_t>(bhip_ctx*, DevImg<const uint8_t>, const DenseHogParams&, float*);

int bhip_launch_dense_hog_blocks(bhip_ctx* ctx, const DenseHogParams& P, const float* cells, int batch, DenseOut out) {
	const long long total = (long long)P.numX * P.numY;
	const int n = (int)std::min<long long>(total, out.cap);
	if (n <= 0 || batch <= 0) return BHIP_OK;
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "dense HOG on the GPU: at most 65535 frames per call");
	const int pitch = P.dof | 1;   // an odd number of doubles between the descriptors: the lanes of the L2 sums read different banks
	const int dpw = std::max(1, std::min(64, 4096 / pitch));
	const size_t lds = ((size_t)dpw * pitch + dpw) * 8;
	ProfScope prof(ctx, "k_dense_hog_blocks");
	hipLaunchKernelGGL(k_dense_hog_blocks, dim3((n + dpw - 1) / dpw, batch), dim3(256), lds, ctx->stream, cells, P, (int)total, dpw, pitch, out);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

template <class T>
int bhip_launch_dense_hog_pixels(bhip_ctx* ctx, DevImg<const T> in, int orientationBins, float* findex, float* sumsq) {
	if (in.batch <= 0) return BHIP_OK;
	if (!denseGridOk(in.height, in.batch)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "dense descriptors on the GPU: at most 65535 rows and 65535 frames per call");
	const float angleBinSize = (float)M_PI / orientationBins;
	ProfScope prof(ctx, "k_dense_hog_pixels");
	hipLaunchKernelGGL(k_dense_hog_pixels<T>, dim3((in.width + 255) / 256, in.height, in.batch), dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, in.width,
					   in.height, angleBinSize, findex, sumsq);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_dense_hog_pixels<float>(bhip_ctx*, DevImg<const float>, int, float*, float*);
template int bhip_launch_dense_hog_pixels<uint8_t>(bhip_ctx*, DevImg<const uint8_t>, int, float*, float*);

int bhip_launch_dense_hog_std(bhip_ctx* ctx, const DenseHogParams& P, const float* findex, const float* sumsq, const double* weights, int width, int height,
							  int batch, DenseOut out) {
	const long long total = (long long)P.numX * P.numY;
	const int n = (int)std::min<long long>(total, out.cap);
	if (n <= 0 || batch <= 0) return BHIP_OK;
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "dense HOG on the GPU: at most 65535 frames per call");
	const int cellsPerStage = std::max(1, kDenseStage / (P.pixelsPerCell * P.pixelsPerCell));
	const size_t lds = ((size_t)P.dof + 1 + 96) * 8 + (size_t)kDenseStage * 16;
	ProfScope prof(ctx, "k_dense_hog_std");
	hipLaunchKernelGGL(k_dense_hog_std, dim3(std::min(n, 1 << 20), batch), dim3(128), lds, ctx->stream, findex, sumsq, weights, width, height, P, (int)total,
					   cellsPerStage, out);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

template <class T>
int bhip_launch_dense_sift_pixels(bhip_ctx* ctx, DevImg<const T> in, double* angle, float* magnitude) {
	if (in.batch <= 0) return BHIP_OK;
	if (!denseGridOk(in.height, in.batch)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "dense descriptors on the GPU: at most 65535 rows and 65535 frames per call");
	ProfScope prof(ctx, "k_dense_sift_pixels");
	hipLaunchKernelGGL((k_dense_sift_pixels<T, std::is_same<T, uint8_t>::value>), dim3((in.width + 255) / 256, in.height, in.batch), dim3(256), 0, ctx->stream, in.data,
					   in.imageStride, in.stride, in.width, in.height, angle, magnitude);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_dense_sift_pixels<float>(bhip_ctx*, DevImg<const float>, double*, float*);
template int bhip_launch_dense_sift_pixels<uint8_t>(bhip_ctx*, DevImg<const uint8_t>, double*, float*);

int bhip_launch_dense_sift(bhip_ctx* ctx, const DenseSiftParams& P, const double* angle, const float* magnitude, const float* gaussianWeight, const double* binAngle,
						   int width, int height, int batch, DenseOut out) {
	const long long total = (long long)P.numX * P.numY;
	const int n = (int)std::min<long long>(total, out.cap);
	if (n <= 0 || batch <= 0) return BHIP_OK;
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "dense SIFT on the GPU: at most 65535 frames per call");
	const bool fast = P.widthSubregion == 4 && P.widthGrid == 4 && P.numHistogramBins == 8 && !bhip_env_flag("BHIP_DENSE_SIFT_GENERIC");
	const int sw = P.widthSubregion * P.widthGrid;
	const size_t lds = (size_t)sw * sw * 12 + (size_t)P.dof * 8 + 8;   // (the limits of boofhip.h keep it under 64 KiB)
	const dim3 grid(std::min(n, 1 << 20), batch);
	ProfScope prof(ctx, fast ? "k_dense_sift" : "k_dense_sift_generic");
	if (fast) hipLaunchKernelGGL(k_dense_sift<true>, grid, dim3(128), lds, ctx->stream, angle, magnitude, gaussianWeight, binAngle, width, height, P, (int)total, out);
	else hipLaunchKernelGGL(k_dense_sift<false>, grid, dim3(128), lds, ctx->stream, angle, magnitude, gaussianWeight, binAngle, width, height, P, (int)total, out);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
