// SIFT orientation and description: the second half of CompleteSift.  All fp32 / fp64 with the reference's evaluation order and no FMA
// contraction (build.py: -ffp-contract=off for every unit); everything discrete -- a sample's histogram bin, a sample's pixel, the peaks,
// the number of angles -- is decided with the reference's own expressions, and every sum is taken in the reference's order.
//
// Reference:
//   CompleteSift.detectFeatures / handleDetection                 F:alg/feature/detdesc/CompleteSift.java:97-134
//   OrientationHistogramSift.process / computeHistogram / findHistogramPeaks / computeAngle / interpolateAngle / computeWeight
//                                                                 F:alg/feature/orientation/OrientationHistogramSift.java:135-309
//     InterpolateArray.interpolate                                F:numerics/InterpolateArray.java:37-48
//     FastHessianFeatureDetector.polyPeak(double)                 F:alg/feature/detect/interest/FastHessianFeatureDetector.java:352-366
//     CircularIndex.addOffset                                     I:misc/CircularIndex.java:64-71
//   DescribePointSift.computeRawDescriptor                        F:alg/feature/describe/DescribePointSift.java:118-165
//   DescribeSiftCommon.trilinearInterpolation / normalizeDescriptor, UtilFeature.normalizeL2
//                                                                 F:alg/feature/describe/DescribeSiftCommon.java:84-131, F:alg/descriptor/UtilFeature.java:101-114
//   GradientThree (FactoryDerivative.three(GrayF32, null): EXTENDED border)
//                                                                 I:alg/filter/derivative/impl/GradientThree_Standard.java:40-62,
//                                                                 I:alg/filter/derivative/DerivativeHelperFunctions.java:140-172
// UtilAngle.domain2PI / dist / bound are georegression's (not in the reference tree): restated from their contract, unpinned.
//
// The gradient is not stored: both kernels evaluate (a - b) * 0.5f on clamped reads of scale image j.  Inside the image that is
// GradientThree_Standard's expression; on the frame the reference forms 0 + a*(-0.5f) + c*0 + b*0.5f (the generic border convolution, or the
// unrolled three taps on the second row / column) over the EXTENDED image, and for finite pixels the two are the same float: the halves
// are exact, so both round a - b once, and both give +0 for a == b.
//
// k_sift_orient, one 256-lane workgroup per detection: the clipped (2r+1)^2 window is walked in chunks of 256 samples in raster order.  The
// lanes compute a chunk's samples in parallel (bin, magnitude*weight, dx*weight, dy*weight, all double) into LDS; then one lane per
// histogram entry (3 * histogramSize of them: magnitude, X, Y) walks the chunk in order and adds the samples of its bin -- the
// reference's ordered sum, bit for bit, whatever r is (no size limit, one form).  Lane 0 then runs findHistogramPeaks and computeAngle.
// k_sift_describe, one workgroup per (detection, angle): the lanes stage the (widthGrid*widthSubregion)^2 samples (float weight, double
// angle) in LDS; one lane per descriptor element walks, in raster order, the samples that can reach its cell ((2*widthSubregion-1)^2 at the
// most) and adds their trilinear shares; lane 0 takes the two L2 sums in index order.  No atomics anywhere: two runs give the same bits.
#include "common.h"
#include "sift_dev.h"
#include <algorithm>

#define SIFT_EXP_TABLE BHIP_CSIFT_EXP_TABLE

// UtilAngle.bound: to [-pi, pi]
__device__ __forceinline__ double siftBound(double a) {
	a = fmod(a, 2.0 * M_PI);
	if (a > M_PI) return a - 2.0 * M_PI;
	if (a < -M_PI) return a + 2.0 * M_PI;
	return a;
}
// FastHessianFeatureDetector.polyPeak(double)
__device__ __forceinline__ double siftPolyPeakF64(double lower, double middle, double upper) {
	const double a = 0.5 * lower - middle + 0.5 * upper;
	const double b = 0.5 * upper - 0.5 * lower;
	if (a == 0.0) return 0.0;
	return -b / (2.0 * a);
}

// computeAngle / interpolateAngle on the three histograms (mag, X, Y: hs entries each)
__device__ double siftComputeAngle(const double* mag, const double* hx, const double* hy, int hs, int index1) {
	const int index0 = index1 - 1 < 0 ? hs + index1 - 1 : (index1 - 1) % hs;
	const int index2 = (index1 + 1) % hs;
	const double offset = siftPolyPeakF64(mag[index0], mag[index1], mag[index2]);
	const double angle1 = siftAtan2(hy[index1], hx[index1]);
	double deltaAngle;
	if (offset < 0) deltaAngle = siftAngleDist(siftAtan2(hy[index0], hx[index0]), angle1);
	else deltaAngle = siftAngleDist(siftAtan2(hy[index2], hx[index2]), angle1);
	return siftBound(angle1 + deltaAngle * offset);
}

// phase 0: every detection; writes nAngles and the first BHIP_CSIFT_ANGLE_SLOTS angles into the detection's slot.
// phase 1 (after the scan): only the detections with more angles than slots; the histogram is formed again and the remaining angles go
// straight to the output records behind count[b] + angleOffset
__global__ __launch_bounds__(256) void k_sift_orient(SiftDescParams P, int phase) {
	__shared__ double sExp[SIFT_EXP_TABLE];
	__shared__ double sHist[3 * BHIP_CSIFT_MAX_HISTOGRAM];
	__shared__ double sVal[3][256];
	__shared__ int sBin[256];
	__shared__ int sPeaks[BHIP_CSIFT_MAX_HISTOGRAM / 2];
	const int b = blockIdx.y, t = threadIdx.x, hs = P.histogramSize;
	const int W = P.width, H = P.height, S = P.stride;
	if (t < SIFT_EXP_TABLE) sExp[t] = P.expTable[t];
	const int n = min(P.detN[b], P.detCap);
	const float* img = P.image + (long long)b * P.imageStride;
	for (int d = blockIdx.x; d < n; d += gridDim.x) {
		const long long o = (long long)b * P.detCap + d;
		if (phase == 1 && P.nAngles[o] <= BHIP_CSIFT_ANGLE_SLOTS) continue;
		__syncthreads();   // the table is staged; the histogram of the detection before has been read
		for (int k = t; k < 3 * hs; k += 256) sHist[k] = 0.0;
		// handleDetection: into the octave's pixels
		const double localX = P.detX[o] / P.pixelScaleToInput, localY = P.detY[o] / P.pixelScaleToInput, sigma = P.detScale[o] / P.pixelScaleToInput;
		const int cx = (int)(localX + 0.5), cy = (int)(localY + 0.5);
		// r beyond the image clips to the whole image whatever its value: 65536 stands for everything larger
		const int r = (int)fmin(ceil(sigma * P.sigmaEnlarge), 65536.0);
		const int x0 = max(cx - r, 0), y0 = max(cy - r, 0), x1 = min(cx + r + 1, W), y1 = min(cy + r + 1, H);
		const int nw = max(x1 - x0, 0), nh = max(y1 - y0, 0);
		const int total = nw * nh;
		const double sigma2 = sigma * sigma;
		for (int base = 0; base < total; base += 256) {
			const int s = base + t;
			if (s < total) {
				const int yy = s / nw, y = y0 + yy, x = x0 + (s - yy * nw);
				float dx, dy;
				siftGradient(img, S, W, H, x, y, dx, dy);
				const double magnitude = sqrt((double)(dx * dx + dy * dy));
				const double theta = siftDomain2PI(siftAtan2((double)dy, (double)dx));
				// computeWeight
				const double deltaX = x - cx, deltaY = y - cy;
				const double dd = ((deltaX * deltaX + deltaY * deltaY) / sigma2) / 0.1;
				double weight = 0;
				if (!(dd < 0)) {
					const int index = (int)dd;
					if (index < SIFT_EXP_TABLE - 1) {
						const double w = dd - index;
						weight = sExp[index] * (1.0 - w) + sExp[index + 1] * w;
					}
				}
				sBin[t] = (int)(theta / P.histAngleBin) % hs;
				sVal[0][t] = magnitude * weight;
				sVal[1][t] = dx * weight;
				sVal[2][t] = dy * weight;
			}
			__syncthreads();
			const int cnt = min(256, total - base);
			for (int k = t; k < 3 * hs; k += 256) {
				const int which = k / hs, bin = k - which * hs;
				double acc = sHist[k];
				for (int i = 0; i < cnt; i++)
					if (sBin[i] == bin) acc += sVal[which][i];
				sHist[k] = acc;
			}
			__syncthreads();
		}
		__syncthreads();
		if (t == 0) {
			const double *mag = sHist, *hx = sHist + hs, *hy = sHist + 2 * hs;
			// findHistogramPeaks
			int np = 0, largestIndex = -1;
			double largest = 0;
			double before = mag[hs - 2], current = mag[hs - 1];
			for (int i = 0; i < hs; i++) {
				const double after = mag[i];
				if (current > before && current > after) {
					const int currentIndex = i - 1 < 0 ? hs + i - 1 : (i - 1) % hs;
					sPeaks[np++] = currentIndex;
					if (current > largest) { largest = current; largestIndex = currentIndex; }
				}
				before = current;
				current = after;
			}
			int na = 0;
			if (largestIndex >= 0) {
				const double threshold = largest * 0.8;
				for (int i = 0; i < np; i++) {
					const int index = sPeaks[i];
					if (mag[index] >= threshold) {
						if (phase == 0) {
							if (na < BHIP_CSIFT_ANGLE_SLOTS) P.angles[o * BHIP_CSIFT_ANGLE_SLOTS + na] = siftComputeAngle(mag, hx, hy, hs, index);
						} else if (na >= BHIP_CSIFT_ANGLE_SLOTS) {
							const long long slot = (long long)P.count[b] + P.angleOffset[o] + na;
							if (slot < P.cap) P.orientation[(long long)b * P.cap + slot] = siftComputeAngle(mag, hx, hy, hs, index);
						}
						na++;
					}
				}
			}
			if (phase == 0) P.nAngles[o] = na;
		}
	}
}

// exclusive scan of a frame's angle counts in detection order: one workgroup per frame, 256 detections per step
__global__ __launch_bounds__(256) void k_sift_angle_scan(const int* __restrict__ nAngles, const int* __restrict__ detN, int detCap, int* __restrict__ angleOffset,
														 int* __restrict__ nFeat) {
	__shared__ int sWave[4];
	const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int n = min(detN[b], detCap);
	int carry = 0;
	for (int base = 0; base < n; base += 256) {
		const int i = base + t;
		const int v = i < n ? nAngles[(long long)b * detCap + i] : 0;
		int s = v;
#pragma unroll
		for (int off = 1; off < 64; off <<= 1) {
			const int u = __shfl_up(s, off, 64);
			if (lane >= off) s += u;
		}
		if (lane == 63) sWave[wave] = s;
		__syncthreads();
		int before = 0, all = 0;
#pragma unroll
		for (int w = 0; w < 4; w++) {
			if (w < wave) before += sWave[w];
			all += sWave[w];
		}
		if (i < n) angleOffset[(long long)b * detCap + i] = carry + before + s - v;
		carry += all;
		__syncthreads();
	}
	if (t == 0) nFeat[b] = carry;
}

// the records of the slice are behind count[b]; afterwards the count moves on and the slice's detection count is cleared for the next slice
__global__ void k_sift_desc_advance(int* __restrict__ count, const int* __restrict__ nFeat, int* __restrict__ detN, int batch) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b < batch) {
		count[b] += nFeat[b];
		detN[b] = 0;
	}
}

// FAST: the default grid (4, 4, 8) with its sizes as constants; otherwise any widthSubregion, widthGrid, numHistogramBins within the limits of
// boofhip.h.  Dynamic LDS: [angle double ns | descriptor double dof | norm double 1 | weight float ns]
template <bool FAST>
__global__ __launch_bounds__(256) void k_sift_describe(SiftDescParams P) {
	extern __shared__ double sDyn[];
	const int ws = FAST ? 4 : P.widthSubregion, wg = FAST ? 4 : P.widthGrid, nb = FAST ? 8 : P.numHistogramBins;
	const int sw = ws * wg, ns = sw * sw, dof = wg * wg * nb;
	double* sAngle = sDyn;
	double* sDesc = sDyn + ns;
	double* sNorm = sDesc + dof;
	float* sW = (float*)(sNorm + 1);
	const int b = blockIdx.y, t = threadIdx.x;
	const int W = P.width, H = P.height, S = P.stride;
	const int n = min(P.detN[b], P.detCap);
	const float* img = P.image + (long long)b * P.imageStride;
	const float fws = (float)ws;
	const double sampleRadius = sw / 2;
	const double bw = P.histogramBinWidth, maxValue = P.maxDescriptorElementValue;
	for (int d = blockIdx.x; d < n; d += gridDim.x) {
		const long long o = (long long)b * P.detCap + d;
		const int na = P.nAngles[o];
		const long long first = (long long)P.count[b] + P.angleOffset[o];
		const double localX = P.detX[o] / P.pixelScaleToInput, localY = P.detY[o] / P.pixelScaleToInput, sigma = P.detScale[o] / P.pixelScaleToInput;
		const double sampleToPixels = sigma * P.sigmaToPixels;
		for (int a = 0; a < na; a++) {
			const long long slot = first + a;
			if (slot >= P.cap) break;   // only the first cap records are written
			const long long oo = (long long)b * P.cap + slot;
			const double orientation = a < BHIP_CSIFT_ANGLE_SLOTS ? P.angles[o * BHIP_CSIFT_ANGLE_SLOTS + a] : P.orientation[oo];
			const double c = cos(orientation), s = sin(orientation);
			__syncthreads();   // the record before has been read out of LDS
			// computeRawDescriptor: the samples
			for (int smp = t; smp < ns; smp += 256) {
				const int sampleY = smp / sw, sampleX = smp - sampleY * sw;
				const double y = sampleToPixels * (sampleY - sampleRadius);
				const double x = sampleToPixels * (sampleX - sampleRadius);
				// (int) truncates toward zero: a coordinate in (-1, 0) reads pixel 0, as in the reference
				const int pixelX = (int)(x * c - y * s + localX + 0.5);
				const int pixelY = (int)(x * s + y * c + localY + 0.5);
				float weight = -1.0f;   // outside the image: skipped
				double angle = 0;
				if (pixelX >= 0 && pixelX < W && pixelY >= 0 && pixelY < H) {
					float spacialDX, spacialDY;
					siftGradient(img, S, W, H, pixelX, pixelY, spacialDX, spacialDY);
					const double adjDX = c * spacialDX + s * spacialDY;
					const double adjDY = -s * spacialDX + c * spacialDY;
					angle = siftDomain2PI(siftAtan2(adjDY, adjDX));
					const float weightGaussian = P.gaussianWeight[smp];
					const float weightGradient = (float)sqrt((double)(spacialDX * spacialDX + spacialDY * spacialDY));
					weight = weightGaussian * weightGradient;
				}
				sW[smp] = weight;
				sAngle[smp] = angle;
			}
			__syncthreads();
			// trilinearInterpolation, turned inside out: element (i, j, k) takes its samples in raster order
			for (int e = t; e < dof; e += 256) {
				const int k = e % nb, ij = e / nb, j = ij % wg, i = ij / wg;
				const double angleBin = P.binAngle[k];
				// a sample at or beyond widthSubregion * (i +- 1) has |sub - i| >= 1 (the float quotient is monotonic and exact there)
				const int sy0 = max(ws * (i - 1), 0), sy1 = min(ws * (i + 1), sw - 1);
				const int sx0 = max(ws * (j - 1), 0), sx1 = min(ws * (j + 1), sw - 1);
				double acc = 0;
				for (int sy = sy0; sy <= sy1; sy++) {
					const float subY = sy / fws;
					const double weightGridY = 1.0 - fabsf(subY - i);
					if (weightGridY <= 0) continue;
					for (int sx = sx0; sx <= sx1; sx++) {
						const float weight = sW[sy * sw + sx];
						if (weight < 0.0f) continue;
						const float subX = sx / fws;
						const double weightGridX = 1.0 - fabsf(subX - j);
						if (weightGridX <= 0) continue;
						const double weightHistogram = 1.0 - siftAngleDist(sAngle[sy * sw + sx], angleBin) / bw;
						if (weightHistogram <= 0) continue;
						acc += weight * weightGridX * weightGridY * weightHistogram;
					}
				}
				sDesc[e] = acc;
			}
			// normalizeDescriptor: L2, clip, L2; the sums in index order on one lane
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
				if (norm != 0) {
					const double root = sqrt(norm);
					for (int e = t; e < dof; e += 256) {
						double v = sDesc[e] / root;
						if (pass == 0 && v > maxValue) v = maxValue;
						sDesc[e] = v;
					}
				} else if (pass == 0) {
					for (int e = t; e < dof; e += 256)
						if (sDesc[e] > maxValue) sDesc[e] = maxValue;
				}
			}
			__syncthreads();
			for (int e = t; e < dof; e += 256) P.desc[oo * dof + e] = sDesc[e];
			if (t == 0) {
				P.x[oo] = P.detX[o];
				P.y[oo] = P.detY[o];
				P.scale[oo] = P.detScale[o];
				P.white[oo] = P.detWhite[o];
				P.orientation[oo] = orientation;
			}
		}
	}
}

int bhip_launch_sift_describe(bhip_ctx* ctx, const SiftDescParams& P, bool generic) {
	if (P.batch <= 0 || P.detCap <= 0) return BHIP_OK;
	if (P.batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "SIFT on the GPU: at most 65535 frames per call");
	const bool fast = !generic && P.widthSubregion == 4 && P.widthGrid == 4 && P.numHistogramBins == 8;
	const int sw = P.widthSubregion * P.widthGrid;
	const size_t lds = (size_t)sw * sw * 12 + (size_t)P.dof * 8 + 8;   // (the limits of boofhip.h keep it under 64 KiB)
	if (P.histogramSize < 3 || P.histogramSize > BHIP_CSIFT_MAX_HISTOGRAM || lds > 64 * 1024) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "SIFT describe: beyond the kernels' LDS");
	const dim3 grid(std::min(P.detCap, 1024), P.batch);
	{
		ProfScope prof(ctx, "k_sift_orient");
		hipLaunchKernelGGL(k_sift_orient, grid, dim3(256), 0, ctx->stream, P, 0);
	}
	{
		ProfScope prof(ctx, "k_sift_angle_scan");
		hipLaunchKernelGGL(k_sift_angle_scan, dim3(P.batch), dim3(256), 0, ctx->stream, P.nAngles, P.detN, P.detCap, P.angleOffset, P.nFeat);
	}
	{
		ProfScope prof(ctx, "k_sift_orient_more");
		hipLaunchKernelGGL(k_sift_orient, grid, dim3(256), 0, ctx->stream, P, 1);
	}
	{
		ProfScope prof(ctx, fast ? "k_sift_describe" : "k_sift_describe_generic");
		if (fast) hipLaunchKernelGGL(k_sift_describe<true>, grid, dim3(256), lds, ctx->stream, P);
		else hipLaunchKernelGGL(k_sift_describe<false>, grid, dim3(256), lds, ctx->stream, P);
		hipLaunchKernelGGL(k_sift_desc_advance, dim3((P.batch + 255) / 256), dim3(256), 0, ctx->stream, P.count, P.nFeat, P.detN, P.batch);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
