// C ABI, dense descriptors (kernels: dense.hip): DescribeImageDenseHoG over DescribeDenseHogFastAlg / DescribeDenseHogAlg and DescribeImageDenseSift
// over DescribeDenseSiftAlg, of FactoryDescribeImageDense.hog / .sift.  Rules, deviations and limits: the bhip_dense_* section of include/boofhip.h.
#include "cabi.h"
#include <climits>

namespace {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr size_t kDenseScratch = (size_t)256 << 20;   // per-pixel values / cell histograms of the frames in flight

// everything the host decides: the grid depends on the frame's size alone
struct HogPlan {
	DenseHogParams P;
	bool fast = true;
	long long total = 0;
};

// BaseDenseHog's constructor :67-93, DescribeDenseHogFastAlg.process / growCellArray :80-118, DescribeDenseHogAlg.process :199-228
int hogPlan(int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant, int width, int height, HogPlan& H,
			const char** msg) {
	*msg = nullptr;
	if (stepBlock <= 0) { *msg = "stepBlock must be >= 1"; return BHIP_ERR_INVALID; }
	if (orientationBins < 1 || pixelsPerCell < 1 || cellsPerBlockX < 1 || cellsPerBlockY < 1) {
		*msg = "dense HOG: orientationBins, pixelsPerCell and cellsPerBlockX / Y must be >= 1";
		return BHIP_ERR_INVALID;
	}
	if (width <= 0 || height <= 0) { *msg = "bad image"; return BHIP_ERR_INVALID; }
	if (orientationBins > BHIP_DENSE_MAX_BINS || pixelsPerCell > BHIP_DENSE_MAX_CELL || (long long)orientationBins * cellsPerBlockX * cellsPerBlockY > BHIP_DENSE_MAX_DOF) {
		*msg = "dense HOG on the GPU: orientationBins <= 64, pixelsPerCell <= 32, descriptors of at most 2048 elements";
		return BHIP_ERR_UNSUPPORTED;
	}
	if (height > 65535) { *msg = "dense descriptors on the GPU: at most 65535 image rows"; return BHIP_ERR_UNSUPPORTED; }
	DenseHogParams& P = H.P;
	P.orientationBins = orientationBins; P.pixelsPerCell = pixelsPerCell; P.cellsPerBlockX = cellsPerBlockX; P.cellsPerBlockY = cellsPerBlockY; P.stepBlock = stepBlock;
	P.dof = orientationBins * cellsPerBlockX * cellsPerBlockY;
	P.cellCols = width / pixelsPerCell;
	P.cellRows = height / pixelsPerCell;
	H.fast = fastVariant != 0;
	long long maxX, maxY, step;
	if (H.fast) {
		maxY = P.cellRows - (cellsPerBlockY - 1);
		maxX = P.cellCols - (cellsPerBlockX - 1);
		step = stepBlock;
	} else {
		maxY = (long long)height - (long long)pixelsPerCell * cellsPerBlockY + 1;
		maxX = (long long)width - (long long)pixelsPerCell * cellsPerBlockX + 1;
		step = (long long)pixelsPerCell * stepBlock;
	}
	// for (i = 0; i < max; i += step)
	P.numY = maxY > 0 ? (int)((maxY + step - 1) / step) : 0;
	P.numX = maxX > 0 ? (int)((maxX + step - 1) / step) : 0;
	if (P.numX == 0 || P.numY == 0) P.numX = P.numY = 0;
	H.total = (long long)P.numX * P.numY;
	if (H.total > INT_MAX) { *msg = "dense HOG on the GPU: more descriptors than an int counts"; return BHIP_ERR_UNSUPPORTED; }
	return BHIP_OK;
}

void hogLocation(const HogPlan& H, long long k, int32_t* xy) {
	const int by = (int)(k / H.P.numX), bx = (int)(k - (long long)by * H.P.numX);
	xy[0] = bx * H.P.stepBlock * H.P.pixelsPerCell;
	xy[1] = by * H.P.stepBlock * H.P.pixelsPerCell;
}

struct DenseSiftPlan {
	DenseSiftParams P;
	long long total = 0;
	std::vector<float> gaussianWeight;
	std::vector<double> binAngle;
};

// DescribeSiftCommon's constructor :60-74 and DescribeDenseSiftAlg.process :120-146
int denseSiftPlan(int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue, double periodX, double periodY,
				  int width, int height, bool tables, DenseSiftPlan& D, const char** msg) {
	*msg = nullptr;
	if (widthSubregion < 1 || widthGrid < 1 || numHistogramBins < 1) { *msg = "dense SIFT: widthSubregion, widthGrid and numHistogramBins must be >= 1"; return BHIP_ERR_INVALID; }
	if (!(weightingSigmaFraction > 0) || !(maxDescriptorElementValue > 0) || !(periodX > 0) || !(periodY > 0)) {
		*msg = "dense SIFT: weightingSigmaFraction, maxDescriptorElementValue and the sampling periods must be > 0";
		return BHIP_ERR_INVALID;
	}
	if (width <= 0 || height <= 0) { *msg = "bad image"; return BHIP_ERR_INVALID; }
	const long long sw = (long long)widthSubregion * widthGrid;
	if (sw <= BHIP_DENSE_MAX_SAMPLE_WIDTH && sw % 2) { *msg = "dense SIFT: widthSubregion * widthGrid must be even (the weight kernel has 2 * (width / 2) columns)"; return BHIP_ERR_INVALID; }
	if (sw > BHIP_DENSE_MAX_SAMPLE_WIDTH) { *msg = "dense SIFT on the GPU: widthSubregion * widthGrid <= 48"; return BHIP_ERR_UNSUPPORTED; }
	if (numHistogramBins > BHIP_DENSE_MAX_BINS || (long long)widthGrid * widthGrid * numHistogramBins > BHIP_DENSE_MAX_DOF) {
		*msg = "dense SIFT on the GPU: numHistogramBins <= 64, descriptors of at most 2048 elements";
		return BHIP_ERR_UNSUPPORTED;
	}
	if (height > 65535) { *msg = "dense descriptors on the GPU: at most 65535 image rows"; return BHIP_ERR_UNSUPPORTED; }
	DenseSiftParams& P = D.P;
	P.widthSubregion = widthSubregion; P.widthGrid = widthGrid; P.numHistogramBins = numHistogramBins;
	P.dof = widthGrid * widthGrid * numHistogramBins;
	P.histogramBinWidth = 2.0 * M_PI / numHistogramBins;
	P.maxDescriptorElementValue = maxDescriptorElementValue;
	const int radius = (int)sw / 2;
	const int X0 = radius, X1 = width - radius, Y0 = radius, Y1 = height - radius;
	P.x0 = X0; P.y0 = Y0; P.spanX = X1 - X0; P.spanY = Y1 - Y0;
	// (int) of a double saturates in Java: below zero either loop is empty whatever the value (-1 stands for it), beyond int is refused
	const double nx = (X1 - X0) / periodX, ny = (Y1 - Y0) / periodY;
	if (nx >= 2147483647.0 || ny >= 2147483647.0) { *msg = "dense SIFT on the GPU: more descriptors than an int counts"; return BHIP_ERR_UNSUPPORTED; }
	const int numX = nx <= -1.0 ? -1 : (int)nx, numY = ny <= -1.0 ? -1 : (int)ny;
	// for (i < numY) { y = (Y1 - Y0) * i / (numY - 1) ...; for (j < numX) { x = (X1 - X0) * j / (numX - 1) ...: ArithmeticException
	if (numY == 1 || (numY > 1 && numX == 1)) { *msg = "dense SIFT: one row or one column of descriptors (the reference divides by zero)"; return BHIP_ERR_INVALID; }
	P.numX = numX > 0 && numY > 0 ? numX : 0;
	P.numY = numX > 0 && numY > 0 ? numY : 0;
	D.total = (long long)P.numX * P.numY;
	if (D.total > INT_MAX || (long long)P.spanX * std::max(P.numX - 1, 0) > INT_MAX || (long long)P.spanY * std::max(P.numY - 1, 0) > INT_MAX) {
		*msg = "dense SIFT on the GPU: a grid beyond int arithmetic";
		return BHIP_ERR_UNSUPPORTED;
	}
	if (tables) {
		D.gaussianWeight = bhip_sift_gaussian_weight(sw * weightingSigmaFraction, radius);   // DescribeSiftCommon :71-73
		D.binAngle.resize(numHistogramBins);
		for (int k = 0; k < numHistogramBins; k++) D.binAngle[k] = k * P.histogramBinWidth;   // trilinearInterpolation :122
	}
	return BHIP_OK;
}

void denseSiftLocation(const DenseSiftPlan& D, long long k, int32_t* xy) {
	const int i = (int)(k / D.P.numX), j = (int)(k - (long long)i * D.P.numX);
	xy[0] = D.P.spanX * j / (D.P.numX - 1) + D.P.x0;
	xy[1] = D.P.spanY * i / (D.P.numY - 1) + D.P.y0;
}

// The tables of a configuration on the device, kept with the context beside the host block they were copied from: uploaded again, with a
// synchronisation (an asynchronous copy's source must outlive it), only when the family's configuration changes.  family: 0 standard HOG, 1 dense
// SIFT -- a slot each, so that a caller who alternates the two uploads nothing
int denseTables(bhip_ctx* ctx, int family, std::vector<char>& blob, char** dev) {
	CtxScratch* sc = scratchOf(ctx);
	DevBuf& slot = sc->denseTables[family];
	std::vector<char>& host = sc->denseTablesHost[family];
	if (!slot.p || host != blob) {
		BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
		host.clear();
		BHIP_TRY(slot.reserve(ctx, std::max(blob.size(), (size_t)8)));
		BHIP_HIP(ctx, hipMemcpyAsync(slot.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
		BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `blob` is this call's
		host.swap(blob);
	}
	*dev = slot.as<char>();
	return BHIP_OK;
}

// frames of one group: as many as keep perFrame bytes each inside kDenseScratch, the groups of a batch about equal
int denseGroup(size_t perFrame, int batch) {
	const int most = (int)std::max<size_t>(1, std::min<size_t>((size_t)batch, kDenseScratch / std::max<size_t>(perFrame, 1)));
	const int groups = (batch + most - 1) / most;
	return (batch + groups - 1) / groups;
}

template <class T>
DevImg<const T> framesFrom(DevImg<const T> in, int b0, int nb) { return {in.data + (long long)b0 * in.imageStride, in.imageStride, in.stride, in.width, in.height, nb}; }
inline DenseOut outFrom(DenseOut out, int b0, int dof) { return {out.desc + (long long)b0 * out.cap * dof, out.xy + (long long)b0 * out.cap * 2, out.cap}; }

template <class T>
int hogDevice(bhip_ctx* ctx, const HogPlan& H, DevImg<const T> in, DenseOut out, int* dev_count, float* dev_cells) {
	const DenseHogParams& P = H.P;
	const int batch = in.batch;
	BHIP_TRY(bhip_launch_dense_count(ctx, dev_count, batch, (int)H.total));
	DevBuf& buf = scratchOf(ctx)->dense;
	if (H.fast) {
		const size_t cellFloats = (size_t)P.cellRows * P.cellCols * P.orientationBins;
		if (cellFloats == 0) return BHIP_OK;
		if (dev_cells) {   // the caller keeps the histograms: no scratch, one group
			BHIP_TRY(bhip_launch_dense_hog_cells<T>(ctx, in, P, dev_cells));
			return bhip_launch_dense_hog_blocks(ctx, P, dev_cells, batch, out);
		}
		if (H.total == 0 || out.cap == 0) return BHIP_OK;
		const size_t perFrame = align256(cellFloats * 4);
		const int group = denseGroup(perFrame, batch);
		BHIP_TRY(buf.reserve(ctx, perFrame * group));
		for (int b0 = 0; b0 < batch; b0 += group) {
			const int nb = std::min(group, batch - b0);
			BHIP_TRY(bhip_launch_dense_hog_cells<T>(ctx, framesFrom(in, b0, nb), P, buf.as<float>()));
			BHIP_TRY(bhip_launch_dense_hog_blocks(ctx, P, buf.as<float>(), nb, outFrom(out, b0, P.dof)));
		}
		return BHIP_OK;
	}
	if (H.total == 0 || out.cap == 0) return BHIP_OK;
	const int rows = P.cellsPerBlockY * P.pixelsPerCell, cols = P.cellsPerBlockX * P.pixelsPerCell;
	const std::vector<double> weights = bhip_dense_hog_weight_table(rows, cols);
	std::vector<char> blob(weights.size() * 8);
	std::memcpy(blob.data(), weights.data(), blob.size());
	char* tables;
	BHIP_TRY(denseTables(ctx, 0, blob, &tables));
	const size_t pixels = (size_t)in.width * in.height, plane = align256(pixels * 4);
	const int group = denseGroup(2 * plane, batch);
	BHIP_TRY(buf.reserve(ctx, 2 * plane * group));
	// [findex of the group's frames | sumsq of the group's frames]: the frames of one array are `pixels` floats apart
	float* findex = buf.as<float>();
	float* sumsq = (float*)(buf.as<char>() + plane * group);
	for (int b0 = 0; b0 < batch; b0 += group) {
		const int nb = std::min(group, batch - b0);
		BHIP_TRY(bhip_launch_dense_hog_pixels<T>(ctx, framesFrom(in, b0, nb), P.orientationBins, findex, sumsq));
		BHIP_TRY(bhip_launch_dense_hog_std(ctx, P, findex, sumsq, (const double*)tables, in.width, in.height, nb, outFrom(out, b0, P.dof)));
	}
	return BHIP_OK;
}

template <class T>
int denseSiftDevice(bhip_ctx* ctx, DenseSiftPlan& D, DevImg<const T> in, DenseOut out, int* dev_count) {
	const int batch = in.batch;
	BHIP_TRY(bhip_launch_dense_count(ctx, dev_count, batch, (int)D.total));
	if (D.total == 0 || out.cap == 0) return BHIP_OK;
	const size_t nB = D.binAngle.size() * 8, nG = D.gaussianWeight.size() * 4;
	std::vector<char> blob(nB + nG);
	std::memcpy(blob.data(), D.binAngle.data(), nB);
	std::memcpy(blob.data() + nB, D.gaussianWeight.data(), nG);
	char* tables;
	BHIP_TRY(denseTables(ctx, 1, blob, &tables));
	const size_t pixels = (size_t)in.width * in.height, planeA = align256(pixels * 8), planeM = align256(pixels * 4);
	const int group = denseGroup(planeA + planeM, batch);
	DevBuf& buf = scratchOf(ctx)->dense;
	BHIP_TRY(buf.reserve(ctx, (planeA + planeM) * group));
	double* angle = buf.as<double>();
	float* magnitude = (float*)(buf.as<char>() + planeA * group);
	for (int b0 = 0; b0 < batch; b0 += group) {
		const int nb = std::min(group, batch - b0);
		BHIP_TRY(bhip_launch_dense_sift_pixels<T>(ctx, framesFrom(in, b0, nb), angle, magnitude));
		BHIP_TRY(bhip_launch_dense_sift(ctx, D.P, angle, magnitude, (const float*)(tables + nB), (const double*)tables, in.width, in.height, nb, outFrom(out, b0, D.P.dof)));
	}
	return BHIP_OK;
}

bool badOut(const DenseOut& out, const int* count) { return !count || out.cap < 0 || (out.cap > 0 && (!out.desc || !out.xy)); }

template <class T>
int hogDev(bhip_ctx* ctx, int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant, const T* dev_in,
		   long long imageStride, int stride, int width, int height, int batch, DenseOut out, int* dev_count, float* dev_cells) {
	CHECK_CTX(ctx);
	const DevImg<const T> in{dev_in, imageStride, stride, width, height, batch};
	HogPlan H;
	const char* msg;
	const int s = hogPlan(orientationBins, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, stepBlock, fastVariant, width, height, H, &msg);
	if (s != BHIP_OK) return bhip_fail(ctx, s, msg);
	CHECK_IMG(ctx, in);
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "dense HOG on the GPU: at most 65535 frames per call");
	if (badOut(out, dev_count)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	if (dev_cells && !H.fast) return bhip_fail(ctx, BHIP_ERR_INVALID, "dense HOG: only the fast variant has cell histograms");
	return hogDevice<T>(ctx, H, in, out, dev_count, dev_cells);
}

template <class T>
int denseSiftDev(bhip_ctx* ctx, int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue, double periodX,
				 double periodY, const T* dev_in, long long imageStride, int stride, int width, int height, int batch, DenseOut out, int* dev_count) {
	CHECK_CTX(ctx);
	const DevImg<const T> in{dev_in, imageStride, stride, width, height, batch};
	DenseSiftPlan D;
	const char* msg;
	const int s = denseSiftPlan(widthSubregion, widthGrid, numHistogramBins, weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY, width, height, true, D, &msg);
	if (s != BHIP_OK) return bhip_fail(ctx, s, msg);
	CHECK_IMG(ctx, in);
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "dense SIFT on the GPU: at most 65535 frames per call");
	if (badOut(out, dev_count)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	return denseSiftDevice<T>(ctx, D, in, out, dev_count);
}

// out0 = [descriptors | xy | count | cells] of the one staged frame
struct DenseStaged {
	DenseOut out;
	int* count;
	float* cells;
};
int denseStageOut(bhip_ctx* ctx, int cap, int dof, size_t cellFloats, DenseStaged& S) {
	CtxScratch* sc = scratchOf(ctx);
	const size_t c1 = (size_t)std::max(cap, 1), cd = align256(c1 * 8 * dof), cx = align256(c1 * 8);
	BHIP_TRY(sc->out0.reserve(ctx, cd + cx + 256 + align256(cellFloats * 4)));
	char* base = sc->out0.as<char>();
	S.out = {(double*)base, (int32_t*)(base + cd), cap};
	S.count = (int*)(base + cd + cx);
	S.cells = cellFloats ? (float*)(base + cd + cx + 256) : nullptr;
	return BHIP_OK;
}
// the count is the host's; the first min(count, cap) records come back
int denseDownload(bhip_ctx* ctx, const DenseStaged& S, long long total, int dof, double* descriptors, int32_t* xy, int* count, float* cells, size_t cellFloats) {
	*count = (int)total;
	const size_t n = (size_t)std::min<long long>(total, S.out.cap);
	if (n > 0) {
		BHIP_HIP(ctx, hipMemcpyAsync(descriptors, S.out.desc, n * 8 * dof, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipMemcpyAsync(xy, S.out.xy, n * 8, hipMemcpyDeviceToHost, ctx->stream));
	}
	if (cells && cellFloats) BHIP_HIP(ctx, hipMemcpyAsync(cells, S.cells, cellFloats * 4, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

template <class T>
int hogHost(bhip_ctx* ctx, int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant, const T* in, int start,
			int stride, int width, int height, double* descriptors, int32_t* xy, int* count, int cap, float* cells) {
	CHECK_CTX(ctx);
	const HostImg<const T> hin{in, start, stride, width, height};
	HogPlan H;
	const char* msg;
	const int s = hogPlan(orientationBins, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, stepBlock, fastVariant, width, height, H, &msg);
	if (s != BHIP_OK) return bhip_fail(ctx, s, msg);
	CHECK_IMG(ctx, hin);
	if (badOut({descriptors, xy, cap}, count)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	if (cells && !H.fast) return bhip_fail(ctx, BHIP_ERR_INVALID, "dense HOG: only the fast variant has cell histograms");
	DevImg<T> din;
	BHIP_TRY(stageIn(ctx, scratchOf(ctx)->in0, hin, width, din));
	const size_t cellFloats = cells ? (size_t)H.P.cellRows * H.P.cellCols * H.P.orientationBins : 0;
	DenseStaged S;
	BHIP_TRY(denseStageOut(ctx, cap, H.P.dof, cellFloats, S));
	BHIP_TRY(hogDevice<T>(ctx, H, DevImg<const T>(din), S.out, S.count, S.cells));
	return denseDownload(ctx, S, H.total, H.P.dof, descriptors, xy, count, cells, cellFloats);
}

template <class T>
int denseSiftHost(bhip_ctx* ctx, int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue, double periodX,
				  double periodY, const T* in, int start, int stride, int width, int height, double* descriptors, int32_t* xy, int* count, int cap) {
	CHECK_CTX(ctx);
	const HostImg<const T> hin{in, start, stride, width, height};
	DenseSiftPlan D;
	const char* msg;
	const int s = denseSiftPlan(widthSubregion, widthGrid, numHistogramBins, weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY, width, height, true, D, &msg);
	if (s != BHIP_OK) return bhip_fail(ctx, s, msg);
	CHECK_IMG(ctx, hin);
	if (badOut({descriptors, xy, cap}, count)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	DevImg<T> din;
	BHIP_TRY(stageIn(ctx, scratchOf(ctx)->in0, hin, width, din));
	DenseStaged S;
	BHIP_TRY(denseStageOut(ctx, cap, D.P.dof, 0, S));
	BHIP_TRY(denseSiftDevice<T>(ctx, D, DevImg<const T>(din), S.out, S.count));
	return denseDownload(ctx, S, D.total, D.P.dof, descriptors, xy, count, nullptr, 0);
}

}   // namespace

extern "C" {

int bhip_dense_hog_layout(int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant, int width, int height,
						  int* perRow, int* perCol, int* dof, int32_t* xy, int cap) {
	HogPlan H;
	const char* msg;
	BHIP_TRY(hogPlan(orientationBins, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, stepBlock, fastVariant, width, height, H, &msg));
	if (perRow) *perRow = H.P.numX;
	if (perCol) *perCol = H.P.numY;
	if (dof) *dof = H.P.dof;
	for (long long k = 0; xy && k < std::min<long long>(H.total, cap); k++) hogLocation(H, k, xy + 2 * k);
	return (int)H.total;
}

int bhip_dense_sift_layout(int widthSubregion, int widthGrid, int numHistogramBins, double periodX, double periodY, int width, int height, int* perRow, int* perCol,
						   int* dof, int32_t* xy, int cap) {
	DenseSiftPlan D;
	const char* msg;
	BHIP_TRY(denseSiftPlan(widthSubregion, widthGrid, numHistogramBins, 0.5, 0.2, periodX, periodY, width, height, false, D, &msg));
	if (perRow) *perRow = D.P.numX;
	if (perCol) *perCol = D.P.numY;
	if (dof) *dof = D.P.dof;
	for (long long k = 0; xy && k < std::min<long long>(D.total, cap); k++) denseSiftLocation(D, k, xy + 2 * k);
	return (int)D.total;
}

int bhip_dense_hog_weights(int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, double* weights) {
	HogPlan H;
	const char* msg;
	BHIP_TRY(hogPlan(1, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, 1, 0, 1, 1, H, &msg));
	const std::vector<double> w = bhip_dense_hog_weight_table(cellsPerBlockY * pixelsPerCell, cellsPerBlockX * pixelsPerCell);
	if (weights) std::copy(w.begin(), w.end(), weights);
	return (int)w.size();
}

int bhip_dense_hog_dev_f32(bhip_ctx* ctx, int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant,
						   const float* dev_in, long long imageStride, int stride, int width, int height, int batch, double* dev_desc, int32_t* dev_xy, int* dev_count,
						   int cap, float* dev_cells) {
	return hogDev<float>(ctx, orientationBins, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, stepBlock, fastVariant, dev_in, imageStride, stride, width, height, batch,
						 {dev_desc, dev_xy, cap}, dev_count, dev_cells);
}
int bhip_dense_hog_dev_u8(bhip_ctx* ctx, int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant,
						  const uint8_t* dev_in, long long imageStride, int stride, int width, int height, int batch, double* dev_desc, int32_t* dev_xy, int* dev_count,
						  int cap, float* dev_cells) {
	return hogDev<uint8_t>(ctx, orientationBins, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, stepBlock, fastVariant, dev_in, imageStride, stride, width, height, batch,
						   {dev_desc, dev_xy, cap}, dev_count, dev_cells);
}
int bhip_dense_sift_dev_f32(bhip_ctx* ctx, int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue,
							double periodX, double periodY, const float* dev_in, long long imageStride, int stride, int width, int height, int batch, double* dev_desc,
							int32_t* dev_xy, int* dev_count, int cap) {
	return denseSiftDev<float>(ctx, widthSubregion, widthGrid, numHistogramBins, weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY, dev_in, imageStride,
							   stride, width, height, batch, {dev_desc, dev_xy, cap}, dev_count);
}
int bhip_dense_sift_dev_u8(bhip_ctx* ctx, int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue,
						   double periodX, double periodY, const uint8_t* dev_in, long long imageStride, int stride, int width, int height, int batch, double* dev_desc,
						   int32_t* dev_xy, int* dev_count, int cap) {
	return denseSiftDev<uint8_t>(ctx, widthSubregion, widthGrid, numHistogramBins, weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY, dev_in, imageStride,
								 stride, width, height, batch, {dev_desc, dev_xy, cap}, dev_count);
}
int bhip_dense_hog_f32(bhip_ctx* ctx, int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant, const float* in,
					   int start, int stride, int width, int height, double* descriptors, int32_t* xy, int* count, int cap, float* cells) {
	return hogHost<float>(ctx, orientationBins, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, stepBlock, fastVariant, in, start, stride, width, height, descriptors, xy,
						  count, cap, cells);
}
int bhip_dense_hog_u8(bhip_ctx* ctx, int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant, const uint8_t* in,
					  int start, int stride, int width, int height, double* descriptors, int32_t* xy, int* count, int cap, float* cells) {
	return hogHost<uint8_t>(ctx, orientationBins, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, stepBlock, fastVariant, in, start, stride, width, height, descriptors, xy,
							count, cap, cells);
}
int bhip_dense_sift_f32(bhip_ctx* ctx, int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue,
						double periodX, double periodY, const float* in, int start, int stride, int width, int height, double* descriptors, int32_t* xy, int* count,
						int cap) {
	return denseSiftHost<float>(ctx, widthSubregion, widthGrid, numHistogramBins, weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY, in, start, stride,
								width, height, descriptors, xy, count, cap);
}
int bhip_dense_sift_u8(bhip_ctx* ctx, int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue,
					   double periodX, double periodY, const uint8_t* in, int start, int stride, int width, int height, double* descriptors, int32_t* xy, int* count,
					   int cap) {
	return denseSiftHost<uint8_t>(ctx, widthSubregion, widthGrid, numHistogramBins, weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY, in, start, stride,
								  width, height, descriptors, xy, count, cap);
}

}   // extern "C"
