// ---------------------------------------------------------------------------------------------------------------
// Line detection on the C boundary: the edge features of a gradient (edge.hip), the binary polar and gradient foot-of-norm Hough
// transforms, the relaxed block NMS and the mean-shift refinement of peaks (hough.hip).  The Prewitt gradient sits with the other
// gradients in cabi_ip.hip.  Every argument check comes before anything touches the device, so a refused call writes nothing.
// ---------------------------------------------------------------------------------------------------------------
#include "cabi.h"

// launch grids carry the rows in y and the images in z
template <class V>
static const char* gridError(V v) { return v.batch > 65535 ? "more than 65535 images in a batch" : v.height > 65535 ? "more than 65535 rows" : nullptr; }

// the bytes a view spans (non-negative strides)
template <class T>
static void spanOf(DevImg<T> v, uintptr_t& lo, uintptr_t& hi) {
	lo = (uintptr_t)v.data;
	hi = lo + (uintptr_t)(((long long)(v.batch - 1) * v.imageStride + (long long)(v.height - 1) * v.stride + v.width) * (long long)sizeof(T));
}

template <class T>
static int crudeDev(bhip_ctx* ctx, DevImg<const float> intensity, DevImg<const T> dx, DevImg<const T> dy, DevImg<float> out) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, intensity);
	CHECK_IMG(ctx, dx);
	CHECK_IMG(ctx, dy);
	CHECK_IMG(ctx, out);
	if (const char* e = gridError(intensity)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, e);
	if (intensity.imageStride < 0 || out.imageStride < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "negative image stride");
	uintptr_t alo, ahi, blo, bhi;
	spanOf(intensity, alo, ahi);
	spanOf(DevImg<const float>(out), blo, bhi);
	if (alo < bhi && blo < ahi) return bhip_fail(ctx, BHIP_ERR_INVALID, "intensity and output must not overlap");
	return bhip_launch_edge_nonmax_crude4<T>(ctx, intensity, dx, dy, out);
}

// HoughParametersPolar.initialize: Java's int products wrap
static void polarBins(int width, int height, double rangeResolution, int& numBinsRange, float& rMax) {
	const int ox = width / 2, oy = height / 2;
	const int sum = (int)((unsigned)ox * (unsigned)ox + (unsigned)oy * (unsigned)oy);
	rMax = (float)std::sqrt((double)sum);
	const double bins = std::ceil((double)rMax / rangeResolution);
	numBinsRange = bins != bins ? 0 : bins >= 2147483647.0 ? 2147483647 : bins <= -2147483648.0 ? (-2147483647 - 1) : (int)bins;   // Java's (int)
}
static int houghBinaryCheck(bhip_ctx* ctx, int width, int height, int batch, double rangeResolution, int numBinsAngle, const float* cosTable, const float* sinTable,
							int tWidth, int tHeight, int& numBinsRange, float& rMax) {
	if ((long long)width * height > (1LL << 24)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "width * height beyond 2^24: a float count stops there");
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	if (numBinsAngle <= 0 || !cosTable || !sinTable) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad angle bins");
	polarBins(width, height, rangeResolution, numBinsRange, rMax);
	if (numBinsRange <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "the transform has no range bins");
	if (numBinsAngle > 65535 || (long long)numBinsAngle * numBinsRange > (1LL << 28)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "transform too large");
	if (tWidth != numBinsRange || tHeight != numBinsAngle) return bhip_fail(ctx, BHIP_ERR_INVALID, "the transform is numBinsRange wide and numBinsAngle high");
	return BHIP_OK;
}
static int houghBinaryImpl(bhip_ctx* ctx, DevImg<const uint8_t> bin, int numBinsAngle, int numBinsRange, float rMax, const float* cosTable, const float* sinTable,
						   DevImg<float> transform) {
	CtxScratch* sc = scratchOf(ctx);
	BHIP_TRY(sc->houghTable.reserve(ctx, (size_t)numBinsAngle * 2 * sizeof(float)));
	BHIP_TRY(sc->hough.reserve(ctx, (size_t)numBinsAngle * numBinsRange * bin.batch * sizeof(int)));
	float* table = sc->houghTable.as<float>();
	BHIP_HIP(ctx, hipMemcpyAsync(table, cosTable, (size_t)numBinsAngle * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(table + numBinsAngle, sinTable, (size_t)numBinsAngle * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	return bhip_launch_hough_binary_polar(ctx, bin, table, table + numBinsAngle, numBinsAngle, numBinsRange, rMax, transform, sc->hough.as<int>());
}

template <class T>
static int houghGradientDev(bhip_ctx* ctx, DevImg<const T> dx, DevImg<const T> dy, DevImg<const uint8_t> bin, DevImg<float> transform, int cap, int* dev_n) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, dx);
	CHECK_IMG(ctx, dy);
	CHECK_IMG(ctx, bin);
	CHECK_IMG(ctx, transform);
	if (cap < 0 || !dev_n) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	if (const char* e = gridError(bin)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, e);
	const long long cells = (long long)bin.width * bin.height;
	if (cells > 2147483646LL) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "width * height beyond an int32 index");
	cap = (int)std::min<long long>(cap, cells);
	// the image is part of the sort key, and the records of a chunk stay within 1 GiB
	int chunk = (int)std::min<long long>(bin.batch, 4294967294LL / cells);
	const size_t budget = (size_t)1 << 30;
	while (chunk > 1 && bhip_hough_gradient_scratch(bin.width, bin.height, chunk, cap) > budget) chunk = (chunk + 1) / 2;
	const size_t bytes = bhip_hough_gradient_scratch(bin.width, bin.height, chunk, cap);
	if (bytes == 0) return bhip_fail(ctx, BHIP_ERR_HIP, "the sort's scratch size could not be determined");
	DevBuf& buf = scratchOf(ctx)->hough;
	BHIP_TRY(buf.reserve(ctx, bytes));
	for (int b0 = 0; b0 < bin.batch; b0 += chunk) {
		DevImg<const T> x = dx, y = dy;
		DevImg<const uint8_t> b = bin;
		DevImg<float> t = transform;
		x.data += (long long)b0 * dx.imageStride;
		y.data += (long long)b0 * dy.imageStride;
		b.data += (long long)b0 * bin.imageStride;
		t.data += (long long)b0 * transform.imageStride;
		x.batch = y.batch = b.batch = t.batch = std::min(chunk, bin.batch - b0);
		BHIP_TRY(bhip_launch_hough_gradient_foot<T>(ctx, x, y, b, t, cap, dev_n + b0, buf.p));
	}
	return BHIP_OK;
}

// relaxed block NMS of a batch of device images: lists and counts as nonmaxDevice (cabi_detect.hip) writes them for the strict rule
static int nonmaxRelaxedDevice(bhip_ctx* ctx, DevImg<const float> img, int radius, float threshold, int border, int16_t* dev_xy, int cap, int* dev_n) {
	const int width = img.width, height = img.height, batch = img.batch;
	if (radius < 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "Search radius must be >= 1");
	if (border < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Ignore border must be >= 0 ");
	if (width >= 32768 || height >= 32768) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "image too large for Point2D_I16");
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	const int step = radius + 1;
	const int rw = width - 2 * border, rh = height - 2 * border;
	const long long nbx = rw > 0 ? (rw + step - 1) / step : 0, nby = rh > 0 ? (rh + step - 1) / step : 0;
	const long long bits = nbx * nby * step * step;   // every block has room for a full one
	if (bits > 2147483647LL - 64) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "NMS radius too large for this image");
	BHIP_HIP(ctx, hipMemsetAsync(dev_n, 0, (size_t)batch * 4, ctx->stream));
	if (rw <= 0 || rh <= 0) return BHIP_OK;
	const int words = (int)((bits + 31) / 32) + 1;
	CtxScratch* sc = scratchOf(ctx);
	const size_t bmBytes = (size_t)words * 4 * batch;
	BHIP_TRY(sc->nmsBitmap.reserve(ctx, bmBytes));
	BHIP_TRY(sc->nmsPrefix.reserve(ctx, bmBytes));
	unsigned int* bitmap = sc->nmsBitmap.as<unsigned int>();
	unsigned int* prefix = sc->nmsPrefix.as<unsigned int>();
	BHIP_HIP(ctx, hipMemsetAsync(bitmap, 0, bmBytes, ctx->stream));
	BHIP_TRY(bhip_launch_nonmax_relaxed(ctx, img, radius, threshold, border, bitmap, words, (int)nbx));
	BHIP_TRY(bhip_launch_word_prefix(ctx, bitmap, words, batch, prefix, dev_n));
	return bhip_launch_relaxed_to_xy(ctx, bitmap, prefix, words, (int)nbx, batch, radius, border, dev_xy, cap);
}

extern "C" {

int bhip_gradient_intensity_abs_dev_s16(bhip_ctx* ctx, const int16_t* dev_dx, const int16_t* dev_dy, long long dImageStride, int dStride, int width, int height,
										int batch, float* dev_out, long long outImageStride, int outStride) {
	const DevImg<const int16_t> dx{dev_dx, dImageStride, dStride, width, height, batch}, dy{dev_dy, dImageStride, dStride, width, height, batch};
	const DevImg<float> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, dx);
	CHECK_IMG(ctx, dy);
	CHECK_IMG(ctx, out);
	if (const char* e = gridError(dx)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, e);
	return bhip_launch_grad_intensity_abs_s16(ctx, dx, dy, out);
}

int bhip_edge_nonmax_crude4_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long iImageStride, int iStride, const float* dev_dx, const float* dev_dy,
									long long dImageStride, int dStride, int width, int height, int batch, float* dev_out, long long outImageStride, int outStride) {
	return crudeDev<float>(ctx, {dev_intensity, iImageStride, iStride, width, height, batch}, {dev_dx, dImageStride, dStride, width, height, batch},
						   {dev_dy, dImageStride, dStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_edge_nonmax_crude4_dev_s16(bhip_ctx* ctx, const float* dev_intensity, long long iImageStride, int iStride, const int16_t* dev_dx, const int16_t* dev_dy,
									long long dImageStride, int dStride, int width, int height, int batch, float* dev_out, long long outImageStride, int outStride) {
	return crudeDev<int16_t>(ctx, {dev_intensity, iImageStride, iStride, width, height, batch}, {dev_dx, dImageStride, dStride, width, height, batch},
							 {dev_dy, dImageStride, dStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}

int bhip_hough_polar_bins(int width, int height, double rangeResolution, int* numBinsRange, float* rMax) {
	if (width <= 0 || height <= 0) return BHIP_ERR_INVALID;
	int bins;
	float r;
	polarBins(width, height, rangeResolution, bins, r);
	if (numBinsRange) *numBinsRange = bins;
	if (rMax) *rMax = r;
	return BHIP_OK;
}

int bhip_hough_binary_polar_dev_u8(bhip_ctx* ctx, const uint8_t* dev_binary, long long imageStride, int stride, int width, int height, int batch,
								   double rangeResolution, int numBinsAngle, const float* cosTable, const float* sinTable, float* dev_transform,
								   long long tImageStride, int tStride, int tWidth, int tHeight) {
	const DevImg<const uint8_t> bin{dev_binary, imageStride, stride, width, height, batch};
	const DevImg<float> transform{dev_transform, tImageStride, tStride, tWidth, tHeight, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, bin);
	int numBinsRange;
	float rMax;
	BHIP_TRY(houghBinaryCheck(ctx, width, height, batch, rangeResolution, numBinsAngle, cosTable, sinTable, tWidth, tHeight, numBinsRange, rMax));
	CHECK_IMG(ctx, transform);
	return houghBinaryImpl(ctx, bin, numBinsAngle, numBinsRange, rMax, cosTable, sinTable, transform);
}
int bhip_hough_binary_polar_u8(bhip_ctx* ctx, const uint8_t* binary, int start, int stride, int width, int height, double rangeResolution, int numBinsAngle,
							   const float* cosTable, const float* sinTable, float* transform, int tStart, int tStride, int tWidth, int tHeight) {
	const HostImg<const uint8_t> hin{binary, start, stride, width, height};
	const HostImg<float> hout{transform, tStart, tStride, tWidth, tHeight};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	int numBinsRange;
	float rMax;
	BHIP_TRY(houghBinaryCheck(ctx, width, height, 1, rangeResolution, numBinsAngle, cosTable, sinTable, tWidth, tHeight, numBinsRange, rMax));
	CHECK_IMG(ctx, hout);
	CtxScratch* sc = scratchOf(ctx);
	DevImg<uint8_t> din;
	DevImg<float> dout;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	BHIP_TRY(stageIn(ctx, sc->out0, hout, tWidth, dout, false));
	BHIP_TRY(houghBinaryImpl(ctx, DevImg<const uint8_t>(din), numBinsAngle, numBinsRange, rMax, cosTable, sinTable, dout));
	BHIP_TRY(stageOut(ctx, hout, dout));
	return bhip_ctx_synchronize(ctx);
}

int bhip_hough_gradient_foot_dev_f32(bhip_ctx* ctx, const float* dev_dx, const float* dev_dy, long long dImageStride, int dStride, const uint8_t* dev_binary,
									 long long bImageStride, int bStride, int width, int height, int batch, float* dev_transform, long long tImageStride,
									 int tStride, int cap, int* dev_n) {
	return houghGradientDev<float>(ctx, {dev_dx, dImageStride, dStride, width, height, batch}, {dev_dy, dImageStride, dStride, width, height, batch},
								   {dev_binary, bImageStride, bStride, width, height, batch}, {dev_transform, tImageStride, tStride, width, height, batch}, cap, dev_n);
}
int bhip_hough_gradient_foot_dev_s16(bhip_ctx* ctx, const int16_t* dev_dx, const int16_t* dev_dy, long long dImageStride, int dStride, const uint8_t* dev_binary,
									 long long bImageStride, int bStride, int width, int height, int batch, float* dev_transform, long long tImageStride,
									 int tStride, int cap, int* dev_n) {
	return houghGradientDev<int16_t>(ctx, {dev_dx, dImageStride, dStride, width, height, batch}, {dev_dy, dImageStride, dStride, width, height, batch},
									 {dev_binary, bImageStride, bStride, width, height, batch}, {dev_transform, tImageStride, tStride, width, height, batch}, cap, dev_n);
}

int bhip_nonmax_block_relaxed_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long imageStride, int stride, int width, int height, int batch, int radius,
									  float threshold, int border, int16_t* dev_xy, int cap, int* dev_n) {
	CHECK_CTX(ctx);
	const DevImg<const float> img{dev_intensity, imageStride, stride, width, height, batch};
	CHECK_IMG(ctx, img);
	if (!dev_n || cap < 0 || (cap > 0 && !dev_xy)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	return nonmaxRelaxedDevice(ctx, img, radius, threshold, border, dev_xy, cap, dev_n);
}
int bhip_nonmax_block_relaxed_f32(bhip_ctx* ctx, const float* intensity, int start, int stride, int width, int height, int radius, float threshold, int border,
								  int16_t* xy, int cap, int* n) {
	const HostImg<const float> hin{intensity, start, stride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	if (!n || cap < 0 || (cap > 0 && !xy)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	*n = 0;
	CtxScratch* sc = scratchOf(ctx);
	DevImg<float> din;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)std::max(cap, 1) * 4));
	BHIP_TRY(sc->out1.reserve(ctx, 16));
	BHIP_TRY(nonmaxRelaxedDevice(ctx, din, radius, threshold, border, sc->out0.as<int16_t>(), cap, sc->out1.as<int>()));
	BHIP_HIP(ctx, hipMemcpyAsync(ctx->hostScratch.p, sc->out1.p, 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the count decides how much of the list to copy
	*n = ctx->hostScratch.as<int>()[0];
	const int ncopy = std::min(*n, cap);
	if (ncopy == 0) return BHIP_OK;
	BHIP_HIP(ctx, hipMemcpyAsync(xy, sc->out0.p, (size_t)ncopy * 4, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

int bhip_mean_shift_peak_dev_f32(bhip_ctx* ctx, const float* dev_image, long long imageStride, int stride, int width, int height, int batch, const int16_t* dev_xy,
								 const int* dev_n, int cap, int radius, int maxIterations, float convergenceTol, const float* weights, float* dev_peak,
								 float* dev_intensity) {
	const DevImg<const float> img{dev_image, imageStride, stride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, img);
	if (cap < 0 || (cap > 0 && (!dev_xy || !dev_peak || !dev_intensity))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad peak lists");
	if (radius > 0 && !weights) return bhip_fail(ctx, BHIP_ERR_INVALID, "null weight table");
	if (radius > 1023) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "mean-shift radius too large");
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	const float* table = nullptr;
	if (radius > 0) {
		const size_t n = (size_t)(2 * radius + 1) * (2 * radius + 1);
		DevBuf& buf = scratchOf(ctx)->houghTable;
		BHIP_TRY(buf.reserve(ctx, n * sizeof(float)));
		BHIP_HIP(ctx, hipMemcpyAsync(buf.p, weights, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
		table = buf.as<float>();
	}
	return bhip_launch_mean_shift_peak(ctx, img, dev_xy, dev_n, cap, radius, maxIterations, convergenceTol, table, dev_peak, dev_intensity);
}

}  // extern "C"
