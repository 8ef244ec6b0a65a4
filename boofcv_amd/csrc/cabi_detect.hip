// C ABI, stage-level detection on host buffers and device batches: integral image, Hessian intensity, block NMS, N-best selection, FAST.
#include "cabi.h"

// bhip_hessian_f32 (T = float) and bhip_hessian_s32 (T = int32_t).  Their argument checks differ (not harmonised): S32 refuses a null or too
// narrow output and an intensity image without pixels, F32 checks the output only after an empty intensity image has returned BHIP_OK
template <class T>
static int hessianHost(bhip_ctx* ctx, HostImg<const T> hin, int skip, int size, float* intensity, int outStart, int outStride) {
	constexpr bool s32 = std::is_same<T, int32_t>::value;
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	if (s32 && !intensity) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image");
	if (skip < 1 || size < 3) return bhip_fail(ctx, BHIP_ERR_INVALID, s32 ? "bad skip / size" : "bad skip/size");
	const int w = hin.width / skip, h = hin.height / skip;
	if (s32 && (w <= 0 || h <= 0 || outStride < w)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad intensity image");
	if (w <= 0 || h <= 0) return BHIP_OK;
	const HostImg<float> hout{intensity, outStart, outStride, w, h};
	CHECK_IMG(ctx, hout);
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> din;
	DevImg<float> dout;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, hin.width, din));
	BHIP_TRY(stageIn(ctx, sc->out0, hout, w, dout, false));
	BHIP_TRY(bhip_launch_hessian(ctx, DevImg<const T>(din), skip, 1, &size, dout, (long long)w * h, nullptr, 0));
	BHIP_TRY(stageOut(ctx, hout, dout));
	return bhip_ctx_synchronize(ctx);
}

// strict block NMS of a batch of device images: lists into dev_xy ([batch][cap] (x,y) int16 pairs, block-raster order), counts into
// dev_n[batch] (a count may exceed cap: only the first cap pairs are written)
// minimum: NonMaxBlockSearchStrict.Min with threshold = thresholdMin.  The maxima pass works in the first half of the context's NMS buffers,
// the minima pass in the second (both halves are reserved before either pass is queued), so Min + Max on one image is two passes.
int nonmaxDevice(bhip_ctx* ctx, DevImg<const float> img, int radius, float threshold, int border, int16_t* dev_xy, int cap, int* dev_n,
						bool minimum) {
	const int width = img.width, height = img.height, batch = img.batch;
	if (radius < 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "Search radius must be >= 1");
	if (border < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Ignore border must be >= 0 ");
	if (width >= 32768 || height >= 32768) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "image too large for Point2D_I16");
	BHIP_HIP(ctx, hipMemsetAsync(dev_n, 0, (size_t)batch * 4, ctx->stream));
	const int step = radius + 1;
	const int rw = width - 2 * border, rh = height - 2 * border;
	if (rw <= 0 || rh <= 0) return BHIP_OK;
	const int nbx = (rw + step - 1) / step, nby = (rh + step - 1) / step;
	const int words = (int)(((long long)nbx * nby + 31) / 32) + 1;
	CtxScratch* sc = scratchOf(ctx);
	const size_t bmBytes = (size_t)words * 4 * batch, posBytes = ((size_t)nbx * nby * 2 * batch + 3) & ~(size_t)3;
	BHIP_TRY(sc->nmsBitmap.reserve(ctx, 2 * bmBytes));
	BHIP_TRY(sc->nmsPrefix.reserve(ctx, 2 * bmBytes));
	BHIP_TRY(sc->nmsPos.reserve(ctx, 2 * posBytes));
	unsigned int* bitmap = (unsigned int*)(sc->nmsBitmap.as<char>() + (minimum ? bmBytes : 0));
	unsigned int* prefix = (unsigned int*)(sc->nmsPrefix.as<char>() + (minimum ? bmBytes : 0));
	unsigned short* pos = (unsigned short*)(sc->nmsPos.as<char>() + (minimum ? posBytes : 0));
	BHIP_HIP(ctx, hipMemsetAsync(bitmap, 0, bmBytes, ctx->stream));
	if (minimum) BHIP_TRY(bhip_launch_nonmin_blocks(ctx, img, radius, threshold, border, bitmap, words, pos, nbx, nby));
	else BHIP_TRY(bhip_launch_nonmax_blocks(ctx, img, radius, threshold, border, bitmap, words, pos, nbx, nby));
	BHIP_TRY(bhip_launch_word_prefix(ctx, bitmap, words, batch, prefix, dev_n));
	BHIP_TRY(bhip_launch_blocks_to_xy(ctx, bitmap, prefix, words, pos, nbx, nby, batch, radius, border, dev_xy, cap));
	return BHIP_OK;
}

// NonMaxBlockSearchStrict.Min / .Max / .MinMax: the side that is not detected gets a count of 0 (when it has a count buffer)
static int nonmaxMinMaxDevice(bhip_ctx* ctx, DevImg<const float> img, int radius, float thresholdMin, float thresholdMax, int border, bool detectMin,
							  bool detectMax, int16_t* dev_xyMin, int* dev_nMin, int16_t* dev_xyMax, int* dev_nMax, int cap) {
	if (!detectMin && !detectMax) return bhip_fail(ctx, BHIP_ERR_INVALID, "Must detect either minimums or maximums");
	if ((detectMin && !dev_nMin) || (detectMax && !dev_nMax) || cap < 0 || (cap > 0 && ((detectMin && !dev_xyMin) || (detectMax && !dev_xyMax))))
		return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	if (detectMax) BHIP_TRY(nonmaxDevice(ctx, img, radius, thresholdMax, border, dev_xyMax, cap, dev_nMax, false));
	else if (dev_nMax) BHIP_HIP(ctx, hipMemsetAsync(dev_nMax, 0, (size_t)img.batch * 4, ctx->stream));
	if (detectMin) BHIP_TRY(nonmaxDevice(ctx, img, radius, thresholdMin, border, dev_xyMin, cap, dev_nMin, true));
	else if (dev_nMin) BHIP_HIP(ctx, hipMemsetAsync(dev_nMin, 0, (size_t)img.batch * 4, ctx->stream));
	return BHIP_OK;
}

// Results of a host export with two lists: the device lists are sc->out0 = [first cap pairs][second cap pairs], the counts sc->out1[0 .. 1].
// Reads the counts back (the one synchronisation that decides how much to copy), then the first min(count, cap) pairs of each list.
static int fetchTwoLists(bhip_ctx* ctx, int cap, int16_t* xyA, int* nA, int16_t* xyB, int* nB) {
	CtxScratch* sc = scratchOf(ctx);
	BHIP_HIP(ctx, hipMemcpyAsync(ctx->hostScratch.p, sc->out1.p, 8, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const int a = ctx->hostScratch.as<int>()[0], b = ctx->hostScratch.as<int>()[1];
	if (nA) *nA = a;
	if (nB) *nB = b;
	if (xyA && std::min(a, cap) > 0) BHIP_HIP(ctx, hipMemcpyAsync(xyA, sc->out0.p, (size_t)std::min(a, cap) * 4, hipMemcpyDeviceToHost, ctx->stream));
	if (xyB && std::min(b, cap) > 0)
		BHIP_HIP(ctx, hipMemcpyAsync(xyB, sc->out0.as<int16_t>() + (size_t)cap * 2, (size_t)std::min(b, cap) * 4, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

// ---- FAST corners (fast.hip): FastCornerDetector.process on a batch of device frames ----
template <class T>
static int fastDevice(bhip_ctx* ctx, DevImg<const T> img, typename FastTol<T>::type pixelTol, int minContinuous, double maxFeaturesFraction, DevImg<float> inten,
					  int16_t* dev_xyLow, int* dev_nLow, int16_t* dev_xyHigh, int* dev_nHigh, int cap) {
	// ConfigFastCorner.checkValidity (F:abst/feature/detect/interest/ConfigFastCorner.java:52-64), FastCornerDetector.setMaxFeaturesFraction (:195-199)
	if (minContinuous < 9 || minContinuous > 12) return bhip_fail(ctx, BHIP_ERR_INVALID, "minContinuous must be from 9 to 12, inclusive");
	if (!(maxFeaturesFraction > 0 && maxFeaturesFraction <= 1)) return bhip_fail(ctx, BHIP_ERR_INVALID, "0 to 1");
	if (!(pixelTol >= 0)) return bhip_fail(ctx, BHIP_ERR_INVALID, "pixelTol must be >= 0");   // the decision trees define nothing sensible there
	if (!dev_nLow || !dev_nHigh || cap < 0 || (cap > 0 && (!dev_xyLow || !dev_xyHigh))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	if (inten.data && inten.stride < img.width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image");
	if (img.width >= 32768 || img.height >= 32768) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "image too large for Point2D_I16");
	const int maxFeatures = (int)(maxFeaturesFraction * img.width * img.height);   // FastCornerDetector.java:124, left to right in double
	DevBuf& scratch = scratchOf(ctx)->fast;
	BHIP_TRY(scratch.reserve(ctx, bhip_fast_scratch(img.width, img.height, img.batch)));
	return bhip_launch_fast<T>(ctx, img, pixelTol, minContinuous, maxFeatures, inten, scratch.p, dev_xyLow, dev_nLow, dev_xyHigh, dev_nHigh, cap);
}

template <class T>
static int fastDev(bhip_ctx* ctx, const T* dev_img, long long imageStride, int stride, int width, int height, int batch, typename FastTol<T>::type pixelTol,
				   int minContinuous, double maxFeaturesFraction, float* dev_intensity, long long iImageStride, int iStride, int16_t* dev_xyLow, int* dev_nLow,
				   int16_t* dev_xyHigh, int* dev_nHigh, int cap) {
	CHECK_CTX(ctx);
	const DevImg<const T> img{dev_img, imageStride, stride, width, height, batch};
	CHECK_IMG(ctx, img);
	return fastDevice<T>(ctx, img, pixelTol, minContinuous, maxFeaturesFraction, {dev_intensity, iImageStride, iStride, width, height, batch}, dev_xyLow, dev_nLow,
						 dev_xyHigh, dev_nHigh, cap);
}

template <class T>
static int fastHost(bhip_ctx* ctx, const T* image, int start, int stride, int width, int height, typename FastTol<T>::type pixelTol, int minContinuous,
					double maxFeaturesFraction, float* intensity, int iStart, int iStride, int16_t* xyLow, int* nLow, int16_t* xyHigh, int* nHigh, int cap) {
	const HostImg<const T> hin{image, start, stride, width, height};
	const HostImg<float> hout{intensity, iStart, iStride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	if (intensity) CHECK_IMG(ctx, hout);
	if (!nLow || !nHigh || cap < 0 || (cap > 0 && (!xyLow || !xyHigh))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> din;
	DevImg<float> dout{nullptr, 0, 0, width, height, 1};
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	if (intensity) BHIP_TRY(stageIn(ctx, sc->tmp0, hout, width, dout, false));
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)std::max(cap, 1) * 8));
	BHIP_TRY(sc->out1.reserve(ctx, 16));
	int16_t* dlow = sc->out0.as<int16_t>();
	BHIP_TRY(fastDevice<T>(ctx, din, pixelTol, minContinuous, maxFeaturesFraction, dout, dlow, sc->out1.as<int>(), dlow + (size_t)cap * 2, sc->out1.as<int>() + 1, cap));
	if (intensity) BHIP_TRY(stageOut(ctx, hout, dout));
	return fetchTwoLists(ctx, cap, xyLow, nLow, xyHigh, nHigh);
}

extern "C" {

// ---------------------------------------------------------------------------------------------------------------
// stage-level entry points (host buffers in / out)
// ---------------------------------------------------------------------------------------------------------------
int bhip_integral_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, float* out, int outStart, int outStride) {
	return hostInOut<float, float>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, false, false, nullptr, [&](auto din, auto dout) {
		return bhip_launch_integral(ctx, din, dout);
	});
}

int bhip_hessian_f32(bhip_ctx* ctx, const float* ii, int iiStart, int iiStride, int width, int height, int skip, int size, float* intensity,
					 int outStart, int outStride) {
	return hessianHost<float>(ctx, {ii, iiStart, iiStride, width, height}, skip, size, intensity, outStart, outStride);
}

int bhip_nonmax_block_minmax_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long imageStride, int stride, int width, int height, int batch, int radius,
									 float thresholdMin, float thresholdMax, int border, int detectMin, int detectMax, int16_t* dev_xyMin, int* dev_nMin,
									 int16_t* dev_xyMax, int* dev_nMax, int cap) {
	CHECK_CTX(ctx);
	const DevImg<const float> img{dev_intensity, imageStride, stride, width, height, batch};
	CHECK_IMG(ctx, img);
	return nonmaxMinMaxDevice(ctx, img, radius, thresholdMin, thresholdMax, border, detectMin != 0, detectMax != 0, dev_xyMin, dev_nMin, dev_xyMax, dev_nMax, cap);
}

int bhip_nonmax_block_minmax_f32(bhip_ctx* ctx, const float* intensity, int start, int stride, int width, int height, int radius, float thresholdMin,
								 float thresholdMax, int border, int detectMin, int detectMax, int16_t* xyMin, int* nMin, int16_t* xyMax, int* nMax, int cap) {
	const HostImg<const float> hin{intensity, start, stride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	if ((detectMin && !nMin) || (detectMax && !nMax) || cap < 0 || (cap > 0 && ((detectMin && !xyMin) || (detectMax && !xyMax))))
		return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	if (nMin) *nMin = 0;
	if (nMax) *nMax = 0;
	CtxScratch* sc = scratchOf(ctx);
	DevImg<float> din;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)std::max(cap, 1) * 8));
	BHIP_TRY(sc->out1.reserve(ctx, 16));
	int16_t* dmin = sc->out0.as<int16_t>();
	BHIP_TRY(nonmaxMinMaxDevice(ctx, din, radius, thresholdMin, thresholdMax, border, detectMin != 0, detectMax != 0, dmin, sc->out1.as<int>(),
								dmin + (size_t)cap * 2, sc->out1.as<int>() + 1, cap));
	return fetchTwoLists(ctx, cap, detectMin ? xyMin : nullptr, nMin, detectMax ? xyMax : nullptr, nMax);
}

int bhip_nonmax_block_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long imageStride, int stride, int width, int height, int batch, int radius,
							  float threshold, int border, int16_t* dev_xy, int cap, int* dev_n) {
	CHECK_CTX(ctx);
	const DevImg<const float> img{dev_intensity, imageStride, stride, width, height, batch};
	CHECK_IMG(ctx, img);
	if (!dev_n || cap < 0 || (cap > 0 && !dev_xy)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	return nonmaxDevice(ctx, img, radius, threshold, border, dev_xy, cap, dev_n);
}

int bhip_nonmax_block_f32(bhip_ctx* ctx, const float* intensity, int start, int stride, int width, int height, int radius, float threshold,
						  int border, int16_t* xy, int cap, int* n) {
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
	BHIP_TRY(nonmaxDevice(ctx, din, radius, threshold, border, sc->out0.as<int16_t>(), cap, sc->out1.as<int>()));
	BHIP_HIP(ctx, hipMemcpyAsync(ctx->hostScratch.p, sc->out1.p, 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the count decides how much of the list to copy
	*n = ctx->hostScratch.as<int>()[0];
	const int ncopy = std::min(*n, cap);
	if (ncopy == 0) return BHIP_OK;
	BHIP_HIP(ctx, hipMemcpyAsync(xy, sc->out0.p, (size_t)ncopy * 4, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

int bhip_fast_u8(bhip_ctx* ctx, const uint8_t* image, int start, int stride, int width, int height, int pixelTol, int minContinuous, double maxFeaturesFraction,
				 float* intensity, int iStart, int iStride, int16_t* xyLow, int* nLow, int16_t* xyHigh, int* nHigh, int cap) {
	return fastHost<uint8_t>(ctx, image, start, stride, width, height, pixelTol, minContinuous, maxFeaturesFraction, intensity, iStart, iStride, xyLow, nLow, xyHigh,
							 nHigh, cap);
}
int bhip_fast_f32(bhip_ctx* ctx, const float* image, int start, int stride, int width, int height, float pixelTol, int minContinuous, double maxFeaturesFraction,
				  float* intensity, int iStart, int iStride, int16_t* xyLow, int* nLow, int16_t* xyHigh, int* nHigh, int cap) {
	return fastHost<float>(ctx, image, start, stride, width, height, pixelTol, minContinuous, maxFeaturesFraction, intensity, iStart, iStride, xyLow, nLow, xyHigh,
						   nHigh, cap);
}
int bhip_fast_dev_u8(bhip_ctx* ctx, const uint8_t* dev_img, long long imageStride, int stride, int width, int height, int batch, int pixelTol, int minContinuous,
					 double maxFeaturesFraction, float* dev_intensity, long long iImageStride, int iStride, int16_t* dev_xyLow, int* dev_nLow, int16_t* dev_xyHigh,
					 int* dev_nHigh, int cap) {
	return fastDev<uint8_t>(ctx, dev_img, imageStride, stride, width, height, batch, pixelTol, minContinuous, maxFeaturesFraction, dev_intensity, iImageStride, iStride,
							dev_xyLow, dev_nLow, dev_xyHigh, dev_nHigh, cap);
}
int bhip_fast_dev_f32(bhip_ctx* ctx, const float* dev_img, long long imageStride, int stride, int width, int height, int batch, float pixelTol, int minContinuous,
					  double maxFeaturesFraction, float* dev_intensity, long long iImageStride, int iStride, int16_t* dev_xyLow, int* dev_nLow, int16_t* dev_xyHigh,
					  int* dev_nHigh, int cap) {
	return fastDev<float>(ctx, dev_img, imageStride, stride, width, height, batch, pixelTol, minContinuous, maxFeaturesFraction, dev_intensity, iImageStride, iStride,
						  dev_xyLow, dev_nLow, dev_xyHigh, dev_nHigh, cap);
}

int bhip_select_nbest_f32(bhip_ctx* ctx, const float* intensity, int start, int stride, int width, int height, const int16_t* xy, int n, int target,
						  int positive, int16_t* out_xy, int* out_n) {
	const HostImg<const float> hin{intensity, start, stride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	if (n < 0 || !out_n || (n > 0 && (!xy || !out_xy))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad corner list");
	for (int i = 0; i < n; i++)
		if (xy[2 * i] < 0 || xy[2 * i] >= width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= height)
			return bhip_fail(ctx, BHIP_ERR_INVALID, "corner outside the intensity image");   // GrayF32.get would throw ImageAccessException
	if (n <= target) {
		// SelectNBestFeatures.java:54-60: already few enough, an unpruned copy in the original order
		if (n > 0) memcpy(out_xy, xy, (size_t)n * 4);
		*out_n = n;
		return BHIP_OK;
	}
	*out_n = 0;
	if (target <= 0) return BHIP_OK;   // n > target, nothing to keep (QuickSelect with k = 0 is never reached with a positive N in the reference)
	CtxScratch* sc = scratchOf(ctx);
	DevImg<float> din;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	BHIP_TRY(sc->in1.reserve(ctx, (size_t)n * 4));
	BHIP_TRY(sc->tmp0.reserve(ctx, (size_t)n * 4));
	BHIP_TRY(sc->tmp1.reserve(ctx, (size_t)n * 4));
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)target * 4));
	BHIP_HIP(ctx, hipMemcpyAsync(sc->in1.p, xy, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_TRY(bhip_launch_select_nbest_xy(ctx, din, sc->in1.as<int16_t>(), n, target, positive != 0, sc->tmp0.as<float>(),
										 sc->tmp1.as<int>(), sc->out0.as<int16_t>()));
	BHIP_HIP(ctx, hipMemcpyAsync(out_xy, sc->out0.p, (size_t)target * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	*out_n = target;
	return BHIP_OK;
}

// ---- integer image variants, stage level ----
int bhip_integral_u8_s32(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int32_t* out, int outStart, int outStride) {
	return hostInOut<uint8_t, int32_t>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, false, false, nullptr,
									   [&](auto din, auto dout) { return bhip_launch_integral_u8(ctx, din, dout); });
}
int bhip_hessian_s32(bhip_ctx* ctx, const int32_t* ii, int iiStart, int iiStride, int width, int height, int skip, int size, float* out, int outStart,
					 int outStride) {
	return hessianHost<int32_t>(ctx, {ii, iiStart, iiStride, width, height}, skip, size, out, outStart, outStride);
}

}  // extern "C"
