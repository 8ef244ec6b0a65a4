// ---------------------------------------------------------------------------------------------------------------
// Thresholding front end: FactoryThresholdBinary.threshold(ConfigThreshold, GrayU8 | GrayF32) and the GrayU8 blurs (threshold.hip).
// A configuration is first turned into a plan -- the checks of the reference and of the GPU paths, the radius or the block grid -- without
// touching the device, so a refused call writes nothing.  The _dev exports run the plan on the caller's views, asynchronous on the ctx
// stream; the host exports stage their views and run the same implementation with batch 1.
// ---------------------------------------------------------------------------------------------------------------
#include "cabi.h"

// ConfigLength.computeI (T:struct/ConfigLength.java:53-80)
static int configLengthI(double length, double fraction, double totalLength) {
	double size = length;
	if (fraction >= 0) size = std::max(fraction * totalLength, length);
	if (!(size >= 0)) return -1;
	size += 0.5;
	return size >= 2147483647.0 ? 2147483647 : (int)size;
}
// ThresholdBlock.selectBlockSize (:112-127)
static void selectBlockSize(int width, int height, int requested, int& bw, int& bh) {
	bh = height < requested ? height : height / (height / requested);
	bw = width < requested ? width : width / (width / requested);
}
static int javaD2I(double v) {
	if (v != v) return 0;
	if (v >= 2147483647.0) return 2147483647;
	if (v <= -2147483648.0) return -2147483647 - 1;
	return (int)v;
}

struct ThreshPlan {
	int type;
	int radius;            // LOCAL_*
	ThreshBlocks blocks;   // BLOCK_*
};
// isU8: the image type.  BHIP_ERR_UNSUPPORTED / BHIP_ERR_INVALID as include/boofhip.h lists them; nothing on the device is touched
static int threshPlan(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, bool isU8, int width, int height, ThreshPlan& p) {
	if (!cfg) return bhip_fail(ctx, BHIP_ERR_INVALID, "null threshold configuration");
	p.type = cfg->type;
	const int side = std::min(width, height);
	switch (cfg->type) {
	case BHIP_THRESHOLD_FIXED:
		return BHIP_OK;
	case BHIP_THRESHOLD_GLOBAL_OTSU:
		if (!isU8) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "GLOBAL_OTSU is implemented for GrayU8");
		if (cfg->minPixelValue != 0 || cfg->maxPixelValue != 255) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "GLOBAL_OTSU is implemented for the pixel range 0..255");
		return BHIP_OK;
	case BHIP_THRESHOLD_LOCAL_MEAN:
	case BHIP_THRESHOLD_LOCAL_GAUSSIAN:
		p.radius = configLengthI(cfg->widthLength, cfg->widthFraction, side) / 2;
		if (p.radius <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, cfg->type == BHIP_THRESHOLD_LOCAL_MEAN ? "Radius must be > 0" : "Sigma must be > 0");
		if (!isU8 && 2LL * p.radius + 1 > 255) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "GrayF32 blur kernels are limited to 255 taps");
		return BHIP_OK;
	case BHIP_THRESHOLD_BLOCK_MIN_MAX:
	case BHIP_THRESHOLD_BLOCK_MEAN:
	case BHIP_THRESHOLD_BLOCK_OTSU: {
		if (cfg->type == BHIP_THRESHOLD_BLOCK_OTSU && !isU8) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "BLOCK_OTSU is implemented for GrayU8");
		const int requested = configLengthI(cfg->widthLength, cfg->widthFraction, side);
		if (requested <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "the requested block width must be > 0");   // the reference divides by it
		ThreshBlocks& b = p.blocks;
		b.kind = cfg->type;
		selectBlockSize(width, height, requested, b.bw, b.bh);
		b.nbx = width / b.bw; b.nby = height / b.bh;
		b.local = cfg->thresholdFromLocalBlocks != 0; b.down = cfg->down != 0; b.useOtsu2 = cfg->useOtsu2 != 0;
		b.scale = cfg->scale; b.minimumSpread = cfg->minimumSpread; b.tuning = cfg->tuning;
		return BHIP_OK;
	}
	case BHIP_THRESHOLD_GLOBAL_ENTROPY: case BHIP_THRESHOLD_GLOBAL_LI: case BHIP_THRESHOLD_GLOBAL_HUANG: case BHIP_THRESHOLD_LOCAL_OTSU:
	case BHIP_THRESHOLD_LOCAL_SAVOLA: case BHIP_THRESHOLD_LOCAL_NICK:
		return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "threshold type not implemented on the GPU");
	}
	return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown type");
}

// The Kernel1D_S32 of FactoryKernelGaussian.gaussian(Kernel1D_S32, -1, radius) in device memory, kept per context for the radius last used:
// a steady stream of calls with one configuration uploads (and synchronises for the upload) once.
static int gaussianTapsU8(bhip_ctx* ctx, int radius, const int32_t** devTaps) {
	CtxScratch* sc = scratchOf(ctx);
	if (sc->thresholdTapsRadius != radius) {
		const std::vector<int32_t> k = bhip_gaussian1d_s32(radius);
		sc->thresholdTapsRadius = 0;
		BHIP_TRY(sc->thresholdTaps.reserve(ctx, k.size() * 4));
		BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // a launch queued with the previous taps has read them
		BHIP_HIP(ctx, hipMemcpy(sc->thresholdTaps.p, k.data(), k.size() * 4, hipMemcpyHostToDevice));
		sc->thresholdTapsRadius = radius;
	}
	*devTaps = sc->thresholdTaps.as<int32_t>();
	return BHIP_OK;
}
static bool fusedU8(int rx, int ry, int width, int height) {
	return rx == ry && rx <= BHIP_THRESH_FUSED_MAX_RADIUS && 2 * rx + 1 <= width && 2 * ry + 1 <= height;
}
// BlurImageOps.mean / gaussian on GrayU8 (gaussian: the Kernel1D_S32 of the radius, rx == ry), or with `compare` the local threshold built on
// it: `out` is then the 0/1 image.  One fused launch where the radius and the image allow it, with the taps as a kernel argument; otherwise two
// passes through context scratch (and a compare pass), with the taps in device memory.
static int blurU8(bhip_ctx* ctx, bool gaussian, int rx, int ry, DevImg<const uint8_t> in, DevImg<uint8_t> out, bool compare, float scale, bool down) {
	if (fusedU8(rx, ry, in.width, in.height)) {
		std::vector<int32_t> k;
		if (gaussian) k = bhip_gaussian1d_s32(rx);
		return bhip_launch_blur_u8_fused(ctx, gaussian ? k.data() : nullptr, rx, in, out, compare, scale, down);
	}
	const int32_t* taps = nullptr;
	if (gaussian) BHIP_TRY(gaussianTapsU8(ctx, rx, &taps));
	DevBuf& buf = scratchOf(ctx)->threshold;
	const size_t plane = (size_t)in.width * in.height * in.batch;
	BHIP_TRY(buf.reserve(ctx, (compare ? 2 : 1) * plane));
	const DevImg<uint8_t> tmp = bhip_img_over<uint8_t>(buf, in.width, in.width, in.height, in.batch);
	BHIP_TRY(bhip_launch_blur_u8_pass(ctx, false, taps, rx, in, tmp));
	if (!compare) return bhip_launch_blur_u8_pass(ctx, true, taps, ry, tmp, out);
	DevImg<uint8_t> blur = tmp;
	blur.data += plane;
	BHIP_TRY(bhip_launch_blur_u8_pass(ctx, true, taps, ry, tmp, blur));
	return bhip_launch_local_compare<uint8_t>(ctx, in, blur, out, scale, down);
}

static int localU8(bhip_ctx* ctx, const bhip_threshold_cfg& cfg, int radius, DevImg<const uint8_t> in, DevImg<uint8_t> out) {
	// the filters hand their double scale to a float parameter
	return blurU8(ctx, cfg.type == BHIP_THRESHOLD_LOCAL_GAUSSIAN, radius, radius, in, out, true, (float)cfg.scale, cfg.down != 0);
}
// GrayF32: the blurs the library already has bit-exact (their float running sums keep the reference's order), then the compare
static int localF32(bhip_ctx* ctx, const bhip_threshold_cfg& cfg, int radius, DevImg<const float> in, DevImg<uint8_t> out) {
	DevBuf& buf = scratchOf(ctx)->threshold;
	const int pitch = pitch4(in.width);
	const size_t plane = (size_t)pitch * in.height;
	BHIP_TRY(buf.reserve(ctx, 2 * plane * in.batch * 4));
	const DevImg<float> blur = bhip_img_over<float>(buf, pitch, in.width, in.height, in.batch);
	if (cfg.type == BHIP_THRESHOLD_LOCAL_GAUSSIAN) {
		BHIP_TRY(gaussianImpl(ctx, -1, radius, in, blur));
	} else {
		DevImg<float> tmp = blur;   // the horizontal pass
		tmp.data += plane * in.batch;
		BHIP_TRY(bhip_launch_mean(ctx, false, in, tmp, radius));
		BHIP_TRY(bhip_launch_mean(ctx, true, tmp, blur, radius));
	}
	return bhip_launch_local_compare<float>(ctx, in, blur, out, (float)cfg.scale, cfg.down != 0);
}

template <class T>
static int blocksImpl(bhip_ctx* ctx, const ThreshBlocks& b, DevImg<const T> in, DevImg<uint8_t> out) {
	// the Otsu histograms are 1 KiB per block: at most 256 MiB of them at a time
	int chunk = in.batch;
	if (b.kind == BHIP_THRESHOLD_BLOCK_OTSU) chunk = (int)std::max<size_t>(1, std::min<size_t>(in.batch, ((size_t)256 << 20) / bhip_block_threshold_scratch(b.kind, b.nbx, b.nby, 1)));
	DevBuf& buf = scratchOf(ctx)->threshold;
	BHIP_TRY(buf.reserve(ctx, bhip_block_threshold_scratch(b.kind, b.nbx, b.nby, chunk)));
	return bhip_launch_block_threshold<T>(ctx, b, in, out, buf.p, chunk);
}

// GlobalBinaryFilter.process: scale when thresholding down, else 1/scale (0 when scale <= 0)
static double globalScale(const bhip_threshold_cfg& cfg) { return cfg.down ? cfg.scale : (cfg.scale <= 0.0 ? 0.0 : 1.0 / cfg.scale); }

static int thresholdImpl(bhip_ctx* ctx, const bhip_threshold_cfg& cfg, const ThreshPlan& p, DevImg<const uint8_t> in, DevImg<uint8_t> out) {
	const int mode = cfg.down ? BHIP_CMP_LE : BHIP_CMP_GT;
	switch (p.type) {
	case BHIP_THRESHOLD_FIXED:
		return bhip_launch_threshold_global(ctx, in, out, javaD2I(cfg.fixedThreshold), nullptr, mode);
	case BHIP_THRESHOLD_GLOBAL_OTSU: {
		DevBuf& buf = scratchOf(ctx)->threshold;
		BHIP_TRY(buf.reserve(ctx, (size_t)in.batch * 257 * 4));
		int* hist = buf.as<int>();
		int* thr = hist + (size_t)in.batch * 256;
		BHIP_HIP(ctx, hipMemsetAsync(hist, 0, (size_t)in.batch * 256 * 4, ctx->stream));
		BHIP_TRY(bhip_launch_hist_u8(ctx, in, hist));
		BHIP_TRY(bhip_launch_otsu_global(ctx, hist, in.batch, in.width * in.height, globalScale(cfg), thr));
		return bhip_launch_threshold_global(ctx, in, out, 0, thr, mode);
	}
	case BHIP_THRESHOLD_LOCAL_MEAN:
	case BHIP_THRESHOLD_LOCAL_GAUSSIAN:
		return localU8(ctx, cfg, p.radius, in, out);
	default:
		return blocksImpl<uint8_t>(ctx, p.blocks, in, out);
	}
}
static int thresholdImpl(bhip_ctx* ctx, const bhip_threshold_cfg& cfg, const ThreshPlan& p, DevImg<const float> in, DevImg<uint8_t> out) {
	switch (p.type) {
	case BHIP_THRESHOLD_FIXED:
		return bhip_launch_threshold_global(ctx, in, out, (float)cfg.fixedThreshold, nullptr, cfg.down ? BHIP_CMP_LE : BHIP_CMP_GT);
	case BHIP_THRESHOLD_LOCAL_MEAN:
	case BHIP_THRESHOLD_LOCAL_GAUSSIAN:
		return localF32(ctx, cfg, p.radius, in, out);
	default:
		return blocksImpl<float>(ctx, p.blocks, in, out);
	}
}

template <class T>
static int thresholdDev(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, DevImg<const T> in, DevImg<uint8_t> out) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	if (in.batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	ThreshPlan p{};
	BHIP_TRY(threshPlan(ctx, cfg, sizeof(T) == 1, in.width, in.height, p));
	return thresholdImpl(ctx, *cfg, p, in, out);
}
template <class T>
static int thresholdHost(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, HostImg<const T> in, HostImg<uint8_t> out) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	ThreshPlan p{};
	BHIP_TRY(threshPlan(ctx, cfg, sizeof(T) == 1, in.width, in.height, p));
	return hostInOut<T, uint8_t>(ctx, in, out, false, false, nullptr, [&](DevImg<T> din, DevImg<uint8_t> dout) { return thresholdImpl(ctx, *cfg, p, DevImg<const T>(din), dout); });
}

static int meanDevU8(bhip_ctx* ctx, int radiusX, int radiusY, DevImg<const uint8_t> in, DevImg<uint8_t> out) {
	if (radiusX <= 0 || radiusY <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Radius must be > 0");
	return blurU8(ctx, false, radiusX, radiusY, in, out, false, 1.0f, true);
}
static int gaussianDevU8(bhip_ctx* ctx, int radius, DevImg<const uint8_t> in, DevImg<uint8_t> out) {
	if (radius <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Radius must be > 0");
	return blurU8(ctx, true, radius, radius, in, out, false, 1.0f, true);
}

extern "C" {

int bhip_threshold_cfg_default(int type, bhip_threshold_cfg* c) {
	if (!c || type < BHIP_THRESHOLD_FIXED || type > BHIP_THRESHOLD_LOCAL_NICK) return BHIP_ERR_INVALID;
	const bool global = type <= BHIP_THRESHOLD_GLOBAL_HUANG;   // ThresholdType.isGlobal
	c->type = type;
	c->fixedThreshold = 0;
	c->scale = global ? 1.0 : 0.95;   // ConfigThreshold.local sets 0.95 whatever the subclass started from
	c->down = 1;
	c->widthLength = 11;
	c->widthFraction = -1;
	c->minPixelValue = 0;
	c->maxPixelValue = 255;
	c->thresholdFromLocalBlocks = 1;
	c->minimumSpread = 10;
	c->useOtsu2 = 1;
	c->tuning = 0;
	return BHIP_OK;
}

int bhip_threshold_block_size(int width, int height, int requestedWidth, int* blockWidth, int* blockHeight) {
	if (width <= 0 || height <= 0 || requestedWidth <= 0 || !blockWidth || !blockHeight) return BHIP_ERR_INVALID;
	selectBlockSize(width, height, requestedWidth, *blockWidth, *blockHeight);
	return BHIP_OK;
}

int bhip_threshold_dev_u8(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height,
						  int batch, uint8_t* dev_out, long long outImageStride, int outStride) {
	return thresholdDev<uint8_t>(ctx, cfg, {dev_in, inImageStride, inStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_threshold_dev_f32(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, const float* dev_in, long long inImageStride, int inStride, int width, int height,
						   int batch, uint8_t* dev_out, long long outImageStride, int outStride) {
	return thresholdDev<float>(ctx, cfg, {dev_in, inImageStride, inStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_threshold_u8(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out,
					  int outStart, int outStride) {
	return thresholdHost<uint8_t>(ctx, cfg, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height});
}
int bhip_threshold_f32(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, const float* in, int inStart, int inStride, int width, int height, uint8_t* out,
					   int outStart, int outStride) {
	return thresholdHost<float>(ctx, cfg, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height});
}

int bhip_mean_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int radiusX, int radiusY,
					 uint8_t* dev_out, long long outImageStride, int outStride) {
	const DevImg<const uint8_t> in{dev_in, inImageStride, inStride, width, height, batch};
	const DevImg<uint8_t> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	return meanDevU8(ctx, radiusX, radiusY, in, out);
}
int bhip_gaussian_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int radius,
						 uint8_t* dev_out, long long outImageStride, int outStride) {
	const DevImg<const uint8_t> in{dev_in, inImageStride, inStride, width, height, batch};
	const DevImg<uint8_t> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	return gaussianDevU8(ctx, radius, in, out);
}
int bhip_mean_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int radiusX, int radiusY, uint8_t* out, int outStart,
				 int outStride) {
	return hostInOut<uint8_t, uint8_t>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, false, false,
									   radiusX <= 0 || radiusY <= 0 ? "Radius must be > 0" : nullptr,
									   [&](DevImg<uint8_t> din, DevImg<uint8_t> dout) { return meanDevU8(ctx, radiusX, radiusY, din, dout); });
}
int bhip_gaussian_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int radius, uint8_t* out, int outStart, int outStride) {
	return hostInOut<uint8_t, uint8_t>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, false, false,
									   radius <= 0 ? "Radius must be > 0" : nullptr,
									   [&](DevImg<uint8_t> din, DevImg<uint8_t> dout) { return gaussianDevU8(ctx, radius, din, dout); });
}

}  // extern "C"
