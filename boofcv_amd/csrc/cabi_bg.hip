// ---- stationary background models (background.hip): FactoryBackgroundModel.stationaryBasic / stationaryGaussian / stationaryGmm ----
#include "cabi.h"

// everything a background object holds on its context's device (CtxChild)
struct BgDevice {
	DevBuf model, state, stageFrames, stageMasks;
};
struct bhip_bg : CtxChild<BgDevice> {
	BgShape sh{};
	BgConfig cfg{};
	bool u8 = false;
	std::vector<int> stateHost;   // [streams][2]: initialised, BackgroundGmmCommon.unknownValue; the device copy follows before the next launch
	bool stateDirty = true;
	int bands() const { return sh.bands ? sh.bands : 1; }
	long long plane() const { return (long long)sh.width * sh.height; }
	long long modelFloats() const { return plane() * bhip_bg_components(sh); }
};

#define CHECK_BG(g)                     \
	if (!(g)) return BHIP_ERR_INVALID;  \
	bhip_ctx* ctx = (g)->ctx;           \
	CHECK_CTX(ctx)

// the kernel reads the per-stream state from device memory; the launches that read the old copy have finished before it is replaced
static int bgSyncState(bhip_bg* g) {
	if (!g->stateDirty) return BHIP_OK;
	bhip_ctx* ctx = g->ctx;
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	BHIP_HIP(ctx, hipMemcpy(g->state.p, g->stateHost.data(), g->stateHost.size() * sizeof(int), hipMemcpyHostToDevice));
	g->stateDirty = false;
	return BHIP_OK;
}

// rejected: what the config's checkValidity or the class's constructor throws for (nullptr: nothing); reported once ctx is known to be live
static int bgCreate(bhip_ctx* ctx, int alg, const BgConfig& cfg, const char* rejected, int maxGaussians, int family, int pixelType, int bands, int width, int height,
					int streams, bhip_bg** out) {
	if (out) *out = nullptr;
	return createChild(ctx, out, [&](std::unique_ptr<bhip_bg>& g) -> int {
		if (!out) return bhip_fail(ctx, BHIP_ERR_INVALID, "null output");
		if (rejected) return bhip_fail(ctx, BHIP_ERR_INVALID, rejected);
		if (width <= 0 || height <= 0 || streams <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "background model: width, height and streams must be positive");
		if (family != BHIP_IMAGE_GRAY && family != BHIP_IMAGE_PLANAR && family != BHIP_IMAGE_INTERLEAVED) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown image type");
		if (family != BHIP_IMAGE_GRAY && bands < 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "background model: a multi-band image has at least one band");
		if (family == BHIP_IMAGE_INTERLEAVED) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "background models on the GPU: Gray and Planar images; for interleaved images use the Java path");
		if (pixelType != BHIP_PIXEL_U8 && pixelType != BHIP_PIXEL_F32) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "background models on the GPU: GrayU8 and GrayF32 bands");
		if (family == BHIP_IMAGE_PLANAR && bands > BHIP_BG_MAX_BANDS) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "background models on the GPU: at most 4 bands");
		if (alg == BHIP_BG_GMM && maxGaussians > BHIP_BG_MAX_GAUSSIANS) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "GMM background on the GPU: at most 8 Gaussians per pixel");
		CHECK_CTX(ctx);
		g.reset(new (std::nothrow) bhip_bg());
		if (!g) return bhip_fail(ctx, BHIP_ERR_NOMEM, "out of host memory");
		g->ctx = ctx;
		g->sh = {alg, family == BHIP_IMAGE_GRAY ? 0 : bands, alg == BHIP_BG_GMM ? maxGaussians : 1, width, height, streams};
		g->cfg = cfg;
		g->u8 = pixelType == BHIP_PIXEL_U8;
		g->stateHost.assign((size_t)streams * 2, 0);
		const size_t bytes = (size_t)g->modelFloats() * streams * sizeof(float);
		BHIP_TRY(g->model.reserve(ctx, bytes));
		BHIP_TRY(g->state.reserve(ctx, g->stateHost.size() * sizeof(int)));
		BHIP_HIP(ctx, hipMemsetAsync(g->model.p, 0, bytes, ctx->stream));
		BHIP_TRY(bhip_ctx_synchronize(ctx));
		return BHIP_OK;
	});
}

template <class T>
static int bgCheckCall(bhip_bg* g, const BgFrames<const T>& f, const BgFrames<uint8_t>& m, bool needMasks) {
	bhip_ctx* ctx = g->ctx;
	if (g->u8 != (sizeof(T) == 1)) return bhip_fail(ctx, BHIP_ERR_INVALID, g->u8 ? "this background model was created for U8 frames" : "this background model was created for F32 frames");
	if (!f.data || f.numFrames < 1 || f.stride < g->sh.width) return bhip_fail(ctx, BHIP_ERR_INVALID, "background model: bad frames (null, numFrames < 1 or stride < width)");
	if (needMasks && !m.data) return bhip_fail(ctx, BHIP_ERR_INVALID, "background model: no mask");
	if (m.data && m.stride < g->sh.width) return bhip_fail(ctx, BHIP_ERR_INVALID, "background model: mask stride < width");
	return BHIP_OK;
}

template <class T>
static int bgUpdateDevice(bhip_bg* g, const BgFrames<const T>& f, const BgFrames<uint8_t>& m) {
	bhip_ctx* ctx = g->ctx;
	BHIP_TRY(bgSyncState(g));
	BHIP_TRY(bhip_launch_background<T>(ctx, g->sh, g->cfg, f, m, g->model.as<float>(), g->state.as<int>(), false));
	for (int s = 0; s < g->sh.streams; s++)
		if (!g->stateHost[2 * s]) { g->stateHost[2 * s] = 1; g->stateDirty = true; }
	return BHIP_OK;
}
template <class T>
static int bgSegmentDevice(bhip_bg* g, const BgFrames<const T>& f, const BgFrames<uint8_t>& m) {
	bhip_ctx* ctx = g->ctx;
	// BackgroundStationaryGmm_SB.java:86, _MB.java:90: segment() on an initialised model installs the unknown value in `common`
	if (g->sh.alg == BHIP_BG_GMM)
		for (int s = 0; s < g->sh.streams; s++)
			if (g->stateHost[2 * s] && g->stateHost[2 * s + 1] != g->cfg.unknownValue) { g->stateHost[2 * s + 1] = g->cfg.unknownValue; g->stateDirty = true; }
	BHIP_TRY(bgSyncState(g));
	return bhip_launch_background<T>(ctx, g->sh, g->cfg, f, m, g->model.as<float>(), g->state.as<int>(), true);
}

template <class T>
static int bgUpdateDev(bhip_bg* g, const T* dev_frames, long long streamStride, long long frameStride, long long bandStride, int stride, int numFrames,
					   uint8_t* dev_masks, long long mStreamStride, long long mFrameStride, int mStride) {
	CHECK_BG(g);
	const BgFrames<const T> f{dev_frames, streamStride, frameStride, bandStride, stride, numFrames};
	const BgFrames<uint8_t> m{dev_masks, mStreamStride, mFrameStride, 0, mStride, numFrames};
	BHIP_TRY(bgCheckCall<T>(g, f, m, false));
	return bgUpdateDevice<T>(g, f, m);
}
template <class T>
static int bgSegmentDev(bhip_bg* g, const T* dev_frames, long long streamStride, long long bandStride, int stride, uint8_t* dev_masks, long long mStreamStride,
						int mStride) {
	CHECK_BG(g);
	const BgFrames<const T> f{dev_frames, streamStride, 0, bandStride, stride, 1};
	const BgFrames<uint8_t> m{dev_masks, mStreamStride, 0, 0, mStride, 1};
	BHIP_TRY(bgCheckCall<T>(g, f, m, true));
	return bgSegmentDevice<T>(g, f, m);
}

// host frames -> a dense [stream][frame][band][h][w] device batch; masks come back from a dense [stream][frame][h][w] one
template <class T>
static int bgHost(bhip_bg* g, bool segment, const T* frames, long long start, long long streamStride, long long frameStride, long long bandStride, int stride,
				  int numFrames, uint8_t* masks, long long mStart, long long mStreamStride, long long mFrameStride, int mStride) {
	CHECK_BG(g);
	const BgFrames<const T> hf{frames, streamStride, frameStride, bandStride, stride, numFrames};
	const BgFrames<uint8_t> hm{masks, mStreamStride, mFrameStride, 0, mStride, numFrames};
	BHIP_TRY(bgCheckCall<T>(g, hf, hm, segment));
	const int w = g->sh.width, h = g->sh.height, B = g->bands(), S = g->sh.streams;
	const long long plane = g->plane();
	BHIP_TRY(g->stageFrames.reserve(ctx, (size_t)plane * B * numFrames * S * sizeof(T)));
	if (masks) BHIP_TRY(g->stageMasks.reserve(ctx, (size_t)plane * numFrames * S));
	T* df = g->stageFrames.as<T>();
	for (int s = 0; s < S; s++)
		for (int t = 0; t < numFrames; t++)
			for (int b = 0; b < B; b++)
				BHIP_TRY(upload<T>(ctx, df + ((long long)(s * numFrames + t) * B + b) * plane, w, frames + start + s * streamStride + t * frameStride + b * bandStride, 0,
								   stride, w, h, ctx->stream));
	const BgFrames<const T> f{df, plane * B * numFrames, plane * B, plane, w, numFrames};
	const BgFrames<uint8_t> m{masks ? g->stageMasks.as<uint8_t>() : nullptr, plane * numFrames, plane, 0, w, numFrames};
	BHIP_TRY(segment ? bgSegmentDevice<T>(g, f, m) : bgUpdateDevice<T>(g, f, m));
	if (masks)
		for (int s = 0; s < S; s++)
			for (int t = 0; t < numFrames; t++)
				BHIP_TRY(download<uint8_t>(ctx, masks + mStart + s * mStreamStride + t * mFrameStride, 0, mStride, m.data + (long long)(s * numFrames + t) * plane, w, w, h,
										   ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

// the device planes [component][y][x] <-> the reference's layout: the same planes for Basic and Gaussian, [y][x][component] for GMM
static void bgPermute(const bhip_bg* g, const float* in, float* out, bool toReference) {
	const long long plane = g->plane();
	const int C = bhip_bg_components(g->sh);
	if (g->sh.alg != BHIP_BG_GMM) { memcpy(out, in, (size_t)plane * C * sizeof(float)); return; }
	for (long long p = 0; p < plane; p++)
		for (int c = 0; c < C; c++) {
			if (toReference) out[p * C + c] = in[c * plane + p];
			else out[c * plane + p] = in[p * C + c];
		}
}

static int bgSetter(bhip_bg* g, unsigned int algs, float BgConfig::*field, float v) {
	CHECK_BG(g);
	if (!(algs >> g->sh.alg & 1u)) return bhip_fail(ctx, BHIP_ERR_INVALID, "this background algorithm has no such parameter");
	g->cfg.*field = v;
	return BHIP_OK;
}

extern "C" {

int bhip_bg_create_basic(bhip_ctx* ctx, const bhip_bg_basic_cfg* cfg, int family, int pixelType, int bands, int width, int height, int streams, bhip_bg** out) {
	BgConfig c{};
	const char* bad = nullptr;
	// ConfigBackgroundBasic.checkValidity, BackgroundStationaryBasic's constructor
	if (!cfg) bad = "ConfigBackgroundBasic: threshold has no default";
	else if (cfg->learnRate < 0 || cfg->learnRate > 1) bad = "Learn rate must be 0 <= rate <= 1";
	else if (cfg->threshold <= 0) bad = "threshold must be > 0";
	else { c.learnRate = cfg->learnRate; c.threshold = cfg->threshold; }
	c.unknownValue = 0;   // FactoryBackgroundModel.java:47-64 does not forward config.unknownValue
	return bgCreate(ctx, BHIP_BG_BASIC, c, bad, 1, family, pixelType, bands, width, height, streams, out);
}
int bhip_bg_create_gaussian(bhip_ctx* ctx, const bhip_bg_gaussian_cfg* cfg, int family, int pixelType, int bands, int width, int height, int streams, bhip_bg** out) {
	BgConfig c{};
	const char* bad = nullptr;
	// ConfigBackgroundGaussian.checkValidity, BackgroundStationaryGaussian's constructor, BackgroundModel.setUnknownValue
	if (!cfg) bad = "ConfigBackgroundGaussian: threshold has no default";
	else if (cfg->learnRate < 0 || cfg->learnRate > 1) bad = "Learn rate must be 0 <= rate <= 1";
	else if (cfg->threshold <= 0) bad = "threshold must be > 0";
	else if (cfg->initialVariance == 0) bad = "Don't set initialVariance to zero, set it to Float.MIN_VALUE instead";
	else if (cfg->initialVariance < 0) bad = "Variance must be set to a value larger than zero";
	else if (cfg->minimumDifference < 0) bad = "minimumDifference must be >= 0";
	else if (cfg->unknownValue < 0 || cfg->unknownValue > 255) bad = "out of range. 0 to 255";
	else {
		c.learnRate = cfg->learnRate; c.threshold = cfg->threshold; c.initialVariance = cfg->initialVariance; c.minimumDifference = cfg->minimumDifference;
		c.unknownValue = cfg->unknownValue;
	}
	return bgCreate(ctx, BHIP_BG_GAUSSIAN, c, bad, 1, family, pixelType, bands, width, height, streams, out);
}
int bhip_bg_create_gmm(bhip_ctx* ctx, const bhip_bg_gmm_cfg* cfg, int family, int pixelType, int bands, int width, int height, int streams, bhip_bg** out) {
	bhip_bg_gmm_cfg d;
	if (cfg) d = *cfg; else bhip_bg_gmm_cfg_default(&d);
	BgConfig c{};
	const char* bad = nullptr;
	// ConfigBackgroundGmm.checkValidity, BackgroundGmmCommon's constructor, BackgroundModel.setUnknownValue
	if (d.learningPeriod <= 0) bad = "Learning period must be more than zero";
	else if (d.decayCoefient < 0) bad = "Decay coeffient must be more than or equal to zero";
	else if (d.initialVariance == 0) bad = "Don't set initialVariance to zero, set it to Float.MIN_VALUE instead";
	else if (d.initialVariance < 0) bad = "Variance must be set to a value larger than zero";
	else if (d.numberOfGaussian >= 256 || d.numberOfGaussian <= 0) bad = "Maximum number of gaussians per pixel is 255";
	else if (d.unknownValue < 0 || d.unknownValue > 255) bad = "out of range. 0 to 255";
	c.learningPeriod = d.learningPeriod; c.decay = d.decayCoefient; c.initialVariance = d.initialVariance;
	c.maxDistance = d.maxDistance; c.significantWeight = d.significantWeight;   // FactoryBackgroundModel.java:219-222
	c.unknownValue = d.unknownValue;
	return bgCreate(ctx, BHIP_BG_GMM, c, bad, d.numberOfGaussian, family, pixelType, bands, width, height, streams, out);
}
int bhip_bg_destroy(bhip_bg* g) { return destroyChild(g); }
int bhip_bg_reset(bhip_bg* g, int stream) {
	CHECK_BG(g);
	if (stream >= g->sh.streams) return bhip_fail(ctx, BHIP_ERR_INVALID, "no such stream");
	for (int s = 0; s < g->sh.streams; s++)
		if ((stream < 0 || s == stream) && g->stateHost[2 * s]) { g->stateHost[2 * s] = 0; g->stateDirty = true; }
	return BHIP_OK;
}
int bhip_bg_set_unknown_value(bhip_bg* g, int unknownValue) {
	CHECK_BG(g);
	if (unknownValue < 0 || unknownValue > 255) return bhip_fail(ctx, BHIP_ERR_INVALID, "out of range. 0 to 255");
	g->cfg.unknownValue = unknownValue;
	return BHIP_OK;
}
int bhip_bg_set_common_unknown_value(bhip_bg* g, int unknownValue) {
	CHECK_BG(g);
	if (g->sh.alg != BHIP_BG_GMM) return bhip_fail(ctx, BHIP_ERR_INVALID, "this background algorithm has no such parameter");
	if (unknownValue < 0 || unknownValue > 255) return bhip_fail(ctx, BHIP_ERR_INVALID, "out of range. 0 to 255");
	for (int s = 0; s < g->sh.streams; s++)
		if (g->stateHost[2 * s + 1] != unknownValue) { g->stateHost[2 * s + 1] = unknownValue; g->stateDirty = true; }
	return BHIP_OK;
}
#define BG_ALGS(a) (1u << (a))
int bhip_bg_set_threshold(bhip_bg* g, float v) { return bgSetter(g, BG_ALGS(BHIP_BG_BASIC) | BG_ALGS(BHIP_BG_GAUSSIAN), &BgConfig::threshold, v); }
int bhip_bg_set_learn_rate(bhip_bg* g, float v) { return bgSetter(g, BG_ALGS(BHIP_BG_BASIC) | BG_ALGS(BHIP_BG_GAUSSIAN), &BgConfig::learnRate, v); }
int bhip_bg_set_initial_variance(bhip_bg* g, float v) { return bgSetter(g, BG_ALGS(BHIP_BG_GAUSSIAN) | BG_ALGS(BHIP_BG_GMM), &BgConfig::initialVariance, v); }
int bhip_bg_set_minimum_difference(bhip_bg* g, float v) { return bgSetter(g, BG_ALGS(BHIP_BG_GAUSSIAN), &BgConfig::minimumDifference, v); }
int bhip_bg_set_learning_period(bhip_bg* g, float v) { return bgSetter(g, BG_ALGS(BHIP_BG_GMM), &BgConfig::learningPeriod, v); }
int bhip_bg_set_significant_weight(bhip_bg* g, float v) { return bgSetter(g, BG_ALGS(BHIP_BG_GMM), &BgConfig::significantWeight, v); }
int bhip_bg_set_max_distance(bhip_bg* g, float v) { return bgSetter(g, BG_ALGS(BHIP_BG_GMM), &BgConfig::maxDistance, v); }

int bhip_bg_update_dev_u8(bhip_bg* g, const uint8_t* dev_frames, long long streamStride, long long frameStride, long long bandStride, int stride, int numFrames,
						  uint8_t* dev_masks, long long mStreamStride, long long mFrameStride, int mStride) {
	return bgUpdateDev<uint8_t>(g, dev_frames, streamStride, frameStride, bandStride, stride, numFrames, dev_masks, mStreamStride, mFrameStride, mStride);
}
int bhip_bg_update_dev_f32(bhip_bg* g, const float* dev_frames, long long streamStride, long long frameStride, long long bandStride, int stride, int numFrames,
						   uint8_t* dev_masks, long long mStreamStride, long long mFrameStride, int mStride) {
	return bgUpdateDev<float>(g, dev_frames, streamStride, frameStride, bandStride, stride, numFrames, dev_masks, mStreamStride, mFrameStride, mStride);
}
int bhip_bg_segment_dev_u8(bhip_bg* g, const uint8_t* dev_frames, long long streamStride, long long bandStride, int stride, uint8_t* dev_masks,
						   long long mStreamStride, int mStride) {
	return bgSegmentDev<uint8_t>(g, dev_frames, streamStride, bandStride, stride, dev_masks, mStreamStride, mStride);
}
int bhip_bg_segment_dev_f32(bhip_bg* g, const float* dev_frames, long long streamStride, long long bandStride, int stride, uint8_t* dev_masks,
							long long mStreamStride, int mStride) {
	return bgSegmentDev<float>(g, dev_frames, streamStride, bandStride, stride, dev_masks, mStreamStride, mStride);
}
int bhip_bg_update_u8(bhip_bg* g, const uint8_t* frames, long long start, long long streamStride, long long frameStride, long long bandStride, int stride,
					  int numFrames, uint8_t* masks, long long mStart, long long mStreamStride, long long mFrameStride, int mStride) {
	return bgHost<uint8_t>(g, false, frames, start, streamStride, frameStride, bandStride, stride, numFrames, masks, mStart, mStreamStride, mFrameStride, mStride);
}
int bhip_bg_update_f32(bhip_bg* g, const float* frames, long long start, long long streamStride, long long frameStride, long long bandStride, int stride,
					   int numFrames, uint8_t* masks, long long mStart, long long mStreamStride, long long mFrameStride, int mStride) {
	return bgHost<float>(g, false, frames, start, streamStride, frameStride, bandStride, stride, numFrames, masks, mStart, mStreamStride, mFrameStride, mStride);
}
int bhip_bg_segment_u8(bhip_bg* g, const uint8_t* frames, long long start, long long streamStride, long long bandStride, int stride, uint8_t* masks,
					   long long mStart, long long mStreamStride, int mStride) {
	return bgHost<uint8_t>(g, true, frames, start, streamStride, 0, bandStride, stride, 1, masks, mStart, mStreamStride, 0, mStride);
}
int bhip_bg_segment_f32(bhip_bg* g, const float* frames, long long start, long long streamStride, long long bandStride, int stride, uint8_t* masks,
						long long mStart, long long mStreamStride, int mStride) {
	return bgHost<float>(g, true, frames, start, streamStride, 0, bandStride, stride, 1, masks, mStart, mStreamStride, 0, mStride);
}

int bhip_bg_model_floats(bhip_bg* g, long long* floats) {
	CHECK_BG(g);
	if (!floats) return bhip_fail(ctx, BHIP_ERR_INVALID, "null output");
	*floats = g->modelFloats();
	return BHIP_OK;
}
int bhip_bg_fetch_model(bhip_bg* g, int stream, float* model) {
	CHECK_BG(g);
	if (stream < 0 || stream >= g->sh.streams || !model) return bhip_fail(ctx, BHIP_ERR_INVALID, "no such stream, or no output");
	if (!g->stateHost[2 * stream]) return bhip_fail(ctx, BHIP_ERR_INVALID, "the stream has no model yet");
	const long long n = g->modelFloats();
	std::vector<float> planes((size_t)n);
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	BHIP_HIP(ctx, hipMemcpy(planes.data(), g->model.as<float>() + stream * n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
	bgPermute(g, planes.data(), model, true);
	return BHIP_OK;
}
int bhip_bg_store_model(bhip_bg* g, int stream, const float* model) {
	CHECK_BG(g);
	if (stream < 0 || stream >= g->sh.streams || !model) return bhip_fail(ctx, BHIP_ERR_INVALID, "no such stream, or no model");
	const long long n = g->modelFloats();
	std::vector<float> planes((size_t)n);
	bgPermute(g, model, planes.data(), false);
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	BHIP_HIP(ctx, hipMemcpy(g->model.as<float>() + stream * n, planes.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
	if (!g->stateHost[2 * stream]) { g->stateHost[2 * stream] = 1; g->stateDirty = true; }
	return BHIP_OK;
}

}  // extern "C"
