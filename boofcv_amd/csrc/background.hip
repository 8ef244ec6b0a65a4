// Stationary background models, host side: the launcher and its dispatch over algorithm and band form.  The kernel template, its design notes
// and the inner dispatch are in background_dev.h; this unit instantiates the Basic and Gaussian kernels, background_gmm_*.hip the GMM ones.
#include "background_dev.h"

template <int ALG, class T>
static void bgLaunch0(int bands, int K, bool seg, dim3 grid, hipStream_t st, const BgParams& P) {
	switch (bands) {
	case 0: bgLaunch1<ALG, T, 1, true>(K, seg, grid, st, P); break;
	case 1: bgLaunch1<ALG, T, 1, false>(K, seg, grid, st, P); break;
	case 2: bgLaunch1<ALG, T, 2, false>(K, seg, grid, st, P); break;
	case 3: bgLaunch1<ALG, T, 3, false>(K, seg, grid, st, P); break;
	default: bgLaunch1<ALG, T, 4, false>(K, seg, grid, st, P); break;
	}
}

int bhip_bg_components(const BgShape& sh) { return bgComponents(sh.alg, sh.bands ? sh.bands : 1, sh.maxGaussians); }

template <class T>
int bhip_launch_background(bhip_ctx* ctx, const BgShape& sh, const BgConfig& cfg, const BgFrames<const T>& f, const BgFrames<uint8_t>& m, float* model,
						   const int* state, bool segment) {
	if (sh.streams <= 0 || f.numFrames <= 0) return BHIP_OK;
	const int B = sh.bands ? sh.bands : 1, C = bhip_bg_components(sh), PX = bgPx(C);
	BgParams P{};
	P.frames = f.data; P.fStreamStride = f.streamStride; P.fFrameStride = f.frameStride; P.fBandStride = f.bandStride; P.fStride = f.stride;
	P.masks = m.data; P.mStreamStride = m.streamStride; P.mFrameStride = m.frameStride; P.mStride = m.stride;
	P.model = model; P.state = state;
	P.w = sh.width; P.h = sh.height; P.T = f.numFrames;
	P.unknownValue = cfg.unknownValue & 255;
	P.neverInit = sh.alg == BHIP_BG_GAUSSIAN && sh.width == 1;
	P.learnRate = sh.alg == BHIP_BG_GMM ? 1.0f / cfg.learningPeriod : cfg.learnRate;
	P.minusLearn = 1.0f - cfg.learnRate;
	// Basic_SB.java:99 threshold*threshold; Basic_PL.java:114 numBands*threshold*threshold, left to right
	P.threshold = sh.alg != BHIP_BG_BASIC ? cfg.threshold : sh.bands ? ((float)B * cfg.threshold) * cfg.threshold : cfg.threshold * cfg.threshold;
	P.initialVariance = cfg.initialVariance;
	P.minimumDifference = cfg.minimumDifference;
	P.adjustedMinimumDifference = cfg.minimumDifference * (float)B;   // Gaussian_PL.java:133
	P.decay = cfg.decay;
	P.maxDistance = sh.bands ? cfg.maxDistance * (float)B : cfg.maxDistance;   // BackgroundGmmCommon.java:116 / :244
	P.significantWeight = cfg.significantWeight;
	// + PX - 1: a row's first lane may start up to PX - 1 columns left of the image
	const dim3 grid((sh.width + PX - 1 + BG_LANES * PX - 1) / (BG_LANES * PX), (sh.height + BG_ROWS - 1) / BG_ROWS, sh.streams);
	static const char* const tags[3][2] = {{"k_bg_basic_update", "k_bg_basic_segment"}, {"k_bg_gaussian_update", "k_bg_gaussian_segment"}, {"k_bg_gmm_update", "k_bg_gmm_segment"}};
	ProfScope ps(ctx, tags[sh.alg][segment], bhip_bg_bytes(sh, (int)sizeof(T), f.numFrames, m.data != nullptr, segment));
	if (sh.alg == BHIP_BG_BASIC) bgLaunch0<BHIP_BG_BASIC, T>(sh.bands, 1, segment, grid, ctx->stream, P);
	else if (sh.alg == BHIP_BG_GAUSSIAN) bgLaunch0<BHIP_BG_GAUSSIAN, T>(sh.bands, 1, segment, grid, ctx->stream, P);
	else bgLaunch0<BHIP_BG_GMM, T>(sh.bands, sh.maxGaussians, segment, grid, ctx->stream, P);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_background(bhip_ctx*, const BgShape&, const BgConfig&, const BgFrames<const uint8_t>&, const BgFrames<uint8_t>&, float*, const int*, bool);
template int bhip_launch_background(bhip_ctx*, const BgShape&, const BgConfig&, const BgFrames<const float>&, const BgFrames<uint8_t>&, float*, const int*, bool);

// the launch's HBM bytes: the model read and written once (a segment only reads it), every frame read, every mask written
double bhip_bg_bytes(const BgShape& sh, int pixelBytes, int numFrames, bool masks, bool segment) {
	const double px = (double)sh.width * sh.height * sh.streams;
	const int B = sh.bands ? sh.bands : 1;
	return px * (4.0 * bhip_bg_components(sh) * (segment ? 1 : 2) + (double)numFrames * (B * pixelBytes + (masks ? 1 : 0)));
}
