// C ABI, whole-image operations: dense stereo disparity, image remap, template matching.
#include "cabi.h"

// ---- dense stereo disparity (disparity.hip): StereoDisparity.process of FactoryStereoDisparity.blockMatch / blockMatchBest5, SAD and CENSUS on GrayU8 pairs ----
// Java's (int) of a double: NaN -> 0, saturating
static int javaDoubleToInt(double v) {
	if (v != v) return 0;
	if (v >= 2147483647.0) return 2147483647;
	if (v <= -2147483648.0) return -2147483647 - 1;
	return (int)v;
}

// the checks of ConfigDisparityBM.checkValidity, DisparityBlockMatchRowFormat.process and SelectDisparityWithChecksWta.configure, then the
// kernel's limits; fills the selector's parameters.  five: blockMatchBest5, whose checks are the same (DisparityBlockMatchRowFormat.process tests
// radiusX, not 2*radiusX) and whose maxError counts three regions
template <class OutT>
static int disparityParams(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int width, int height, DispBmParams& p, bool five = false) {
	bhip_disparity_bm_cfg c;
	if (cfg) c = *cfg; else bhip_disparity_bm_cfg_default(&c);
	if (c.minDisparity < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "miDisparity < 0");
	if (c.rangeDisparity < 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "rangeDisparity < 1");
	if (c.regionRadiusX < 0 || c.regionRadiusY < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "region radius < 0");
	const long long maxD = (long long)c.minDisparity + c.rangeDisparity;
	if (maxD > (long long)width - 2LL * c.regionRadiusX)
		return bhip_fail(ctx, BHIP_ERR_INVALID, "The maximum disparity is too large for this image size: max size " + std::to_string((long long)width - 2LL * c.regionRadiusX));
	if ((long long)height < 2LL * c.regionRadiusY + 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "the image is lower than the region");
	if (sizeof(OutT) == 1 && c.rangeDisparity + 1LL > 254)
		return bhip_fail(ctx, BHIP_ERR_INVALID, "Max range exceeds maximum value in disparity image. v=" + std::to_string(c.rangeDisparity + 1LL));
	if (c.regionRadiusX > BHIP_DISP_MAX_RADIUS || c.regionRadiusY > BHIP_DISP_MAX_RADIUS || c.rangeDisparity > BHIP_DISP_MAX_RANGE)
		return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "block matching on the GPU: region radius <= 7, rangeDisparity <= 256");
	const int rw = 2 * c.regionRadiusX + 1, rh = 2 * c.regionRadiusY + 1;
	double maxErrorD = (rw * rh) * c.maxPerPixelError;                      // FactoryStereoDisparity.java:75,79
	if (five) maxErrorD *= 3;                                               // :159-162
	const int maxError = javaDoubleToInt(maxErrorD);
	p.minD = c.minDisparity; p.range = c.rangeDisparity; p.rx = c.regionRadiusX; p.ry = c.regionRadiusY;
	p.maxError = maxError <= 0 ? 2147483647 : maxError;                     // SelectDisparityWithChecksWta.java:83
	p.rtolTol = c.validateRtoL;
	p.textureThr = javaDoubleToInt(10000 * c.texture);                      // SelectErrorWithChecks_S32.setTexture
	return BHIP_OK;
}

// errorType = CENSUS: the census form a CensusVariants ordinal is matched with -- wordBytes 1 (BLOCK_3_3, GrayU8), 4 (BLOCK_5_5, GrayS32) or 8 (a
// GrayS64 sample list, in s) -- after the checks of the census transform; nothing for SAD (variant == DISP_SAD)
#define DISP_SAD (-1)
struct DispCensusForm {
	int wordBytes = 0;
	CensusSamples s;
};
static int disparityCensusForm(bhip_ctx* ctx, int variant, int width, int height, DispCensusForm& f) {
	if (variant == DISP_SAD) return BHIP_OK;
	int xy[2 * BHIP_CENSUS_MAX_SAMPLES];
	const int n = bhip_census_variant_list(variant, xy);
	if (n < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown type " + std::to_string(variant));
	BHIP_TRY(bhip_census_samples(xy, n, f.s));
	if (width < f.s.radius + 1 || height < f.s.radius + 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "the image is smaller than the census region's radius + 1");
	f.wordBytes = variant == BHIP_CENSUS_BLOCK_3_3 ? 1 : variant == BHIP_CENSUS_BLOCK_5_5 ? 4 : 8;
	return BHIP_OK;
}

template <class OutT>
static int disparityDevice(bhip_ctx* ctx, const DispBmParams& p, const DispCensusForm& f, DevImg<const uint8_t> left, DevImg<const uint8_t> right,
						   DevImg<OutT> disp, bool five = false) {
	DevBuf& scratch = scratchOf(ctx)->disparity;
	if (f.wordBytes) {
		BHIP_TRY(scratch.reserve(ctx, bhip_disparity_census_scratch(left.width, left.height, left.batch, f.wordBytes)));
		if (five) return bhip_launch_disparity_bm5_census<OutT>(ctx, left, right, p, f.wordBytes, &f.s, scratch.as<uint8_t>(), disp);
		return bhip_launch_disparity_bm_census<OutT>(ctx, left, right, p, f.wordBytes, &f.s, scratch.as<uint8_t>(), disp);
	}
	BHIP_TRY(scratch.reserve(ctx, bhip_disparity_scratch(left.width, left.height, left.batch)));
	if (five) return bhip_launch_disparity_bm5<OutT>(ctx, left, right, p, scratch.as<uint8_t>(), disp);
	return bhip_launch_disparity_bm<OutT>(ctx, left, right, p, scratch.as<uint8_t>(), disp);
}

template <class OutT>
static int disparityDev(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* dev_left, long long lImageStride, int lStride, const uint8_t* dev_right,
						long long rImageStride, int rStride, int width, int height, int batch, OutT* dev_disp, long long dImageStride, int dStride, bool five = false) {
	CHECK_CTX(ctx);
	const DevImg<const uint8_t> left{dev_left, lImageStride, lStride, width, height, batch}, right{dev_right, rImageStride, rStride, width, height, batch};
	const DevImg<OutT> disp{dev_disp, dImageStride, dStride, width, height, batch};
	CHECK_IMG(ctx, left);
	CHECK_IMG(ctx, right);
	CHECK_IMG(ctx, disp);
	DispBmParams p;
	DispCensusForm f;
	BHIP_TRY(disparityParams<OutT>(ctx, cfg, width, height, p, five));
	BHIP_TRY(disparityCensusForm(ctx, variant, width, height, f));
	return disparityDevice<OutT>(ctx, p, f, left, right, disp, five);
}

template <class OutT>
static int disparityHost(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart, int rStride,
						 int width, int height, OutT* disp, int dStart, int dStride, bool five = false) {
	const HostImg<const uint8_t> hl{left, lStart, lStride, width, height}, hr{right, rStart, rStride, width, height};
	const HostImg<OutT> hd{disp, dStart, dStride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hl);
	CHECK_IMG(ctx, hr);
	CHECK_IMG(ctx, hd);
	DispBmParams p;
	DispCensusForm f;
	BHIP_TRY(disparityParams<OutT>(ctx, cfg, width, height, p, five));
	BHIP_TRY(disparityCensusForm(ctx, variant, width, height, f));
	CtxScratch* sc = scratchOf(ctx);
	DevImg<uint8_t> dl, dr;
	DevImg<OutT> dd;
	BHIP_TRY(stageIn(ctx, sc->in0, hl, width, dl));
	BHIP_TRY(stageIn(ctx, sc->in1, hr, width, dr));
	BHIP_TRY(stageIn(ctx, sc->out0, hd, width, dd, false));
	BHIP_TRY(disparityDevice<OutT>(ctx, p, f, dl, dr, dd, five));
	BHIP_TRY(stageOut(ctx, hd, dd));
	return bhip_ctx_synchronize(ctx);
}

// ---- image remap (distort.hip): ImageDistort.apply of FactoryDistort.distortSB, GrayU8 / GrayF32, NEAREST_NEIGHBOR / BILINEAR, ZERO / EXTENDED ----
// the checks every form shares: what is refused (include/boofhip.h), before anything is staged or launched
static int distortCheck(bhip_ctx* ctx, const DistortCoords& co, int dw, int dh, const DistortCrop& crop, int interp, int border) {
	if (co.model == 0 ? !co.map : ((co.model != BHIP_DISTORT_AFFINE && co.model != BHIP_DISTORT_HOMOGRAPHY) || !co.coeff))
		return bhip_fail(ctx, BHIP_ERR_INVALID, "distort: no map, or no such model");
	if (co.mapImageStride < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "distort: negative map stride");
	if (crop.x0 < 0 || crop.y0 < 0 || crop.x0 > crop.x1 || crop.y0 > crop.y1 || crop.x1 > dw || crop.y1 > dh)
		return bhip_fail(ctx, BHIP_ERR_INVALID, "distort: the crop is not inside the destination");
	if (interp != BHIP_INTERP_NEAREST_NEIGHBOR && interp != BHIP_INTERP_BILINEAR)
		return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "distort on the GPU: NEAREST_NEIGHBOR or BILINEAR interpolation");
	if (border != BHIP_BORDER_ZERO && border != BHIP_BORDER_EXTENDED) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "distort on the GPU: ZERO or EXTENDED border");
	return BHIP_OK;
}

template <class T>
static int distortDev(bhip_ctx* ctx, const T* dev_src, long long sImageStride, int sStride, int sw, int sh, int batch, const DistortCoords& co, int dw, int dh,
					  const DistortCrop& crop, int interp, int border, int renderAll, T* dev_dst, long long dImageStride, int dStride, uint8_t* dev_mask,
					  long long mImageStride, int mStride) {
	CHECK_CTX(ctx);
	const DevImg<const T> src{dev_src, sImageStride, sStride, sw, sh, batch};
	const DevImg<T> dst{dev_dst, dImageStride, dStride, dw, dh, batch};
	DevImg<uint8_t> mask{nullptr, 0, 0, dw, dh, batch};
	CHECK_IMG(ctx, src);
	CHECK_IMG(ctx, dst);
	if (dev_mask) {
		mask = {dev_mask, mImageStride, mStride, dw, dh, batch};
		CHECK_IMG(ctx, mask);
	}
	BHIP_TRY(distortCheck(ctx, co, dw, dh, crop, interp, border));
	return bhip_launch_distort<T>(ctx, src, co, crop, interp, border, renderAll, dst, mask);
}

template <class T>
static int distortHost(bhip_ctx* ctx, const T* src, int sStart, int sStride, int sw, int sh, DistortCoords co, int dw, int dh, const DistortCrop& crop, int interp,
					   int border, int renderAll, T* dst, int dStart, int dStride, uint8_t* mask, int mStart, int mStride) {
	const HostImg<const T> hs{src, sStart, sStride, sw, sh};
	const HostImg<T> hd{dst, dStart, dStride, dw, dh};
	const HostImg<uint8_t> hm{mask, mStart, mStride, dw, dh};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hs);
	CHECK_IMG(ctx, hd);
	if (mask) CHECK_IMG(ctx, hm);
	BHIP_TRY(distortCheck(ctx, co, dw, dh, crop, interp, border));
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> ds, dd;
	DevImg<uint8_t> dm{nullptr, 0, 0, dw, dh, 1};
	// the destination is written as a whole only when every pixel is rendered; the mask whenever the crop is the whole image
	const bool whole = crop.x0 == 0 && crop.y0 == 0 && crop.x1 == dw && crop.y1 == dh;
	BHIP_TRY(stageIn(ctx, sc->in0, hs, sw, ds));
	if (co.model == 0) {   // co.map is the caller's host map
		BHIP_TRY(sc->distortMap.reserve(ctx, (size_t)dw * dh * 8));
		BHIP_HIP(ctx, hipMemcpyAsync(sc->distortMap.as<float>(), co.map, (size_t)dw * dh * 8, hipMemcpyHostToDevice, ctx->stream));
		co.map = sc->distortMap.as<float>();
	}
	BHIP_TRY(stageIn(ctx, sc->out0, hd, dw, dd, !(whole && renderAll)));
	if (mask) BHIP_TRY(stageIn(ctx, sc->out1, hm, dw, dm, !whole));
	BHIP_TRY(bhip_launch_distort<T>(ctx, ds, co, crop, interp, border, renderAll, dd, dm));
	BHIP_TRY(stageOut(ctx, hd, dd));
	if (mask) BHIP_TRY(stageOut(ctx, hm, dm));
	return bhip_ctx_synchronize(ctx);
}

// ---- template matching (template.hip, k_template_select in detect.hip): TemplateMatchingIntensity.process and the selection of TemplateMatching.process ----
// the checks the reference leaves to an array index exception, then the kernel's limit
template <class T>
static int templateCheck(bhip_ctx* ctx, int score, DevImg<const T> img, DevImg<const T> tpl, DevImg<const T> mask) {
	if (score == BHIP_TEMPLATE_CORRELATION) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "TemplateCorrelationFFT is not implemented on the GPU (use the Java path)");
	if (score < BHIP_TEMPLATE_SAD || score > BHIP_TEMPLATE_CORRELATION) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown");
	if (tpl.width > img.width || tpl.height > img.height) return bhip_fail(ctx, BHIP_ERR_INVALID, "the template is larger than the image");
	if (mask.data && (mask.width != tpl.width || mask.height != tpl.height)) return bhip_fail(ctx, BHIP_ERR_INVALID, "the mask must have the template's size");
	if (tpl.width > BHIP_TEMPLATE_MAX_WIDTH)
		return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "template matching on the GPU: template width <= " + std::to_string(BHIP_TEMPLATE_MAX_WIDTH) + " (use the Java path)");
	return BHIP_OK;
}

template <class T>
static int templateDevice(bhip_ctx* ctx, int score, DevImg<const T> img, DevImg<const T> tpl, DevImg<const T> mask, DevImg<float> out) {
	DevBuf& stats = scratchOf(ctx)->templ;
	BHIP_TRY(stats.reserve(ctx, bhip_template_scratch(img.batch)));
	return bhip_launch_template_intensity<T>(ctx, score, img, tpl, mask, stats.as<float>(), out);
}

template <class T>
static int templateDev(bhip_ctx* ctx, int score, const T* dev_image, long long iImageStride, int iStride, int width, int height, int batch, const T* dev_templ,
					   long long tImageStride, int tStride, int tWidth, int tHeight, const T* dev_mask, long long mImageStride, int mStride, int mWidth, int mHeight,
					   float* dev_intensity, long long oImageStride, int oStride) {
	CHECK_CTX(ctx);
	const DevImg<const T> img{dev_image, iImageStride, iStride, width, height, batch}, tpl{dev_templ, tImageStride, tStride, tWidth, tHeight, batch};
	const DevImg<const T> mask{dev_mask, mImageStride, mStride, mWidth, mHeight, batch};
	const DevImg<float> out{dev_intensity, oImageStride, oStride, width, height, batch};
	CHECK_IMG(ctx, img);
	CHECK_IMG(ctx, tpl);
	if (dev_mask) CHECK_IMG(ctx, mask);
	CHECK_IMG(ctx, out);
	if (tImageStride < 0 || mImageStride < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image");
	BHIP_TRY(templateCheck<T>(ctx, score, img, tpl, mask));
	return templateDevice<T>(ctx, score, img, tpl, mask, out);
}

template <class T>
static int templateHost(bhip_ctx* ctx, int score, const T* image, int iStart, int iStride, int width, int height, const T* templ, int tStart, int tStride, int tWidth,
						int tHeight, const T* mask, int mStart, int mStride, int mWidth, int mHeight, float* intensity, int oStart, int oStride) {
	const HostImg<const T> hi{image, iStart, iStride, width, height}, ht{templ, tStart, tStride, tWidth, tHeight}, hm{mask, mStart, mStride, mWidth, mHeight};
	const HostImg<float> ho{intensity, oStart, oStride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hi);
	CHECK_IMG(ctx, ht);
	if (mask) CHECK_IMG(ctx, hm);
	CHECK_IMG(ctx, ho);
	BHIP_TRY(templateCheck<T>(ctx, score, {image, 0, iStride, width, height, 1}, {templ, 0, tStride, tWidth, tHeight, 1}, {mask, 0, mStride, mWidth, mHeight, 1}));
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> di, dt, dm{nullptr, 0, 0, tWidth, tHeight, 1};
	DevImg<float> dout;
	BHIP_TRY(stageIn(ctx, sc->in0, hi, width, di));
	BHIP_TRY(stageIn(ctx, sc->in1, ht, tWidth, dt));
	if (mask) BHIP_TRY(stageIn(ctx, sc->tmp0, hm, mWidth, dm));
	BHIP_TRY(stageIn(ctx, sc->out0, ho, width, dout, false));
	BHIP_TRY(templateDevice<T>(ctx, score, di, dt, dm, dout));
	BHIP_TRY(stageOut(ctx, ho, dout));
	return bhip_ctx_synchronize(ctx);
}

// selection scratch: [batch][cap] keys and indexes (the slot of the NCC statistics, which no kernel still in flight on another stream reads:
// everything runs on the context's stream)
static int templateSelectDevice(bhip_ctx* ctx, DevImg<const float> img, const int16_t* dev_xy, const int* dev_n, int cap, int maxMatches, bool maximize,
								int16_t* dev_out_xy, float* dev_out_score, int* dev_out_n) {
	if (cap > BHIP_TEMPLATE_MAX_CANDIDATES)
		return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "template matching on the GPU: at most " + std::to_string(BHIP_TEMPLATE_MAX_CANDIDATES) + " candidates per image");
	DevBuf& work = scratchOf(ctx)->templ;
	const size_t per = (size_t)std::max(cap, 1) * img.batch;
	BHIP_TRY(work.reserve(ctx, per * 8));
	float* key = work.as<float>();
	return bhip_launch_template_select(ctx, img, dev_xy, dev_n, cap, maxMatches, maximize, key, (int*)(key + per), dev_out_xy, dev_out_score, dev_out_n);
}

extern "C" {

int bhip_disparity_bm_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart,
							int rStride, int width, int height, uint8_t* disp, int dStart, int dStride) {
	return disparityHost<uint8_t>(ctx, cfg, DISP_SAD, left, lStart, lStride, right, rStart, rStride, width, height, disp, dStart, dStride);
}
int bhip_disparity_bm_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart,
							 int rStride, int width, int height, float* disp, int dStart, int dStride) {
	return disparityHost<float>(ctx, cfg, DISP_SAD, left, lStart, lStride, right, rStart, rStride, width, height, disp, dStart, dStride);
}
int bhip_disparity_bm_dev_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride,
								const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, uint8_t* dev_disp,
								long long dImageStride, int dStride) {
	return disparityDev<uint8_t>(ctx, cfg, DISP_SAD, dev_left, lImageStride, lStride, dev_right, rImageStride, rStride, width, height, batch, dev_disp, dImageStride, dStride);
}
int bhip_disparity_bm_dev_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride,
								 const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, float* dev_disp,
								 long long dImageStride, int dStride) {
	return disparityDev<float>(ctx, cfg, DISP_SAD, dev_left, lImageStride, lStride, dev_right, rImageStride, rStride, width, height, batch, dev_disp, dImageStride, dStride);
}

int bhip_disparity_bm_census_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* left, int lStart, int lStride,
								   const uint8_t* right, int rStart, int rStride, int width, int height, uint8_t* disp, int dStart, int dStride) {
	if (variant == DISP_SAD) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown type -1");
	return disparityHost<uint8_t>(ctx, cfg, variant, left, lStart, lStride, right, rStart, rStride, width, height, disp, dStart, dStride);
}
int bhip_disparity_bm_census_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* left, int lStart, int lStride,
									const uint8_t* right, int rStart, int rStride, int width, int height, float* disp, int dStart, int dStride) {
	if (variant == DISP_SAD) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown type -1");
	return disparityHost<float>(ctx, cfg, variant, left, lStart, lStride, right, rStart, rStride, width, height, disp, dStart, dStride);
}
int bhip_disparity_bm_census_dev_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* dev_left, long long lImageStride, int lStride,
									   const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, uint8_t* dev_disp,
									   long long dImageStride, int dStride) {
	if (variant == DISP_SAD) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown type -1");
	return disparityDev<uint8_t>(ctx, cfg, variant, dev_left, lImageStride, lStride, dev_right, rImageStride, rStride, width, height, batch, dev_disp, dImageStride,
								 dStride);
}
int bhip_disparity_bm_census_dev_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* dev_left, long long lImageStride, int lStride,
										const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, float* dev_disp,
										long long dImageStride, int dStride) {
	if (variant == DISP_SAD) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown type -1");
	return disparityDev<float>(ctx, cfg, variant, dev_left, lImageStride, lStride, dev_right, rImageStride, rStride, width, height, batch, dev_disp, dImageStride,
							   dStride);
}

// blockMatchBest5: the same staging and checks, the five-region launches
int bhip_disparity_bm5_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart,
							int rStride, int width, int height, uint8_t* disp, int dStart, int dStride) {
	return disparityHost<uint8_t>(ctx, cfg, DISP_SAD, left, lStart, lStride, right, rStart, rStride, width, height, disp, dStart, dStride, true);
}
int bhip_disparity_bm5_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart,
							 int rStride, int width, int height, float* disp, int dStart, int dStride) {
	return disparityHost<float>(ctx, cfg, DISP_SAD, left, lStart, lStride, right, rStart, rStride, width, height, disp, dStart, dStride, true);
}
int bhip_disparity_bm5_dev_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride,
								const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, uint8_t* dev_disp,
								long long dImageStride, int dStride) {
	return disparityDev<uint8_t>(ctx, cfg, DISP_SAD, dev_left, lImageStride, lStride, dev_right, rImageStride, rStride, width, height, batch, dev_disp, dImageStride, dStride, true);
}
int bhip_disparity_bm5_dev_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride,
								 const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, float* dev_disp,
								 long long dImageStride, int dStride) {
	return disparityDev<float>(ctx, cfg, DISP_SAD, dev_left, lImageStride, lStride, dev_right, rImageStride, rStride, width, height, batch, dev_disp, dImageStride, dStride, true);
}

int bhip_disparity_bm5_census_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* left, int lStart, int lStride,
								   const uint8_t* right, int rStart, int rStride, int width, int height, uint8_t* disp, int dStart, int dStride) {
	if (variant == DISP_SAD) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown type -1");
	return disparityHost<uint8_t>(ctx, cfg, variant, left, lStart, lStride, right, rStart, rStride, width, height, disp, dStart, dStride, true);
}
int bhip_disparity_bm5_census_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* left, int lStart, int lStride,
									const uint8_t* right, int rStart, int rStride, int width, int height, float* disp, int dStart, int dStride) {
	if (variant == DISP_SAD) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown type -1");
	return disparityHost<float>(ctx, cfg, variant, left, lStart, lStride, right, rStart, rStride, width, height, disp, dStart, dStride, true);
}
int bhip_disparity_bm5_census_dev_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* dev_left, long long lImageStride, int lStride,
									   const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, uint8_t* dev_disp,
									   long long dImageStride, int dStride) {
	if (variant == DISP_SAD) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown type -1");
	return disparityDev<uint8_t>(ctx, cfg, variant, dev_left, lImageStride, lStride, dev_right, rImageStride, rStride, width, height, batch, dev_disp, dImageStride,
								 dStride, true);
}
int bhip_disparity_bm5_census_dev_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* dev_left, long long lImageStride, int lStride,
										const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, float* dev_disp,
										long long dImageStride, int dStride) {
	if (variant == DISP_SAD) return bhip_fail(ctx, BHIP_ERR_INVALID, "Unknown type -1");
	return disparityDev<float>(ctx, cfg, variant, dev_left, lImageStride, lStride, dev_right, rImageStride, rStride, width, height, batch, dev_disp, dImageStride,
							   dStride, true);
}

int bhip_distort_map_u8(bhip_ctx* ctx, const uint8_t* src, int sStart, int sStride, int sw, int sh, const float* map, int dw, int dh, int x0, int y0, int x1,
						int y1, int interp, int border, int renderAll, uint8_t* dst, int dStart, int dStride, uint8_t* mask, int mStart, int mStride) {
	return distortHost<uint8_t>(ctx, src, sStart, sStride, sw, sh, {0, map, 0, nullptr}, dw, dh, {x0, y0, x1, y1}, interp, border, renderAll, dst, dStart, dStride, mask, mStart, mStride);
}
int bhip_distort_map_f32(bhip_ctx* ctx, const float* src, int sStart, int sStride, int sw, int sh, const float* map, int dw, int dh, int x0, int y0, int x1,
						 int y1, int interp, int border, int renderAll, float* dst, int dStart, int dStride, uint8_t* mask, int mStart, int mStride) {
	return distortHost<float>(ctx, src, sStart, sStride, sw, sh, {0, map, 0, nullptr}, dw, dh, {x0, y0, x1, y1}, interp, border, renderAll, dst, dStart, dStride, mask, mStart, mStride);
}
// a model of 0 would select the map form: it is no model
int bhip_distort_model_u8(bhip_ctx* ctx, const uint8_t* src, int sStart, int sStride, int sw, int sh, int model, const float* coeff, int dw, int dh, int x0, int y0,
						  int x1, int y1, int interp, int border, int renderAll, uint8_t* dst, int dStart, int dStride, uint8_t* mask, int mStart, int mStride) {
	return distortHost<uint8_t>(ctx, src, sStart, sStride, sw, sh, {model ? model : -1, nullptr, 0, coeff}, dw, dh, {x0, y0, x1, y1}, interp, border, renderAll, dst,
								dStart, dStride, mask, mStart, mStride);
}
int bhip_distort_model_f32(bhip_ctx* ctx, const float* src, int sStart, int sStride, int sw, int sh, int model, const float* coeff, int dw, int dh, int x0, int y0,
						   int x1, int y1, int interp, int border, int renderAll, float* dst, int dStart, int dStride, uint8_t* mask, int mStart, int mStride) {
	return distortHost<float>(ctx, src, sStart, sStride, sw, sh, {model ? model : -1, nullptr, 0, coeff}, dw, dh, {x0, y0, x1, y1}, interp, border, renderAll, dst,
							  dStart, dStride, mask, mStart, mStride);
}
int bhip_distort_map_dev_u8(bhip_ctx* ctx, const uint8_t* dev_src, long long sImageStride, int sStride, int sw, int sh, int batch, const float* dev_map,
							long long mapImageStride, int dw, int dh, int x0, int y0, int x1, int y1, int interp, int border, int renderAll, uint8_t* dev_dst,
							long long dImageStride, int dStride, uint8_t* dev_mask, long long mImageStride, int mStride) {
	return distortDev<uint8_t>(ctx, dev_src, sImageStride, sStride, sw, sh, batch, {0, dev_map, mapImageStride, nullptr}, dw, dh, {x0, y0, x1, y1}, interp, border,
							   renderAll, dev_dst, dImageStride, dStride, dev_mask, mImageStride, mStride);
}
int bhip_distort_map_dev_f32(bhip_ctx* ctx, const float* dev_src, long long sImageStride, int sStride, int sw, int sh, int batch, const float* dev_map,
							 long long mapImageStride, int dw, int dh, int x0, int y0, int x1, int y1, int interp, int border, int renderAll, float* dev_dst,
							 long long dImageStride, int dStride, uint8_t* dev_mask, long long mImageStride, int mStride) {
	return distortDev<float>(ctx, dev_src, sImageStride, sStride, sw, sh, batch, {0, dev_map, mapImageStride, nullptr}, dw, dh, {x0, y0, x1, y1}, interp, border,
							 renderAll, dev_dst, dImageStride, dStride, dev_mask, mImageStride, mStride);
}
int bhip_distort_model_dev_u8(bhip_ctx* ctx, const uint8_t* dev_src, long long sImageStride, int sStride, int sw, int sh, int batch, int model, const float* coeff,
							  int dw, int dh, int x0, int y0, int x1, int y1, int interp, int border, int renderAll, uint8_t* dev_dst, long long dImageStride,
							  int dStride, uint8_t* dev_mask, long long mImageStride, int mStride) {
	return distortDev<uint8_t>(ctx, dev_src, sImageStride, sStride, sw, sh, batch, {model ? model : -1, nullptr, 0, coeff}, dw, dh, {x0, y0, x1, y1}, interp, border,
							   renderAll, dev_dst, dImageStride, dStride, dev_mask, mImageStride, mStride);
}
int bhip_distort_model_dev_f32(bhip_ctx* ctx, const float* dev_src, long long sImageStride, int sStride, int sw, int sh, int batch, int model, const float* coeff,
							   int dw, int dh, int x0, int y0, int x1, int y1, int interp, int border, int renderAll, float* dev_dst, long long dImageStride,
							   int dStride, uint8_t* dev_mask, long long mImageStride, int mStride) {
	return distortDev<float>(ctx, dev_src, sImageStride, sStride, sw, sh, batch, {model ? model : -1, nullptr, 0, coeff}, dw, dh, {x0, y0, x1, y1}, interp, border,
							 renderAll, dev_dst, dImageStride, dStride, dev_mask, mImageStride, mStride);
}
int bhip_distort_build_map(bhip_ctx* ctx, int model, const float* coeff, int dw, int dh, float* dev_map) {
	CHECK_CTX(ctx);
	if ((model != BHIP_DISTORT_AFFINE && model != BHIP_DISTORT_HOMOGRAPHY) || !coeff || !dev_map || dw <= 0 || dh <= 0)
		return bhip_fail(ctx, BHIP_ERR_INVALID, "bhip_distort_build_map: no such model, or no coefficients / map / size");
	return bhip_launch_distort_build_map(ctx, model, coeff, dw, dh, dev_map);
}

int bhip_template_intensity_u8(bhip_ctx* ctx, int score, const uint8_t* image, int iStart, int iStride, int width, int height, const uint8_t* templ, int tStart,
							   int tStride, int tWidth, int tHeight, const uint8_t* mask, int mStart, int mStride, int mWidth, int mHeight, float* intensity, int oStart,
							   int oStride) {
	return templateHost<uint8_t>(ctx, score, image, iStart, iStride, width, height, templ, tStart, tStride, tWidth, tHeight, mask, mStart, mStride, mWidth, mHeight,
								 intensity, oStart, oStride);
}
int bhip_template_intensity_f32(bhip_ctx* ctx, int score, const float* image, int iStart, int iStride, int width, int height, const float* templ, int tStart,
								int tStride, int tWidth, int tHeight, const float* mask, int mStart, int mStride, int mWidth, int mHeight, float* intensity, int oStart,
								int oStride) {
	return templateHost<float>(ctx, score, image, iStart, iStride, width, height, templ, tStart, tStride, tWidth, tHeight, mask, mStart, mStride, mWidth, mHeight,
							   intensity, oStart, oStride);
}
int bhip_template_intensity_dev_u8(bhip_ctx* ctx, int score, const uint8_t* dev_image, long long iImageStride, int iStride, int width, int height, int batch,
								   const uint8_t* dev_templ, long long tImageStride, int tStride, int tWidth, int tHeight, const uint8_t* dev_mask,
								   long long mImageStride, int mStride, int mWidth, int mHeight, float* dev_intensity, long long oImageStride, int oStride) {
	return templateDev<uint8_t>(ctx, score, dev_image, iImageStride, iStride, width, height, batch, dev_templ, tImageStride, tStride, tWidth, tHeight, dev_mask,
								mImageStride, mStride, mWidth, mHeight, dev_intensity, oImageStride, oStride);
}
int bhip_template_intensity_dev_f32(bhip_ctx* ctx, int score, const float* dev_image, long long iImageStride, int iStride, int width, int height, int batch,
									const float* dev_templ, long long tImageStride, int tStride, int tWidth, int tHeight, const float* dev_mask,
									long long mImageStride, int mStride, int mWidth, int mHeight, float* dev_intensity, long long oImageStride, int oStride) {
	return templateDev<float>(ctx, score, dev_image, iImageStride, iStride, width, height, batch, dev_templ, tImageStride, tStride, tWidth, tHeight, dev_mask,
							  mImageStride, mStride, mWidth, mHeight, dev_intensity, oImageStride, oStride);
}

int bhip_template_select_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long imageStride, int stride, int width, int height, int batch,
								 const int16_t* dev_xy, const int* dev_n, int cap, int maxMatches, int maximize, int16_t* dev_out_xy, float* dev_out_score,
								 int* dev_out_n) {
	CHECK_CTX(ctx);
	const DevImg<const float> img{dev_intensity, imageStride, stride, width, height, batch};
	CHECK_IMG(ctx, img);
	if (cap < 0 || maxMatches < 0 || !dev_n || !dev_out_n || (cap > 0 && !dev_xy) || (maxMatches > 0 && (!dev_out_xy || !dev_out_score)))
		return bhip_fail(ctx, BHIP_ERR_INVALID, "bad candidate list");
	return templateSelectDevice(ctx, img, dev_xy, dev_n, cap, maxMatches, maximize != 0, dev_out_xy, dev_out_score, dev_out_n);
}

int bhip_template_select_f32(bhip_ctx* ctx, const float* intensity, int start, int stride, int width, int height, const int16_t* xy, int n, int maxMatches,
							 int maximize, int16_t* out_xy, float* out_score, int* out_n) {
	const HostImg<const float> hin{intensity, start, stride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	if (n < 0 || maxMatches < 0 || !out_n || (n > 0 && !xy) || (std::min(n, maxMatches) > 0 && (!out_xy || !out_score)))
		return bhip_fail(ctx, BHIP_ERR_INVALID, "bad candidate list");
	for (int i = 0; i < n; i++)
		if (xy[2 * i] < 0 || xy[2 * i] >= width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= height)
			return bhip_fail(ctx, BHIP_ERR_INVALID, "candidate outside the intensity image");   // GrayF32.get would throw ImageAccessException
	if (n > BHIP_TEMPLATE_MAX_CANDIDATES)
		return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "template matching on the GPU: at most " + std::to_string(BHIP_TEMPLATE_MAX_CANDIDATES) + " candidates per image");
	const int N = std::min(n, maxMatches);
	*out_n = 0;
	if (N == 0) return BHIP_OK;   // no candidates or nothing asked for: no matches
	CtxScratch* sc = scratchOf(ctx);
	DevImg<float> din;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	BHIP_TRY(sc->in1.reserve(ctx, (size_t)n * 4));
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)N * 4));
	BHIP_TRY(sc->out1.reserve(ctx, (size_t)N * 4 + 16));
	BHIP_HIP(ctx, hipMemcpyAsync(sc->in1.p, xy, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
	int* dcount = (int*)(sc->out1.as<char>() + (size_t)N * 4);
	BHIP_TRY(templateSelectDevice(ctx, din, sc->in1.as<int16_t>(), nullptr, n, N, maximize != 0, sc->out0.as<int16_t>(), sc->out1.as<float>(), dcount));
	BHIP_HIP(ctx, hipMemcpyAsync(out_xy, sc->out0.p, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(out_score, sc->out1.p, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	*out_n = N;
	return BHIP_OK;
}

}  // extern "C"
