// C ABI, SIFT detector (kernels: sift.hip; the normalised convolutions: conv.hip; the strict block NMS: detect.hip): SiftScaleSpace, SiftDetector,
// NonMaxLimiter and WrapSiftDetector of FactoryInterestPoint.sift.  Rules, deviations and limits: bhip_sift_cfg in include/boofhip.h.
// SIFT detect + describe (kernels: sift_describe.hip): CompleteSift and DetectDescribe_CompleteSift of FactoryDetectDescribe.sift, hooked into
// the detector's per-octave loop.  Rules and limits: bhip_csift_cfg in include/boofhip.h.
#include "cabi.h"

namespace {

// everything the host decides before the first launch: the kernels and the octave sizes (no device value decides them)
struct SiftPlan {
	bhip_sift_cfg cfg;
	std::vector<float> k0;                   // kernelSigma0
	std::vector<std::vector<float>> ks;      // kernelSigmaToK[0 .. numScales+1]
	int w0 = 0, h0 = 0;                      // the frame
	int upW = 0, upH = 0;                    // the first octave's size
	std::vector<int> dims;                   // (w, h) per octave
	int nOct = 0;
	long long scaleFloats = 0, dogFloats = 0;
	bool twoPass = false;
};

inline long long planeOf(int w, int h) { return ((long long)w * h + 3) & ~3LL; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// SiftScaleSpace.computeSigmaScale(octave, scale) :162-164
inline double sigmaScale(const bhip_sift_cfg& c, int octave, int scale) { return c.sigma0 * std::pow(2, octave + scale / (double)c.numScales); }

// the constructor of SiftScaleSpace (:102-141) and the sizes initialize / computeNextOctave (:170-212) go through.  `msg` names what was refused
int siftPlan(const bhip_sift_cfg* cfg, int width, int height, SiftPlan& P, const char** msg) {
	*msg = nullptr;
	if (!cfg) { *msg = "SIFT: null config"; return BHIP_ERR_INVALID; }
	const bhip_sift_cfg& c = *cfg;
	P.cfg = c;
	if (c.lastOctave <= c.firstOctave) { *msg = "Last octave must be more than the first octave"; return BHIP_ERR_INVALID; }
	if (c.numScales < 1) { *msg = "Number of scales must be >= 1"; return BHIP_ERR_INVALID; }
	if (!(c.sigma0 > 0)) { *msg = "SIFT: sigma0 must be > 0"; return BHIP_ERR_INVALID; }
	if (width <= 0 || height <= 0) { *msg = "bad image"; return BHIP_ERR_INVALID; }
	if (c.numScales > 1024 || c.firstOctave < -8 || c.firstOctave > 30) { *msg = "SIFT on the GPU: numScales <= 1024, firstOctave -8 .. 30"; return BHIP_ERR_UNSUPPORTED; }
	const double levelK = std::pow(2, 1.0 / c.numScales);
	P.k0 = bhip_gaussian1d_f32(c.sigma0, -1);
	P.ks.clear();
	for (int i = 1; i < c.numScales + 3; i++) P.ks.push_back(bhip_gaussian1d_f32(sigmaScale(c, 0, i - 1) * std::sqrt(levelK - 1.0), -1));
	size_t widest = P.k0.size();
	bool emptyKernel = P.k0.empty();
	for (const auto& k : P.ks) { widest = std::max(widest, k.size()); emptyKernel = emptyKernel || k.empty(); }
	if (emptyKernel) { *msg = "SIFT: a blur kernel has no taps"; return BHIP_ERR_INVALID; }
	if (widest > 255) { *msg = "SIFT on the GPU: blur kernels of at most 255 taps"; return BHIP_ERR_UNSUPPORTED; }   // BHIP_MAX_TAPS of the launchers
	long long w = width, h = height;
	if (c.firstOctave < 0) {
		w *= -2 * c.firstOctave;
		h *= -2 * c.firstOctave;
	} else {
		for (int i = 0; i < c.firstOctave; i++) { w /= 2; h /= 2; }
	}
	if (w <= 0 || h <= 0) { *msg = "SIFT: the first octave has no pixels"; return BHIP_ERR_INVALID; }
	if (w > 32767 || h > 32767 || width > 32767 || height > 32767) { *msg = "image too large for Point2D_I16"; return BHIP_ERR_UNSUPPORTED; }
	P.w0 = width; P.h0 = height; P.upW = (int)w; P.upH = (int)h;
	P.dims.clear();
	P.scaleFloats = P.dogFloats = 0;
	for (int octave = c.firstOctave;;) {
		P.dims.push_back((int)w);
		P.dims.push_back((int)h);
		P.scaleFloats += (c.numScales + 3) * planeOf((int)w, (int)h);
		P.dogFloats += (c.numScales + 2) * planeOf((int)w, (int)h);
		if (++octave > c.lastOctave || w <= 5 || h <= 5) break;
		w /= 2;
		h /= 2;
	}
	P.nOct = (int)P.dims.size() / 2;
	P.twoPass = bhip_env_flag("BHIP_SIFT_TWO_PASS");
	return BHIP_OK;
}

// what SiftDetector's constructor (:119-130) and ConfigExtract.checkValidity refuse
int siftDetectorCheck(const bhip_sift_cfg& c, const char** msg) {
	if (!c.extractDetectMax || !c.extractDetectMin) { *msg = "The extractor must be able to detect maximums and minimums"; return BHIP_ERR_INVALID; }
	if (!(c.edgeR >= 1)) { *msg = "R must be >= 1"; return BHIP_ERR_INVALID; }
	if (c.extractIgnoreBorder != 1) { *msg = "Non-max should have an ignore border of 1"; return BHIP_ERR_INVALID; }
	if (c.extractRadius < 1) { *msg = "Search radius must be >= 1"; return BHIP_ERR_INVALID; }
	if (!c.extractUseStrictRule) { *msg = "SIFT on the GPU: the strict extractor only"; return BHIP_ERR_UNSUPPORTED; }
	return BHIP_OK;
}

// everything the host decides for orientation and description: the tables the kernels read (the C library's exp, cos, sqrt)
struct SiftDescPlan {
	bhip_csift_cfg cfg;
	int dof = 0;
	double histAngleBin = 0, histogramBinWidth = 0;
	std::vector<double> expTable, binAngle;
	std::vector<float> gaussianWeight;
	bool generic = false;
};

// what the constructors of OrientationHistogramSift and DescribeSiftCommon need, and the limits of the kernels
int siftDescCheck(const bhip_csift_cfg* desc, const char** msg) {
	*msg = nullptr;
	if (!desc) { *msg = "SIFT describe: null config"; return BHIP_ERR_INVALID; }
	const bhip_csift_cfg& c = *desc;
	if (c.histogramSize < 3) { *msg = "SIFT orientation: histogramSize must be >= 3"; return BHIP_ERR_INVALID; }
	if (!(c.sigmaEnlarge > 0)) { *msg = "SIFT orientation: sigmaEnlarge must be > 0"; return BHIP_ERR_INVALID; }
	if (c.widthSubregion < 1 || c.widthGrid < 1 || c.numHistogramBins < 1) { *msg = "SIFT describe: widthSubregion, widthGrid and numHistogramBins must be >= 1"; return BHIP_ERR_INVALID; }
	if (!(c.sigmaToPixels > 0) || !(c.weightingSigmaFraction > 0) || !(c.maxDescriptorElementValue > 0)) {
		*msg = "SIFT describe: sigmaToPixels, weightingSigmaFraction and maxDescriptorElementValue must be > 0";
		return BHIP_ERR_INVALID;
	}
	if (c.histogramSize > BHIP_CSIFT_MAX_HISTOGRAM) { *msg = "SIFT on the GPU: histogramSize <= 256"; return BHIP_ERR_UNSUPPORTED; }
	const long long sw = (long long)c.widthSubregion * c.widthGrid;
	if (sw <= BHIP_CSIFT_MAX_SAMPLE_WIDTH && sw % 2) { *msg = "SIFT describe: widthSubregion * widthGrid must be even (the weight kernel has 2 * (width / 2) columns)"; return BHIP_ERR_INVALID; }
	if (sw > BHIP_CSIFT_MAX_SAMPLE_WIDTH) { *msg = "SIFT on the GPU: widthSubregion * widthGrid <= 48"; return BHIP_ERR_UNSUPPORTED; }
	if ((long long)c.widthGrid * c.widthGrid * c.numHistogramBins > BHIP_CSIFT_MAX_DOF) { *msg = "SIFT on the GPU: descriptors of at most 2048 elements"; return BHIP_ERR_UNSUPPORTED; }
	return BHIP_OK;
}

int siftDescPlan(const bhip_csift_cfg* desc, SiftDescPlan& D, const char** msg) {
	BHIP_TRY(siftDescCheck(desc, msg));
	const bhip_csift_cfg& c = *desc;
	D.cfg = c;
	D.dof = c.widthGrid * c.widthGrid * c.numHistogramBins;                 // DescribeSiftCommon.getDescriptorLength
	D.histAngleBin = 2.0 * M_PI / c.histogramSize;                          // OrientationHistogramSift :106
	D.histogramBinWidth = 2.0 * M_PI / c.numHistogramBins;                  // DescribeSiftCommon :68
	D.expTable = bhip_sift_exp_table();
	D.binAngle.resize(c.numHistogramBins);
	for (int k = 0; k < c.numHistogramBins; k++) D.binAngle[k] = k * D.histogramBinWidth;   // trilinearInterpolation :122
	const int descriptorWindow = c.widthSubregion * c.widthGrid;
	D.gaussianWeight = bhip_sift_gaussian_weight(descriptorWindow * c.weightingSigmaFraction, descriptorWindow / 2);   // :71-73
	D.generic = bhip_env_flag("BHIP_SIFT_DESCRIBE_GENERIC");
	return BHIP_OK;
}

// applyGaussian :241-245 through the launchers of bhip_conv_norm_h / _v; tmp: tempBlur, same shape
int siftBlur(bhip_ctx* ctx, const std::vector<float>& k, DevImg<const float> in, DevImg<float> tmp, DevImg<float> out) {
	const int kw = (int)k.size();
	BHIP_TRY(bhip_launch_conv(ctx, false, true, k.data(), kw, kw / 2, in, tmp));
	return bhip_launch_conv(ctx, true, true, k.data(), kw, kw / 2, DevImg<const float>(tmp), out);
}

DevImg<float> shaped(DevImg<float> v, int w, int h) { return {v.data, planeOf(w, h), w, w, h, v.batch}; }

// initialize :170-189 up to octaveImages[0] of the first octave.  in: the frames as floats; work0 / work1 / tmp: scratch of batch planes of
// the larger of the frame and the first octave
int siftFirstImage(bhip_ctx* ctx, const SiftPlan& P, DevImg<const float> in, DevImg<float> work0, DevImg<float> work1, DevImg<float> tmp, DevImg<float> oct0) {
	const int fo = P.cfg.firstOctave;
	if (fo < 0) {
		const DevImg<float> up = shaped(work0, P.upW, P.upH);
		BHIP_TRY(bhip_launch_sift_scale_up(ctx, in, up, -2 * fo));
		return siftBlur(ctx, P.k0, DevImg<const float>(up), shaped(tmp, P.upW, P.upH), oct0);
	}
	if (fo == 0) return siftBlur(ctx, P.k0, in, shaped(tmp, P.w0, P.h0), oct0);
	int w = P.w0, h = P.h0;
	DevImg<float> t0 = shaped(work0, w, h);
	BHIP_TRY(siftBlur(ctx, P.k0, in, shaped(tmp, w, h), t0));
	for (int i = 0; i < fo; i++) {
		const DevImg<float> t1 = shaped(work1, w, h);
		BHIP_TRY(siftBlur(ctx, P.k0, DevImg<const float>(t0), shaped(tmp, w, h), t1));
		w /= 2;
		h /= 2;
		t0 = i + 1 == fo ? oct0 : shaped(work0, w, h);
		BHIP_TRY(bhip_launch_sift_scale_down2(ctx, DevImg<const float>(t1), t0));
	}
	return BHIP_OK;
}

// computeOctaveScales :217-228: oct[0] is there; oct[1 ..] and dog[0 ..] are written
int siftOctaveScales(bhip_ctx* ctx, const SiftPlan& P, const std::vector<DevImg<float>>& oct, const std::vector<DevImg<float>>& dog, DevImg<float> tmp) {
	for (int i = 1; i < P.cfg.numScales + 3; i++) {
		const std::vector<float>& k = P.ks[i - 1];
		bool done = false;
		if (!P.twoPass) BHIP_TRY(bhip_launch_sift_level(ctx, k.data(), (int)k.size(), DevImg<const float>(oct[i - 1]), oct[i], dog[i - 1], &done));
		if (done) continue;
		BHIP_TRY(siftBlur(ctx, k, DevImg<const float>(oct[i - 1]), shaped(tmp, oct[i].width, oct[i].height), oct[i]));
		BHIP_TRY(bhip_launch_sift_subtract(ctx, DevImg<const float>(oct[i]), DevImg<const float>(oct[i - 1]), dog[i - 1]));
	}
	return BHIP_OK;
}

// scratch of one call: [float frames | work0 | work1 | tempBlur | octave images | DoG images | NMS lists ...], every part 256-byte aligned
struct SiftScratch {
	char* base = nullptr;
	size_t used = 0;
	template <class T>
	T* take(size_t n) {
		T* p = base ? (T*)(base + used) : nullptr;
		used += align256(n * sizeof(T));
		return p;
	}
};

struct SiftBuffers {
	float *frames, *work0, *work1, *tmp, *oct, *dog;
	int16_t *xyMin, *xyMax;
	int *nMin, *nMax, *nPass, *sel;
	unsigned int *bitmap, *prefix;
	float* key;
	long long bigPlane;   // floats of the largest image any buffer holds
	int listCap, words;
	// detect + describe: the detections of one (octave, j) -- at most 2 * listCap a frame, the whole list -- with their angle counts, scan and
	// first angles; the tables (siftTables)
	double *detX, *detY, *detScale, *angles, *expTable, *binAngle;
	uint8_t* detWhite;
	int16_t* detWhere;
	int *detN, *nAngles, *angleOffset, *nFeat;
	float* gaussianWeight;
	int detCap;
};

// detect: the octave images and the lists live in scratch; scaleSpaceOnly: the caller holds the images
void siftCarve(SiftScratch& S, const SiftPlan& P, int batch, bool needFrames, bool scaleSpaceOnly, SiftBuffers& B, const SiftDescPlan* D = nullptr) {
	const long long frame = planeOf(P.w0, P.h0), first = planeOf(P.upW, P.upH);
	B.bigPlane = std::max(frame, first);
	B.frames = needFrames ? S.take<float>((size_t)frame * batch) : nullptr;
	B.work0 = P.cfg.firstOctave != 0 ? S.take<float>((size_t)B.bigPlane * batch) : nullptr;
	B.work1 = P.cfg.firstOctave > 0 ? S.take<float>((size_t)B.bigPlane * batch) : nullptr;
	B.tmp = S.take<float>((size_t)B.bigPlane * batch);
	B.oct = B.dog = nullptr;
	B.listCap = B.words = 0;
	if (scaleSpaceOnly) return;
	B.oct = S.take<float>((size_t)first * batch * (P.cfg.numScales + 3));
	B.dog = S.take<float>((size_t)first * batch * (P.cfg.numScales + 2));
	// at most one minimum and one maximum per block of the largest octave
	const int step = P.cfg.extractRadius + 1;
	const long long nbx = (std::max(P.upW - 2, 0) + step - 1) / step, nby = (std::max(P.upH - 2, 0) + step - 1) / step;
	B.listCap = (int)std::max(nbx * nby, 1LL);
	B.words = bhip_sift_cand_words(B.listCap);
	B.xyMin = S.take<int16_t>((size_t)B.listCap * 2 * batch);
	B.xyMax = S.take<int16_t>((size_t)B.listCap * 2 * batch);
	B.nMin = S.take<int>(batch);
	B.nMax = S.take<int>(batch);
	B.nPass = S.take<int>(batch);
	B.bitmap = S.take<unsigned int>((size_t)B.words * batch);
	B.prefix = S.take<unsigned int>((size_t)B.words * batch);
	const bool cut = P.cfg.maxFeaturesPerScale > 0;
	B.sel = cut ? S.take<int>((size_t)B.listCap * 2 * batch) : nullptr;
	B.key = cut ? S.take<float>((size_t)B.listCap * 2 * batch) : nullptr;
	B.detCap = 0;
	if (!D) return;
	B.detCap = 2 * B.listCap;
	const size_t dets = (size_t)B.detCap * batch;
	B.detX = S.take<double>(dets);
	B.detY = S.take<double>(dets);
	B.detScale = S.take<double>(dets);
	B.angles = S.take<double>(dets * BHIP_CSIFT_ANGLE_SLOTS);
	B.detWhere = S.take<int16_t>(dets * 4);
	B.nAngles = S.take<int>(dets);
	B.angleOffset = S.take<int>(dets);
	B.detWhite = S.take<uint8_t>(dets);
	B.detN = S.take<int>(batch);
	B.nFeat = S.take<int>(batch);
}

template <class T>
int siftFrames(bhip_ctx* ctx, DevImg<const T> in, float* frames, DevImg<const float>& out);
template <>
int siftFrames<float>(bhip_ctx*, DevImg<const float> in, float*, DevImg<const float>& out) {
	out = in;
	return BHIP_OK;
}
template <>
int siftFrames<uint8_t>(bhip_ctx* ctx, DevImg<const uint8_t> in, float* frames, DevImg<const float>& out) {
	const DevImg<float> f{frames, planeOf(in.width, in.height), in.width, in.width, in.height, in.batch};
	out = f;
	return bhip_launch_sift_u8_to_f32(ctx, in, f);
}

int siftReserve(bhip_ctx* ctx, const SiftPlan& P, int batch, bool needFrames, bool scaleSpaceOnly, SiftBuffers& B, const SiftDescPlan* D = nullptr) {
	SiftScratch measure;
	siftCarve(measure, P, batch, needFrames, scaleSpaceOnly, B, D);
	DevBuf& buf = scratchOf(ctx)->sift;
	BHIP_TRY(buf.reserve(ctx, measure.used));
	SiftScratch S;
	S.base = buf.as<char>();
	siftCarve(S, P, batch, needFrames, scaleSpaceOnly, B, D);
	return BHIP_OK;
}

// bhip_sift_scale_space_dev_*: every octave into the caller's buffers
template <class T>
int scaleSpaceDevice(bhip_ctx* ctx, const SiftPlan& P, DevImg<const T> in, float* dev_scale, float* dev_dog) {
	const int batch = in.batch, ns = P.cfg.numScales;
	SiftBuffers B;
	BHIP_TRY(siftReserve(ctx, P, batch, std::is_same<T, uint8_t>::value, true, B));
	DevImg<const float> frames;
	BHIP_TRY(siftFrames<T>(ctx, in, B.frames, frames));
	const DevImg<float> work0{B.work0, B.bigPlane, 0, 0, 0, batch}, work1{B.work1, B.bigPlane, 0, 0, 0, batch}, tmp{B.tmp, B.bigPlane, 0, 0, 0, batch};
	long long oS = 0, oD = 0;
	std::vector<DevImg<float>> oct(ns + 3), dog(ns + 2), prev;
	for (int o = 0; o < P.nOct; o++) {
		const int w = P.dims[2 * o], h = P.dims[2 * o + 1];
		const long long plane = planeOf(w, h);
		for (int i = 0; i < ns + 3; i++) oct[i] = {dev_scale + oS + i * plane, P.scaleFloats, w, w, h, batch};
		for (int i = 0; i < ns + 2; i++) dog[i] = {dev_dog + oD + i * plane, P.dogFloats, w, w, h, batch};
		if (o == 0) BHIP_TRY(siftFirstImage(ctx, P, frames, work0, work1, tmp, oct[0]));
		else BHIP_TRY(bhip_launch_sift_scale_down2(ctx, DevImg<const float>(prev[ns]), oct[0]));   // computeNextOctave :209
		BHIP_TRY(siftOctaveScales(ctx, P, oct, dog, tmp));
		prev = oct;
		oS += (ns + 3) * plane;
		oD += (ns + 2) * plane;
	}
	return BHIP_OK;
}

// The tables of a describe config on the device.  They stay with the context, next to a host copy to compare with, and are uploaded again
// only when the config changes: an asynchronous copy's source must outlive it, so an upload is followed by a synchronisation -- paid on a
// change alone, and before the first launch
int siftTables(bhip_ctx* ctx, const SiftDescPlan& D, SiftBuffers& B) {
	CtxScratch* sc = scratchOf(ctx);
	const size_t nE = D.expTable.size() * 8, nB = D.binAngle.size() * 8, nG = D.gaussianWeight.size() * 4;
	std::vector<char> blob(nE + nB + nG);
	std::memcpy(blob.data(), D.expTable.data(), nE);
	std::memcpy(blob.data() + nE, D.binAngle.data(), nB);
	std::memcpy(blob.data() + nE + nB, D.gaussianWeight.data(), nG);
	if (!sc->siftTables.p || sc->siftTablesHost != blob) {
		BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
		sc->siftTablesHost.clear();
		BHIP_TRY(sc->siftTables.reserve(ctx, blob.size()));
		BHIP_HIP(ctx, hipMemcpyAsync(sc->siftTables.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
		BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `blob` is this call's
		sc->siftTablesHost.swap(blob);
	}
	char* p = sc->siftTables.as<char>();
	B.expTable = (double*)p;
	B.binAngle = (double*)(p + nE);
	B.gaussianWeight = (float*)(p + nE + nB);
	return BHIP_OK;
}

struct SiftOut {
	double *x, *y, *scale;
	uint8_t* white;
	int16_t* where;
	int* count;
	int cap;
	double *orientation = nullptr, *desc = nullptr;   // detect + describe (where is not an output then)
};

// bhip_sift_detect_dev_*: SiftDetector.process :165-191.  With D, bhip_csift_dev_*: CompleteSift.process -- detectFeatures (:97-111) takes the
// gradient of scale image j and handleDetection (:113-134) turns every detection into its features while the octave is in scratch
template <class T>
int detectDevice(bhip_ctx* ctx, const SiftPlan& P, DevImg<const T> in, const SiftOut& out, const SiftDescPlan* D = nullptr) {
	const int batch = in.batch, ns = P.cfg.numScales;
	const bhip_sift_cfg& c = P.cfg;
	SiftBuffers B;
	BHIP_TRY(siftReserve(ctx, P, batch, std::is_same<T, uint8_t>::value, false, B, D));
	BHIP_HIP(ctx, hipMemsetAsync(out.count, 0, (size_t)batch * 4, ctx->stream));
	if (D) {
		BHIP_HIP(ctx, hipMemsetAsync(B.detN, 0, (size_t)batch * 4, ctx->stream));
		BHIP_TRY(siftTables(ctx, *D, B));
	}
	DevImg<const float> frames;
	BHIP_TRY(siftFrames<T>(ctx, in, B.frames, frames));
	const DevImg<float> work0{B.work0, B.bigPlane, 0, 0, 0, batch}, work1{B.work1, B.bigPlane, 0, 0, 0, batch}, tmp{B.tmp, B.bigPlane, 0, 0, 0, batch};
	const long long slot = planeOf(P.upW, P.upH) * batch;   // one level of the largest octave
	std::vector<DevImg<float>> oct(ns + 3), dog(ns + 2);
	for (int o = 0; o < P.nOct; o++) {
		const int w = P.dims[2 * o], h = P.dims[2 * o + 1];
		const long long plane = planeOf(w, h);
		// the next octave's first image is read out of slot numScales and written to slot 0: different slots
		const DevImg<const float> top = o > 0 ? DevImg<const float>(oct[ns]) : DevImg<const float>{};
		for (int i = 0; i < ns + 3; i++) oct[i] = {B.oct + i * slot, plane, w, w, h, batch};
		for (int i = 0; i < ns + 2; i++) dog[i] = {B.dog + i * slot, plane, w, w, h, batch};
		if (o == 0) BHIP_TRY(siftFirstImage(ctx, P, frames, work0, work1, tmp, oct[0]));
		else BHIP_TRY(bhip_launch_sift_scale_down2(ctx, top, oct[0]));
		BHIP_TRY(siftOctaveScales(ctx, P, oct, dog, tmp));
		const int octave = c.firstOctave + o;
		for (int j = 1; j < ns + 1; j++) {
			const DevImg<const float> target = dog[j];
			// NonMaxLimiter.process :62-78: FactoryFeatureExtractor.nonmax sets thresholdMax = threshold, thresholdMin = -threshold
			BHIP_TRY(nonmaxDevice(ctx, target, c.extractRadius, c.extractThreshold, 1, B.xyMax, B.listCap, B.nMax, false));
			BHIP_TRY(nonmaxDevice(ctx, target, c.extractRadius, -c.extractThreshold, 1, B.xyMin, B.listCap, B.nMin, true));
			SiftCandParams K;
			K.lower = dog[j - 1].data; K.target = dog[j].data; K.upper = dog[j + 1].data;
			K.imageStride = plane; K.stride = w; K.width = w; K.height = h; K.batch = batch;
			K.xyMin = B.xyMin; K.xyMax = B.xyMax; K.nMin = B.nMin; K.nMax = B.nMax; K.listCap = B.listCap;
			K.sel = B.sel; K.maxFeatures = c.maxFeaturesPerScale > 0 ? c.maxFeaturesPerScale : 0;
			K.edgeThreshold = (c.edgeR + 1) * (c.edgeR + 1) / c.edgeR;        // SiftDetector :135
			K.pixelScaleToInput = std::pow(2.0, octave);                       // SiftScaleSpace.pixelScaleCurrentToInput :268
			K.sigmaLower = sigmaScale(c, octave, j - 1); K.sigmaTarget = sigmaScale(c, octave, j); K.sigmaUpper = sigmaScale(c, octave, j + 1);
			K.octave = octave; K.j = j;
			K.x = out.x; K.y = out.y; K.scale = out.scale; K.white = out.white; K.where = out.where; K.count = out.count; K.cap = out.cap;
			if (D) {   // the slice's detections stay in scratch: detN is zero here, so the list starts at record 0 and always fits
				K.x = B.detX; K.y = B.detY; K.scale = B.detScale; K.white = B.detWhite; K.where = B.detWhere; K.count = B.detN; K.cap = B.detCap;
			}
			if (K.sel) BHIP_TRY(bhip_launch_sift_select(ctx, K, B.key, B.sel));
			BHIP_TRY(bhip_launch_sift_candidates(ctx, K, B.bitmap, B.prefix, B.nPass));
			if (!D) continue;
			SiftDescParams Q;
			Q.image = oct[j].data; Q.imageStride = plane; Q.stride = w; Q.width = w; Q.height = h; Q.batch = batch;
			Q.detX = B.detX; Q.detY = B.detY; Q.detScale = B.detScale; Q.detWhite = B.detWhite; Q.detN = B.detN; Q.detCap = B.detCap;
			Q.pixelScaleToInput = K.pixelScaleToInput;
			Q.histogramSize = D->cfg.histogramSize; Q.sigmaEnlarge = D->cfg.sigmaEnlarge; Q.histAngleBin = D->histAngleBin; Q.expTable = B.expTable;
			Q.nAngles = B.nAngles; Q.angleOffset = B.angleOffset; Q.angles = B.angles; Q.nFeat = B.nFeat;
			Q.widthSubregion = D->cfg.widthSubregion; Q.widthGrid = D->cfg.widthGrid; Q.numHistogramBins = D->cfg.numHistogramBins; Q.dof = D->dof;
			Q.sigmaToPixels = D->cfg.sigmaToPixels; Q.histogramBinWidth = D->histogramBinWidth; Q.maxDescriptorElementValue = D->cfg.maxDescriptorElementValue;
			Q.binAngle = B.binAngle; Q.gaussianWeight = B.gaussianWeight;
			Q.x = out.x; Q.y = out.y; Q.scale = out.scale; Q.orientation = out.orientation; Q.desc = out.desc; Q.white = out.white; Q.count = out.count; Q.cap = out.cap;
			BHIP_TRY(bhip_launch_sift_describe(ctx, Q, D->generic));
		}
	}
	return BHIP_OK;
}

template <class T>
int planFor(bhip_ctx* ctx, const bhip_sift_cfg* cfg, DevImg<const T> in, bool detector, SiftPlan& P) {
	const char* msg;
	int s = siftPlan(cfg, in.width > 0 ? in.width : 0, in.height > 0 ? in.height : 0, P, &msg);
	if (s == BHIP_OK && detector) s = siftDetectorCheck(P.cfg, &msg);
	if (s != BHIP_OK) return bhip_fail(ctx, s, msg);
	if (in.batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "SIFT on the GPU: at most 65535 frames per call");
	return BHIP_OK;
}

template <class T>
int scaleSpaceDev(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const T* dev_in, long long imageStride, int stride, int width, int height, int batch, float* dev_scale,
				  float* dev_dog) {
	CHECK_CTX(ctx);
	const DevImg<const T> in{dev_in, imageStride, stride, width, height, batch};
	SiftPlan P;
	BHIP_TRY(planFor<T>(ctx, cfg, in, false, P));
	CHECK_IMG(ctx, in);
	if (!dev_scale || !dev_dog) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	return scaleSpaceDevice<T>(ctx, P, in, dev_scale, dev_dog);
}

template <class T>
int detectDev(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const T* dev_in, long long imageStride, int stride, int width, int height, int batch, const SiftOut& out) {
	CHECK_CTX(ctx);
	const DevImg<const T> in{dev_in, imageStride, stride, width, height, batch};
	SiftPlan P;
	BHIP_TRY(planFor<T>(ctx, cfg, in, true, P));
	CHECK_IMG(ctx, in);
	if (!out.count || out.cap < 0 || (out.cap > 0 && (!out.x || !out.y || !out.scale || !out.white || !out.where))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	return detectDevice<T>(ctx, P, in, out);
}

template <class T>
int scaleSpaceHost(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const T* in, int start, int stride, int width, int height, float* scale, float* dog) {
	CHECK_CTX(ctx);
	const HostImg<const T> hin{in, start, stride, width, height};
	SiftPlan P;
	BHIP_TRY(planFor<T>(ctx, cfg, DevImg<const T>{in, 0, stride, width, height, 1}, false, P));
	CHECK_IMG(ctx, hin);
	if (!scale || !dog) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> din;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)P.scaleFloats * 4));
	BHIP_TRY(sc->out1.reserve(ctx, (size_t)P.dogFloats * 4));
	BHIP_HIP(ctx, hipMemsetAsync(sc->out0.p, 0, (size_t)P.scaleFloats * 4, ctx->stream));   // the padding floats of a plane
	BHIP_HIP(ctx, hipMemsetAsync(sc->out1.p, 0, (size_t)P.dogFloats * 4, ctx->stream));
	BHIP_TRY(scaleSpaceDevice<T>(ctx, P, DevImg<const T>(din), sc->out0.as<float>(), sc->out1.as<float>()));
	BHIP_HIP(ctx, hipMemcpyAsync(scale, sc->out0.p, (size_t)P.scaleFloats * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(dog, sc->out1.p, (size_t)P.dogFloats * 4, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

template <class T>
int detectHost(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const T* in, int start, int stride, int width, int height, double* x, double* y, double* scale, uint8_t* white,
			   int16_t* where, int* count, int cap) {
	CHECK_CTX(ctx);
	const HostImg<const T> hin{in, start, stride, width, height};
	SiftPlan P;
	BHIP_TRY(planFor<T>(ctx, cfg, DevImg<const T>{in, 0, stride, width, height, 1}, true, P));
	CHECK_IMG(ctx, hin);
	if (!count || cap < 0 || (cap > 0 && (!x || !y || !scale || !white || !where))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> din;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	// out0 = [x | y | scale | where | white | count]
	const size_t c8 = align256((size_t)std::max(cap, 1) * 8);
	BHIP_TRY(sc->out0.reserve(ctx, 4 * c8 + align256((size_t)std::max(cap, 1)) + 256));
	char* base = sc->out0.as<char>();
	SiftOut out;
	out.x = (double*)base; out.y = (double*)(base + c8); out.scale = (double*)(base + 2 * c8); out.where = (int16_t*)(base + 3 * c8);
	out.white = (uint8_t*)(base + 4 * c8); out.count = (int*)(base + 4 * c8 + align256((size_t)std::max(cap, 1)));
	out.cap = cap;
	BHIP_TRY(detectDevice<T>(ctx, P, DevImg<const T>(din), out));
	BHIP_HIP(ctx, hipMemcpyAsync(ctx->hostScratch.p, out.count, 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the one synchronisation that decides how much to copy
	*count = ctx->hostScratch.as<int>()[0];
	const size_t n = (size_t)std::min(*count, cap);
	if (n > 0) {
		BHIP_HIP(ctx, hipMemcpyAsync(x, out.x, n * 8, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipMemcpyAsync(y, out.y, n * 8, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipMemcpyAsync(scale, out.scale, n * 8, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipMemcpyAsync(where, out.where, n * 8, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipMemcpyAsync(white, out.white, n, hipMemcpyDeviceToHost, ctx->stream));
	}
	return bhip_ctx_synchronize(ctx);
}

template <class T>
int csiftDev(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const bhip_csift_cfg* desc, const T* dev_in, long long imageStride, int stride, int width, int height, int batch,
			 const SiftOut& out) {
	CHECK_CTX(ctx);
	const DevImg<const T> in{dev_in, imageStride, stride, width, height, batch};
	SiftPlan P;
	BHIP_TRY(planFor<T>(ctx, cfg, in, true, P));
	SiftDescPlan D;
	const char* msg;
	const int s = siftDescPlan(desc, D, &msg);
	if (s != BHIP_OK) return bhip_fail(ctx, s, msg);
	CHECK_IMG(ctx, in);
	if (!out.count || out.cap < 0 || (out.cap > 0 && (!out.x || !out.y || !out.scale || !out.orientation || !out.white || !out.desc))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	return detectDevice<T>(ctx, P, in, out, &D);
}

template <class T>
int csiftHost(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const bhip_csift_cfg* desc, const T* in, int start, int stride, int width, int height, double* x, double* y,
			  double* scale, double* orientation, uint8_t* white, double* descriptors, int* count, int cap) {
	CHECK_CTX(ctx);
	const HostImg<const T> hin{in, start, stride, width, height};
	SiftPlan P;
	BHIP_TRY(planFor<T>(ctx, cfg, DevImg<const T>{in, 0, stride, width, height, 1}, true, P));
	SiftDescPlan D;
	const char* msg;
	const int s = siftDescPlan(desc, D, &msg);
	if (s != BHIP_OK) return bhip_fail(ctx, s, msg);
	CHECK_IMG(ctx, hin);
	if (!count || cap < 0 || (cap > 0 && (!x || !y || !scale || !orientation || !white || !descriptors))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> din;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	// out0 = [x | y | scale | orientation | descriptors | white | count]
	const size_t c1 = (size_t)std::max(cap, 1), c8 = align256(c1 * 8), cd = align256(c1 * 8 * D.dof);
	BHIP_TRY(sc->out0.reserve(ctx, 4 * c8 + cd + align256(c1) + 256));
	char* base = sc->out0.as<char>();
	SiftOut out;
	out.x = (double*)base; out.y = (double*)(base + c8); out.scale = (double*)(base + 2 * c8); out.orientation = (double*)(base + 3 * c8);
	out.desc = (double*)(base + 4 * c8); out.white = (uint8_t*)(base + 4 * c8 + cd); out.count = (int*)(base + 4 * c8 + cd + align256(c1));
	out.where = nullptr;
	out.cap = cap;
	BHIP_TRY(detectDevice<T>(ctx, P, DevImg<const T>(din), out, &D));
	BHIP_HIP(ctx, hipMemcpyAsync(ctx->hostScratch.p, out.count, 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the one synchronisation that decides how much to copy
	*count = ctx->hostScratch.as<int>()[0];
	const size_t n = (size_t)std::min(*count, cap);
	if (n > 0) {
		BHIP_HIP(ctx, hipMemcpyAsync(x, out.x, n * 8, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipMemcpyAsync(y, out.y, n * 8, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipMemcpyAsync(scale, out.scale, n * 8, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipMemcpyAsync(orientation, out.orientation, n * 8, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipMemcpyAsync(descriptors, out.desc, n * 8 * D.dof, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipMemcpyAsync(white, out.white, n, hipMemcpyDeviceToHost, ctx->stream));
	}
	return bhip_ctx_synchronize(ctx);
}

}   // namespace

extern "C" {

int bhip_csift_cfg_default(bhip_csift_cfg* desc) {
	if (!desc) return BHIP_ERR_INVALID;
	desc->histogramSize = 36; desc->sigmaEnlarge = 2.0;
	desc->widthSubregion = 4; desc->widthGrid = 4; desc->numHistogramBins = 8;
	desc->sigmaToPixels = 1.0; desc->weightingSigmaFraction = 0.5; desc->maxDescriptorElementValue = 0.2;
	return BHIP_OK;
}

int bhip_csift_dof(const bhip_csift_cfg* desc) {
	const char* msg;
	const int s = siftDescCheck(desc, &msg);
	return s != BHIP_OK ? s : desc->widthGrid * desc->widthGrid * desc->numHistogramBins;
}

int bhip_csift_weights(const bhip_csift_cfg* desc, double* expTable, float* gaussianWeight) {
	SiftDescPlan D;
	const char* msg;
	BHIP_TRY(siftDescPlan(desc, D, &msg));
	if (expTable) std::copy(D.expTable.begin(), D.expTable.end(), expTable);
	if (gaussianWeight) std::copy(D.gaussianWeight.begin(), D.gaussianWeight.end(), gaussianWeight);
	return BHIP_OK;
}

int bhip_csift_dev_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const bhip_csift_cfg* desc, const float* dev_in, long long imageStride, int stride, int width,
					   int height, int batch, double* dev_x, double* dev_y, double* dev_scale, double* dev_orientation, uint8_t* dev_white, double* dev_desc,
					   int* dev_count, int cap) {
	return csiftDev<float>(ctx, cfg, desc, dev_in, imageStride, stride, width, height, batch, {dev_x, dev_y, dev_scale, dev_white, nullptr, dev_count, cap, dev_orientation, dev_desc});
}
int bhip_csift_dev_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const bhip_csift_cfg* desc, const uint8_t* dev_in, long long imageStride, int stride, int width,
					  int height, int batch, double* dev_x, double* dev_y, double* dev_scale, double* dev_orientation, uint8_t* dev_white, double* dev_desc,
					  int* dev_count, int cap) {
	return csiftDev<uint8_t>(ctx, cfg, desc, dev_in, imageStride, stride, width, height, batch, {dev_x, dev_y, dev_scale, dev_white, nullptr, dev_count, cap, dev_orientation, dev_desc});
}
int bhip_csift_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const bhip_csift_cfg* desc, const float* in, int start, int stride, int width, int height, double* x,
				   double* y, double* scale, double* orientation, uint8_t* white, double* descriptors, int* count, int cap) {
	return csiftHost<float>(ctx, cfg, desc, in, start, stride, width, height, x, y, scale, orientation, white, descriptors, count, cap);
}
int bhip_csift_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const bhip_csift_cfg* desc, const uint8_t* in, int start, int stride, int width, int height, double* x,
				  double* y, double* scale, double* orientation, uint8_t* white, double* descriptors, int* count, int cap) {
	return csiftHost<uint8_t>(ctx, cfg, desc, in, start, stride, width, height, x, y, scale, orientation, white, descriptors, count, cap);
}


int bhip_sift_cfg_default(bhip_sift_cfg* cfg) {
	if (!cfg) return BHIP_ERR_INVALID;
	cfg->firstOctave = 0; cfg->lastOctave = 5; cfg->numScales = 3; cfg->sigma0 = 2.75f;
	cfg->extractRadius = 2; cfg->extractThreshold = 0; cfg->extractIgnoreBorder = 1; cfg->extractUseStrictRule = 1; cfg->extractDetectMin = 1; cfg->extractDetectMax = 1;
	cfg->maxFeaturesPerScale = 0; cfg->edgeR = 10;
	return BHIP_OK;
}

int bhip_sift_layout(const bhip_sift_cfg* cfg, int width, int height, int* dims, int cap, long long* scaleFloats, long long* dogFloats) {
	SiftPlan P;
	const char* msg;
	const int s = siftPlan(cfg, width, height, P, &msg);
	if (s != BHIP_OK) return s;
	for (int i = 0; dims && i < std::min(P.nOct, cap); i++) { dims[2 * i] = P.dims[2 * i]; dims[2 * i + 1] = P.dims[2 * i + 1]; }
	if (scaleFloats) *scaleFloats = P.scaleFloats;
	if (dogFloats) *dogFloats = P.dogFloats;
	return P.nOct;
}

int bhip_sift_scale_space_dev_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const float* dev_in, long long imageStride, int stride, int width, int height,
								  int batch, float* dev_scale, float* dev_dog) {
	return scaleSpaceDev<float>(ctx, cfg, dev_in, imageStride, stride, width, height, batch, dev_scale, dev_dog);
}
int bhip_sift_scale_space_dev_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const uint8_t* dev_in, long long imageStride, int stride, int width, int height,
								 int batch, float* dev_scale, float* dev_dog) {
	return scaleSpaceDev<uint8_t>(ctx, cfg, dev_in, imageStride, stride, width, height, batch, dev_scale, dev_dog);
}
int bhip_sift_detect_dev_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const float* dev_in, long long imageStride, int stride, int width, int height, int batch,
							 double* dev_x, double* dev_y, double* dev_scale, uint8_t* dev_white, int16_t* dev_where, int* dev_count, int cap) {
	return detectDev<float>(ctx, cfg, dev_in, imageStride, stride, width, height, batch, {dev_x, dev_y, dev_scale, dev_white, dev_where, dev_count, cap});
}
int bhip_sift_detect_dev_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const uint8_t* dev_in, long long imageStride, int stride, int width, int height, int batch,
							double* dev_x, double* dev_y, double* dev_scale, uint8_t* dev_white, int16_t* dev_where, int* dev_count, int cap) {
	return detectDev<uint8_t>(ctx, cfg, dev_in, imageStride, stride, width, height, batch, {dev_x, dev_y, dev_scale, dev_white, dev_where, dev_count, cap});
}
int bhip_sift_scale_space_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const float* in, int start, int stride, int width, int height, float* scale, float* dog) {
	return scaleSpaceHost<float>(ctx, cfg, in, start, stride, width, height, scale, dog);
}
int bhip_sift_scale_space_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const uint8_t* in, int start, int stride, int width, int height, float* scale, float* dog) {
	return scaleSpaceHost<uint8_t>(ctx, cfg, in, start, stride, width, height, scale, dog);
}
int bhip_sift_detect_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const float* in, int start, int stride, int width, int height, double* x, double* y,
						 double* scale, uint8_t* white, int16_t* where, int* count, int cap) {
	return detectHost<float>(ctx, cfg, in, start, stride, width, height, x, y, scale, white, where, count, cap);
}
int bhip_sift_detect_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const uint8_t* in, int start, int stride, int width, int height, double* x, double* y,
						double* scale, uint8_t* white, int16_t* where, int* count, int cap) {
	return detectHost<uint8_t>(ctx, cfg, in, start, stride, width, height, x, y, scale, white, where, count, cap);
}

}   // extern "C"
