// C ABI, dense KLT optical flow (kernels: flow.hip, the wave-per-pixel track kernel in klt.hip): DenseOpticalFlow.process of
// FactoryDenseOpticalFlow.flowKlt.  Rules, deviations and limits: bhip_flow_klt_dev_f32 in include/boofhip.h.  Below it, Horn-Schunck
// (FactoryDenseOpticalFlow.hornSchunck; kernels: hornschunck.hip).
#include "cabi.h"

namespace {
template <class TI_, class TD_>
struct FlowTypes {
	using TI = TI_;
	using TD = TD_;
	static constexpr bool u8 = std::is_same_v<TI_, uint8_t>;
};
using FlowF32 = FlowTypes<float, float>;      // GrayF32 frames and derivatives
using FlowU8 = FlowTypes<uint8_t, int16_t>;   // GrayU8 frames, GrayS16 derivatives

struct FlowPlan {
	bhip_klt_cfg cfg;
	int r, L, form;
	int scales[BHIP_KLT_MAX_LAYERS];
	int dims[2 * BHIP_KLT_MAX_LAYERS];
	long long offs[BHIP_KLT_MAX_LAYERS], total;
};

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
}  // namespace

// the argument checks every form shares, before anything is staged or launched (ctx has been checked)
static int flowPlan(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, int width, int height, int batch, int form, FlowPlan& p) {
	if (radius < 1 || numLayers < 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "dense flow: radius and numLayers must be >= 1");
	if (!scales || width <= 0 || height <= 0 || batch <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "dense flow: bad arguments");
	if (form != BHIP_FLOW_FORM_AUTO && form != BHIP_FLOW_FORM_LANE && form != BHIP_FLOW_FORM_WAVE) return bhip_fail(ctx, BHIP_ERR_INVALID, "dense flow: no such form");
	if (radius > BHIP_KLT_MAX_RADIUS || numLayers > BHIP_KLT_MAX_LAYERS) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "dense flow on the GPU: radius <= 7, numLayers <= 8");
	if (scales[0] != 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "dense flow: the first layer must have scale 1");
	for (int l = 1; l < numLayers; l++) {
		if (scales[l] < scales[l - 1]) return bhip_fail(ctx, BHIP_ERR_INVALID, "Higher layers must be the same size or larger than previous layers.");
		if (scales[l] % scales[l - 1] != 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Layer " + std::to_string(l) + " is not evenly divisible by its lower layer.");
	}
	if (cfg) p.cfg = *cfg; else bhip_klt_cfg_default(&p.cfg);
	if (p.cfg.maxIterations < 1) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "maxIterations must be >= 1");
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "dense flow on the GPU: at most 65535 pairs per call");
	if (form == BHIP_FLOW_FORM_LANE && radius > BHIP_FLOW_LANE_MAX_RADIUS) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "the lane-per-pixel form takes radius <= 3");
	p.r = radius; p.L = numLayers;
	p.form = form != BHIP_FLOW_FORM_AUTO ? form : radius <= BHIP_FLOW_LANE_MAX_RADIUS ? BHIP_FLOW_FORM_LANE : BHIP_FLOW_FORM_WAVE;
	for (int l = 0; l < numLayers; l++) p.scales[l] = scales[l];
	if (bhip_pyramid_layout(width, height, scales, numLayers, p.dims, p.offs, &p.total) != BHIP_OK) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad pyramid scales");
	return BHIP_OK;
}

// FlowKlt_to_DenseOpticalFlow.process :76-86 on device pairs, then the two stages of DenseOpticalFlowKlt.process
template <class Px>
static int flowDevice(bhip_ctx* ctx, const FlowPlan& p, DevImg<const typename Px::TI> src, DevImg<const typename Px::TI> dst, DevImg<float> flow, FlowRec* tracks) {
	using TI = typename Px::TI;
	using TD = typename Px::TD;
	CtxScratch* sc = scratchOf(ctx);
	const int W = src.width, H = src.height, B = src.batch;
	// scratch: [counter | source pyramid | destination pyramid | derivX | derivY | records]
	const size_t elems = (size_t)p.total * B;
	const size_t oSrc = 256, oDst = oSrc + align256(elems * sizeof(TI)), oDx = oDst + align256(elems * sizeof(TI)), oDy = oDx + align256(elems * sizeof(TD)),
				 oRec = oDy + align256(elems * sizeof(TD)), end = oRec + (tracks ? 0 : (size_t)W * H * B * sizeof(FlowRec));
	BHIP_TRY(sc->flow.reserve(ctx, end));
	char* base = (char*)sc->flow.p;
	unsigned long long* stats = (unsigned long long*)base;
	TI* pyrSrc = (TI*)(base + oSrc);
	TI* pyrDst = (TI*)(base + oDst);
	TD* dx = (TD*)(base + oDx);
	TD* dy = (TD*)(base + oDy);
	FlowRec* rec = tracks ? tracks : (FlowRec*)(base + oRec);
	BHIP_HIP(ctx, hipMemsetAsync(stats, 0, 8, ctx->stream));
	sc->flowPixels = (long long)W * H * B;
	// FactoryPyramid.discreteGaussian(scales, -1, 2, true): GrayF32 the Gaussian kernel of sigma -1 / radius 2, GrayU8 [1,4,7,4,1] / 17
	if constexpr (Px::u8) {
		static const std::vector<int32_t> k = bhip_gaussian1d_s32(2);   // static: the upload is asynchronous
		BHIP_TRY(pyramidImpl<TI>(ctx, k.data(), (int)k.size(), p.scales, p.L, src, pyrSrc));
		BHIP_TRY(pyramidImpl<TI>(ctx, k.data(), (int)k.size(), p.scales, p.L, dst, pyrDst));
	} else {
		static const std::vector<float> k = bhip_gaussian1d_f32(-1, 2);
		BHIP_TRY(pyramidImpl<TI>(ctx, k.data(), (int)k.size(), p.scales, p.L, src, pyrSrc));
		BHIP_TRY(pyramidImpl<TI>(ctx, k.data(), (int)k.size(), p.scales, p.L, dst, pyrDst));
	}
	for (int l = 0; l < p.L; l++)
		BHIP_TRY(bhip_launch_gradient(ctx, 0, bhip_pyr_layer<const TI>(pyrSrc, p.total, p.dims, p.offs, l, B), bhip_pyr_layer<TD>(dx, p.total, p.dims, p.offs, l, B),
									  bhip_pyr_layer<TD>(dy, p.total, p.dims, p.offs, l, B), 2));
	KltPyrT<TI, TD> P{};
	P.img = pyrSrc; P.dx = dx; P.dy = dy;
	P.frameStride = p.total;
	for (int l = 0; l < p.L; l++) { P.off[l] = p.offs[l]; P.w[l] = p.dims[2 * l]; P.h[l] = p.dims[2 * l + 1]; P.stride[l] = p.dims[2 * l]; P.scale[l] = (float)(double)p.scales[l]; }
	P.numLayers = p.L; P.frameW = W; P.frameH = H;
	if (p.form == BHIP_FLOW_FORM_LANE) BHIP_TRY(bhip_launch_flow_track_lane(ctx, P, pyrDst, p.r, p.cfg, B, rec, stats));
	else BHIP_TRY(bhip_launch_flow_track_wave(ctx, P, pyrDst, p.r, p.cfg, B, rec, stats));
	return bhip_launch_flow_reduce(ctx, rec, p.r, flow);
}

template <class Px>
static int flowDev(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, const typename Px::TI* dev_src, long long sImageStride, int sStride,
				   const typename Px::TI* dev_dst, long long dImageStride, int dStride, int width, int height, int batch, float* dev_flow, long long fImageStride,
				   int fStride, void* dev_tracks, int form) {
	CHECK_CTX(ctx);
	FlowPlan p;
	BHIP_TRY(flowPlan(ctx, cfg, radius, scales, numLayers, width, height, batch, form, p));
	const DevImg<const typename Px::TI> src{dev_src, sImageStride, sStride, width, height, batch}, dst{dev_dst, dImageStride, dStride, width, height, batch};
	CHECK_IMG(ctx, src);
	CHECK_IMG(ctx, dst);
	if (!dev_flow || fStride < 2 * width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad flow image (null or stride < 2 * width)");
	return flowDevice<Px>(ctx, p, src, dst, {dev_flow, fImageStride, fStride, width, height, batch}, (FlowRec*)dev_tracks);
}

template <class Px>
static int flowHost(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, const typename Px::TI* src, int sStart, int sStride,
					const typename Px::TI* dst, int dStart, int dStride, int width, int height, float* flow, int fStart, int fStride) {
	using TI = typename Px::TI;
	CHECK_CTX(ctx);
	FlowPlan p;
	BHIP_TRY(flowPlan(ctx, cfg, radius, scales, numLayers, width, height, 1, BHIP_FLOW_FORM_AUTO, p));
	const HostImg<const TI> hs{src, sStart, sStride, width, height}, hd{dst, dStart, dStride, width, height};
	CHECK_IMG(ctx, hs);
	CHECK_IMG(ctx, hd);
	if (!flow || fStride < 2 * width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad flow image (null or stride < 2 * width)");
	const HostImg<float> hf{flow, fStart, fStride, 2 * width, height};   // a row of (x, y) pairs
	CtxScratch* sc = scratchOf(ctx);
	DevImg<TI> ds, dd;
	DevImg<float> df;
	BHIP_TRY(stageIn(ctx, sc->in0, hs, width, ds));
	BHIP_TRY(stageIn(ctx, sc->in1, hd, width, dd));
	BHIP_TRY(stageIn(ctx, sc->out0, hf, 2 * width, df, false));
	BHIP_TRY(flowDevice<Px>(ctx, p, ds, dd, {df.data, df.imageStride, df.stride, width, height, 1}, nullptr));
	BHIP_TRY(stageOut(ctx, hf, df));
	return bhip_ctx_synchronize(ctx);
}

// ---------------------------------------------------------------------------------------------------------------
// Horn-Schunck dense optical flow (kernels: hornschunck.hip): HornSchunck.process of FactoryDenseOpticalFlow.hornSchunck.  Rules, deviations and
// limits: bhip_flow_hs_dev_f32 in include/boofhip.h.
// ---------------------------------------------------------------------------------------------------------------
// itersPerLaunch 0: the depth that scripts/bench_hornschunck.py measures as the fastest on 1080p pairs
#define HS_AUTO_DEPTH BHIP_FLOW_HS_MAX_FUSED

// the argument checks both forms share, before anything is staged or launched (ctx has been checked)
static int hsCheck(bhip_ctx* ctx, int width, int height, int batch, int itersPerLaunch) {
	if (width <= 0 || height <= 0 || batch <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Horn-Schunck: bad arguments");
	if (itersPerLaunch < 0 || itersPerLaunch > BHIP_FLOW_HS_MAX_FUSED) return bhip_fail(ctx, BHIP_ERR_INVALID, "Horn-Schunck: itersPerLaunch must be 0 .. 8");
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "Horn-Schunck on the GPU: at most 65535 pairs per call");
	if (width > (1 << 20) || height > (1 << 20) || (long long)width * height > (1LL << 28))
		return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "Horn-Schunck on the GPU: width, height <= 1048576 and width * height <= 2^28");
	return BHIP_OK;
}

// HornSchunck.process :92-110 on device pairs: the three derivatives, then findFlow as launches of up to `depth` iterations that alternate
// between the two scratch flows; the first starts from the zero flow (no buffer is read) and the last writes `flow`
template <class T>
static int hsDevice(bhip_ctx* ctx, float alpha, int numIterations, DevImg<const T> src, DevImg<const T> dst, DevImg<float> flow, float* deriv, int itersPerLaunch) {
	CtxScratch* sc = scratchOf(ctx);
	const int depth = itersPerLaunch ? itersPerLaunch : HS_AUTO_DEPTH;
	int left = std::max(numIterations, 0);
	const size_t px = (size_t)src.width * src.height * src.batch;
	const size_t oFlow = deriv ? 0 : align256(px * 3 * sizeof(float)), flowBytes = align256(px * 2 * sizeof(float));
	BHIP_TRY(sc->flowHs.reserve(ctx, oFlow + (left > depth ? 2 * flowBytes : 0)));
	char* base = (char*)sc->flowHs.p;
	if (!deriv) deriv = (float*)base;
	float* tmp[2] = {(float*)(base + oFlow), (float*)(base + oFlow + flowBytes)};
	BHIP_TRY(bhip_launch_hs_derivatives<T>(ctx, src, dst, deriv));
	const float alpha2 = alpha * alpha;   // HornSchunck.java:68
	const float* in = nullptr;
	int which = 0;
	do {
		const int step = std::min(left, depth);
		left -= step;
		const DevImg<float> out = left == 0 ? flow : DevImg<float>{tmp[which], (long long)2 * src.width * src.height, 2 * src.width, src.width, src.height, src.batch};
		BHIP_TRY(bhip_launch_hs_iterate(ctx, deriv, in, out, alpha2, step));
		in = out.data;
		which ^= 1;
	} while (left > 0);
	return BHIP_OK;
}

template <class T>
static int hsDev(bhip_ctx* ctx, float alpha, int numIterations, const T* dev_src, long long sImageStride, int sStride, const T* dev_dst, long long dImageStride,
				 int dStride, int width, int height, int batch, float* dev_flow, long long fImageStride, int fStride, float* dev_deriv, int itersPerLaunch) {
	CHECK_CTX(ctx);
	BHIP_TRY(hsCheck(ctx, width, height, batch, itersPerLaunch));
	const DevImg<const T> src{dev_src, sImageStride, sStride, width, height, batch}, dst{dev_dst, dImageStride, dStride, width, height, batch};
	CHECK_IMG(ctx, src);
	CHECK_IMG(ctx, dst);
	if (!dev_flow || fStride < 2 * width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad flow image (null or stride < 2 * width)");
	return hsDevice<T>(ctx, alpha, numIterations, src, dst, {dev_flow, fImageStride, fStride, width, height, batch}, dev_deriv, itersPerLaunch);
}

template <class T>
static int hsHost(bhip_ctx* ctx, float alpha, int numIterations, const T* src, int sStart, int sStride, const T* dst, int dStart, int dStride, int width, int height,
				  float* flow, int fStart, int fStride) {
	CHECK_CTX(ctx);
	BHIP_TRY(hsCheck(ctx, width, height, 1, 0));
	const HostImg<const T> hs{src, sStart, sStride, width, height}, hd{dst, dStart, dStride, width, height};
	CHECK_IMG(ctx, hs);
	CHECK_IMG(ctx, hd);
	if (!flow || fStride < 2 * width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad flow image (null or stride < 2 * width)");
	const HostImg<float> hf{flow, fStart, fStride, 2 * width, height};   // a row of (x, y) pairs
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> ds, dd;
	DevImg<float> df;
	BHIP_TRY(stageIn(ctx, sc->in0, hs, width, ds));
	BHIP_TRY(stageIn(ctx, sc->in1, hd, width, dd));
	BHIP_TRY(stageIn(ctx, sc->out0, hf, 2 * width, df, false));
	BHIP_TRY(hsDevice<T>(ctx, alpha, numIterations, DevImg<const T>(ds), DevImg<const T>(dd), {df.data, df.imageStride, df.stride, width, height, 1}, nullptr, 0));
	BHIP_TRY(stageOut(ctx, hf, df));
	return bhip_ctx_synchronize(ctx);
}

extern "C" {

int bhip_flow_hs_dev_f32(bhip_ctx* ctx, float alpha, int numIterations, const float* dev_src, long long sImageStride, int sStride, const float* dev_dst,
						 long long dImageStride, int dStride, int width, int height, int batch, float* dev_flow, long long fImageStride, int fStride,
						 float* dev_deriv, int itersPerLaunch) {
	return hsDev<float>(ctx, alpha, numIterations, dev_src, sImageStride, sStride, dev_dst, dImageStride, dStride, width, height, batch, dev_flow, fImageStride, fStride,
						dev_deriv, itersPerLaunch);
}
int bhip_flow_hs_dev_u8(bhip_ctx* ctx, float alpha, int numIterations, const uint8_t* dev_src, long long sImageStride, int sStride, const uint8_t* dev_dst,
						long long dImageStride, int dStride, int width, int height, int batch, float* dev_flow, long long fImageStride, int fStride,
						float* dev_deriv, int itersPerLaunch) {
	return hsDev<uint8_t>(ctx, alpha, numIterations, dev_src, sImageStride, sStride, dev_dst, dImageStride, dStride, width, height, batch, dev_flow, fImageStride,
						  fStride, dev_deriv, itersPerLaunch);
}
int bhip_flow_hs_f32(bhip_ctx* ctx, float alpha, int numIterations, const float* src, int sStart, int sStride, const float* dst, int dStart, int dStride,
					 int width, int height, float* flow, int fStart, int fStride) {
	return hsHost<float>(ctx, alpha, numIterations, src, sStart, sStride, dst, dStart, dStride, width, height, flow, fStart, fStride);
}
int bhip_flow_hs_u8(bhip_ctx* ctx, float alpha, int numIterations, const uint8_t* src, int sStart, int sStride, const uint8_t* dst, int dStart, int dStride,
					int width, int height, float* flow, int fStart, int fStride) {
	return hsHost<uint8_t>(ctx, alpha, numIterations, src, sStart, sStride, dst, dStart, dStride, width, height, flow, fStart, fStride);
}

int bhip_flow_klt_dev_f32(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, const float* dev_src, long long sImageStride,
						  int sStride, const float* dev_dst, long long dImageStride, int dStride, int width, int height, int batch, float* dev_flow,
						  long long fImageStride, int fStride, void* dev_tracks, int form) {
	return flowDev<FlowF32>(ctx, cfg, radius, scales, numLayers, dev_src, sImageStride, sStride, dev_dst, dImageStride, dStride, width, height, batch, dev_flow,
							fImageStride, fStride, dev_tracks, form);
}
int bhip_flow_klt_dev_u8(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, const uint8_t* dev_src, long long sImageStride,
						 int sStride, const uint8_t* dev_dst, long long dImageStride, int dStride, int width, int height, int batch, float* dev_flow,
						 long long fImageStride, int fStride, void* dev_tracks, int form) {
	return flowDev<FlowU8>(ctx, cfg, radius, scales, numLayers, dev_src, sImageStride, sStride, dev_dst, dImageStride, dStride, width, height, batch, dev_flow,
						   fImageStride, fStride, dev_tracks, form);
}
int bhip_flow_klt_f32(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, const float* src, int sStart, int sStride,
					  const float* dst, int dStart, int dStride, int width, int height, float* flow, int fStart, int fStride) {
	return flowHost<FlowF32>(ctx, cfg, radius, scales, numLayers, src, sStart, sStride, dst, dStart, dStride, width, height, flow, fStart, fStride);
}
int bhip_flow_klt_u8(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, const uint8_t* src, int sStart, int sStride,
					 const uint8_t* dst, int dStart, int dStride, int width, int height, float* flow, int fStart, int fStride) {
	return flowHost<FlowU8>(ctx, cfg, radius, scales, numLayers, src, sStart, sStride, dst, dStart, dStride, width, height, flow, fStart, fStride);
}

int bhip_flow_klt_stats(bhip_ctx* ctx, long long* pixels, long long* iterations) {
	CHECK_CTX(ctx);
	CtxScratch* sc = scratchOf(ctx);
	long long it = 0;
	if (sc->flow.p) {
		BHIP_HIP(ctx, hipMemcpyAsync(&it, sc->flow.p, 8, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	}
	if (pixels) *pixels = sc->flowPixels;
	if (iterations) *iterations = it;
	return BHIP_OK;
}

}  // extern "C"
