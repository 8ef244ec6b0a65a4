// ---------------------------------------------------------------------------------------------------------------
// Pyramid KLT point tracker (kernels: klt.hip)
// ---------------------------------------------------------------------------------------------------------------
#include "cabi.h"

// The track table: every per-track array of KltTab carved out of one device block, the per-sequence counters out of another (they do not
// depend on the capacity, so a regrown table keeps them).
namespace {
struct KltArr { size_t elem; int outer; size_t inner; };   // [outer][batch][cap * inner] elements of `elem` bytes
enum { KA_ACT, KA_DRP, KA_SPW, KA_FREE, KA_ID, KA_X, KA_Y, KA_TX, KA_TY, KA_ERR, KA_FAULT, KA_KEEP, KA_ITERS, KA_LX, KA_LY, KA_GXX, KA_GXY, KA_GYY, KA_TMPL, KA_N };

struct KltTable {
	DevBuf buf, cnt;
	KltTab v{};
	KltArr arr[KA_N];
	size_t off[KA_N + 1];

	int alloc(bhip_ctx* ctx, int batch, int cap, int L, int r, DevBuf* keepCnt = nullptr) {
		const int len = (2 * r + 1) * (2 * r + 1);
		for (int i = 0; i < KA_N; i++) arr[i] = KltArr{4, 1, 1};
		arr[KA_ID].elem = 8;
		for (int i = KA_LX; i <= KA_GYY; i++) arr[i].outer = L;
		arr[KA_TMPL].inner = (size_t)L * 3 * len;
		off[0] = 0;
		for (int i = 0; i < KA_N; i++) off[i + 1] = off[i] + ((arr[i].elem * arr[i].outer * batch * cap * arr[i].inner + 15) & ~(size_t)15);
		BHIP_TRY(buf.reserve(ctx, off[KA_N]));
		BHIP_HIP(ctx, hipMemsetAsync(buf.p, 0, off[KA_N], ctx->stream));
		if (keepCnt) cnt = std::move(*keepCnt);
		else {
			BHIP_TRY(cnt.reserve(ctx, (size_t)batch * 24));
			BHIP_HIP(ctx, hipMemsetAsync(cnt.p, 0, (size_t)batch * 24, ctx->stream));
		}
		char* p = (char*)buf.p;
		v.cap = cap; v.batch = batch; v.L = L; v.r = r; v.len = len;
		v.act = (int*)(p + off[KA_ACT]); v.drp = (int*)(p + off[KA_DRP]); v.spw = (int*)(p + off[KA_SPW]); v.freeL = (int*)(p + off[KA_FREE]);
		v.id = (long long*)(p + off[KA_ID]);
		v.x = (float*)(p + off[KA_X]); v.y = (float*)(p + off[KA_Y]); v.tx = (float*)(p + off[KA_TX]); v.ty = (float*)(p + off[KA_TY]);
		v.err = (float*)(p + off[KA_ERR]); v.fault = (int*)(p + off[KA_FAULT]); v.keep = (int*)(p + off[KA_KEEP]); v.iters = (int*)(p + off[KA_ITERS]);
		v.lx = (float*)(p + off[KA_LX]); v.ly = (float*)(p + off[KA_LY]); v.gxx = (float*)(p + off[KA_GXX]); v.gxy = (float*)(p + off[KA_GXY]);
		v.gyy = (float*)(p + off[KA_GYY]); v.tmpl = (float*)(p + off[KA_TMPL]);
		v.total = (long long*)cnt.p;
		v.nAct = (int*)((char*)cnt.p + (size_t)batch * 8);
		v.nDrp = v.nAct + batch; v.nSpw = v.nDrp + batch; v.nFree = v.nSpw + batch;
		return BHIP_OK;
	}
};
}  // namespace

// the pixel types a tracker runs on: image / derivative (KltPyrT)
template <class TI_, class TD_>
struct KltTypes {
	using TI = TI_;
	using TD = TD_;
	static constexpr bool u8 = std::is_same_v<TI_, uint8_t>;
};
using KltF32 = KltTypes<float, float>;      // bhip_klt_create: GrayF32 frames and derivatives
using KltU8 = KltTypes<uint8_t, int16_t>;   // bhip_klt_create_u8: GrayU8 frames, GrayS16 derivatives

// everything a tracker holds on its context's device (CtxChild)
struct KltDevice {
	KltTable tab;
	DevBuf frames, pyr, dx, dy, intensity, candXY, candN, stage;
	PinnedBuf pinned;
};

struct bhip_klt : CtxChild<KltDevice> {
	void onRelease() { haveFrame = false; }
	bhip_klt_cfg cfg;
	int r = 0, L = 0, W = 0, H = 0, batch = 0;
	int scales[BHIP_KLT_MAX_LAYERS];
	int dims[2 * BHIP_KLT_MAX_LAYERS];
	long long offs[BHIP_KLT_MAX_LAYERS], total = 0;
	int detectRadius = 0, detectBorder = 0;
	float detectThreshold = 0;
	std::vector<float> kernel;   // FactoryPyramid.discreteGaussian(scales, -1, 2)
	std::vector<int32_t> kernelS32;   // the same for a GrayU8 tracker: Kernel1D_S32 [1,4,7,4,1]
	bool u8 = false;             // GrayU8 frames with GrayS16 derivatives (bhip_klt_create_u8); pyr holds bytes, dx / dy shorts
	bool haveFrame = false;
	int ub = 0;                  // no sequence has more active tracks than this (exact after a spawn or bhip_klt_counts)
	// f(KltF32{}) or f(KltU8{}): the one place that turns `u8` into types
	template <class F>
	int withTypes(F f) const { return u8 ? f(KltU8{}) : f(KltF32{}); }
	// layer l of every frame in the image (which 0), dx (1) or dy (2) pyramid
	template <class T>
	DevImg<T> layer(int which, int l) const { return bhip_pyr_layer((which == 0 ? pyr : which == 1 ? dx : dy).as<T>(), total, dims, offs, l, batch); }
	template <class Px>
	KltPyrT<typename Px::TI, typename Px::TD> view() const {
		KltPyrT<typename Px::TI, typename Px::TD> P{};
		P.img = pyr.as<typename Px::TI>(); P.dx = dx.as<typename Px::TD>(); P.dy = dy.as<typename Px::TD>();
		P.frameStride = total;
		for (int l = 0; l < L; l++) { P.off[l] = offs[l]; P.w[l] = dims[2 * l]; P.h[l] = dims[2 * l + 1]; P.stride[l] = dims[2 * l]; P.scale[l] = (float)(double)scales[l]; }
		P.numLayers = L; P.frameW = W; P.frameH = H;
		return P;
	}
};

static bool kltRangeOk(int radius, int numLayers) { return radius >= 1 && radius <= BHIP_KLT_MAX_RADIUS && numLayers >= 1 && numLayers <= BHIP_KLT_MAX_LAYERS; }

// the table regrows like the other device lists: a larger block, the old contents copied array by array, the new slots appended to every
// sequence's unused list
static int kltGrow(bhip_klt* k, int newCap) {
	bhip_ctx* ctx = k->ctx;
	KltTable nt;
	const KltTable& ot = k->tab;
	const int oldCap = ot.v.cap;
	if (nt.alloc(ctx, k->batch, newCap, k->L, k->r, &k->tab.cnt) != BHIP_OK) {
		if (nt.cnt.p) k->tab.cnt = std::move(nt.cnt);
		return bhip_fail(ctx, BHIP_ERR_CAPACITY, "the track table could not grow");
	}
	for (int i = 0; i < KA_N; i++) {
		const size_t oldRow = ot.arr[i].elem * ot.arr[i].inner * oldCap, newRow = nt.arr[i].elem * nt.arr[i].inner * newCap;
		BHIP_HIP(ctx, hipMemcpy2DAsync((char*)nt.buf.p + nt.off[i], newRow, (const char*)ot.buf.p + ot.off[i], oldRow, oldRow,
									   (size_t)ot.arr[i].outer * k->batch, hipMemcpyDeviceToDevice, ctx->stream));
	}
	BHIP_TRY(bhip_launch_klt_init(ctx, nt.v, oldCap));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	k->tab = std::move(nt);
	return BHIP_OK;
}

// counters of every sequence to the host: [nAct | nDrp | nSpw | nFree][batch] ints
static int kltReadCounts(bhip_klt* k, const int** out) {
	bhip_ctx* ctx = k->ctx;
	BHIP_TRY(k->pinned.reserve(ctx, (size_t)k->batch * 32));
	BHIP_HIP(ctx, hipMemcpyAsync(k->pinned.p, k->tab.v.nAct, (size_t)k->batch * 16, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	*out = k->pinned.as<int>();
	return BHIP_OK;
}

// setDescription of the tracks `mode` selects (bhip_launch_klt_describe) on the tracker's own pixel types
static int kltDescribe(bhip_klt* k, int mode, const int* count, int maxCount) {
	return k->withTypes([&](auto px) { return bhip_launch_klt_describe(k->ctx, k->view<decltype(px)>(), k->tab.v, k->cfg, mode, count, maxCount); });
}

// process() once the pyramid and its gradient are in place
static int kltTrackFrame(bhip_klt* k) {
	bhip_ctx* ctx = k->ctx;
	k->haveFrame = true;
	BHIP_TRY(bhip_launch_klt_begin(ctx, k->tab.v));
	BHIP_TRY(k->withTypes([&](auto px) { return bhip_launch_klt_track(ctx, k->view<decltype(px)>(), k->tab.v, k->cfg, k->ub); }));
	BHIP_TRY(kltDescribe(k, 0, nullptr, k->ub));
	return bhip_launch_klt_compact(ctx, k->tab.v, 0);
}

// process() on device frames: PyramidDiscreteSampleBlur (GrayF32: FactoryPyramid.discreteGaussian's kernel, GrayU8: [1,4,7,4,1] / 17), then
// PyramidOps.gradient with FactoryDerivative.sobel -- BorderType.EXTENDED; GrayU8 -> GrayS16 -- then the tracking.
// inLayer0: the frames are already in layer 0 of the pyramid, which `frames` views
template <class Px>
static int kltProcess(bhip_klt* k, DevImg<const typename Px::TI> frames, bool inLayer0) {
	using TI = typename Px::TI;
	using TD = typename Px::TD;
	bhip_ctx* ctx = k->ctx;
	if constexpr (Px::u8) BHIP_TRY(pyramidImpl<TI>(ctx, k->kernelS32.data(), (int)k->kernelS32.size(), k->scales, k->L, frames, k->pyr.as<TI>(), inLayer0));
	else BHIP_TRY(pyramidImpl<TI>(ctx, k->kernel.data(), (int)k->kernel.size(), k->scales, k->L, frames, k->pyr.as<TI>(), inLayer0));
	for (int l = 0; l < k->L; l++) BHIP_TRY(bhip_launch_gradient(ctx, 0, k->layer<const TI>(0, l), k->layer<TD>(1, l), k->layer<TD>(2, l), 2));
	return kltTrackFrame(k);
}

// spawnTracks from candidate lists on the device (dev_xy [batch][xyCap] (x,y) int16 pairs in layer-0 pixels, dev_n [batch], each <= xyCap)
static int kltSpawnFrom(bhip_klt* k, const int16_t* dev_xy, int xyCap, const int* dev_n) {
	bhip_ctx* ctx = k->ctx;
	BHIP_TRY(k->pinned.reserve(ctx, (size_t)k->batch * 32));
	int* h = k->pinned.as<int>();
	BHIP_HIP(ctx, hipMemcpyAsync(h, k->tab.v.nAct, (size_t)k->batch * 16, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(h + 4 * k->batch, dev_n, (size_t)k->batch * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const int B = k->batch;
	int need = 0, maxCand = 0, ub = 0;
	for (int b = 0; b < B; b++) {
		const int c = h[4 * B + b];
		if (c > xyCap) return bhip_fail(ctx, BHIP_ERR_CAPACITY, "candidate list overflowed");
		need = std::max(need, c - h[3 * B + b]);
		maxCand = std::max(maxCand, c);
		ub = std::max(ub, h[b] + c);
	}
	if (need > 0) BHIP_TRY(kltGrow(k, (k->tab.v.cap + std::max(need, k->tab.v.cap / 2) + 255) & ~255));
	const float scale0 = (float)(double)k->scales[0];
	BHIP_TRY(bhip_launch_klt_spawn_place(ctx, k->tab.v, dev_xy, xyCap, dev_n, scale0, maxCand));
	BHIP_TRY(kltDescribe(k, 1, dev_n, maxCand));
	BHIP_TRY(bhip_launch_klt_spawn_commit(ctx, k->tab.v, dev_n));
	k->ub = std::max(k->ub, ub);
	return BHIP_OK;
}

#define CHECK_KLT(k)                    \
	if (!(k)) return BHIP_ERR_INVALID;  \
	bhip_ctx* ctx = (k)->ctx;           \
	CHECK_CTX(ctx)
#define CHECK_KLT_TYPE(k, wantU8) \
	if ((k)->u8 != (wantU8)) return bhip_fail(ctx, BHIP_ERR_INVALID, (k)->u8 ? "this tracker was created for GrayU8 frames" : "this tracker was created for GrayF32 frames")

// a one-layer, one-sequence table for the stage-level calls: n tracks at xy, all active
static int kltStageTable(bhip_ctx* ctx, KltTable& tab, int radius, const float* xy, int n) {
	BHIP_TRY(tab.alloc(ctx, 1, std::max(n, 1), 1, radius));
	BHIP_TRY(bhip_launch_klt_init(ctx, tab.v, 0));
	std::vector<int> act(n);
	std::vector<float> x(n), y(n);
	for (int i = 0; i < n; i++) { act[i] = i; x[i] = xy[2 * i]; y[i] = xy[2 * i + 1]; }
	BHIP_HIP(ctx, hipMemcpyAsync(tab.v.act, act.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(tab.v.x, x.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(tab.v.y, y.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(tab.v.nAct, &n, 4, hipMemcpyHostToDevice, ctx->stream));
	return bhip_ctx_synchronize(ctx);   // the host vectors leave scope
}
template <class TI, class TD>
static KltPyrT<TI, TD> kltStagePyr(const TI* img, const TD* dx, const TD* dy, int width, int height) {
	KltPyrT<TI, TD> P{};
	P.img = img; P.dx = dx; P.dy = dy;
	P.w[0] = width; P.h[0] = height; P.stride[0] = width; P.scale[0] = 1.0f;
	P.numLayers = 1; P.frameW = width; P.frameH = height;
	return P;
}

template <class Px>
static int kltProcessDev(bhip_klt* k, const typename Px::TI* dev_frames, long long imageStride, int stride) {
	CHECK_KLT(k);
	CHECK_KLT_TYPE(k, Px::u8);
	if (!dev_frames || stride < k->W) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image batch");
	return kltProcess<Px>(k, {dev_frames, imageStride, stride, k->W, k->H, k->batch}, false);
}

template <class Px>
static int kltProcessHost(bhip_klt* k, const typename Px::TI* const* img, const int* startIndex, const int* stride) {
	using TI = typename Px::TI;
	CHECK_KLT(k);
	CHECK_KLT_TYPE(k, Px::u8);
	if (!img) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image batch");
	for (int b = 0; b < k->batch; b++)
		if (!img[b] || (stride ? stride[b] : k->W) < k->W) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image (null or stride < width)");
	// A GrayU8 tracker whose layer 0 is the frame itself (scale[0] == 1) takes the frames straight into the pyramid; every other tracker
	// stages them in `frames`.
	const bool uploadToLayer0 = Px::u8 && k->scales[0] == 1;
	if (!uploadToLayer0) BHIP_TRY(k->frames.reserve(ctx, (size_t)k->W * k->H * sizeof(TI) * k->batch));
	const DevImg<TI> dst = uploadToLayer0 ? k->layer<TI>(0, 0) : bhip_img_over<TI>(k->frames, k->W, k->W, k->H, k->batch);
	for (int b = 0; b < k->batch; b++)
		BHIP_TRY(upload<TI>(ctx, dst.data + b * dst.imageStride, k->W, img[b], startIndex ? startIndex[b] : 0, stride ? stride[b] : k->W, k->W, k->H, ctx->stream));
	BHIP_TRY(kltProcess<Px>(k, dst, uploadToLayer0));
	return bhip_ctx_synchronize(ctx);   // the caller's frames have been consumed
}

// bhip_klt_fetch_layer*: layer `layer` of sequence seq from the image (which 0), dx (1) or dy (2) pyramid, as T; which >= whichMin
template <class T>
static int kltFetchLayer(bhip_klt* k, int seq, int layer, int which, int whichMin, T* out) {
	CHECK_KLT(k);
	CHECK_KLT_TYPE(k, (!std::is_same_v<T, float>));
	if (!k->haveFrame) return bhip_fail(ctx, BHIP_ERR_INVALID, "no frame processed");
	if (seq < 0 || seq >= k->batch || layer < 0 || layer >= k->L || which < whichMin || which > 2 || !out) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad layer selector");
	const DevImg<const T> v = k->layer<const T>(which, layer);
	BHIP_HIP(ctx, hipMemcpyAsync(out, v.data + seq * v.imageStride, (size_t)v.width * v.height * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

template <class Px>
static int kltDevView(bhip_klt* k, const int** dev_activeSlots, const int** dev_activeCount, const float** dev_x, const float** dev_y,
					  const long long** dev_featureId, const typename Px::TI** dev_pyramid, const typename Px::TD** dev_derivX, const typename Px::TD** dev_derivY,
					  int* slotsPerSequence, long long* elementsPerFrame) {
	CHECK_KLT(k);
	CHECK_KLT_TYPE(k, Px::u8);
	const KltTab& T = k->tab.v;
	if (dev_activeSlots) *dev_activeSlots = T.act;
	if (dev_activeCount) *dev_activeCount = T.nAct;
	if (dev_x) *dev_x = T.x;
	if (dev_y) *dev_y = T.y;
	if (dev_featureId) *dev_featureId = T.id;
	if (dev_pyramid) *dev_pyramid = k->pyr.as<typename Px::TI>();
	if (dev_derivX) *dev_derivX = k->dx.as<typename Px::TD>();
	if (dev_derivY) *dev_derivY = k->dy.as<typename Px::TD>();
	if (slotsPerSequence) *slotsPerSequence = T.cap;
	if (elementsPerFrame) *elementsPerFrame = k->total;
	return BHIP_OK;
}

static int kltCreate(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int templateRadius, const int* scales, int numLayers, int detectRadius, float detectThreshold,
					 int detectBorder, int width, int height, int batch, bool u8, bhip_klt** out) {
	if (out) *out = nullptr;
	if (!kltRangeOk(templateRadius, numLayers)) return BHIP_ERR_UNSUPPORTED;   // templateRadius 1..7, numLayers 1..8; nothing is touched, not even ctx
	return createChild(ctx, out, [&](std::unique_ptr<bhip_klt>& k) -> int {
		if (!out) return bhip_fail(ctx, BHIP_ERR_INVALID, "null output");
		if (cfg && cfg->maxIterations < 1) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "maxIterations must be >= 1");
		if (!scales || width <= 0 || height <= 0 || batch <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad tracker arguments");
		CHECK_CTX(ctx);
		k.reset(new (std::nothrow) bhip_klt());
		if (!k) return bhip_fail(ctx, BHIP_ERR_NOMEM, "out of host memory");
		k->ctx = ctx;
		if (cfg) k->cfg = *cfg; else bhip_klt_cfg_default(&k->cfg);
		k->r = templateRadius; k->L = numLayers; k->W = width; k->H = height; k->batch = batch;
		k->detectRadius = detectRadius; k->detectThreshold = detectThreshold; k->detectBorder = detectBorder;
		for (int l = 0; l < numLayers; l++) k->scales[l] = scales[l];
		if (bhip_pyramid_layout(width, height, scales, numLayers, k->dims, k->offs, &k->total) != BHIP_OK) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad pyramid scales");
		for (int l = 1; l < numLayers; l++)
			if (scales[l] / scales[l - 1] <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Skip must be >= 1");
		k->u8 = u8;
		if (u8) k->kernelS32 = bhip_gaussian1d_s32(2);
		else k->kernel = bhip_gaussian1d_f32(-1, 2);
		const size_t elems = (size_t)k->total * batch;
		BHIP_TRY(k->pyr.reserve(ctx, elems * (u8 ? 1 : 4)));
		BHIP_TRY(k->dx.reserve(ctx, elems * (u8 ? 2 : 4)));
		BHIP_TRY(k->dy.reserve(ctx, elems * (u8 ? 2 : 4)));
		BHIP_TRY(k->tab.alloc(ctx, batch, BHIP_KLT_INITIAL_CAPACITY, numLayers, templateRadius));
		BHIP_TRY(bhip_launch_klt_init(ctx, k->tab.v, 0));
		BHIP_TRY(bhip_ctx_synchronize(ctx));
		return BHIP_OK;
	});
}

template <class TI, class TD>
static int kltSetDescriptionStage(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const TI* image, int imgStart, int imgStride, const TD* derivX,
								  const TD* derivY, int dStart, int dStride, int width, int height, const float* xy, int n, float* desc, float* descX,
								  float* descY, float* G, uint8_t* ok) {
	if (!kltRangeOk(radius, 1)) return BHIP_ERR_UNSUPPORTED;   // templateRadius 1..7; nothing is written
	const HostImg<const TI> himg{image, imgStart, imgStride, width, height};
	const HostImg<const TD> hdx{derivX, dStart, dStride, width, height}, hdy{derivY, dStart, dStride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, himg);
	CHECK_IMG(ctx, hdx);
	CHECK_IMG(ctx, hdy);
	if (n < 0 || (n > 0 && (!xy || !desc || !descX || !descY || !G || !ok))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad feature list");
	if (n == 0) return BHIP_OK;
	bhip_klt_cfg c;
	if (cfg) c = *cfg; else bhip_klt_cfg_default(&c);
	CtxScratch* sc = scratchOf(ctx);
	DevImg<TI> dimg;
	DevImg<TD> ddx, ddy;
	BHIP_TRY(stageIn(ctx, sc->in0, himg, width, dimg));
	BHIP_TRY(stageIn(ctx, sc->in1, hdx, width, ddx));
	BHIP_TRY(stageIn(ctx, sc->tmp0, hdy, width, ddy));
	KltTable tab;
	BHIP_TRY(kltStageTable(ctx, tab, radius, xy, n));
	BHIP_TRY(bhip_launch_klt_describe(ctx, kltStagePyr<TI, TD>(dimg.data, ddx.data, ddy.data, width, height), tab.v, c, 2, nullptr, n));
	const int len = tab.v.len;
	std::vector<float> t((size_t)n * 3 * len), g((size_t)3 * n);
	std::vector<int> keep(n), fault(n);
	BHIP_HIP(ctx, hipMemcpyAsync(t.data(), tab.v.tmpl, t.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(g.data(), tab.v.gxx, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(g.data() + n, tab.v.gyy, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(g.data() + 2 * n, tab.v.gxy, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(keep.data(), tab.v.keep, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(fault.data(), tab.v.fault, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_TRY(bhip_ctx_synchronize(ctx));
	for (int i = 0; i < n; i++) {
		memcpy(desc + (size_t)i * len, t.data() + ((size_t)i * 3 + 0) * len, (size_t)len * 4);
		memcpy(descX + (size_t)i * len, t.data() + ((size_t)i * 3 + 1) * len, (size_t)len * 4);
		memcpy(descY + (size_t)i * len, t.data() + ((size_t)i * 3 + 2) * len, (size_t)len * 4);
		G[3 * i] = g[i]; G[3 * i + 1] = g[n + i]; G[3 * i + 2] = g[2 * n + i];
		ok[i] = fault[i] == BHIP_KLT_REFERENCE_THROWS ? 2 : keep[i] ? 1 : 0;
	}
	return BHIP_OK;
}

template <class TI, class TD>
static int kltTrackStage(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const TI* image, int imgStart, int imgStride, int width, int height,
						 const float* desc, const float* descX, const float* descY, const float* G, float* xy, int n, int* fault, float* error) {
	if (!kltRangeOk(radius, 1)) return BHIP_ERR_UNSUPPORTED;   // templateRadius 1..7; nothing is written
	CHECK_CTX(ctx);
	bhip_klt_cfg c;
	if (cfg) c = *cfg; else bhip_klt_cfg_default(&c);
	if (c.maxIterations < 1) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "maxIterations must be >= 1");
	const HostImg<const TI> himg{image, imgStart, imgStride, width, height};
	CHECK_IMG(ctx, himg);
	if (n < 0 || (n > 0 && (!xy || !desc || !descX || !descY || !G || !fault || !error))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad feature list");
	if (n == 0) return BHIP_OK;
	CtxScratch* sc = scratchOf(ctx);
	DevImg<TI> dimg;
	BHIP_TRY(stageIn(ctx, sc->in0, himg, width, dimg));
	KltTable tab;
	BHIP_TRY(kltStageTable(ctx, tab, radius, xy, n));
	const int len = tab.v.len;
	std::vector<float> t((size_t)n * 3 * len), g((size_t)3 * n), pos((size_t)2 * n);
	for (int i = 0; i < n; i++) {
		memcpy(t.data() + ((size_t)i * 3 + 0) * len, desc + (size_t)i * len, (size_t)len * 4);
		memcpy(t.data() + ((size_t)i * 3 + 1) * len, descX + (size_t)i * len, (size_t)len * 4);
		memcpy(t.data() + ((size_t)i * 3 + 2) * len, descY + (size_t)i * len, (size_t)len * 4);
		g[i] = G[3 * i]; g[n + i] = G[3 * i + 1]; g[2 * n + i] = G[3 * i + 2];
	}
	BHIP_HIP(ctx, hipMemcpyAsync(tab.v.tmpl, t.data(), t.size() * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(tab.v.gxx, g.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(tab.v.gyy, g.data() + n, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(tab.v.gxy, g.data() + 2 * n, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_TRY(bhip_launch_klt_track(ctx, kltStagePyr<TI, TD>(dimg.data, nullptr, nullptr, width, height), tab.v, c, n));
	BHIP_HIP(ctx, hipMemcpyAsync(pos.data(), tab.v.lx, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(pos.data() + n, tab.v.ly, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(fault, tab.v.fault, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(error, tab.v.err, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_TRY(bhip_ctx_synchronize(ctx));
	for (int i = 0; i < n; i++) { xy[2 * i] = pos[i]; xy[2 * i + 1] = pos[n + i]; }
	return BHIP_OK;
}

extern "C" {

int bhip_klt_create(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int templateRadius, const int* scales, int numLayers, int detectRadius, float detectThreshold,
					int detectBorder, int width, int height, int batch, bhip_klt** out) {
	return kltCreate(ctx, cfg, templateRadius, scales, numLayers, detectRadius, detectThreshold, detectBorder, width, height, batch, false, out);
}
int bhip_klt_create_u8(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int templateRadius, const int* scales, int numLayers, int detectRadius, float detectThreshold,
					   int detectBorder, int width, int height, int batch, bhip_klt** out) {
	return kltCreate(ctx, cfg, templateRadius, scales, numLayers, detectRadius, detectThreshold, detectBorder, width, height, batch, true, out);
}

int bhip_klt_destroy(bhip_klt* k) { return destroyChild(k); }

int bhip_klt_process_dev_f32(bhip_klt* k, const float* dev_frames, long long imageStride, int stride) {
	return kltProcessDev<KltF32>(k, dev_frames, imageStride, stride);
}
int bhip_klt_process_dev_u8(bhip_klt* k, const uint8_t* dev_frames, long long imageStride, int stride) {
	return kltProcessDev<KltU8>(k, dev_frames, imageStride, stride);
}
int bhip_klt_process_u8(bhip_klt* k, const uint8_t* const* img, const int* startIndex, const int* stride) {
	return kltProcessHost<KltU8>(k, img, startIndex, stride);
}
int bhip_klt_process_f32(bhip_klt* k, const float* const* img, const int* startIndex, const int* stride) {
	return kltProcessHost<KltF32>(k, img, startIndex, stride);
}

int bhip_klt_spawn(bhip_klt* k, int maxFeatures) {
	CHECK_KLT(k);
	if (!k->haveFrame) return bhip_fail(ctx, BHIP_ERR_INVALID, "spawnTracks before the first process()");
	if (maxFeatures > 0) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "maxFeatures > 0 (SelectNBestFeatures) is a host call: use bhip_klt_spawn_points");
	const int w0 = k->dims[0], h0 = k->dims[1];
	const long long px = (long long)w0 * h0;
	BHIP_TRY(k->intensity.reserve(ctx, (size_t)px * 4 * k->batch));
	const DevImg<float> inten = bhip_img_over<float>(k->intensity, w0, w0, h0, k->batch);
	// FactoryIntensityPointAlg.shiTomasi(1, false, derivType): ImplSsdCorner_F32, or ImplSsdCorner_S16 on the GrayS16 derivatives of a GrayU8 tracker
	BHIP_TRY(k->withTypes([&](auto t) {
		using TD = typename decltype(t)::TD;
		return cornerImpl<TD>(ctx, false, 0, 1, 0.0f, k->layer<const TD>(1, 0), k->layer<const TD>(2, 0), inten);
	}));
	BHIP_TRY(bhip_launch_klt_mark_exclude(ctx, k->tab.v, (float)(double)k->scales[0], inten, k->ub));
	const int step = k->detectRadius + 1;
	const int rw = std::max(w0 - 2 * k->detectBorder, 0), rh = std::max(h0 - 2 * k->detectBorder, 0);
	const int cap = step > 0 ? std::max(1, ((rw + step - 1) / step) * ((rh + step - 1) / step)) : 1;   // one maximum per block at most
	BHIP_TRY(k->candXY.reserve(ctx, (size_t)cap * 4 * k->batch));
	BHIP_TRY(k->candN.reserve(ctx, (size_t)k->batch * 4));
	BHIP_TRY(nonmaxDevice(ctx, inten, k->detectRadius, k->detectThreshold, k->detectBorder, k->candXY.as<int16_t>(), cap, k->candN.as<int>()));
	return kltSpawnFrom(k, k->candXY.as<int16_t>(), cap, k->candN.as<int>());
}

int bhip_klt_spawn_points(bhip_klt* k, const int16_t* xy, const int* count, int capacity) {
	CHECK_KLT(k);
	if (!k->haveFrame) return bhip_fail(ctx, BHIP_ERR_INVALID, "spawnTracks before the first process()");
	if (!count || capacity < 0 || (capacity > 0 && !xy)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad candidate lists");
	for (int b = 0; b < k->batch; b++)
		if (count[b] < 0 || count[b] > capacity) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad candidate count");
	BHIP_TRY(k->candXY.reserve(ctx, (size_t)std::max(capacity, 1) * 4 * k->batch));
	BHIP_TRY(k->candN.reserve(ctx, (size_t)k->batch * 4));
	if (capacity > 0) BHIP_HIP(ctx, hipMemcpyAsync(k->candXY.p, xy, (size_t)capacity * 4 * k->batch, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(k->candN.p, count, (size_t)k->batch * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_TRY(kltSpawnFrom(k, k->candXY.as<int16_t>(), std::max(capacity, 1), k->candN.as<int>()));
	return bhip_ctx_synchronize(ctx);
}

int bhip_klt_add_tracks(bhip_klt* k, const int* seq, const double* xy, int n, uint8_t* ok) {
	CHECK_KLT(k);
	if (!k->haveFrame) return bhip_fail(ctx, BHIP_ERR_INVALID, "addTrack before the first process()");
	if (n < 0 || (n > 0 && (!seq || !xy || !ok))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad track list");
	if (n == 0) return BHIP_OK;
	const int* h = nullptr;
	BHIP_TRY(kltReadCounts(k, &h));
	std::vector<int> want(k->batch, 0);
	int need = 0;
	for (int i = 0; i < n; i++)
		if (seq[i] >= 0 && seq[i] < k->batch) need = std::max(need, ++want[seq[i]] - h[3 * k->batch + seq[i]]);
	if (need > 0) BHIP_TRY(kltGrow(k, (k->tab.v.cap + std::max(need, k->tab.v.cap / 2) + 255) & ~255));
	// stage: [xy 16n | seq 4n | list 4n | ok n]
	BHIP_TRY(k->stage.reserve(ctx, (size_t)n * 25 + 16));
	char* st = (char*)k->stage.p;
	double* dxy = (double*)st;
	int* dseq = (int*)(st + (size_t)n * 16);
	int* dlist = dseq + n;
	unsigned char* dok = (unsigned char*)(dlist + n);
	BHIP_HIP(ctx, hipMemcpyAsync(dxy, xy, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(dseq, seq, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_TRY(bhip_launch_klt_add(ctx, k->tab.v, dseq, dxy, n, k->W, k->H, dok, dlist));
	BHIP_TRY(kltDescribe(k, 3, dlist, n));   // tracker.setDescription(t): the result is not looked at
	BHIP_HIP(ctx, hipMemcpyAsync(ok, dok, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
	k->ub += *std::max_element(want.begin(), want.end());
	return bhip_ctx_synchronize(ctx);
}

int bhip_klt_drop_tracks(bhip_klt* k, const int* seq, const long long* featureId, int n, uint8_t* ok) {
	CHECK_KLT(k);
	if (n < 0 || (n > 0 && (!seq || !featureId))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad track list");
	if (n == 0) return BHIP_OK;
	// stage: [featureId 8n | seq 4n | ok n]
	BHIP_TRY(k->stage.reserve(ctx, (size_t)n * 13 + 16));
	char* st = (char*)k->stage.p;
	long long* did = (long long*)st;
	int* dseq = (int*)(st + (size_t)n * 8);
	unsigned char* dok = (unsigned char*)(dseq + n);
	BHIP_HIP(ctx, hipMemcpyAsync(did, featureId, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(dseq, seq, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_TRY(bhip_launch_klt_match_drop(ctx, k->tab.v, dseq, did, n, dok, k->ub));
	BHIP_TRY(bhip_launch_klt_compact(ctx, k->tab.v, 1));
	if (ok) BHIP_HIP(ctx, hipMemcpyAsync(ok, dok, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

int bhip_klt_drop_all(bhip_klt* k) {
	CHECK_KLT(k);
	k->ub = 0;
	return bhip_launch_klt_drop_all(ctx, k->tab.v, 0);
}

int bhip_klt_reset(bhip_klt* k) {
	CHECK_KLT(k);
	k->ub = 0;
	return bhip_launch_klt_drop_all(ctx, k->tab.v, 1);
}

int bhip_klt_counts(bhip_klt* k, int* active, int* spawned, int* dropped) {
	CHECK_KLT(k);
	const int* h = nullptr;
	BHIP_TRY(kltReadCounts(k, &h));
	const int B = k->batch;
	k->ub = 0;
	for (int b = 0; b < B; b++) {
		k->ub = std::max(k->ub, h[b]);
		if (active) active[b] = h[b];
		if (dropped) dropped[b] = h[B + b];
		if (spawned) spawned[b] = h[2 * B + b];
	}
	return BHIP_OK;
}

int bhip_klt_fetch(bhip_klt* k, int which, int seq, long long* featureId, float* xy, int* fault, float* error) {
	CHECK_KLT(k);
	if (which < 0 || which > 2 || seq < 0 || seq >= k->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad list selector");
	const int* h = nullptr;
	BHIP_TRY(kltReadCounts(k, &h));
	const int n = h[(which == 0 ? 0 : which == 1 ? 2 : 1) * k->batch + seq];
	if (n == 0) return BHIP_OK;
	// stage: [featureId 8n | xy 8n | fault 4n | error 4n]
	BHIP_TRY(k->stage.reserve(ctx, (size_t)n * 24));
	char* st = (char*)k->stage.p;
	long long* did = (long long*)st;
	float* dxy = (float*)(st + (size_t)n * 8);
	int* df = (int*)(st + (size_t)n * 16);
	float* de = (float*)(st + (size_t)n * 20);
	BHIP_TRY(bhip_launch_klt_gather(ctx, k->tab.v, which, seq, n, did, dxy, df, de));
	if (featureId) BHIP_HIP(ctx, hipMemcpyAsync(featureId, did, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (xy) BHIP_HIP(ctx, hipMemcpyAsync(xy, dxy, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (fault) BHIP_HIP(ctx, hipMemcpyAsync(fault, df, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	if (error) BHIP_HIP(ctx, hipMemcpyAsync(error, de, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

int bhip_klt_fetch_templates(bhip_klt* k, int which, int seq, int layer, float* tmpl, float* G) {
	CHECK_KLT(k);
	if (which < 0 || which > 2 || seq < 0 || seq >= k->batch || layer < 0 || layer >= k->L) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad list selector");
	const int* h = nullptr;
	BHIP_TRY(kltReadCounts(k, &h));
	const int n = h[(which == 0 ? 0 : which == 1 ? 2 : 1) * k->batch + seq];
	if (n == 0) return BHIP_OK;
	// stage: [templates 3 len n floats | G 3n floats]
	const size_t nt = (size_t)n * 3 * k->tab.v.len;
	BHIP_TRY(k->stage.reserve(ctx, (nt + (size_t)3 * n) * 4));
	float* dt = k->stage.as<float>();
	float* dg = dt + nt;
	BHIP_TRY(bhip_launch_klt_gather_templates(ctx, k->tab.v, which, seq, layer, n, dt, dg));
	if (tmpl) BHIP_HIP(ctx, hipMemcpyAsync(tmpl, dt, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
	if (G) BHIP_HIP(ctx, hipMemcpyAsync(G, dg, (size_t)3 * n * 4, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

int bhip_klt_stats(bhip_klt* k, long long* tracks, long long* iterations, long long* borderIterations) {
	CHECK_KLT(k);
	BHIP_TRY(k->stage.reserve(ctx, 32));
	BHIP_TRY(k->pinned.reserve(ctx, (size_t)k->batch * 32));
	BHIP_HIP(ctx, hipMemsetAsync(k->stage.p, 0, 24, ctx->stream));
	BHIP_TRY(bhip_launch_klt_stats(ctx, k->tab.v, k->stage.as<unsigned long long>()));
	BHIP_HIP(ctx, hipMemcpyAsync(k->pinned.p, k->stage.p, 24, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const long long* h = k->pinned.as<long long>();
	if (tracks) *tracks = h[0];
	if (iterations) *iterations = h[1];
	if (borderIterations) *borderIterations = h[2];
	return BHIP_OK;
}

int bhip_klt_fetch_layer(bhip_klt* k, int seq, int layer, int which, float* out) { return kltFetchLayer(k, seq, layer, which, 0, out); }
int bhip_klt_fetch_layer_u8(bhip_klt* k, int seq, int layer, uint8_t* out) { return kltFetchLayer(k, seq, layer, 0, 0, out); }
int bhip_klt_fetch_layer_s16(bhip_klt* k, int seq, int layer, int which, int16_t* out) { return kltFetchLayer(k, seq, layer, which, 1, out); }

int bhip_klt_dev_view_u8(bhip_klt* k, const int** dev_activeSlots, const int** dev_activeCount, const float** dev_x, const float** dev_y,
						 const long long** dev_featureId, const uint8_t** dev_pyramid, const int16_t** dev_derivX, const int16_t** dev_derivY, int* slotsPerSequence,
						 long long* elementsPerFrame) {
	return kltDevView<KltU8>(k, dev_activeSlots, dev_activeCount, dev_x, dev_y, dev_featureId, dev_pyramid, dev_derivX, dev_derivY, slotsPerSequence, elementsPerFrame);
}
int bhip_klt_dev_view(bhip_klt* k, const int** dev_activeSlots, const int** dev_activeCount, const float** dev_x, const float** dev_y,
					  const long long** dev_featureId, const float** dev_pyramid, const float** dev_derivX, const float** dev_derivY, int* slotsPerSequence,
					  long long* floatsPerFrame) {
	return kltDevView<KltF32>(k, dev_activeSlots, dev_activeCount, dev_x, dev_y, dev_featureId, dev_pyramid, dev_derivX, dev_derivY, slotsPerSequence, floatsPerFrame);
}

int bhip_klt_set_description_f32(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const float* image, int imgStart, int imgStride, const float* derivX,
								 const float* derivY, int dStart, int dStride, int width, int height, const float* xy, int n, float* desc, float* descX,
								 float* descY, float* G, uint8_t* ok) {
	return kltSetDescriptionStage<float, float>(ctx, cfg, radius, image, imgStart, imgStride, derivX, derivY, dStart, dStride, width, height, xy, n, desc, descX,
												descY, G, ok);
}
int bhip_klt_set_description_u8(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const uint8_t* image, int imgStart, int imgStride, const int16_t* derivX,
								const int16_t* derivY, int dStart, int dStride, int width, int height, const float* xy, int n, float* desc, float* descX,
								float* descY, float* G, uint8_t* ok) {
	return kltSetDescriptionStage<uint8_t, int16_t>(ctx, cfg, radius, image, imgStart, imgStride, derivX, derivY, dStart, dStride, width, height, xy, n, desc,
													descX, descY, G, ok);
}
int bhip_klt_track_f32(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const float* image, int imgStart, int imgStride, int width, int height,
					   const float* desc, const float* descX, const float* descY, const float* G, float* xy, int n, int* fault, float* error) {
	return kltTrackStage<float, float>(ctx, cfg, radius, image, imgStart, imgStride, width, height, desc, descX, descY, G, xy, n, fault, error);
}
int bhip_klt_track_u8(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const uint8_t* image, int imgStart, int imgStride, int width, int height,
					  const float* desc, const float* descX, const float* descY, const float* G, float* xy, int n, int* fault, float* error) {
	return kltTrackStage<uint8_t, int16_t>(ctx, cfg, radius, image, imgStart, imgStride, width, height, desc, descX, descY, G, xy, n, fault, error);
}

}  // extern "C"
