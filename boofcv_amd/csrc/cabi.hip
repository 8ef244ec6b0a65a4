// C ABI of libboofhip.so (include/boofhip.h): context, the SURF detect+describe object, association, stage-level entry points.
// Host orchestration only -- all arithmetic lives in the kernels.  There is deliberately no CPU fallback.
#include "common.h"
#include <cmath>
#include <cfloat>
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <unordered_set>

// Per-context scratch that the stateless entry points reuse (freed with the context).  The staging slots belong to the host-buffer export
// that is running: the caller's views it uploads, the results it downloads, its own working buffers.  Code on device pointers (the
// implementations behind the _dev exports, which host exports run on their staged copies) uses only the device-side slots, so nothing a
// host export calls can overwrite what it staged.
struct CtxScratch {
	DevBuf in0, in1, out0, out1, tmp0, tmp1;                                 // staging
	DevBuf work, assocCol, nmsBitmap, nmsPrefix, nmsPos, ipTmp, ipKernel, fast, disparity, distortMap, templ;   // device side
	AssocMfmaWork mfma;
	int assocExactOnly = -1;  // BHIP_ASSOC_EXACT=1 forces the exact VALU association kernels (parity cross-check)
};
static CtxScratch* scratchOf(bhip_ctx* ctx);

struct bhip_ctx_full : bhip_ctx {
	CtxScratch scratch;
};
static CtxScratch* scratchOf(bhip_ctx* ctx) { return &static_cast<bhip_ctx_full*>(ctx)->scratch; }

// Handle registry: which bhip_ctx pointers and which of their children (bhip_surf, bhip_klt, bhip_bg) are live.  The destroy calls may
// arrive in any order (a garbage-collected host language finalises objects in no particular order; a caller may close the context first)
// and more than once: destroying a context releases the device side of every child created on it and leaves those objects as inert shells
// (every call on them returns BHIP_ERR_INVALID, their destroy only frees the shell); a pointer that is not in the registry, or is a child
// of another kind, is refused instead of dereferenced.  Once the process has started to exit (atexit) the destroy calls touch neither the
// HIP runtime nor the handles -- the runtime's own teardown may already have run.  The registry is a leaked singleton so it outlives
// every static destructor.
using OrphanFn = void (*)(void* child, bhip_ctx* ctx);   // orphanIfOn<X>; its address is also what tells the kinds of children apart
struct HandleRegistry {
	std::mutex m;
	std::unordered_set<bhip_ctx*> ctxs;
	std::unordered_map<void*, OrphanFn> children;
	std::atomic<bool> exiting{false};
};
static HandleRegistry& registry() {
	static HandleRegistry* r = [] {
		HandleRegistry* p = new HandleRegistry();
		atexit([] { registry().exiting = true; });   // registered after the HIP runtime loaded, so it runs before the runtime's teardown
		return p;
	}();
	return *r;
}

// What the three kinds of children share: Dev is everything the object holds on its context's device, dropped as a whole by destruction
// or by releaseDevice; ctx == nullptr marks the inert shell.
template <class Dev>
struct CtxChild : Dev {
	using Device = Dev;
	bhip_ctx* ctx = nullptr;
	void onRelease() {}   // a type's own part of releaseDevice; the context's stream has been synchronized, the device side is still there
};
// Frees everything x holds on the device (its context must still be alive) and detaches it from the context.  Registry lock held.
template <class X>
static void releaseDevice(X* x) {
	if (!x->ctx) return;   // the context went first
	(void)hipSetDevice(x->ctx->device);
	(void)hipStreamSynchronize(x->ctx->stream);
	x->onRelease();
	static_cast<typename X::Device&>(*x) = typename X::Device();
	x->ctx = nullptr;
}
template <class X>
static void orphanIfOn(void* child, bhip_ctx* ctx) {
	if (static_cast<X*>(child)->ctx == ctx) releaseDevice(static_cast<X*>(child));
}
// The create call of a child: holds the registry lock from the context's liveness check to the insert, so a concurrent bhip_ctx_destroy
// waits for it.  build(std::unique_ptr<X>&) does the type's own argument checks (a null `out` among them) and the construction.
template <class X, class Build>
static int createChild(bhip_ctx* ctx, X** out, Build build) {
	HandleRegistry& R = registry();
	std::lock_guard<std::mutex> lock(R.m);
	if (!ctx || !R.ctxs.count(ctx)) return BHIP_ERR_INVALID;
	std::unique_ptr<X> x;
	BHIP_TRY(build(x));
	R.children.emplace(x.get(), &orphanIfOn<X>);
	*out = x.release();
	return BHIP_OK;
}
template <class X>
static int destroyChild(X* x) {
	if (!x) return BHIP_OK;
	HandleRegistry& R = registry();
	std::lock_guard<std::mutex> lock(R.m);
	if (R.exiting) return BHIP_OK;                                                       // process teardown: the runtime reclaims everything
	auto it = R.children.find(x);
	if (it == R.children.end() || it->second != &orphanIfOn<X>) return BHIP_ERR_INVALID;   // not a live object of this kind (destroyed twice, never created, another kind)
	R.children.erase(it);
	releaseDevice(x);
	delete x;
	return BHIP_OK;
}

extern "C" {

const char* bhip_version(void) { return "boofhip 0.1 (gfx950)"; }

void bhip_fh_cfg_default(bhip_fh_cfg* c) {
	c->detectThreshold = 1; c->extractRadius = 2; c->maxFeaturesPerScale = -1; c->initialSampleSize = 1; c->initialSize = 9;
	c->numberScalesPerOctave = 4; c->numberOfOctaves = 4; c->scaleStepSize = 6;
}
void bhip_klt_cfg_default(bhip_klt_cfg* c) {
	c->forbiddenBorder = 0; c->maxPerPixelError = 25; c->maxIterations = 15; c->minDeterminant = 0.001f; c->minPositionDelta = 0.01f;
}
void bhip_bg_basic_cfg_default(bhip_bg_basic_cfg* c) { c->learnRate = 0.05f; c->threshold = 0; c->unknownValue = 0; }
void bhip_bg_gaussian_cfg_default(bhip_bg_gaussian_cfg* c) {
	c->learnRate = 0.05f; c->threshold = 0; c->initialVariance = FLT_TRUE_MIN; c->minimumDifference = 0; c->unknownValue = 0;
}
void bhip_bg_gmm_cfg_default(bhip_bg_gmm_cfg* c) {
	c->learningPeriod = 1000.0f; c->initialVariance = 400; c->decayCoefient = 0.005f; c->maxDistance = 3; c->numberOfGaussian = 5; c->significantWeight = 0.01f;
	c->unknownValue = 0;
}
void bhip_disparity_bm_cfg_default(bhip_disparity_bm_cfg* c) {
	c->minDisparity = 0; c->rangeDisparity = 100; c->regionRadiusX = 3; c->regionRadiusY = 3; c->maxPerPixelError = 0; c->validateRtoL = 1; c->texture = 0.15;
}
void bhip_surf_cfg_default(bhip_surf_cfg* c) {
	c->widthLargeGrid = 4; c->widthSubRegion = 5; c->widthSample = 3; c->weightSigma = 4.5; c->overLap = 2; c->sigmaLargeGrid = 2.5;
	c->sigmaSubRegion = 2.5;
}
void bhip_ori_cfg_default(bhip_ori_cfg* c, int stable) {
	c->objectRadiusToScale = 1.0 / 2.0;
	c->weightSigma = -1;
	c->sampleWidth = 6;
	if (stable) { c->samplePeriod = 0.65; c->windowSize = M_PI / 3.0; c->radius = 8; }
	else { c->samplePeriod = 1; c->windowSize = 0; c->radius = 6; }
}

static int ctxCreate(int device, void* stream, bool useGiven, bhip_ctx** out) {
	if (!out) return BHIP_ERR_INVALID;
	*out = nullptr;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return BHIP_ERR_HIP;  // no GPU: fail loudly, never fall back
	if (device < 0 || device >= count) return BHIP_ERR_INVALID;
	if (hipSetDevice(device) != hipSuccess) return BHIP_ERR_HIP;
	std::unique_ptr<bhip_ctx_full> ctx(new (std::nothrow) bhip_ctx_full());
	if (!ctx) return BHIP_ERR_NOMEM;
	ctx->device = device;
	if (useGiven) {
		ctx->stream = (hipStream_t)stream;
	} else {
		if (hipStreamCreateWithFlags(&ctx->ownedStream.h, hipStreamNonBlocking) != hipSuccess) return BHIP_ERR_HIP;
		ctx->stream = ctx->ownedStream;
	}
	if (ctx->hostScratch.reserve(ctx.get(), 1 << 20) != BHIP_OK) return BHIP_ERR_HIP;
	HandleRegistry& R = registry();
	std::lock_guard<std::mutex> lock(R.m);
	R.ctxs.insert(ctx.get());
	*out = ctx.release();
	return BHIP_OK;
}
int bhip_ctx_create(int device, bhip_ctx** out) { return ctxCreate(device, nullptr, false, out); }
int bhip_ctx_create_on_stream(int device, void* hip_stream, bhip_ctx** out) { return ctxCreate(device, hip_stream, true, out); }
int bhip_ctx_destroy(bhip_ctx* c) {
	if (!c) return BHIP_OK;
	HandleRegistry& R = registry();
	std::lock_guard<std::mutex> lock(R.m);
	if (R.exiting) return BHIP_OK;                        // process teardown: the runtime reclaims everything
	if (!R.ctxs.count(c)) return BHIP_ERR_INVALID;        // not a live context (destroyed twice, or never created)
	R.ctxs.erase(c);
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	for (auto& child : R.children) child.second(child.first, c);   // children still alive on this context become inert shells now
	delete static_cast<bhip_ctx_full*>(c);   // scratch, profiling events, staging block, then the stream it owns
	return BHIP_OK;
}
int bhip_ctx_synchronize(bhip_ctx* ctx) {
	if (!ctx) return BHIP_ERR_INVALID;
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}
const char* bhip_last_error(bhip_ctx* ctx) { return ctx ? ctx->error.c_str() : "null context"; }
// Page-locked host memory for the arrays that cross the boundary (results of bhip_surf_fetch, descriptor lists handed to
// bhip_assoc_l2_f64, frames): copies to and from such memory are DMA transfers at PCIe speed, copies from pageable memory go through
// the runtime's staging buffer (1.1 MB of descriptors: ~0.15 ms instead of ~0.03 ms).  The block belongs to the process, not to the
// context: it stays valid after bhip_ctx_destroy and is released by bhip_host_free (after exit has begun: by the runtime).
int bhip_host_alloc(bhip_ctx* ctx, long long bytes, uint8_t** host_mem) {
	if (!ctx || !host_mem) return BHIP_ERR_INVALID;
	*host_mem = nullptr;
	if (bytes <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bhip_host_alloc: size must be positive");
	BHIP_HIP(ctx, hipSetDevice(ctx->device));
	void* p = nullptr;
	const hipError_t e = hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault);
	if (e != hipSuccess) { (void)hipGetLastError(); return bhip_fail(ctx, BHIP_ERR_NOMEM, "bhip_host_alloc: out of page-locked memory"); }
	*host_mem = (uint8_t*)p;
	return BHIP_OK;
}
int bhip_host_free(void* host_mem) {
	if (!host_mem) return BHIP_OK;
	if (registry().exiting) return BHIP_OK;   // process teardown: the runtime reclaims it
	return hipHostFree(host_mem) == hipSuccess ? BHIP_OK : BHIP_ERR_HIP;
}

}  // extern "C"

#define CHECK_CTX(ctx)                                   \
	do {                                                 \
		if (!(ctx)) return BHIP_ERR_INVALID;             \
		BHIP_HIP((ctx), hipSetDevice((ctx)->device));    \
	} while (0)

// a caller's host image: width x height elements, rows `stride` elements apart, the first at data[start]
template <class T>
struct HostImg {
	T* data;
	int start, stride, width, height;
	static constexpr int batch = 1;
};

// v: a HostImg or a DevImg
#define CHECK_IMG(ctx, v)                                                                                         \
	do {                                                                                                          \
		if (!(v).data || (v).width <= 0 || (v).height <= 0 || (v).batch <= 0 || (v).stride < (v).width)          \
			return bhip_fail((ctx), BHIP_ERR_INVALID, "bad image");                                               \
	} while (0)

// Host view (rows `stride` elements apart from `start`) to / from a device image with rows `pitch` elements apart, enqueued on `st`.  Two
// dense sides are one linear copy (the 2-D form is several times slower over PCIe even when the pitches match).  Neither synchronizes: an
// export synchronizes once, before it returns.
template <class T>
static int upload(bhip_ctx* ctx, T* dev, int pitch, const T* in, int start, int stride, int w, int h, hipStream_t st) {
	if (pitch == w && stride == w) BHIP_HIP(ctx, hipMemcpyAsync(dev, in + start, sizeof(T) * w * h, hipMemcpyHostToDevice, st));
	else BHIP_HIP(ctx, hipMemcpy2DAsync(dev, sizeof(T) * pitch, in + start, sizeof(T) * stride, sizeof(T) * w, h, hipMemcpyHostToDevice, st));
	return BHIP_OK;
}
template <class T>
static int download(bhip_ctx* ctx, T* out, int start, int stride, const T* dev, int pitch, int w, int h, hipStream_t st) {
	if (pitch == w && stride == w) BHIP_HIP(ctx, hipMemcpyAsync(out + start, dev, sizeof(T) * w * h, hipMemcpyDeviceToHost, st));
	else BHIP_HIP(ctx, hipMemcpy2DAsync(out + start, sizeof(T) * stride, dev, sizeof(T) * pitch, sizeof(T) * w, h, hipMemcpyDeviceToHost, st));
	return BHIP_OK;
}

// Staging of a host-buffer export (see CtxScratch): stageIn reserves `slot` for one image shaped like `h` with rows `pitch` elements apart,
// uploads h into it unless `copy` is false (an output the implementation writes as a whole) and hands back the device view; stageOut
// enqueues the download.  The export synchronizes once after its last stageOut.
template <class T>
static int stageIn(bhip_ctx* ctx, DevBuf& slot, HostImg<T> h, int pitch, DevImg<std::remove_const_t<T>>& dev, bool copy = true) {
	using E = std::remove_const_t<T>;
	BHIP_TRY(slot.reserve(ctx, (size_t)pitch * h.height * sizeof(E)));
	dev = bhip_img_over<E>(slot, pitch, h.width, h.height, 1);
	return copy ? upload<E>(ctx, dev.data, pitch, h.data, h.start, h.stride, h.width, h.height, ctx->stream) : BHIP_OK;
}
template <class T>
static int stageOut(bhip_ctx* ctx, HostImg<T> h, DevImg<T> dev) {
	return download<T>(ctx, h.data, h.start, h.stride, dev.data, dev.stride, h.width, h.height, ctx->stream);
}
// pitch4(w): device rows 16-byte aligned so that the tiled ip kernels apply
static inline int pitch4(int w) { return (w + 3) & ~3; }

// The usual host export: one input view, one output view.  After the context and image checks and the export's own argument check
// (argError: its message, nullptr when it passed) `in` is staged into in0 and `out` into out0 -- rows pitch4(width) apart when `pitched`,
// dense otherwise; `out` is uploaded too when `keepOut`, i.e. when the operation leaves some pixels as the caller had them -- then
// run(din, dout), the download and the synchronize.  When run fails, nothing is downloaded.
template <class TI, class TO, class Run>
static int hostInOut(bhip_ctx* ctx, HostImg<const TI> in, HostImg<TO> out, bool pitched, bool keepOut, const char* argError, Run run) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	if (argError) return bhip_fail(ctx, BHIP_ERR_INVALID, argError);
	CtxScratch* sc = scratchOf(ctx);
	DevImg<TI> din;
	DevImg<TO> dout;
	BHIP_TRY(stageIn(ctx, sc->in0, in, pitched ? pitch4(in.width) : in.width, din));
	BHIP_TRY(stageIn(ctx, sc->out0, out, pitched ? pitch4(out.width) : out.width, dout, keepOut));
	BHIP_TRY(run(din, dout));
	BHIP_TRY(stageOut(ctx, out, dout));
	return bhip_ctx_synchronize(ctx);
}

// ---------------------------------------------------------------------------------------------------------------
// Fast-Hessian detector: octave schedule + buffers (FastHessianFeatureDetector.detect :156-188, detectOctave :198-221)
// ---------------------------------------------------------------------------------------------------------------
struct FhLevelPlan {
	DetectLevelParams p;
	int level;  // index of the mid level inside its octave
};
struct FhOctavePlan {
	int skip, w, h, nlevels;
	int sizes[BHIP_MAX_LEVELS];
	std::vector<FhLevelPlan> mids;
	// execution plan (FhDetector::planExecution)
	bool fused = false, fixed = false;
	int shareFrom[BHIP_MAX_LEVELS];   // level of the previous octave with the same kernel size, or -1
	bool onDemand[BHIP_MAX_LEVELS];   // stand-alone octave: outer level left to k_nms_scalespace (evaluated around the NMS maxima only)
	int exportSlot[BHIP_MAX_LEVELS];  // fused producer: slot of this level in the export buffer, or -1
	int nexport = 0;
	size_t intenOff = 0, expOff = 0;  // floats, per-image strides below
	long long intenImageStride = 0, expImageStride = 0;
};

struct FhDetector {
	bhip_fh_cfg cfg;
	int W = 0, H = 0, batch = 0, cap = 0;
	bool plannedInt = false;   // the plan is for GrayS32 integral images (from GrayU8 frames; integer taps) instead of GrayF32 ones
	std::vector<FhOctavePlan> plan;
	int bitmapWords = 0;
	DevBuf inten, bitmap, prefix, cand, sorted, count, selKey, selIdx, selLevels;
	bool nBest() const { return cfg.maxFeaturesPerScale > 0; }   // SelectNBestFeatures between the NMS and the scale-space test
	std::vector<int> counts;   // per image, host
	long long total = 0;

	static bool unfusedOnly() { return bhip_env_flag("BHIP_DETECT_UNFUSED"); }   // parity cross-check of the two detector paths
	int makePlan(bhip_ctx* ctx, int width, int height) {
		plan.clear();
		if (cfg.numberScalesPerOctave > BHIP_MAX_LEVELS || cfg.numberScalesPerOctave < 1) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "numberScalesPerOctave out of range");
		if (cfg.extractRadius < 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "Search radius must be >= 1");
		if (cfg.initialSampleSize < 1 || cfg.initialSize < 3) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sample size / initial size");
		if (width >= 32768 || height >= 32768) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "image too large for Point2D_I16");
		int skip = cfg.initialSampleSize, sizeStep = cfg.scaleStepSize, octaveSize = cfg.initialSize;
		unsigned int bits = 0;
		const int step = cfg.extractRadius + 1;
		for (int octave = 0; octave < cfg.numberOfOctaves; octave++) {
			FhOctavePlan o;
			o.nlevels = cfg.numberScalesPerOctave;
			for (int i = 0; i < o.nlevels; i++) o.sizes[i] = octaveSize + i * sizeStep;
			const int maxSize = o.sizes[o.nlevels - 1];
			if (maxSize > width || maxSize > height) break;
			o.skip = skip;
			o.w = width / skip;
			o.h = height / skip;
			for (int i = 2; i < o.nlevels; i++) {
				FhLevelPlan m;
				m.level = i - 1;
				DetectLevelParams& p = m.p;
				p.skip = skip; p.w = o.w; p.h = o.h;
				p.sizeLower = o.sizes[m.level - 1]; p.sizeMid = o.sizes[m.level]; p.sizeUpper = o.sizes[m.level + 1];
				p.border = p.sizeMid / (2 * skip);
				const int rw = p.w - 2 * p.border, rh = p.h - 2 * p.border;
				p.nbx = rw > 0 ? (rw + step - 1) / step : 0;
				p.nby = rh > 0 ? (rh + step - 1) / step : 0;
				p.bitBase = bits;
				bits += (unsigned)p.nbx * (unsigned)p.nby;
				o.mids.push_back(m);
			}
			plan.push_back(o);
			skip += skip;
			octaveSize += sizeStep;
			sizeStep += sizeStep;
		}
		bitmapWords = (int)((bits + 31) / 32) + 1;
		return BHIP_OK;
	}

	static bool noShare() { return bhip_env_flag("BHIP_DETECT_NOSHARE"); }   // parity cross-check of the shared-level plan
	static bool denseOuter() { return bhip_env_flag("BHIP_DETECT_DENSE"); }  // parity cross-check: compute the outer levels of every octave densely
	// Which octaves run fused, and which levels are copied from the octave below instead of being recomputed.  A box-filter response
	// depends on (pixel, kernel size) only, and the default schedule repeats sizes: 15,27 | 27,51 | 51,99 are levels 1,3 of one octave and
	// levels 0,1 of the next, on a lattice twice as coarse.  Sharing is enabled where the unrolled inner form and the clamped border
	// form of the reference cover the same boxes (size = 3*blockSmall, odd), between a producer that keeps or exports its intensity and a
	// stand-alone consumer.  The two forms still round Dyy differently, and which pixels are "inner" depends on the step, so the
	// consumer (k_hessian) copies a pixel only when both octaves evaluate it with the same form and computes the rest itself.
	void planExecution() {
		for (auto& o : plan) {
			int ftx, fty, flds;
			// N-best selection needs every level's NMS list and intensity images in memory: stand-alone kernels
			o.fused = !unfusedOnly() && !nBest() && !o.mids.empty() && bhip_fused_plan(o.skip, o.nlevels, o.sizes, cfg.extractRadius, &ftx, &fty, &flds);
			o.fixed = o.fused && bhip_fused_is_fixed(o.skip, o.nlevels, o.sizes, cfg.extractRadius);
			if (plannedInt && !o.fixed) o.fused = false;   // integer taps: compile-time-geometry fused kernel or the stand-alone kernels
			o.nexport = 0;
			for (int i = 0; i < BHIP_MAX_LEVELS; i++) { o.shareFrom[i] = -1; o.exportSlot[i] = -1; o.onDemand[i] = false; }
		}
		// The first and last level of an octave are only read around the NMS maxima of their neighbour level: a stand-alone octave leaves
		// them to k_nms_scalespace unless they can be copied from the octave below.  (N-best selection reads whole levels: dense.)
		const bool sparseOuter = !denseOuter() && !nBest();
		for (size_t k = 0; k < plan.size(); k++) {
			FhOctavePlan& c = plan[k];
			if (k > 0 && !noShare()) shareLevels(c, plan[k - 1]);
			if (!c.fused && sparseOuter && c.nlevels >= 3)
				for (int i : {0, c.nlevels - 1})
					if (c.shareFrom[i] < 0) c.onDemand[i] = true;
		}
	}
	void shareLevels(FhOctavePlan& c, FhOctavePlan& p) {
		{
			if (c.fused || c.skip != 2 * p.skip) return;
			if (p.fused && !p.fixed) return;
			for (int i = 0; i < c.nlevels; i++) {
				const int size = c.sizes[i];
				if (size % 3 != 0 || size % 2 != 1) continue;
				for (int j = 0; j < p.nlevels; j++) {
					if (p.sizes[j] != size) continue;
					if (!p.fused && p.onDemand[j]) break;   // the producer does not hold this level
					if (p.fused) {
						if (p.exportSlot[j] < 0) {
							if (p.nexport >= 2) break;
							p.exportSlot[j] = p.nexport++;
						}
					}
					c.shareFrom[i] = j;
					break;
				}
			}
		}
	}

	// T: element type of the integral images that run() will be given (float or int32_t)
	template <class T>
	int prepare(bhip_ctx* ctx, int width, int height, int batch_) {
		constexpr bool isInt = std::is_same<T, int32_t>::value;
		if (width != W || height != H || plannedInt != isInt) { BHIP_TRY(makePlan(ctx, width, height)); plannedInt = isInt; planExecution(); }
		W = width; H = height; batch = batch_;
		if (cap == 0) cap = 8192;
		return allocate(ctx);
	}
	int allocate(bhip_ctx* ctx) {
		size_t intenFloats = 0;
		for (size_t k = 0; k < plan.size(); k++) {
			FhOctavePlan& o = plan[k];
			if (!o.fused) {
				o.intenImageStride = (long long)o.nlevels * o.w * o.h;
				o.intenOff = intenFloats;
				intenFloats += (size_t)o.intenImageStride * batch;
			}
		}
		BHIP_TRY(inten.reserve(ctx, intenFloats * 4 + 16));
		BHIP_TRY(bitmap.reserve(ctx, (size_t)bitmapWords * 4 * batch));
		BHIP_TRY(prefix.reserve(ctx, (size_t)bitmapWords * 4 * batch));
		BHIP_TRY(cand.reserve(ctx, (size_t)cap * sizeof(KeyPoint) * batch));
		BHIP_TRY(sorted.reserve(ctx, (size_t)cap * sizeof(KeyPoint) * batch));
		BHIP_TRY(count.reserve(ctx, (size_t)batch * 4 * 2));
		if (nBest()) {
			size_t nlv = 0;
			for (auto& o : plan) nlv += o.mids.size();
			BHIP_TRY(selKey.reserve(ctx, (size_t)cap * 4 * batch));
			BHIP_TRY(selIdx.reserve(ctx, (size_t)cap * 4 * batch));
			BHIP_TRY(selLevels.reserve(ctx, std::max<size_t>(nlv, 1) * 4 * 2 * batch));
		}
		return BHIP_OK;
	}

	// level l of the intensity planes of stand-alone octave o
	DevImg<float> level(const FhOctavePlan& o, int l) const { return {inten.as<float>() + o.intenOff + (size_t)l * o.w * o.h, o.intenImageStride, o.w, o.w, o.h, batch}; }
	// ii: the dense integral images prepare<T>() planned for.  Leaves the ordered key points in `sorted` ([image][cap]) and their counts in `counts`.
	template <class T>
	int run(bhip_ctx* ctx, DevImg<const T> ii) {
		for (int attempt = 0; attempt < 8; attempt++) {
			BHIP_HIP(ctx, hipMemsetAsync(bitmap.p, 0, (size_t)bitmapWords * 4 * batch, ctx->stream));
			BHIP_HIP(ctx, hipMemsetAsync(count.p, 0, (size_t)batch * 4 * 2, ctx->stream));
			for (size_t k = 0; k < plan.size(); k++) {
				FhOctavePlan& o = plan[k];
				if (o.fused) {
					// LDS-tiled fused octave: intensity never leaves the CU (except the levels the next octave shares)
					DetectLevelParams mp[BHIP_MAX_LEVELS];
					int ml[BHIP_MAX_LEVELS];
					for (size_t q = 0; q < o.mids.size(); q++) { mp[q] = o.mids[q].p; ml[q] = o.mids[q].level; }
					FusedExport ex{0, {0, 0}, nullptr, 0, 0, 0, {0, 0}};
					if (o.nexport > 0 && k + 1 < plan.size()) {
						// the shared levels go straight into the consuming octave's level planes: its k_hessian then only recomputes the
						// pixels the two octaves evaluate with different forms
						const FhOctavePlan& c = plan[k + 1];
						ex.n = o.nexport;
						for (int j = 0; j < o.nlevels; j++) if (o.exportSlot[j] >= 0) ex.level[o.exportSlot[j]] = j;
						ex.out = level(c, 0).data; ex.w = c.w; ex.h = c.h; ex.imageStride = c.intenImageStride;
						for (int i = 0; i < c.nlevels; i++) {
							const int j = c.shareFrom[i];
							if (j >= 0 && o.exportSlot[j] >= 0) ex.slotOffset[o.exportSlot[j]] = (long long)i * c.w * c.h;
						}
					}
					BHIP_TRY(bhip_launch_detect_fused(ctx, ii, o.skip, o.nlevels, o.sizes, (int)o.mids.size(), mp, ml, cfg.extractRadius,
													  cfg.detectThreshold, bitmap.as<unsigned int>(), bitmapWords, cand.as<KeyPoint>(), count.as<int>(), cap,
													  ex.n > 0 ? &ex : nullptr));
					continue;
				}
				HessLevelSource from[BHIP_MAX_LEVELS];
				for (int i = 0; i < o.nlevels; i++) {
					from[i] = HessLevelSource{nullptr, 0, 0, 1, 0};
					const int j = o.shareFrom[i];
					if (j < 0 || k == 0) continue;
					const FhOctavePlan& p = plan[k - 1];
					if (p.fused) from[i] = HessLevelSource{level(o, i).data, o.intenImageStride, o.w, 1, 1};   // written in place by the fused octave
					else from[i] = HessLevelSource{level(p, j).data, p.intenImageStride, p.w, 2, 0};
				}
				unsigned int skipMask = 0;
				for (int i = 0; i < o.nlevels; i++)
					if (o.onDemand[i]) skipMask |= 1u << i;
				BHIP_TRY(bhip_launch_hessian(ctx, ii, o.skip, o.nlevels, o.sizes, level(o, 0), (long long)o.w * o.h, from, skipMask));
				auto held = [&](int l) { DevImg<const float> v = level(o, l); if (o.onDemand[l]) v.data = nullptr; return v; };   // nullptr: not in memory
				for (auto& m : o.mids)
					BHIP_TRY(bhip_launch_nms_scalespace(ctx, held(m.level - 1), level(o, m.level), held(m.level + 1), m.p, cfg.extractRadius, cfg.detectThreshold,
														bitmap.as<unsigned int>(), bitmapWords, cand.as<KeyPoint>(), count.as<int>(), cap, nBest(), ii));
			}
			BHIP_TRY(bhip_launch_word_prefix(ctx, bitmap.as<unsigned int>(), bitmapWords, batch, prefix.as<unsigned int>(), count.as<int>() + batch));
			counts.resize(batch);
			if ((size_t)batch * 4 <= (1u << 20)) {
				BHIP_HIP(ctx, hipMemcpyAsync(ctx->hostScratch.p, count.p, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
				BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
				memcpy(counts.data(), ctx->hostScratch.p, (size_t)batch * 4);
			} else {
				BHIP_HIP(ctx, hipMemcpyAsync(counts.data(), count.p, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
				BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
			}
			int maxCount = 0;
			total = 0;
			for (int c : counts) { maxCount = std::max(maxCount, c); total += c; }
			if (maxCount <= cap) {
				BHIP_TRY(bhip_launch_rank_scatter(ctx, bitmap.as<unsigned int>(), bitmapWords, prefix.as<unsigned int>(), cand.as<KeyPoint>(), count.as<int>(),
												  cap, batch, sorted.as<KeyPoint>()));
				if (nBest()) BHIP_TRY(selectNBest(ctx));
				return BHIP_OK;
			}
			// candidate list overflowed: grow and run the detector again
			cap = maxCount + maxCount / 4 + 64;
			BHIP_TRY(allocate(ctx));
		}
		return bhip_fail(ctx, BHIP_ERR_CAPACITY, "key point list kept overflowing");
	}
	// maxFeaturesPerScale > 0: `sorted` holds every level's NMS maxima (ranked, with intensities).  Per level: select, scale-space test,
	// sub-pixel fit (k_select_nbest, results into `cand`), then the levels are packed back into `sorted` and the counts re-read.
	int selectNBest(bhip_ctx* ctx) {
		int nlv = 0;
		for (auto& o : plan) nlv += (int)o.mids.size();
		int* levelStart = selLevels.as<int>();
		int* levelCount = levelStart + (size_t)std::max(nlv, 1) * batch;
		int li = 0;
		for (auto& o : plan)
			for (auto& m : o.mids) {
				BHIP_TRY(bhip_launch_select_nbest(ctx, level(o, m.level - 1), level(o, m.level), level(o, m.level + 1), m.p, cfg.extractRadius,
												  cfg.maxFeaturesPerScale, bitmap.as<unsigned int>(), prefix.as<unsigned int>(), bitmapWords, sorted.as<KeyPoint>(),
												  cap, selKey.as<float>(), selIdx.as<int>(), cand.as<KeyPoint>(), levelStart, levelCount, li, nlv));
				li++;
			}
		BHIP_TRY(bhip_launch_compact_levels(ctx, cand.as<KeyPoint>(), cap, levelStart, levelCount, nlv, batch, sorted.as<KeyPoint>(), count.as<int>()));
		BHIP_HIP(ctx, hipMemcpyAsync(counts.data(), count.p, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
		total = 0;
		for (int c : counts) total += c;
		return BHIP_OK;
	}
};

// ---------------------------------------------------------------------------------------------------------------
// SURF detect + describe object
// ---------------------------------------------------------------------------------------------------------------
// Everything a detect+describe object holds on its context's device (CtxChild); its owner synchronizes the copy stream too before dropping it.
struct SurfDevice {
	FhDetector det;
	DevBuf tabBuf, inBuf, iiBuf, startBuf, angBuf, descBuf, whiteBuf, xysBuf, tmpKp, tmpAng, tmpDesc, tmpWhite, permBuf;
	DevBuf briefTab, wordsBuf;   // BRIEF: [samplePoints | compare] on the device; words of the whole batch, compact [total][briefWords]
	PinnedBuf startsPinned;      // page-locked staging copy of `starts` for its upload
	// host-frame batches are processed in chunks so that the upload of chunk k+1 (copy stream) runs under the kernels of chunk k: the
	// chunks go through `worker` (same configuration, chunk-sized work buffers), whose results are appended to this object's arrays
	std::unique_ptr<bhip_surf> worker;
	HipStream copyStream;
	const int* briefBorrow = nullptr;   // chunk worker: the owner's BRIEF table (not owned: never freed twice)
};

struct bhip_surf : CtxChild<SurfDevice> {
	void onRelease() {   // the chunk worker is owned by this object and is not in the registry: it goes with the SurfDevice
		if (copyStream) (void)hipStreamSynchronize(copyStream);
		haveResult = false;
	}
	int stable = 1;
	bhip_surf_cfg sd;
	bhip_ori_cfg ori;
	SurfTables tables;
	std::vector<int> starts;  // batch+1
	int W = 0, H = 0, batch = 0;
	bool haveResult = false;
	bool iiInt = false;        // the integral images of the last detect (iiBuf, [batch][H][W]; see withIntegral) are GrayS32, from GrayU8 frames, not GrayF32
	int planarBands = 0;       // > 0: the last detect was colour SURF on that many bands (descriptor = planarBands * dof values)
	int dofOut() const { return tables.dof * (planarBands > 0 ? planarBands : 1); }
	// colour SURF: the bands' integral images follow the grey one in iiBuf
	DescPlanar planar() const {
		const long long px = (long long)W * H;
		return planarBands > 0 ? DescPlanar{iiBuf.as<float>() + px, px * (1 + planarBands), px, planarBands} : DescPlanar{};
	}
	const DevBuf* iiOwner = nullptr; int iiFirst = 0;   // worker only: the current chunk's integral images go into the owner's iiBuf, from image iiFirst on
	// describe = BRIEF (DetectDescribeFusion(fastHessian, null, brief), bhip_surf_create_brief): no orientation / SURF stage; every detected
	// point gets its TupleDesc_B words from the input frame itself
	bool brief = false;
	int briefRadius = 0, briefPoints = 0, briefWords = 0;
	bool briefPatch = false;            // the definition fits the LDS-patch kernel
	const int* briefSample() const { return briefBorrow ? briefBorrow : briefTab.as<int>(); }
	const int* briefCompare() const { return briefSample() + briefCompareOff; }
	size_t briefCompareOff = 0;
};

// The one place where the stored integral images' element type becomes a static type again: f(DevImg<const float>) or f(DevImg<const int32_t>)
template <class F>
static int withIntegral(const bhip_surf* s, F f) {
	return s->iiInt ? f(bhip_img_over<const int32_t>(s->iiBuf, s->W, s->W, s->H, s->batch)) : f(bhip_img_over<const float>(s->iiBuf, s->W, s->W, s->H, s->batch));
}
// frame type -> integral image type (GIntegralImageOps.getIntegralType): GrayF32 -> GrayF32, GrayU8 -> GrayS32 (every stage then runs on integer taps)
template <class T> struct SurfTraits;
template <> struct SurfTraits<float> { using II = float; };
template <> struct SurfTraits<uint8_t> { using II = int32_t; };
constexpr int GREY = 0;   // surfRun's `bands` for single-band frames (otherwise the band count of one colour frame)
// SYNCHRONIZED: host-frame callers get their frames (and the upload buffer) back only after a final synchronize.  QUEUED: the caller's device-
// resident batch (bhip_surf_detect_dev_f32) -- the call may return with the describe kernels still queued on the context's stream (its contract)
enum class SurfReturn { SYNCHRONIZED, QUEUED };

static int buildTables(bhip_surf* s) {
	bhip_ctx* ctx = s->ctx;
	SurfTables& t = s->tables;
	memset(&t, 0, sizeof(t));
	const bhip_surf_cfg& c = s->sd;
	const bhip_ori_cfg& o = s->ori;
	if (c.widthLargeGrid < 1 || c.widthSubRegion < 1 || c.widthSample < 1 || c.overLap < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad SURF config");
	if (o.radius < 1 || o.radius > 10) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "orientation radius out of range (1..10 on the GPU)");
	std::vector<double> all;
	auto push = [&](const std::vector<double>& v) { size_t off = all.size(); all.insert(all.end(), v.begin(), v.end()); return off; };
	t.oriStable = s->stable;
	t.oriRadius = o.radius;
	t.oriWidth = 2 * o.radius + 1;
	t.oriKernelWidth = o.sampleWidth;
	t.oriHasWeights = o.weightSigma != 0 ? 1 : 0;
	t.oriPeriod = o.samplePeriod;
	t.oriWindow = o.windowSize;
	t.oriRadiusToScale = o.objectRadiusToScale;
	size_t offOri = 0, offSub = 0, offGrid = 0, offFast = 0;
	// OrientationIntegralBase :85-86 weights = FactoryKernelGaussian.gaussian(2,true,64,weightSigma,sampleRadius)
	if (t.oriHasWeights) offOri = push(bhip_gaussian2d_f64(o.weightSigma, o.radius));
	t.stable = s->stable;
	t.widthLargeGrid = c.widthLargeGrid; t.widthSubRegion = c.widthSubRegion; t.widthSample = c.widthSample; t.overLap = c.overLap;
	t.dof = c.widthLargeGrid * c.widthLargeGrid * 4;
	const int regionSize = c.widthLargeGrid * c.widthSubRegion;
	if (s->stable) {
		// DescribePointSurfMod :76-106
		std::vector<double> wg = bhip_gaussian_width(c.sigmaLargeGrid, c.widthLargeGrid);
		std::vector<double> ws = bhip_gaussian_width(c.sigmaSubRegion, c.widthSubRegion + 2 * c.overLap);
		const int gw = c.widthLargeGrid, sw = c.widthSubRegion + 2 * c.overLap;
		double div = wg[(size_t)(gw / 2) * gw + gw / 2];
		for (double& v : wg) v /= div;
		div = ws[(size_t)(sw / 2) * sw + sw / 2];
		for (double& v : ws) v /= div;
		offGrid = push(wg);
		offSub = push(ws);
		t.radiusDescriptor = regionSize / 2 + c.overLap;
	} else {
		// DescribePointSurf :110-141
		const int radius = regionSize / 2;
		std::vector<double> w = bhip_gaussian_width(c.weightSigma, radius * 2);
		if ((int)w.size() != regionSize * regionSize) return bhip_fail(ctx, BHIP_ERR_INVALID, "Weighting kernel has an unexpected size");
		const double div = w[(size_t)radius * (radius * 2) + radius];
		for (double& v : w) v /= div;
		offFast = push(w);
		t.radiusDescriptor = regionSize / 2;
	}
	BHIP_TRY(s->tabBuf.reserve(ctx, all.size() * 8 + 8));
	BHIP_HIP(ctx, hipMemcpyAsync(s->tabBuf.p, all.data(), all.size() * 8, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const double* base = s->tabBuf.as<double>();
	t.oriWeights = t.oriHasWeights ? base + offOri : nullptr;
	t.weightSub = s->stable ? base + offSub : nullptr;
	t.weightGrid = s->stable ? base + offGrid : nullptr;
	t.weightFast = s->stable ? nullptr : base + offFast;
	return BHIP_OK;
}

// in: a batch of GrayF32 or GrayU8 (dense) frames, bands == GREY; or, bands > 0, one colour frame as [1 + bands] GrayF32 images -- the band
// average first, then the bands
template <class T>
static int surfRun(bhip_surf* s, DevImg<const T> in, int bands, SurfReturn ret) {
	using II = typename SurfTraits<T>::II;
	bhip_ctx* ctx = s->ctx;
	const int W = in.width, H = in.height, batch = bands > 0 ? 1 : in.batch;
	const long long px = (long long)W * H;
	s->haveResult = false;
	BHIP_TRY(s->det.prepare<II>(ctx, W, H, batch));
	if (!s->iiOwner) BHIP_TRY(s->iiBuf.reserve(ctx, (size_t)px * 4 * in.batch));
	II* iiBase = s->iiOwner ? s->iiOwner->as<II>() + px * s->iiFirst : s->iiBuf.as<II>();
	s->W = W; s->H = H; s->batch = batch;
	s->iiInt = std::is_same<II, int32_t>::value; s->planarBands = bands;
	const DevImg<II> iiAll{iiBase, px, W, W, H, in.batch};
	if constexpr (std::is_same<T, uint8_t>::value) BHIP_TRY(bhip_launch_integral_u8(ctx, in, iiAll));
	else BHIP_TRY(bhip_launch_integral(ctx, in, iiAll));
	const DevImg<const II> ii{iiBase, px, W, W, H, batch};
	BHIP_TRY(s->det.run(ctx, ii));
	// exclusive prefix of counts -> start of every image in the compact result arrays
	s->starts.assign(batch + 1, 0);
	for (int i = 0; i < batch; i++) s->starts[i + 1] = s->starts[i] + s->det.counts[i];
	const long long total = s->det.total;
	if (total > 0x7fffffffLL) return bhip_fail(ctx, BHIP_ERR_CAPACITY, "more than 2^31 key points in one batch");
	BHIP_TRY(s->startBuf.reserve(ctx, (size_t)(batch + 1) * 4));
	{
		// through a page-locked staging copy owned by the object: the transfer then reads it in stream order, and nothing rewrites it before the
		// next detect has synchronized on its own count read-back
		const size_t need = (size_t)(batch + 1) * 4;
		if (need > s->startsPinned.cap) BHIP_TRY(s->startsPinned.reserve(ctx, need * 2));
		memcpy(s->startsPinned.p, s->starts.data(), need);
		BHIP_HIP(ctx, hipMemcpyAsync(s->startBuf.p, s->startsPinned.p, need, hipMemcpyHostToDevice, ctx->stream));
	}
	if (s->brief) {
		// DetectDescribeFusion.detect (F:abst/feature/detdesc/DetectDescribeFusion.java:95-127) with orientation == null and
		// describe = WrapDescribeBrief (process always returns true, so every detected point is kept, in detector order):
		// yaw = detector.getOrientation(i) = 0 (WrapFHtoInterestPoint.java:77-79); DescribePointBrief.process samples the frame handed to
		// setImage (:71-75,86-88 -- the blurred copy it makes is never read)
		if (bands > 0) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "BRIEF runs on single-band frames");
		BHIP_TRY(s->angBuf.reserve(ctx, (size_t)std::max<long long>(total, 1) * 8));
		BHIP_TRY(s->whiteBuf.reserve(ctx, (size_t)std::max<long long>(total, 1)));
		BHIP_TRY(s->wordsBuf.reserve(ctx, (size_t)std::max<long long>(total, 1) * 4 * s->briefWords));
		if (total > 0) {
			BHIP_HIP(ctx, hipMemsetAsync(s->angBuf.p, 0, (size_t)total * 8, ctx->stream));
			BHIP_HIP(ctx, hipMemsetAsync(s->whiteBuf.p, 0, (size_t)total, ctx->stream));
			int maxCount = 0;
			for (int c : s->det.counts) maxCount = std::max(maxCount, c);
			BHIP_TRY(bhip_launch_brief(ctx, in, s->briefRadius, s->briefPoints, s->briefSample(), s->briefCompare(), (const double*)s->det.sorted.p, (int)total,
									   s->wordsBuf.as<int>(), s->startBuf.as<int>(), maxCount, (int)(sizeof(KeyPoint) / 8),
									   (long long)s->det.cap * (long long)(sizeof(KeyPoint) / 8), s->briefPatch));
		}
		BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
		s->haveResult = true;
		return BHIP_OK;
	}
	const int dof = s->dofOut();
	BHIP_TRY(s->angBuf.reserve(ctx, (size_t)std::max<long long>(total, 1) * 8));
	BHIP_TRY(s->descBuf.reserve(ctx, (size_t)std::max<long long>(total, 1) * 8 * dof));
	BHIP_TRY(s->whiteBuf.reserve(ctx, (size_t)std::max<long long>(total, 1)));
	// processing order of the describe stage: key points of one image grouped by coarse tile (L2 locality of the gathers)
	const int* perm = nullptr;
	{
#ifdef BHIP_EXPERIMENTS
		const bool noOrder = bhip_env_flag("BHIP_DESCRIBE_NOORDER");
#else
		const bool noOrder = false;
#endif
		int maxCount = 0;
		for (int c : s->det.counts) maxCount = std::max(maxCount, c);
		if (!noOrder && total > 0) {
			BHIP_TRY(s->permBuf.reserve(ctx, (size_t)total * 4 + (size_t)batch * 64 * 4));
			int* hist = s->permBuf.as<int>() + total;
			BHIP_TRY(bhip_launch_kp_spatial_order(ctx, s->det.sorted.as<KeyPoint>(), s->det.cap, s->startBuf.as<int>(), batch, maxCount, W, H, hist,
												  s->permBuf.as<int>()));
			perm = s->permBuf.as<int>();
		}
	}
	BHIP_TRY(bhip_launch_describe_ex(ctx, ii, s->det.sorted.as<KeyPoint>(), s->det.cap, s->startBuf.as<int>(), 0, total, s->tables, nullptr,
									 s->angBuf.as<double>(), s->descBuf.as<double>(), s->whiteBuf.as<uint8_t>(), perm, s->planar()));
	// host-frame callers may reuse their frames (and the upload buffer) as soon as the call returns; a device-resident batch was consumed before
	// the detector's count read-back, so its call returns with the describe kernels still in flight (stream order covers every later use)
	if (ret == SurfReturn::SYNCHRONIZED) BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	s->haveResult = true;
	return BHIP_OK;
}

static int surfCreateUnregistered(bhip_ctx* ctx, const bhip_fh_cfg* fh, const bhip_surf_cfg* surf, const bhip_ori_cfg* ori, int stable,
								  std::unique_ptr<bhip_surf>& out);

// device buffer growth that keeps the first `keep` bytes (result arrays that chunks are appended to)
static int growKeep(bhip_ctx* ctx, DevBuf& b, size_t bytes, size_t keep) {
	if (bytes <= b.cap) return BHIP_OK;
	DevBuf n;
	BHIP_TRY(n.reserve(ctx, bytes + bytes / 4));
	if (b.p && keep) BHIP_HIP(ctx, hipMemcpyAsync(n.p, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream));
	if (b.p) BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	b = std::move(n);   // the old block (now in n) is freed on return, after the copy out of it has finished
	return BHIP_OK;
}

#define SURF_CHUNK 32   // frames per chunk of a host batch (265 MB of 1080p GrayF32: ~5 ms of PCIe, ~3 ms of kernels)

// Host frames -> device in chunks on the copy stream, each chunk detected + described by the worker object as soon as it has arrived;
// results are appended to the owner's arrays, which end up exactly as one surfRun over the whole batch leaves them.
// upload(i, dst, stream) enqueues the copy of frame i (T: the frames' element type).  Returns BHIP_OK with *done = false when the batch has
// to go through the plain path (small batch, or a key-point list outgrew the owner's capacity half way).
template <class T, class Upload>
static int surfRunChunked(bhip_surf* s, int width, int height, int batch, Upload upload, bool* done) {
	using II = typename SurfTraits<T>::II;
	bhip_ctx* ctx = s->ctx;
	*done = false;
	int chunk = SURF_CHUNK;
	{ const char* e = getenv("BHIP_SURF_CHUNK"); if (e && atoi(e) > 0) chunk = atoi(e); }   // tests: chunk small batches too
	if (batch < 2 * chunk) return BHIP_OK;
	if (!s->worker) {
		BHIP_TRY(surfCreateUnregistered(ctx, &s->det.cfg, &s->sd, &s->ori, s->stable, s->worker));
		if (s->brief) {
			// the worker samples with the owner's definition (it borrows the device table; briefTab stays empty so it is never freed twice)
			bhip_surf* w0 = s->worker.get();
			w0->brief = true; w0->briefRadius = s->briefRadius; w0->briefPoints = s->briefPoints; w0->briefWords = s->briefWords;
			w0->briefBorrow = s->briefTab.as<int>(); w0->briefCompareOff = s->briefCompareOff; w0->briefPatch = s->briefPatch;
		}
		BHIP_HIP(ctx, hipStreamCreateWithFlags(&s->copyStream.h, hipStreamNonBlocking));
	}
	bhip_surf* w = s->worker.get();
	const size_t px = (size_t)width * height;
	s->haveResult = false;
	BHIP_TRY(s->det.prepare<II>(ctx, width, height, batch));
	BHIP_TRY(s->iiBuf.reserve(ctx, px * 4 * batch));
	// everything queued on the compute stream so far (an earlier batch may still read inBuf) precedes the first upload
	const int nchunks = (batch + chunk - 1) / chunk;
	// events are destroyed on every way out of this function
	std::vector<HipEvent> events(nchunks + 1);
	HipEvent& ev = events[nchunks];
	HipEvent* arrived = events.data();
	BHIP_HIP(ctx, hipEventCreateWithFlags(&ev.h, hipEventDisableTiming));
	BHIP_HIP(ctx, hipEventRecord(ev, ctx->stream));
	BHIP_HIP(ctx, hipStreamWaitEvent(s->copyStream, ev, 0));
	int status = BHIP_OK;
	for (int c = 0; c < nchunks && status == BHIP_OK; c++) {
		const int a = c * chunk, n = std::min(chunk, batch - a);
		for (int i = a; i < a + n && status == BHIP_OK; i++) status = upload(i, s->inBuf.as<T>() + px * i, s->copyStream);
		if (status == BHIP_OK && (hipEventCreateWithFlags(&arrived[c].h, hipEventDisableTiming) != hipSuccess || hipEventRecord(arrived[c], s->copyStream) != hipSuccess))
			status = bhip_fail(ctx, BHIP_ERR_HIP, "event");
	}
	const int dof = s->tables.dof;
	s->starts.assign(batch + 1, 0);
	s->det.counts.assign(batch, 0);
	long long total = 0;
	bool fits = true;
	for (int c = 0; c < nchunks && status == BHIP_OK && fits; c++) {
		const int a = c * chunk, n = std::min(chunk, batch - a);
		if (hipStreamWaitEvent(ctx->stream, arrived[c], 0) != hipSuccess) { status = bhip_fail(ctx, BHIP_ERR_HIP, "wait"); break; }
		w->iiOwner = &s->iiBuf; w->iiFirst = a;
		status = surfRun(w, DevImg<const T>{s->inBuf.as<T>() + px * a, (long long)px, width, width, height, n}, GREY, SurfReturn::SYNCHRONIZED);
		if (status != BHIP_OK) break;
		int maxCount = 0;
		for (int i = 0; i < n; i++) maxCount = std::max(maxCount, w->det.counts[i]);
		if (maxCount > s->det.cap) { fits = false; break; }   // the owner's [image][cap] key-point array is too narrow: plain path (it grows there)
		const long long ct = w->det.total;
		status = growKeep(ctx, s->angBuf, (size_t)std::max<long long>(total + ct, 1) * 8, (size_t)total * 8);
		if (status == BHIP_OK && !s->brief) status = growKeep(ctx, s->descBuf, (size_t)std::max<long long>(total + ct, 1) * 8 * dof, (size_t)total * 8 * dof);
		if (status == BHIP_OK) status = growKeep(ctx, s->whiteBuf, (size_t)std::max<long long>(total + ct, 1), (size_t)total);
		if (status == BHIP_OK && s->brief) status = growKeep(ctx, s->wordsBuf, (size_t)std::max<long long>(total + ct, 1) * 4 * s->briefWords, (size_t)total * 4 * s->briefWords);
		if (status != BHIP_OK) break;
		hipError_t e = hipSuccess;
		if (maxCount > 0)
			e = hipMemcpy2DAsync(s->det.sorted.as<KeyPoint>() + (long long)a * s->det.cap, (size_t)s->det.cap * sizeof(KeyPoint), w->det.sorted.p,
								 (size_t)w->det.cap * sizeof(KeyPoint), (size_t)maxCount * sizeof(KeyPoint), n, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess && ct > 0) e = hipMemcpyAsync(s->angBuf.as<double>() + total, w->angBuf.p, (size_t)ct * 8, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess && ct > 0 && !s->brief) e = hipMemcpyAsync(s->descBuf.as<double>() + total * dof, w->descBuf.p, (size_t)ct * 8 * dof, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess && ct > 0 && s->brief) e = hipMemcpyAsync(s->wordsBuf.as<int>() + total * s->briefWords, w->wordsBuf.p, (size_t)ct * 4 * s->briefWords, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess && ct > 0) e = hipMemcpyAsync(s->whiteBuf.as<uint8_t>() + total, w->whiteBuf.p, (size_t)ct, hipMemcpyDeviceToDevice, ctx->stream);
		if (e != hipSuccess) { status = bhip_fail(ctx, BHIP_ERR_HIP, hipGetErrorString(e)); break; }
		for (int i = 0; i < n; i++) {
			s->det.counts[a + i] = w->det.counts[i];
			s->starts[a + i + 1] = s->starts[a + i] + w->det.counts[i];
		}
		total += ct;
	}
	// every upload has to be over before the caller's frames may change (and before the plain path re-uses inBuf)
	(void)hipStreamSynchronize(s->copyStream);
	(void)hipStreamSynchronize(ctx->stream);
	w->iiOwner = nullptr;
	if (status != BHIP_OK) return status;
	if (!fits) {
		// the frames are all on the device: run the whole batch the plain way (its detector grows the key-point capacity as needed)
		*done = true;
		return surfRun(s, bhip_img_over<const T>(s->inBuf, width, width, height, batch), GREY, SurfReturn::SYNCHRONIZED);
	}
	if (total > 0x7fffffffLL) return bhip_fail(ctx, BHIP_ERR_CAPACITY, "more than 2^31 key points in one batch");
	s->det.total = total;
	s->W = width; s->H = height; s->batch = batch;
	s->iiInt = std::is_same<II, int32_t>::value;
	s->planarBands = 0;
	BHIP_TRY(s->startBuf.reserve(ctx, (size_t)(batch + 1) * 4));
	BHIP_HIP(ctx, hipMemcpyAsync(s->startBuf.p, s->starts.data(), (size_t)(batch + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	s->haveResult = true;
	*done = true;
	return BHIP_OK;
}

static int surfCreateUnregistered(bhip_ctx* ctx, const bhip_fh_cfg* fh, const bhip_surf_cfg* surf, const bhip_ori_cfg* ori, int stable,
								  std::unique_ptr<bhip_surf>& out) {
	std::unique_ptr<bhip_surf> s(new (std::nothrow) bhip_surf());
	if (!s) return bhip_fail(ctx, BHIP_ERR_NOMEM, "out of host memory");
	s->ctx = ctx;
	s->stable = stable ? 1 : 0;
	if (fh) s->det.cfg = *fh; else bhip_fh_cfg_default(&s->det.cfg);
	if (surf) s->sd = *surf; else bhip_surf_cfg_default(&s->sd);
	if (ori) s->ori = *ori; else bhip_ori_cfg_default(&s->ori, s->stable);
	BHIP_TRY(buildTables(s.get()));
	out = std::move(s);
	return BHIP_OK;
}

// every sample point the pairs use lies within [-radius, radius]^2: the LDS-patch BRIEF kernel may be used (ip.hip, k_brief_patch)
static bool briefPatchOk(const int32_t* samplePoints, int nSamples, int radius) {
	for (int i = 0; i < 2 * nSamples; i++)
		if (samplePoints[i] < -radius || samplePoints[i] > radius) return false;
	return radius >= 0 && radius <= 40;
}

// bhip_surf_detect_f32 (T = float) and bhip_surf_detect_u8 (T = uint8_t: GrayS32 integral images, integer taps)
template <class T>
static int surfDetectHost(bhip_surf* s, const T* const* img, const int* startIndex, const int* stride, int width, int height, int batch) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!img || width <= 0 || height <= 0 || batch <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image batch");
	const size_t px = (size_t)width * height;
	BHIP_TRY(s->inBuf.reserve(ctx, px * sizeof(T) * batch));
	for (int i = 0; i < batch; i++)
		if (!img[i] || (stride ? stride[i] : width) < width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image (null or stride < width)");
	auto put = [&](int i, T* dst, hipStream_t st) {
		return upload(ctx, dst, width, img[i], startIndex ? startIndex[i] : 0, stride ? stride[i] : width, width, height, st);
	};
	bool done = false;
	BHIP_TRY(surfRunChunked<T>(s, width, height, batch, put, &done));
	if (done) return BHIP_OK;
	for (int i = 0; i < batch; i++) BHIP_TRY(put(i, s->inBuf.as<T>() + px * i, ctx->stream));
	return surfRun(s, bhip_img_over<const T>(s->inBuf, width, width, height, batch), GREY, SurfReturn::SYNCHRONIZED);
}

// AssociateDescription over the descriptors still resident from the last detect of `s`: checks the problem table of
// bhip_assoc_l2_surf / bhip_assoc_hamming_surf, has `match` write problem p (source image srcImage[p], destination dstImage[p]) into device
// arrays prefilled with "no match", and downloads them.
template <class Match>
static int assocSurf(bhip_surf* s, int count, const int* srcImage, const int* dstImage, int* pairs, double* fit, Match match) {
	bhip_ctx* ctx = s->ctx;
	if (!s->haveResult) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result");
	if (count < 0 || (count > 0 && (!srcImage || !dstImage || !pairs || !fit))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad problem table");
	if (count == 0) return BHIP_OK;
	const long long total = s->det.total;
	std::vector<long long> so(count), doff(count);
	std::vector<int> ns(count), nd(count);
	std::vector<char> used(s->batch, 0);
	for (int p = 0; p < count; p++) {
		const int a = srcImage[p], b = dstImage[p];
		if (a < 0 || a >= s->batch || b < 0 || b >= s->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "image index outside the last batch");
		if (used[a]) return bhip_fail(ctx, BHIP_ERR_INVALID, "an image may be the source of one problem per call");
		used[a] = 1;
		so[p] = s->starts[a]; ns[p] = s->det.counts[a];
		doff[p] = s->starts[b]; nd[p] = s->det.counts[b];
	}
	if (total == 0) return BHIP_OK;
	CtxScratch* sc = scratchOf(ctx);
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)total * 4));
	BHIP_TRY(sc->out1.reserve(ctx, (size_t)total * 8));
	// rows of images that are the source of no problem in this call come back as "no match" (-1, 0), not as whatever an earlier call left
	BHIP_HIP(ctx, hipMemsetAsync(sc->out0.p, 0xff, (size_t)total * 4, ctx->stream));
	BHIP_HIP(ctx, hipMemsetAsync(sc->out1.p, 0, (size_t)total * 8, ctx->stream));
	BHIP_TRY(match(so.data(), ns.data(), doff.data(), nd.data(), sc->out0.as<int>(), sc->out1.as<double>()));
	BHIP_HIP(ctx, hipMemcpyAsync(pairs, sc->out0.p, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(fit, sc->out1.p, (size_t)total * 8, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

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

// FastHessianFeatureDetector.detect(integral) on a GrayF32 (T = float) or a GrayS32 (T = int32_t, from a GrayU8 frame) integral image
template <class T>
static int fhDetect(bhip_ctx* ctx, const bhip_fh_cfg* cfg, HostImg<const T> hin, double* xy_scale, int cap, int* n) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	if (!n || cap < 0 || (cap > 0 && !xy_scale)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	*n = 0;
	FhDetector det;
	if (cfg) det.cfg = *cfg; else bhip_fh_cfg_default(&det.cfg);
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> din;
	int status = stageIn(ctx, sc->in0, hin, hin.width, din);
	if (status == BHIP_OK) status = det.prepare<T>(ctx, hin.width, hin.height, 1);
	if (status == BHIP_OK) status = det.run(ctx, DevImg<const T>(din));
	if (status == BHIP_OK) {
		*n = det.counts[0];
		const int ncopy = std::min(*n, cap);
		if (ncopy > 0) {
			std::vector<KeyPoint> kps(ncopy);
			hipError_t e = hipMemcpyAsync(kps.data(), det.sorted.p, (size_t)ncopy * sizeof(KeyPoint), hipMemcpyDeviceToHost, ctx->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
			if (e != hipSuccess) status = bhip_fail(ctx, BHIP_ERR_HIP, hipGetErrorString(e));
			else for (int i = 0; i < ncopy; i++) { xy_scale[3 * i] = kps[i].x; xy_scale[3 * i + 1] = kps[i].y; xy_scale[3 * i + 2] = kps[i].scale; }
		}
	}
	(void)hipStreamSynchronize(ctx->stream);   // det's buffers are freed on return
	return status;
}

extern "C" {

int bhip_surf_create(bhip_ctx* ctx, const bhip_fh_cfg* fh, const bhip_surf_cfg* surf, const bhip_ori_cfg* ori, int stable, bhip_surf** out) {
	return createChild(ctx, out, [&](std::unique_ptr<bhip_surf>& s) -> int {
		CHECK_CTX(ctx);
		if (!out) return bhip_fail(ctx, BHIP_ERR_INVALID, "null output");
		*out = nullptr;
		return surfCreateUnregistered(ctx, fh, surf, ori, stable, s);
	});
}

int bhip_surf_destroy(bhip_surf* s) { return destroyChild(s); }

int bhip_surf_dof(bhip_surf* s) { return s ? s->dofOut() : 0; }

int bhip_surf_detect_dev_f32(bhip_surf* s, const float* dev_images, long long imageStride, int stride, int width, int height, int batch) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!dev_images || width <= 0 || height <= 0 || batch <= 0 || stride < width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image batch");
	return surfRun(s, DevImg<const float>{dev_images, imageStride, stride, width, height, batch}, GREY, SurfReturn::QUEUED);
}

int bhip_surf_detect_f32(bhip_surf* s, const float* const* img, const int* startIndex, const int* stride, int width, int height, int batch) {
	return surfDetectHost(s, img, startIndex, stride, width, height, batch);
}

// FactoryDetectDescribe.surfColorStable / surfColorFast on one Planar<GrayF32> frame:
//   SurfPlanar_to_DetectDescribePoint.detect      F:abst/feature/detdesc/SurfPlanar_to_DetectDescribePoint.java:62-77
//   ImplConvertPlanarToGray.average               I:core/image/impl/ImplConvertPlanarToGray.java:296-336
//   DetectDescribeSurfPlanar.detect / describe    F:alg/feature/detdesc/DetectDescribeSurfPlanar.java:91-124
//   DescribePointSurfPlanar.describe              F:alg/feature/describe/DescribePointSurfPlanar.java:100-114
int bhip_surf_detect_planar_f32(bhip_surf* s, const float* const* bands, int numBands, int startIndex, int stride, int width, int height) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!bands || numBands < 1 || numBands > 16 || width <= 0 || height <= 0 || stride < width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad planar image");
	const size_t px = (size_t)width * height;
	BHIP_TRY(s->inBuf.reserve(ctx, px * 4 * (1 + numBands)));
	for (int b = 0; b < numBands; b++) {
		if (!bands[b]) return bhip_fail(ctx, BHIP_ERR_INVALID, "null band");
		BHIP_TRY(upload(ctx, s->inBuf.as<float>() + px * (1 + b), width, bands[b], startIndex, stride, width, height, ctx->stream));
	}
	BHIP_TRY(bhip_launch_planar_average(ctx, s->inBuf.as<float>() + px, (long long)px, numBands, (long long)px, s->inBuf.as<float>()));
	return surfRun(s, bhip_img_over<const float>(s->inBuf, width, width, height, 1 + numBands), numBands, SurfReturn::SYNCHRONIZED);
}

// FactoryDetectDescribe.surfStable / surfFast on GrayU8 frames (integral type GrayS32, GIntegralImageOps.getIntegralType): same results
// interface as bhip_surf_detect_f32
int bhip_surf_detect_u8(bhip_surf* s, const uint8_t* const* img, const int* startIndex, const int* stride, int width, int height, int batch) {
	return surfDetectHost(s, img, startIndex, stride, width, height, batch);
}

int bhip_surf_count(bhip_surf* s, int image, int* n) {
	if (!s || !n) return BHIP_ERR_INVALID;
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(s->ctx, BHIP_ERR_INVALID, "no detect result for that image");
	*n = s->det.counts[image];
	return BHIP_OK;
}
// getNumberOfFeatures() of every image of the last detect in one call (a batch-level caller's prefix sums)
int bhip_surf_counts(bhip_surf* s, int* counts, int capacity) {
	if (!s || !counts) return BHIP_ERR_INVALID;
	if (!s->haveResult || capacity < s->batch) return bhip_fail(s->ctx, BHIP_ERR_INVALID, "no detect result / counts array too short");
	for (int i = 0; i < s->batch; i++) counts[i] = s->det.counts[i];
	return BHIP_OK;
}
int bhip_surf_total(bhip_surf* s, long long* n) {
	if (!s || !n) return BHIP_ERR_INVALID;
	*n = s->haveResult ? s->det.total : 0;
	return BHIP_OK;
}

int bhip_surf_fetch(bhip_surf* s, int image, double* xy_scale, double* angle, uint8_t* white, double* desc) {
	// (dof below is the full descriptor length: numBands * 64 after a planar detect)
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result for that image");
	if (desc && s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "this object describes with BRIEF: fetch the words with bhip_surf_fetch_brief");
	const int n = s->det.counts[image];
	if (n == 0) return BHIP_OK;
	const long long off = s->starts[image];
	const int dof = s->dofOut();
	std::vector<KeyPoint> kps;
	if (xy_scale) {
		kps.resize(n);
		BHIP_HIP(ctx, hipMemcpyAsync(kps.data(), s->det.sorted.as<KeyPoint>() + (long long)image * s->det.cap, (size_t)n * sizeof(KeyPoint),
									 hipMemcpyDeviceToHost, ctx->stream));
	}
	if (angle) BHIP_HIP(ctx, hipMemcpyAsync(angle, s->angBuf.as<double>() + off, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (white) BHIP_HIP(ctx, hipMemcpyAsync(white, s->whiteBuf.as<uint8_t>() + off, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
	if (desc) BHIP_HIP(ctx, hipMemcpyAsync(desc, s->descBuf.as<double>() + off * dof, (size_t)n * 8 * dof, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (xy_scale)
		for (int i = 0; i < n; i++) { xy_scale[3 * i] = kps[i].x; xy_scale[3 * i + 1] = kps[i].y; xy_scale[3 * i + 2] = kps[i].scale; }
	return BHIP_OK;
}

// the whole batch of the last detect in ONE set of copies (per-image slices start at the exclusive prefix of bhip_surf_count):
// what a batched caller (DetectDescribeSurfHip.detectBatch) uses instead of `batch` bhip_surf_fetch calls
int bhip_surf_fetch_all(bhip_surf* s, double* xy_scale, double* angle, uint8_t* white, double* desc) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->haveResult) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result");
	if (desc && s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "this object describes with BRIEF: fetch the words with bhip_surf_fetch_brief");
	const long long total = s->det.total;
	if (total == 0) return BHIP_OK;
	const int dof = s->dofOut();
	if (xy_scale) {
		// key points sit in [image][cap] KeyPoint records: pack x, y, scale of every image into the compact layout on the device first
		BHIP_TRY(s->xysBuf.reserve(ctx, (size_t)total * 24));
		for (int i = 0; i < s->batch; i++) {
			const int n = s->det.counts[i];
			if (n > 0)
				BHIP_HIP(ctx, hipMemcpy2DAsync((char*)s->xysBuf.p + (size_t)s->starts[i] * 24, 24, s->det.sorted.as<KeyPoint>() + (long long)i * s->det.cap,
											   sizeof(KeyPoint), 24, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
		}
		BHIP_HIP(ctx, hipMemcpyAsync(xy_scale, s->xysBuf.p, (size_t)total * 24, hipMemcpyDeviceToHost, ctx->stream));
	}
	if (angle) BHIP_HIP(ctx, hipMemcpyAsync(angle, s->angBuf.p, (size_t)total * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (white) BHIP_HIP(ctx, hipMemcpyAsync(white, s->whiteBuf.p, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
	if (desc) BHIP_HIP(ctx, hipMemcpyAsync(desc, s->descBuf.p, (size_t)total * 8 * dof, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}

int bhip_surf_dev_view(bhip_surf* s, int image, const double** dev_desc, const double** dev_xy_scale, const uint8_t** dev_white, int* n) {
	if (!s) return BHIP_ERR_INVALID;
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(s->ctx, BHIP_ERR_INVALID, "no detect result for that image");
	const long long off = s->starts[image];
	if (dev_desc) *dev_desc = s->descBuf.as<double>() + off * s->dofOut();
	// key points are KeyPoint records {x,y,scale,key,pad}: 32-byte stride, first three doubles are x,y,scale
	if (dev_xy_scale) *dev_xy_scale = (const double*)(s->det.sorted.as<KeyPoint>() + (long long)image * s->det.cap);
	if (dev_white) *dev_white = s->whiteBuf.as<uint8_t>() + off;
	if (n) *n = s->det.counts[image];
	return BHIP_OK;
}

// FactoryDetectDescribe.fuseTogether(FactoryInterestPoint.fastHessian(fh), null, FactoryDescribeRegionPoint.brief(config, imageType))
// (F:factory/feature/detdesc/FactoryDetectDescribe.java:279-284, F:factory/feature/describe/FactoryDescribeRegionPoint.java:187-202 with
// config.fixed): the returned object is driven through the same bhip_surf_detect_* / _count / _fetch calls as the SURF one.
int bhip_surf_create_brief(bhip_ctx* ctx, const bhip_fh_cfg* fh, int radius, int numPoints, const int32_t* samplePoints, const int32_t* compare, bhip_surf** out) {
	return createChild(ctx, out, [&](std::unique_ptr<bhip_surf>& s) -> int {
		CHECK_CTX(ctx);
		if (!out) return bhip_fail(ctx, BHIP_ERR_INVALID, "null output");
		*out = nullptr;
		if (radius < 0 || numPoints <= 0 || !samplePoints || !compare) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad BRIEF definition");
		int maxIdx = 0;
		for (int i = 0; i < 2 * numPoints; i++) {
			if (compare[i] < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "negative sample index");
			maxIdx = std::max(maxIdx, compare[i]);
		}
		BHIP_TRY(surfCreateUnregistered(ctx, fh, nullptr, nullptr, 0, s));   // (the SURF tables of the shell are never used)
		s->brief = true;
		s->briefRadius = radius; s->briefPoints = numPoints; s->briefWords = (numPoints + 31) / 32;
		const size_t nSample = (size_t)(maxIdx + 1) * 2, nCompare = (size_t)numPoints * 2;
		s->briefCompareOff = nSample;
		s->briefPatch = briefPatchOk(samplePoints, maxIdx + 1, radius);
		BHIP_TRY(s->briefTab.reserve(ctx, (nSample + nCompare) * 4));
		if (hipMemcpy(s->briefTab.p, samplePoints, nSample * 4, hipMemcpyHostToDevice) != hipSuccess) return bhip_fail(ctx, BHIP_ERR_HIP, "BRIEF table upload");
		if (hipMemcpy(s->briefTab.as<int>() + nSample, compare, nCompare * 4, hipMemcpyHostToDevice) != hipSuccess) return bhip_fail(ctx, BHIP_ERR_HIP, "BRIEF table upload");
		return BHIP_OK;
	});
}

// getDescription(i).data of every feature of one image (image >= 0: count * words ints) or of the whole batch (image = -1: total * words
// ints, image i's slice at the exclusive prefix of the counts); words = ceil(numPoints / 32) (TupleDesc_B, T:struct/feature/TupleDesc_B.java)
int bhip_surf_fetch_brief(bhip_surf* s, int image, int32_t* words) {
	if (!s || !words) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "not a BRIEF detect+describe object");
	if (!s->haveResult || image < -1 || image >= s->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result for that image");
	const long long off = image < 0 ? 0 : s->starts[image];
	const long long n = image < 0 ? s->det.total : s->det.counts[image];
	if (n == 0) return BHIP_OK;
	BHIP_HIP(ctx, hipMemcpyAsync(words, s->wordsBuf.as<int>() + off * s->briefWords, (size_t)n * 4 * s->briefWords, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}
int bhip_surf_dev_view_brief(bhip_surf* s, int image, const int32_t** dev_words, int* words, int* n) {
	if (!s) return BHIP_ERR_INVALID;
	if (!s->brief) return bhip_fail(s->ctx, BHIP_ERR_INVALID, "not a BRIEF detect+describe object");
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(s->ctx, BHIP_ERR_INVALID, "no detect result for that image");
	if (dev_words) *dev_words = s->wordsBuf.as<int>() + (long long)s->starts[image] * s->briefWords;
	if (words) *words = s->briefWords;
	if (n) *n = s->det.counts[image];
	return BHIP_OK;
}

int bhip_surf_fetch_integral(bhip_surf* s, int image, float* out) {
	if (!s || !out) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result for that image");
	BHIP_HIP(ctx, hipMemcpyAsync(out, s->iiBuf.as<float>() + (long long)image * s->W * s->H, (size_t)s->W * s->H * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}

int bhip_surf_describe_points(bhip_surf* s, int image, const double* xy_scale, int n, double* angle, uint8_t* white, double* desc) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result for that image");
	if (s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "this object describes with BRIEF");
	if (n < 0 || (n > 0 && !xy_scale)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad point list");
	if (n == 0) return BHIP_OK;
	std::vector<KeyPoint> kps(n);
	for (int i = 0; i < n; i++) { kps[i].x = xy_scale[3 * i]; kps[i].y = xy_scale[3 * i + 1]; kps[i].scale = xy_scale[3 * i + 2]; kps[i].key = 0; kps[i].pad = 0; }
	const int dof = s->dofOut();
	BHIP_TRY(s->tmpKp.reserve(ctx, (size_t)n * sizeof(KeyPoint)));
	BHIP_TRY(s->tmpAng.reserve(ctx, (size_t)n * 8));
	BHIP_TRY(s->tmpDesc.reserve(ctx, (size_t)n * 8 * dof));
	BHIP_TRY(s->tmpWhite.reserve(ctx, (size_t)n));
	BHIP_HIP(ctx, hipMemcpyAsync(s->tmpKp.p, kps.data(), (size_t)n * sizeof(KeyPoint), hipMemcpyHostToDevice, ctx->stream));
	BHIP_TRY(withIntegral(s, [&](auto ii) {
		return bhip_launch_describe_ex(ctx, ii, s->tmpKp.as<KeyPoint>(), 0, nullptr, image, n, s->tables, nullptr, s->tmpAng.as<double>(),
									   s->tmpDesc.as<double>(), s->tmpWhite.as<uint8_t>(), nullptr, s->planar());
	}));
	if (angle) BHIP_HIP(ctx, hipMemcpyAsync(angle, s->tmpAng.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (white) BHIP_HIP(ctx, hipMemcpyAsync(white, s->tmpWhite.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
	if (desc) BHIP_HIP(ctx, hipMemcpyAsync(desc, s->tmpDesc.p, (size_t)n * 8 * dof, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}

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

// strict block NMS of a batch of device images: lists into dev_xy ([batch][cap] (x,y) int16 pairs, block-raster order), counts into
// dev_n[batch] (a count may exceed cap: only the first cap pairs are written)
// minimum: NonMaxBlockSearchStrict.Min with threshold = thresholdMin.  The maxima pass works in the first half of the context's NMS buffers,
// the minima pass in the second (both halves are reserved before either pass is queued), so Min + Max on one image is two passes.
static int nonmaxDevice(bhip_ctx* ctx, DevImg<const float> img, int radius, float threshold, int border, int16_t* dev_xy, int cap, int* dev_n,
						bool minimum = false) {
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

int bhip_nonmax_block_minmax_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long imageStride, int stride, int width, int height, int batch, int radius,
									 float thresholdMin, float thresholdMax, int border, int detectMin, int detectMax, int16_t* dev_xyMin, int* dev_nMin,
									 int16_t* dev_xyMax, int* dev_nMax, int cap) {
	CHECK_CTX(ctx);
	const DevImg<const float> img{dev_intensity, imageStride, stride, width, height, batch};
	CHECK_IMG(ctx, img);
	return nonmaxMinMaxDevice(ctx, img, radius, thresholdMin, thresholdMax, border, detectMin != 0, detectMax != 0, dev_xyMin, dev_nMin, dev_xyMax, dev_nMax, cap);
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

// ---- FAST corners (fast.hip): FastCornerDetector.process on a batch of device frames ----
extern "C++" {
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

}  // extern "C++"

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

// ---- dense stereo disparity (disparity.hip): StereoDisparity.process of FactoryStereoDisparity.blockMatch, SAD on GrayU8 pairs ----
extern "C++" {
// Java's (int) of a double: NaN -> 0, saturating
static int javaDoubleToInt(double v) {
	if (v != v) return 0;
	if (v >= 2147483647.0) return 2147483647;
	if (v <= -2147483648.0) return -2147483647 - 1;
	return (int)v;
}

// the checks of ConfigDisparityBM.checkValidity, DisparityBlockMatchRowFormat.process and SelectDisparityWithChecksWta.configure, then the
// kernel's limits; fills the selector's parameters
template <class OutT>
static int disparityParams(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int width, int height, DispBmParams& p) {
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
	const int maxError = javaDoubleToInt((rw * rh) * c.maxPerPixelError);   // FactoryStereoDisparity.java:75,79
	p.minD = c.minDisparity; p.range = c.rangeDisparity; p.rx = c.regionRadiusX; p.ry = c.regionRadiusY;
	p.maxError = maxError <= 0 ? 2147483647 : maxError;                     // SelectDisparityWithChecksWta.java:83
	p.rtolTol = c.validateRtoL;
	p.textureThr = javaDoubleToInt(10000 * c.texture);                      // SelectErrorWithChecks_S32.setTexture
	return BHIP_OK;
}

template <class OutT>
static int disparityDevice(bhip_ctx* ctx, const DispBmParams& p, DevImg<const uint8_t> left, DevImg<const uint8_t> right, DevImg<OutT> disp) {
	DevBuf& scratch = scratchOf(ctx)->disparity;
	BHIP_TRY(scratch.reserve(ctx, bhip_disparity_scratch(left.width, left.height, left.batch)));
	return bhip_launch_disparity_bm<OutT>(ctx, left, right, p, scratch.as<uint8_t>(), disp);
}

template <class OutT>
static int disparityDev(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride, const uint8_t* dev_right,
						long long rImageStride, int rStride, int width, int height, int batch, OutT* dev_disp, long long dImageStride, int dStride) {
	CHECK_CTX(ctx);
	const DevImg<const uint8_t> left{dev_left, lImageStride, lStride, width, height, batch}, right{dev_right, rImageStride, rStride, width, height, batch};
	const DevImg<OutT> disp{dev_disp, dImageStride, dStride, width, height, batch};
	CHECK_IMG(ctx, left);
	CHECK_IMG(ctx, right);
	CHECK_IMG(ctx, disp);
	DispBmParams p;
	BHIP_TRY(disparityParams<OutT>(ctx, cfg, width, height, p));
	return disparityDevice<OutT>(ctx, p, left, right, disp);
}

template <class OutT>
static int disparityHost(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart, int rStride,
						 int width, int height, OutT* disp, int dStart, int dStride) {
	const HostImg<const uint8_t> hl{left, lStart, lStride, width, height}, hr{right, rStart, rStride, width, height};
	const HostImg<OutT> hd{disp, dStart, dStride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hl);
	CHECK_IMG(ctx, hr);
	CHECK_IMG(ctx, hd);
	DispBmParams p;
	BHIP_TRY(disparityParams<OutT>(ctx, cfg, width, height, p));
	CtxScratch* sc = scratchOf(ctx);
	DevImg<uint8_t> dl, dr;
	DevImg<OutT> dd;
	BHIP_TRY(stageIn(ctx, sc->in0, hl, width, dl));
	BHIP_TRY(stageIn(ctx, sc->in1, hr, width, dr));
	BHIP_TRY(stageIn(ctx, sc->out0, hd, width, dd, false));
	BHIP_TRY(disparityDevice<OutT>(ctx, p, dl, dr, dd));
	BHIP_TRY(stageOut(ctx, hd, dd));
	return bhip_ctx_synchronize(ctx);
}
}  // extern "C++"

int bhip_disparity_bm_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart,
							int rStride, int width, int height, uint8_t* disp, int dStart, int dStride) {
	return disparityHost<uint8_t>(ctx, cfg, left, lStart, lStride, right, rStart, rStride, width, height, disp, dStart, dStride);
}
int bhip_disparity_bm_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart,
							 int rStride, int width, int height, float* disp, int dStart, int dStride) {
	return disparityHost<float>(ctx, cfg, left, lStart, lStride, right, rStart, rStride, width, height, disp, dStart, dStride);
}
int bhip_disparity_bm_dev_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride,
								const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, uint8_t* dev_disp,
								long long dImageStride, int dStride) {
	return disparityDev<uint8_t>(ctx, cfg, dev_left, lImageStride, lStride, dev_right, rImageStride, rStride, width, height, batch, dev_disp, dImageStride, dStride);
}
int bhip_disparity_bm_dev_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride,
								 const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, float* dev_disp,
								 long long dImageStride, int dStride) {
	return disparityDev<float>(ctx, cfg, dev_left, lImageStride, lStride, dev_right, rImageStride, rStride, width, height, batch, dev_disp, dImageStride, dStride);
}

// ---- image remap (distort.hip): ImageDistort.apply of FactoryDistort.distortSB, GrayU8 / GrayF32, NEAREST_NEIGHBOR / BILINEAR, ZERO / EXTENDED ----
extern "C++" {
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
}  // extern "C++"

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

// ---- template matching (template.hip, k_template_select in detect.hip): TemplateMatchingIntensity.process and the selection of TemplateMatching.process ----
extern "C++" {
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
}  // extern "C++"

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

int bhip_fh_detect_f32(bhip_ctx* ctx, const bhip_fh_cfg* cfg, const float* ii, int iiStart, int iiStride, int width, int height, double* xy_scale,
					   int cap, int* n) {
	return fhDetect<float>(ctx, cfg, {ii, iiStart, iiStride, width, height}, xy_scale, cap, n);
}
int bhip_fh_detect_s32(bhip_ctx* ctx, const bhip_fh_cfg* cfg, const int32_t* ii, int iiStart, int iiStride, int width, int height, double* xy_scale,
					   int cap, int* n) {
	return fhDetect<int32_t>(ctx, cfg, {ii, iiStart, iiStride, width, height}, xy_scale, cap, n);
}

// ---------------------------------------------------------------------------------------------------------------
// association
// ---------------------------------------------------------------------------------------------------------------
int bhip_assoc_coltop_bytes(void) { return bhip_assoc_coltop_size(); }

static bool assocExactOnly(bhip_ctx* ctx) {
	CtxScratch* sc = scratchOf(ctx);
	if (sc->assocExactOnly < 0) {
		const char* e = getenv("BHIP_ASSOC_EXACT");
		sc->assocExactOnly = (e && e[0] == '1') ? 1 : 0;
	}
	return sc->assocExactOnly == 1;
}

static int assocL2Exact(bhip_ctx* ctx, const double* dev_src, int ns, const double* dev_dst, int nd, int dof, double maxErr, int backwards,
						int sqrtScore, int* dev_pairs, double* dev_fit);

int bhip_assoc_l2_dev(bhip_ctx* ctx, const double* dev_src, int ns, const double* dev_dst, int nd, int dof, double maxErr, int backwards,
					  int sqrtScore, int* dev_pairs, double* dev_fit) {
	CHECK_CTX(ctx);
	if (ns < 0 || nd < 0 || dof <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
	if (ns == 0) return BHIP_OK;
	if (dof == 64 && !sqrtScore && nd > 0 && !assocExactOnly(ctx)) {
		// matrix-core path (fp32 MFMA candidates + exact fp64 re-score); falls through on degenerate inputs
		const long long zero = 0;
		int used = 0;
		BHIP_TRY(bhip_assoc_l2_mfma_batched(ctx, scratchOf(ctx)->mfma, dev_src, dev_dst, 1, &zero, &ns, &zero, &nd, maxErr, backwards, dev_pairs, dev_fit,
											&used));
		if (used) return BHIP_OK;
	}
	return assocL2Exact(ctx, dev_src, ns, dev_dst, nd, dof, maxErr, backwards, sqrtScore, dev_pairs, dev_fit);
}

static int assocL2Exact(bhip_ctx* ctx, const double* dev_src, int ns, const double* dev_dst, int nd, int dof, double maxErr, int backwards,
						int sqrtScore, int* dev_pairs, double* dev_fit) {
	CtxScratch* sc = scratchOf(ctx);
	void* col = nullptr;
	if (backwards && nd > 0) { BHIP_TRY(sc->assocCol.reserve(ctx, (size_t)nd * bhip_assoc_coltop_size())); col = sc->assocCol.p; }
	BHIP_TRY(bhip_assoc_phase1_l2(ctx, dev_src, ns, 0, dev_dst, nd, dof, maxErr, sqrtScore, dev_pairs, dev_fit, col, sc->work));
	if (col) BHIP_TRY(bhip_assoc_phase2(ctx, col, 1, nd, ns, 0, dev_pairs, dev_fit));
	return BHIP_OK;
}
int bhip_assoc_hamming_dev(bhip_ctx* ctx, const int32_t* dev_src, int ns, const int32_t* dev_dst, int nd, int words, double maxErr, int backwards,
						   int* dev_pairs, double* dev_fit) {
	CHECK_CTX(ctx);
	if (ns < 0 || nd < 0 || words <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
	if (ns == 0) return BHIP_OK;
	CtxScratch* sc = scratchOf(ctx);
	void* col = nullptr;
	if (backwards && nd > 0) { BHIP_TRY(sc->assocCol.reserve(ctx, (size_t)nd * bhip_assoc_coltop_size())); col = sc->assocCol.p; }
	BHIP_TRY(bhip_assoc_phase1_ham(ctx, dev_src, ns, 0, dev_dst, nd, words, maxErr, dev_pairs, dev_fit, col, sc->work));
	if (col) BHIP_TRY(bhip_assoc_phase2(ctx, col, 1, nd, ns, 0, dev_pairs, dev_fit));
	return BHIP_OK;
}

int bhip_assoc_l2_dev_batched(bhip_ctx* ctx, const double* dev_src, const double* dev_dst, int dof, int count, const long long* srcOff, const int* ns,
							  const long long* dstOff, const int* nd, double maxErr, int backwards, int* dev_pairs, double* dev_fit) {
	CHECK_CTX(ctx);
	if (count < 0 || dof <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
	if (count == 0) return BHIP_OK;
	if (!srcOff || !ns || !dstOff || !nd) return bhip_fail(ctx, BHIP_ERR_INVALID, "null problem table");
	if (dof == 64 && !assocExactOnly(ctx)) {
		int used = 0;
		BHIP_TRY(bhip_assoc_l2_mfma_batched(ctx, scratchOf(ctx)->mfma, dev_src, dev_dst, count, srcOff, ns, dstOff, nd, maxErr, backwards, dev_pairs,
											dev_fit, &used));
		if (used) return BHIP_OK;
	}
	for (int p = 0; p < count; p++) {
		if (ns[p] < 0 || nd[p] < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
		if (ns[p] == 0) continue;
		BHIP_TRY(assocL2Exact(ctx, dev_src + srcOff[p] * dof, ns[p], dev_dst + dstOff[p] * dof, nd[p], dof, maxErr, backwards, 0, dev_pairs + srcOff[p],
							  dev_fit + srcOff[p]));
	}
	return BHIP_OK;
}


// AssociateDescription over descriptors that are still resident from the last detect of `s` (FastQueue<BrightFeature> lists a provider
// recognises as its own): problem p associates image srcImage[p] (source) with image dstImage[p] (destination) -- same rules as
// bhip_assoc_l2_f64, no descriptor upload.  pairs / fit are host arrays over the compact key-point index space of the batch: the results
// of problem p start at the exclusive prefix of the counts of srcImage[p] (every image may be a source at most once per call).
// batched device form of bhip_assoc_hamming_dev (contract of bhip_assoc_l2_dev_batched): many small problems in three launches
int bhip_assoc_hamming_dev_batched(bhip_ctx* ctx, const int32_t* dev_src, const int32_t* dev_dst, int words, int count, const long long* srcOff, const int* ns,
								   const long long* dstOff, const int* nd, double maxErr, int backwards, int* dev_pairs, double* dev_fit) {
	CHECK_CTX(ctx);
	if (count < 0 || words <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
	if (count == 0) return BHIP_OK;
	if (!srcOff || !ns || !dstOff || !nd || !dev_pairs || !dev_fit) return bhip_fail(ctx, BHIP_ERR_INVALID, "null problem table");
	return bhip_assoc_hamming_batched(ctx, dev_src, dev_dst, words, count, srcOff, ns, dstOff, nd, maxErr, backwards, dev_pairs, dev_fit, scratchOf(ctx)->work);
}

// AssociateDescription<TupleDesc_B>.associate() with ScoreAssociateHamming_B on the words still resident from the last detect of a BRIEF
// object: same contract as bhip_assoc_l2_surf, same rules and results as bhip_assoc_hamming, no descriptor upload.
int bhip_assoc_hamming_surf(bhip_surf* s, int count, const int* srcImage, const int* dstImage, double maxErr, int backwards, int* pairs, double* fit) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "not a BRIEF detect+describe object");
	const int32_t* W = s->wordsBuf.as<int32_t>();
	return assocSurf(s, count, srcImage, dstImage, pairs, fit, [&](const long long* so, const int* ns, const long long* doff, const int* nd, int* dp, double* df) {
		return bhip_assoc_hamming_batched(ctx, W, W, s->briefWords, count, so, ns, doff, nd, maxErr, backwards, dp, df, scratchOf(ctx)->work);
	});
}

int bhip_assoc_l2_surf(bhip_surf* s, int count, const int* srcImage, const int* dstImage, double maxErr, int backwards, int* pairs, double* fit) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "this object describes with BRIEF: use bhip_assoc_hamming_surf");
	const double* D = s->descBuf.as<double>();
	return assocSurf(s, count, srcImage, dstImage, pairs, fit, [&](const long long* so, const int* ns, const long long* doff, const int* nd, int* dp, double* df) {
		return bhip_assoc_l2_dev_batched(ctx, D, D, s->dofOut(), count, so, ns, doff, nd, maxErr, backwards, dp, df);
	});
}

}  // extern "C"

template <class E>
static int assocHost(bhip_ctx* ctx, bool hamming, const E* src, int ns, const E* dst, int nd, int len, double maxErr, int backwards, int sqrtScore,
					 int* pairs, double* fit) {
	if (ns < 0 || nd < 0 || len <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
	if (ns == 0) return BHIP_OK;
	if (!src || (nd > 0 && !dst) || !pairs || !fit) return bhip_fail(ctx, BHIP_ERR_INVALID, "null buffer");
	CtxScratch* sc = scratchOf(ctx);
	BHIP_TRY(sc->in0.reserve(ctx, (size_t)ns * len * sizeof(E)));
	BHIP_TRY(sc->in1.reserve(ctx, (size_t)std::max(nd, 1) * len * sizeof(E)));
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)ns * 4));
	BHIP_TRY(sc->out1.reserve(ctx, (size_t)ns * 8));
	BHIP_HIP(ctx, hipMemcpyAsync(sc->in0.p, src, (size_t)ns * len * sizeof(E), hipMemcpyHostToDevice, ctx->stream));
	if (nd > 0) BHIP_HIP(ctx, hipMemcpyAsync(sc->in1.p, dst, (size_t)nd * len * sizeof(E), hipMemcpyHostToDevice, ctx->stream));
	if (hamming) BHIP_TRY(bhip_assoc_hamming_dev(ctx, sc->in0.as<int32_t>(), ns, sc->in1.as<int32_t>(), nd, len, maxErr, backwards, sc->out0.as<int>(), sc->out1.as<double>()));
	else BHIP_TRY(bhip_assoc_l2_dev(ctx, sc->in0.as<double>(), ns, sc->in1.as<double>(), nd, len, maxErr, backwards, sqrtScore, sc->out0.as<int>(), sc->out1.as<double>()));
	BHIP_HIP(ctx, hipMemcpyAsync(pairs, sc->out0.p, (size_t)ns * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(fit, sc->out1.p, (size_t)ns * 8, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}

extern "C" {

int bhip_assoc_l2_f64(bhip_ctx* ctx, const double* src, int ns, const double* dst, int nd, int dof, double maxErr, int backwards, int sqrtScore,
					  int* pairs, double* fit) {
	CHECK_CTX(ctx);
	return assocHost<double>(ctx, false, src, ns, dst, nd, dof, maxErr, backwards, sqrtScore, pairs, fit);
}
int bhip_assoc_hamming(bhip_ctx* ctx, const int32_t* src, int ns, const int32_t* dst, int nd, int words, double maxErr, int backwards, int* pairs,
					   double* fit) {
	CHECK_CTX(ctx);
	return assocHost<int32_t>(ctx, true, src, ns, dst, nd, words, maxErr, backwards, 0, pairs, fit);
}

int bhip_assoc_l2_shard_phase1(bhip_ctx* ctx, const double* dev_src, int nsLocal, int srcBegin, const double* dev_dst, int nd, int dof, double maxErr,
							   int* dev_pairs, double* dev_fit, void* dev_colTop) {
	CHECK_CTX(ctx);
	if (!dev_colTop) return bhip_fail(ctx, BHIP_ERR_INVALID, "null column buffer");
	return bhip_assoc_phase1_l2(ctx, dev_src, nsLocal, srcBegin, dev_dst, nd, dof, maxErr, 0, dev_pairs, dev_fit, dev_colTop, scratchOf(ctx)->work);
}
int bhip_assoc_hamming_shard_phase1(bhip_ctx* ctx, const int32_t* dev_src, int nsLocal, int srcBegin, const int32_t* dev_dst, int nd, int words,
									double maxErr, int* dev_pairs, double* dev_fit, void* dev_colTop) {
	CHECK_CTX(ctx);
	if (!dev_colTop) return bhip_fail(ctx, BHIP_ERR_INVALID, "null column buffer");
	return bhip_assoc_phase1_ham(ctx, dev_src, nsLocal, srcBegin, dev_dst, nd, words, maxErr, dev_pairs, dev_fit, dev_colTop, scratchOf(ctx)->work);
}
int bhip_assoc_shard_phase2(bhip_ctx* ctx, const void* dev_colTopAll, int nranks, int nd, int nsLocal, int srcBegin, int* dev_pairs, double* dev_fit) {
	CHECK_CTX(ctx);
	if (nranks < 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "nranks < 1");
	return bhip_assoc_phase2(ctx, dev_colTopAll, nranks, nd, nsLocal, srcBegin, dev_pairs, dev_fit);
}

// ---------------------------------------------------------------------------------------------------------------
// boofcv-ip front end.  Most operations have a host-buffer export (the caller's image view) and a device-batched _dev export (BASELINE
// config 5: pyramid -> gradient -> NMS -> SURF on a 4K stream without leaving HBM).  Both run one implementation -- an ip.hip launcher or
// an xxxImpl around several -- on DevImg views of device images, asynchronous on the ctx stream.  The _dev export wraps the caller's
// pointers into views and calls it after its argument checks.  The host export checks its HostImg views, stages them (stageIn / hostInOut:
// rows pitch4(width) apart where the tiled kernels apply, dense otherwise), calls it with batch 1, downloads and synchronizes; when the
// implementation fails, nothing is downloaded.
// ---------------------------------------------------------------------------------------------------------------
}  // extern "C"

// BlurImageOps.gaussian: one fused pass, or a horizontal pass into the library's `storage` and a vertical pass into `out`
static int gaussianImpl(bhip_ctx* ctx, double sigma, int radius, DevImg<const float> in, DevImg<float> out) {
	std::vector<float> k = bhip_gaussian1d_f32(sigma, radius);
	const int kw = (int)k.size(), koff = kw / 2;
	bool fused = false;
	BHIP_TRY(bhip_launch_blur_fused(ctx, k.data(), kw, in, out, &fused));
	if (fused) return BHIP_OK;
	const int pitch = pitch4(in.width);
	DevBuf& buf = scratchOf(ctx)->ipTmp;
	BHIP_TRY(buf.reserve(ctx, (size_t)pitch * in.height * 4 * in.batch));
	const DevImg<float> tmp = bhip_img_over<float>(buf, pitch, in.width, in.height, in.batch);
	BHIP_TRY(bhip_launch_conv(ctx, false, true, k.data(), kw, koff, in, tmp));
	return bhip_launch_conv(ctx, true, true, k.data(), kw, koff, tmp, out);
}

// GradientCornerIntensity.process (FactoryIntensityPointAlg.shiTomasi / harris) on GrayF32 or GrayS16 derivatives (T): box window
// (ImplSsdCornerBox, ImplSsdCorner_S16) or Gaussian-weighted window (ImplSsdCornerWeighted_F32 / _S16)
template <class T>
static int cornerImpl(bhip_ctx* ctx, bool weighted, int kind, int radius, float kappa, DevImg<const T> dx, DevImg<const T> dy, DevImg<float> intensity) {
	if (weighted) return bhip_launch_corner_weighted(ctx, kind, radius, kappa, dx, dy, intensity);
	const int width = dx.width, height = dx.height, batch = dx.batch;
	DevBuf& tmp = scratchOf(ctx)->ipTmp;
	if constexpr (std::is_same_v<T, int16_t>) {
		if (radius >= 0 && 2 * radius + 1 <= width && 2 * radius + 1 <= height) {
			const size_t bytes = bhip_corner_box_s16_scratch(radius, width, height, batch);
			if (bytes) BHIP_TRY(tmp.reserve(ctx, bytes));
		}
		return bhip_launch_corner_box_s16(ctx, kind, radius, kappa, dx, dy, intensity, tmp.p);
	} else {
		BHIP_TRY(tmp.reserve(ctx, (size_t)width * height * 4 * 3 * batch));
		// ImageMiscOps.fillBorder(intensity, 0, radius): clear every image, the interior is overwritten
		for (int b = 0; b < batch; b++)
			BHIP_HIP(ctx, hipMemset2DAsync(intensity.data + b * intensity.imageStride, (size_t)intensity.stride * 4, 0, (size_t)width * 4, (size_t)height, ctx->stream));
		return bhip_launch_corner_intensity(ctx, kind, radius, kappa, dx, dy, intensity, tmp.as<float>());
	}
}

// DescribePointBrief.process: the points of image b are xy[start[b] .. start[b+1]) (host prefix, batch+1 entries, at most maxCount per
// image), or with start == nullptr the n points of one image; words of point p at out[p * ceil(numPoints/32)].  The first nSample sample
// points are uploaded and decide between the LDS-patch and the gather kernel.
template <class T>
static int briefImpl(bhip_ctx* ctx, DevImg<const T> img, int radius, int numPoints, const int32_t* samplePoints, int nSample, const int32_t* compare,
					 const double* xy, const int* start, int n, int maxCount, int32_t* out) {
	const size_t nS = (size_t)nSample * 2, nC = (size_t)numPoints * 2;
	DevBuf& tab = scratchOf(ctx)->ipKernel;
	BHIP_TRY(tab.reserve(ctx, (nS + nC + (start ? img.batch + 1 : 0)) * 4));
	int* dSample = tab.as<int>();
	int* dCompare = dSample + nS;
	int* dStart = start ? dCompare + nC : nullptr;
	BHIP_HIP(ctx, hipMemcpyAsync(dSample, samplePoints, nS * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(dCompare, compare, nC * 4, hipMemcpyHostToDevice, ctx->stream));
	if (start) BHIP_HIP(ctx, hipMemcpyAsync(dStart, start, (size_t)(img.batch + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
	return bhip_launch_brief(ctx, img, radius, numPoints, dSample, dCompare, xy, n, out, dStart, maxCount, 2, 0, briefPatchOk(samplePoints, nSample, radius));
}

static bool gradBorderOk(int kind, int border) { return border == 0 || border == 1 || (border == 2 && kind == 0); }   // 2 = BorderType.EXTENDED: GradientSobel only

// host forms: GrayF32 gradients re-pitch rows to pitch4 (the streaming kernels), GrayU8 ones stay dense; without a border policy the frame
// keeps the caller's values, so dx and dy are staged too
template <class TI, class TO>
static int gradHost(bhip_ctx* ctx, int kind, HostImg<const TI> in, HostImg<TO> dx, HostImg<TO> dy, int border) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, dx);
	CHECK_IMG(ctx, dy);
	if (!gradBorderOk(kind, border)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "border policy not supported on the GPU");
	CtxScratch* sc = scratchOf(ctx);
	const int pitch = sizeof(TI) == 4 ? pitch4(in.width) : in.width;
	DevImg<TI> din;
	DevImg<TO> ddx, ddy;
	BHIP_TRY(stageIn(ctx, sc->in0, in, pitch, din));
	BHIP_TRY(stageIn(ctx, sc->out0, dx, pitch, ddx));
	BHIP_TRY(stageIn(ctx, sc->out1, dy, pitch, ddy));
	BHIP_TRY(bhip_launch_gradient(ctx, kind, din, ddx, ddy, border));
	BHIP_TRY(stageOut(ctx, dx, ddx));
	BHIP_TRY(stageOut(ctx, dy, ddy));
	return bhip_ctx_synchronize(ctx);
}
template <class TI, class TO>
static int gradDev(bhip_ctx* ctx, int kind, DevImg<const TI> in, DevImg<TO> dx, DevImg<TO> dy, int border) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, dx);
	CHECK_IMG(ctx, dy);
	if (!gradBorderOk(kind, border)) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "border policy not supported on the GPU");
	return bhip_launch_gradient(ctx, kind, in, dx, dy, border);
}

// host forms of the corner intensity: dense derivatives (T = float or int16_t)
template <class T>
static int cornerHost(bhip_ctx* ctx, bool weighted, int kind, int radius, float kappa, HostImg<const T> dx, HostImg<const T> dy, HostImg<float> intensity) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, dx);
	CHECK_IMG(ctx, dy);
	CHECK_IMG(ctx, intensity);
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> ddx, ddy;
	DevImg<float> dout;
	BHIP_TRY(stageIn(ctx, sc->in0, dx, dx.width, ddx));
	BHIP_TRY(stageIn(ctx, sc->in1, dy, dx.width, ddy));
	BHIP_TRY(stageIn(ctx, sc->out0, intensity, dx.width, dout, false));
	BHIP_TRY(cornerImpl<T>(ctx, weighted, kind, radius, kappa, ddx, ddy, dout));
	BHIP_TRY(stageOut(ctx, intensity, dout));
	return bhip_ctx_synchronize(ctx);
}
template <class T>
static int cornerDev(bhip_ctx* ctx, bool weighted, int kind, int radius, float kappa, DevImg<const T> dx, DevImg<const T> dy, DevImg<float> intensity) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, dx);
	CHECK_IMG(ctx, dy);
	CHECK_IMG(ctx, intensity);
	return cornerImpl<T>(ctx, weighted, kind, radius, kappa, dx, dy, intensity);
}

// bhip_brief_f32 / bhip_brief_u8 after their checks: the view staged dense, the n points as given
template <class T>
static int briefHost(bhip_ctx* ctx, HostImg<const T> img, int radius, int numPoints, const int32_t* samplePoints, int nSample, const int32_t* compare,
					 const double* xy, int n, int32_t* out) {
	CtxScratch* sc = scratchOf(ctx);
	const size_t words = (numPoints + 31) / 32;
	DevImg<T> dimg;
	BHIP_TRY(stageIn(ctx, sc->in0, img, img.width, dimg));
	BHIP_TRY(sc->in1.reserve(ctx, (size_t)n * 16));
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)n * words * 4));
	BHIP_HIP(ctx, hipMemcpyAsync(sc->in1.p, xy, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
	BHIP_TRY(briefImpl<T>(ctx, dimg, radius, numPoints, samplePoints, nSample, compare, sc->in1.as<double>(), nullptr, n, 0, sc->out0.as<int32_t>()));
	BHIP_HIP(ctx, hipMemcpyAsync(out, sc->out0.p, (size_t)n * words * 4, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

static int convHost(bhip_ctx* ctx, bool vertical, bool normalized, const float* kernel, int kw, int koff, HostImg<const float> in, HostImg<float> out) {
	// the no-border variants leave the frame of `out` untouched: it starts from the caller's pixels
	return hostInOut<float, float>(ctx, in, out, true, true, kernel ? nullptr : "null kernel",
								   [&](auto din, auto dout) { return bhip_launch_conv(ctx, vertical, normalized, kernel, kw, koff, din, dout); });
}
static int convDev(bhip_ctx* ctx, bool vertical, bool normalized, const float* kernel, int kw, int koff, DevImg<const float> in, DevImg<float> out) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	if (!kernel) return bhip_fail(ctx, BHIP_ERR_INVALID, "null kernel");
	return bhip_launch_conv(ctx, vertical, normalized, kernel, kw, koff, in, out);
}

// ConvolveImageDownNormalized on a host view: Kernel1D_F32 on GrayF32 or Kernel1D_S32 on GrayU8, dense on the device; pixels the reference
// does not write keep the caller's values
template <class K, class T>
static int convDownHost(bhip_ctx* ctx, bool vertical, const K* kernel, int kw, HostImg<const T> in, HostImg<T> out, int skip) {
	return hostInOut<T, T>(ctx, in, out, false, true, kernel ? nullptr : "null kernel",
						   [&](auto din, auto dout) { return bhip_launch_conv_down(ctx, vertical, kernel, kw, din, dout, skip); });
}

// PyramidDiscreteSampleBlur<T>.process on `batch` device frames: GrayF32 with a Kernel1D_F32, GrayU8 with a Kernel1D_S32; `out` holds the
// layers of frame b from out + b * total (bhip_pyramid_layout).  The two pixel types differ where PyrTraits says so and nowhere else.
// layer0Present (GrayU8 only): the caller has already put the frames into layer 0 (scale[0] == 1), so no copy is made.
template <class T> struct PyrTraits;
template <> struct PyrTraits<float> {
	using Kernel = float;
	static constexpr bool fusedLayer = true;    // bhip_launch_pyr_layer_fused is tried before the two passes
	static constexpr bool clearLayer0 = true;   // the whole output is cleared, layer 0 at scale 1 included
	static constexpr const char* copyTag = "pyramid_copy";
	static constexpr double copyBytes = 8.0;    // per pixel
};
template <> struct PyrTraits<uint8_t> {
	using Kernel = int32_t;
	static constexpr bool fusedLayer = false;
	static constexpr bool clearLayer0 = false;  // layer 0 at scale 1 is written (or already there) as a whole
	static constexpr const char* copyTag = "pyramid_copy_u8";
	static constexpr double copyBytes = 2.0;
};
template <class T>
static int pyramidImpl(bhip_ctx* ctx, const typename PyrTraits<T>::Kernel* kernel, int kw, const int* scales, int n, DevImg<const T> in, T* out,
					   bool layer0Present = false) {
	using Tr = PyrTraits<T>;
	const int width = in.width, height = in.height, batch = in.batch;
	if (n > 32) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 32 layers");
	int dims[64];
	long long offs[32], total = 0;
	if (bhip_pyramid_layout(width, height, scales, n, dims, offs, &total) != BHIP_OK) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad pyramid scales");
	for (int i = 1; i < n; i++)
		if (scales[i] / scales[i - 1] <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Skip must be >= 1");
	CtxScratch* sc = scratchOf(ctx);
	const bool copy0 = scales[0] == 1;
	// freshly created layers are zero (pixels outside floor(prev/skip) are never written)
	if (Tr::clearLayer0) {
		BHIP_HIP(ctx, hipMemsetAsync(out, 0, (size_t)total * batch * sizeof(T), ctx->stream));
	} else {
		const long long clearFrom = copy0 ? (n > 1 ? offs[1] : total) : 0;
		if (total > clearFrom)
			BHIP_HIP(ctx, hipMemset2DAsync(out + clearFrom, (size_t)total * sizeof(T), 0, (size_t)(total - clearFrom) * sizeof(T), (size_t)batch, ctx->stream));
	}
	// `temp` of the reference is one grow-only image shared by all layers: zero when first allocated, afterwards it keeps the
	// previous layer's values wherever the off-grid skip>=3 case leaves a column unwritten.  Same here: one dense region per
	// frame, sized for the first convolved layer, cleared once per call (= first process() of a fresh pyramid object).
	long long tempCap = 0;
	{
		int pw0 = width, ph0 = height;
		for (int i = 0; i < n; i++) {
			if (!(i == 0 && copy0)) {
				const int skip = i == 0 ? scales[0] : scales[i] / scales[i - 1];
				tempCap = std::max(tempCap, (long long)(pw0 / skip) * ph0);
			}
			pw0 = dims[2 * i]; ph0 = dims[2 * i + 1];
		}
	}
	if (tempCap > 0) {
		BHIP_TRY(sc->ipTmp.reserve(ctx, (size_t)tempCap * sizeof(T) * batch));
		BHIP_HIP(ctx, hipMemsetAsync(sc->ipTmp.p, 0, (size_t)tempCap * sizeof(T) * batch, ctx->stream));
	}
	DevImg<const T> prev = in;
	for (int i = 0; i < n; i++) {
		const DevImg<T> layer = bhip_pyr_layer(out, total, dims, offs, i, batch);
		if (i == 0 && copy0) {
			if (!layer0Present) {
				ProfScope prof(ctx, Tr::copyTag, Tr::copyBytes * width * height * batch);
				BHIP_TRY(bhip_launch_copy_images(ctx, in, layer));
			}
		} else {
			const int skip = i == 0 ? scales[0] : scales[i] / scales[i - 1];
			const int tw = prev.width / skip;   // 0 when the layer below is narrower than the step: both passes then write nothing and the (ceil-sized) layer stays zero, as in the reference
			bool fused = false;
			if constexpr (Tr::fusedLayer) BHIP_TRY(bhip_launch_pyr_layer_fused(ctx, kernel, kw, prev, layer, skip, &fused));
			if (!fused) {
				const DevImg<T> tmp{sc->ipTmp.as<T>(), tempCap, tw, tw, prev.height, batch};
				BHIP_TRY(bhip_launch_conv_down(ctx, false, kernel, kw, prev, tmp, skip));
				BHIP_TRY(bhip_launch_conv_down(ctx, true, kernel, kw, tmp, layer, skip));
			}
		}
		prev = layer;
	}
	return BHIP_OK;
}

// host pyramid: the view staged dense, all layers downloaded as one block
template <class T>
static int pyramidHost(bhip_ctx* ctx, const typename PyrTraits<T>::Kernel* kernel, int kw, const int* scales, int n, HostImg<const T> in, T* out) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	if (!out || !kernel || !scales) return bhip_fail(ctx, BHIP_ERR_INVALID, "null buffer");
	long long total = 0;
	if (bhip_pyramid_layout(in.width, in.height, scales, n, nullptr, nullptr, &total) != BHIP_OK) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad pyramid scales");
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> din;
	BHIP_TRY(stageIn(ctx, sc->in0, in, in.width, din));
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)total * sizeof(T)));
	BHIP_TRY(pyramidImpl<T>(ctx, kernel, kw, scales, n, din, sc->out0.as<T>()));
	BHIP_HIP(ctx, hipMemcpyAsync(out, sc->out0.p, (size_t)total * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

extern "C" {

int bhip_conv_h_f32(bhip_ctx* ctx, const float* kernel, int kw, int koff, const float* in, int inStart, int inStride, int width, int height, float* out,
					int outStart, int outStride) {
	return convHost(ctx, false, false, kernel, kw, koff, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height});
}
int bhip_conv_v_f32(bhip_ctx* ctx, const float* kernel, int kw, int koff, const float* in, int inStart, int inStride, int width, int height, float* out,
					int outStart, int outStride) {
	return convHost(ctx, true, false, kernel, kw, koff, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height});
}
int bhip_conv_norm_h_f32(bhip_ctx* ctx, const float* kernel, int kw, int koff, const float* in, int inStart, int inStride, int width, int height,
						 float* out, int outStart, int outStride) {
	return convHost(ctx, false, true, kernel, kw, koff, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height});
}
int bhip_conv_norm_v_f32(bhip_ctx* ctx, const float* kernel, int kw, int koff, const float* in, int inStart, int inStride, int width, int height,
						 float* out, int outStart, int outStride) {
	return convHost(ctx, true, true, kernel, kw, koff, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height});
}

int bhip_gaussian_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, double sigma, int radius, float* out,
					  int outStart, int outStride) {
	return hostInOut<float, float>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, true, false,
								   sigma <= 0 && radius <= 0 ? "Sigma must be > 0" : nullptr, [&](auto din, auto dout) { return gaussianImpl(ctx, sigma, radius, din, dout); });
}

int bhip_conv_down_norm_h_f32(bhip_ctx* ctx, const float* kernel, int kw, const float* in, int inStart, int inStride, int width, int height, float* out,
							  int outStart, int outStride, int outWidth, int outHeight, int skip) {
	return convDownHost<float, float>(ctx, false, kernel, kw, {in, inStart, inStride, width, height}, {out, outStart, outStride, outWidth, outHeight}, skip);
}
int bhip_conv_down_norm_v_f32(bhip_ctx* ctx, const float* kernel, int kw, const float* in, int inStart, int inStride, int width, int height, float* out,
							  int outStart, int outStride, int outWidth, int outHeight, int skip) {
	return convDownHost<float, float>(ctx, true, kernel, kw, {in, inStart, inStride, width, height}, {out, outStart, outStride, outWidth, outHeight}, skip);
}
int bhip_conv_down_norm_h_u8(bhip_ctx* ctx, const int32_t* kernel, int kw, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out,
							 int outStart, int outStride, int outWidth, int outHeight, int skip) {
	return convDownHost<int32_t, uint8_t>(ctx, false, kernel, kw, {in, inStart, inStride, width, height}, {out, outStart, outStride, outWidth, outHeight}, skip);
}
int bhip_conv_down_norm_v_u8(bhip_ctx* ctx, const int32_t* kernel, int kw, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out,
							 int outStart, int outStride, int outWidth, int outHeight, int skip) {
	return convDownHost<int32_t, uint8_t>(ctx, true, kernel, kw, {in, inStart, inStride, width, height}, {out, outStart, outStride, outWidth, outHeight}, skip);
}

// FactoryKernelGaussian.gaussian(Kernel1D_F32.class, sigma, radius) (I:factory/filter/kernel/FactoryKernelGaussian.java:120-153)
int bhip_gaussian_kernel1d_f32(double sigma, int radius, float* out, int capacity) {
	if (sigma <= 0 && radius <= 0) return -1;
	std::vector<float> k = bhip_gaussian1d_f32(sigma, radius);
	if (!out || (int)k.size() > capacity) return -(int)k.size();
	for (size_t i = 0; i < k.size(); i++) out[i] = k[i];
	return (int)k.size();
}

int bhip_pyramid_dev_f32(bhip_ctx* ctx, const float* kernel, int kw, const int* scales, int n, const float* dev_in, long long inImageStride, int inStride,
						 int width, int height, int batch, float* dev_out) {
	CHECK_CTX(ctx);
	if (!kernel || !dev_in || !dev_out || batch <= 0 || inStride < width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad pyramid arguments");
	return pyramidImpl<float>(ctx, kernel, kw, scales, n, {dev_in, inImageStride, inStride, width, height, batch}, dev_out);
}
int bhip_pyramid_dev_u8(bhip_ctx* ctx, const int32_t* kernel, int kw, const int* scales, int n, const uint8_t* dev_in, long long inImageStride, int inStride,
						int width, int height, int batch, uint8_t* dev_out) {
	CHECK_CTX(ctx);
	if (!kernel || !scales || !dev_in || !dev_out || batch <= 0 || width <= 0 || height <= 0 || inStride < width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad pyramid arguments");
	return pyramidImpl<uint8_t>(ctx, kernel, kw, scales, n, {dev_in, inImageStride, inStride, width, height, batch}, dev_out);
}
int bhip_pyramid_u8(bhip_ctx* ctx, const int32_t* kernel, int kw, const int* scales, int n, const uint8_t* in, int inStart, int inStride, int width, int height,
					uint8_t* out) {
	return pyramidHost<uint8_t>(ctx, kernel, kw, scales, n, {in, inStart, inStride, width, height}, out);
}
int bhip_pyramid_f32(bhip_ctx* ctx, const float* kernel, int kw, const int* scales, int n, const float* in, int inStart, int inStride, int width,
					 int height, float* out) {
	return pyramidHost<float>(ctx, kernel, kw, scales, n, {in, inStart, inStride, width, height}, out);
}

// PyramidDiscreteSampleBlur: layer geometry (ImagePyramidBase.initialize) + scale checks (ImagePyramidBase.checkScales)
int bhip_pyramid_layout(int width, int height, const int* scales, int n, int* dims, long long* offsets, long long* totalFloats) {
	if (width <= 0 || height <= 0 || !scales || n <= 0) return BHIP_ERR_INVALID;
	if (scales[0] <= 0) return BHIP_ERR_INVALID;
	int prev = 0;
	long long off = 0;
	for (int i = 0; i < n; i++) {
		if (scales[i] < prev) return BHIP_ERR_INVALID;
		prev = scales[i];
		const double sf = scales[i];
		int w = (int)std::ceil(width / sf), h = (int)std::ceil(height / sf);
		if (i == 0 && scales[0] == 1) { w = width; h = height; }
		if (dims) { dims[2 * i] = w; dims[2 * i + 1] = h; }
		if (offsets) offsets[i] = off;
		off += (long long)w * h;
	}
	if (totalFloats) *totalFloats = off;
	return BHIP_OK;
}

int bhip_conv2d_f32(bhip_ctx* ctx, const float* kernel, int kw, int koff, const float* in, int inStart, int inStride, int width, int height, float* out,
					int outStart, int outStride) {
	// the frame keeps the caller's pixels
	return hostInOut<float, float>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, false, true, kernel ? nullptr : "null kernel",
								   [&](auto din, auto dout) { return bhip_launch_conv2d(ctx, kernel, kw, koff, din, dout); });
}
int bhip_mean_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, int radiusX, int radiusY, float* out, int outStart,
				  int outStride) {
	return hostInOut<float, float>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, false, false,
								   radiusX <= 0 || radiusY <= 0 ? "Radius must be > 0" : nullptr, [&](auto din, DevImg<float> dout) {
		DevBuf& buf = scratchOf(ctx)->tmp0;   // the horizontal pass's result
		BHIP_TRY(buf.reserve(ctx, (size_t)width * height * 4));
		const DevImg<float> dtmp = bhip_img_over<float>(buf, width, width, height, 1);
		BHIP_TRY(bhip_launch_mean(ctx, false, din, dtmp, radiusX));
		return bhip_launch_mean(ctx, true, dtmp, dout, radiusY);
	});
}
int bhip_median_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, int radius, float* out, int outStart, int outStride) {
	return hostInOut<float, float>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, false, false,
								   radius <= 0 ? "Radius must be > 0" : nullptr, [&](auto din, auto dout) { return bhip_launch_median(ctx, din, dout, radius); });
}

int bhip_sobel_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, float* dx, float* dy, int outStart, int outStride,
				   int border) {
	return gradHost<float, float>(ctx, 0, {in, inStart, inStride, width, height}, {dx, outStart, outStride, width, height}, {dy, outStart, outStride, width, height}, border);
}
int bhip_three_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, float* dx, float* dy, int outStart, int outStride,
				   int border) {
	return gradHost<float, float>(ctx, 1, {in, inStart, inStride, width, height}, {dx, outStart, outStride, width, height}, {dy, outStart, outStride, width, height}, border);
}
int bhip_sobel_u8_s16(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int16_t* dx, int16_t* dy, int outStart,
					  int outStride, int border) {
	return gradHost<uint8_t, int16_t>(ctx, 0, {in, inStart, inStride, width, height}, {dx, outStart, outStride, width, height}, {dy, outStart, outStride, width, height}, border);
}
int bhip_three_u8_s16(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int16_t* dx, int16_t* dy, int outStart,
					  int outStride, int border) {
	return gradHost<uint8_t, int16_t>(ctx, 1, {in, inStart, inStride, width, height}, {dx, outStart, outStride, width, height}, {dy, outStart, outStride, width, height}, border);
}

int bhip_corner_intensity_f32(bhip_ctx* ctx, int kind, int radius, float kappa, const float* derivX, const float* derivY, int dStart, int dStride, int width,
							  int height, float* intensity, int iStart, int iStride) {
	return cornerHost<float>(ctx, false, kind, radius, kappa, {derivX, dStart, dStride, width, height}, {derivY, dStart, dStride, width, height},
							 {intensity, iStart, iStride, width, height});
}
int bhip_corner_intensity_s16(bhip_ctx* ctx, int kind, int radius, float kappa, int weighted, const int16_t* derivX, const int16_t* derivY, int dStart,
							  int dStride, int width, int height, float* intensity, int iStart, int iStride) {
	return cornerHost<int16_t>(ctx, weighted != 0, kind, radius, kappa, {derivX, dStart, dStride, width, height}, {derivY, dStart, dStride, width, height},
							   {intensity, iStart, iStride, width, height});
}
int bhip_corner_intensity_weighted_f32(bhip_ctx* ctx, int kind, int radius, float kappa, const float* derivX, const float* derivY, int dStart, int dStride,
									   int width, int height, float* intensity, int iStart, int iStride) {
	return cornerHost<float>(ctx, true, kind, radius, kappa, {derivX, dStart, dStride, width, height}, {derivY, dStart, dStride, width, height},
							 {intensity, iStart, iStride, width, height});
}
int bhip_gaussian_kernel1d_s32(int radius, int32_t* out, int capacity) {
	if (radius <= 0) return -1;
	std::vector<int32_t> k = bhip_gaussian1d_s32(radius);
	if (!out || (int)k.size() > capacity) return -(int)k.size();
	for (size_t i = 0; i < k.size(); i++) out[i] = k[i];
	return (int)k.size();
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

// The BRIEF exports differ in what they accept (not harmonised): bhip_brief_f32 rejects a pair index >= numPoints and decides the kernel over
// numPoints sample points; bhip_brief_u8 and bhip_brief_dev_f32 accept any non-negative index and use maxIdx + 1 points.
int bhip_brief_u8(bhip_ctx* ctx, const uint8_t* img, int start, int stride, int width, int height, int radius, int numPoints, const int32_t* samplePoints,
				  const int32_t* compare, const double* xy, int n, int32_t* out) {
	const HostImg<const uint8_t> himg{img, start, stride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, himg);
	if (numPoints <= 0 || !samplePoints || !compare || n < 0 || (n > 0 && (!xy || !out))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad BRIEF arguments");
	if (n == 0) return BHIP_OK;
	int maxIdx = 0;
	for (int i = 0; i < 2 * numPoints; i++) { if (compare[i] < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "negative sample index"); maxIdx = std::max(maxIdx, compare[i]); }
	return briefHost(ctx, himg, radius, numPoints, samplePoints, maxIdx + 1, compare, xy, n, out);
}

int bhip_brief_f32(bhip_ctx* ctx, const float* img, int start, int stride, int width, int height, int radius, int numPoints,
				   const int32_t* samplePoints, const int32_t* compare, const double* xy, int n, int32_t* out) {
	const HostImg<const float> himg{img, start, stride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, himg);
	if (numPoints <= 0 || !samplePoints || !compare || n < 0 || (n > 0 && (!xy || !out))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad BRIEF arguments");
	if (n == 0) return BHIP_OK;
	for (int i = 0; i < 2 * numPoints; i++)
		if (compare[i] < 0 || compare[i] >= numPoints) return bhip_fail(ctx, BHIP_ERR_INVALID, "pair index outside the sample point list");
	return briefHost(ctx, himg, radius, numPoints, samplePoints, numPoints, compare, xy, n, out);
}

// ---- device-batched forms ----
int bhip_conv_h_dev_f32(bhip_ctx* ctx, const float* kernel, int kw, int koff, const float* dev_in, long long inImageStride, int inStride, int width, int height,
						int batch, float* dev_out, long long outImageStride, int outStride) {
	return convDev(ctx, false, false, kernel, kw, koff, {dev_in, inImageStride, inStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_conv_v_dev_f32(bhip_ctx* ctx, const float* kernel, int kw, int koff, const float* dev_in, long long inImageStride, int inStride, int width, int height,
						int batch, float* dev_out, long long outImageStride, int outStride) {
	return convDev(ctx, true, false, kernel, kw, koff, {dev_in, inImageStride, inStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_conv_norm_h_dev_f32(bhip_ctx* ctx, const float* kernel, int kw, int koff, const float* dev_in, long long inImageStride, int inStride, int width,
							 int height, int batch, float* dev_out, long long outImageStride, int outStride) {
	return convDev(ctx, false, true, kernel, kw, koff, {dev_in, inImageStride, inStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_conv_norm_v_dev_f32(bhip_ctx* ctx, const float* kernel, int kw, int koff, const float* dev_in, long long inImageStride, int inStride, int width,
							 int height, int batch, float* dev_out, long long outImageStride, int outStride) {
	return convDev(ctx, true, true, kernel, kw, koff, {dev_in, inImageStride, inStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}

int bhip_gaussian_dev_f32(bhip_ctx* ctx, const float* dev_in, long long inImageStride, int inStride, int width, int height, int batch, double sigma, int radius,
						  float* dev_out, long long outImageStride, int outStride) {
	const DevImg<const float> in{dev_in, inImageStride, inStride, width, height, batch};
	const DevImg<float> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	if (sigma <= 0 && radius <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Sigma must be > 0");
	return gaussianImpl(ctx, sigma, radius, in, out);
}

int bhip_sobel_dev_f32(bhip_ctx* ctx, const float* dev_in, long long inImageStride, int inStride, int width, int height, int batch, float* dev_dx, float* dev_dy,
					   long long outImageStride, int outStride, int border) {
	return gradDev<float, float>(ctx, 0, {dev_in, inImageStride, inStride, width, height, batch}, {dev_dx, outImageStride, outStride, width, height, batch},
								 {dev_dy, outImageStride, outStride, width, height, batch}, border);
}
int bhip_three_dev_f32(bhip_ctx* ctx, const float* dev_in, long long inImageStride, int inStride, int width, int height, int batch, float* dev_dx, float* dev_dy,
					   long long outImageStride, int outStride, int border) {
	return gradDev<float, float>(ctx, 1, {dev_in, inImageStride, inStride, width, height, batch}, {dev_dx, outImageStride, outStride, width, height, batch},
								 {dev_dy, outImageStride, outStride, width, height, batch}, border);
}
int bhip_sobel_dev_u8_s16(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int16_t* dev_dx,
						  int16_t* dev_dy, long long outImageStride, int outStride, int border) {
	return gradDev<uint8_t, int16_t>(ctx, 0, {dev_in, inImageStride, inStride, width, height, batch}, {dev_dx, outImageStride, outStride, width, height, batch},
									 {dev_dy, outImageStride, outStride, width, height, batch}, border);
}
int bhip_three_dev_u8_s16(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int16_t* dev_dx,
						  int16_t* dev_dy, long long outImageStride, int outStride, int border) {
	return gradDev<uint8_t, int16_t>(ctx, 1, {dev_in, inImageStride, inStride, width, height, batch}, {dev_dx, outImageStride, outStride, width, height, batch},
									 {dev_dy, outImageStride, outStride, width, height, batch}, border);
}

int bhip_gradient_intensity_dev_f32(bhip_ctx* ctx, int kind, const float* dev_dx, const float* dev_dy, long long dImageStride, int dStride, int width, int height,
									int batch, float* dev_out, long long outImageStride, int outStride) {
	const DevImg<const float> dx{dev_dx, dImageStride, dStride, width, height, batch}, dy{dev_dy, dImageStride, dStride, width, height, batch};
	const DevImg<float> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, dx);
	CHECK_IMG(ctx, dy);
	CHECK_IMG(ctx, out);
	return bhip_launch_grad_intensity(ctx, kind, dx, dy, out);
}

int bhip_corner_intensity_dev_f32(bhip_ctx* ctx, int kind, int radius, float kappa, const float* dev_dx, const float* dev_dy, long long dImageStride, int dStride,
								  int width, int height, int batch, float* dev_intensity, long long iImageStride, int iStride) {
	return cornerDev<float>(ctx, false, kind, radius, kappa, {dev_dx, dImageStride, dStride, width, height, batch}, {dev_dy, dImageStride, dStride, width, height, batch},
							{dev_intensity, iImageStride, iStride, width, height, batch});
}
int bhip_corner_intensity_dev_s16(bhip_ctx* ctx, int kind, int radius, float kappa, int weighted, const int16_t* dev_dx, const int16_t* dev_dy,
								  long long dImageStride, int dStride, int width, int height, int batch, float* dev_intensity, long long iImageStride, int iStride) {
	return cornerDev<int16_t>(ctx, weighted != 0, kind, radius, kappa, {dev_dx, dImageStride, dStride, width, height, batch},
							  {dev_dy, dImageStride, dStride, width, height, batch}, {dev_intensity, iImageStride, iStride, width, height, batch});
}
int bhip_corner_intensity_weighted_dev_f32(bhip_ctx* ctx, int kind, int radius, float kappa, const float* dev_dx, const float* dev_dy, long long dImageStride,
										   int dStride, int width, int height, int batch, float* dev_intensity, long long iImageStride, int iStride) {
	return cornerDev<float>(ctx, true, kind, radius, kappa, {dev_dx, dImageStride, dStride, width, height, batch}, {dev_dy, dImageStride, dStride, width, height, batch},
							{dev_intensity, iImageStride, iStride, width, height, batch});
}

// DescribePointBrief.process over a batch: the points of image b are dev_xy[start[b] .. start[b+1]) (host prefix `start`, batch+1 entries);
// words of point p at dev_out[p * ceil(numPoints/32)]
int bhip_brief_dev_f32(bhip_ctx* ctx, const float* dev_img, long long imageStride, int stride, int width, int height, int batch, int radius, int numPoints,
					   const int32_t* samplePoints, const int32_t* compare, const double* dev_xy, const int* start, int32_t* dev_out) {
	const DevImg<const float> img{dev_img, imageStride, stride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, img);
	if (numPoints <= 0 || !samplePoints || !compare || !start) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad BRIEF arguments");
	int maxCount = 0;
	for (int b = 0; b < batch; b++) {
		if (start[b + 1] < start[b]) return bhip_fail(ctx, BHIP_ERR_INVALID, "point prefix must not decrease");
		maxCount = std::max(maxCount, start[b + 1] - start[b]);
	}
	const int n = start[batch] - start[0];
	if (n == 0) return BHIP_OK;
	if (!dev_xy || !dev_out) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad BRIEF arguments");
	int maxIdx = 0;
	for (int i = 0; i < 2 * numPoints; i++) { if (compare[i] < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "negative sample index"); maxIdx = std::max(maxIdx, compare[i]); }
	BHIP_TRY(briefImpl<float>(ctx, img, radius, numPoints, samplePoints, maxIdx + 1, compare, dev_xy, start, n, maxCount, dev_out));
	return bhip_ctx_synchronize(ctx);   // the host tables were handed to async copies
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// Pyramid KLT point tracker (kernels: klt.hip)
// ---------------------------------------------------------------------------------------------------------------
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
		BHIP_TRY(k->tab.alloc(ctx, batch, 1024, numLayers, templateRadius));
		BHIP_TRY(bhip_launch_klt_init(ctx, k->tab.v, 0));
		BHIP_TRY(bhip_ctx_synchronize(ctx));
		return BHIP_OK;
	});
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

}  // extern "C"

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

// ---- stationary background models (background.hip): FactoryBackgroundModel.stationaryBasic / stationaryGaussian / stationaryGmm ----
extern "C++" {
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
}  // extern "C++"

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
