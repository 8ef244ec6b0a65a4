// What the host files of the C ABI (cabi*.hip) share: the per-context scratch, the handle registry and the children of a context, the
// argument checks, the staging of host views, and the few host functions one family calls in another.  Internal: include/boofhip.h is
// the boundary.
#pragma once
#include "common.h"
#include <cmath>
#include <cfloat>
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <unordered_set>

// internal to the library: the functions declared here link the cabi*.hip files to each other and stay out of the dynamic symbol
// table, as they did while they were static (the types have no symbols that a caller of the library could use)
#pragma GCC visibility push(hidden)

// Per-context scratch that the stateless entry points reuse (freed with the context).  The staging slots belong to the host-buffer export
// that is running: the caller's views it uploads, the results it downloads, its own working buffers.  Code on device pointers (the
// implementations behind the _dev exports, which host exports run on their staged copies) uses only the device-side slots, so nothing a
// host export calls can overwrite what it staged.
struct CtxScratch {
	DevBuf in0, in1, out0, out1, tmp0, tmp1;                                 // staging
	DevBuf work, assocCol, nmsBitmap, nmsPrefix, nmsPos, ipTmp, ipKernel, fast, disparity, distortMap, templ, flow, threshold;   // device side
	long long flowPixels = 0;   // pixels of the last bhip_flow_klt_* call (bhip_flow_klt_stats)
	DevBuf flowHs;                  // cabi_flow.hip, Horn-Schunck: [derivatives when the caller keeps none | the two ping-pong flows]
	DevBuf binary, label;           // cabi_binary.hip: the two ping-pong images of a long erode / dilate run; parent[] and row counts of the labelling
	DevBuf binaryTable;             // the host forms' relabel / labelToBinary lookup table
	DevBuf hough, houghTable;       // cabi_line.hip: vote counts / sort records of the Hough transforms; the sine / cosine and mean-shift weight tables
	DevBuf enhance;                 // cabi_enhance.hip: the histogram / transform table of the host forms
	DevBuf sift;                    // cabi_sift.hip: float frames, tempBlur, one octave's scale and DoG images, the NMS lists and candidate bitmaps
	DevBuf siftTables;              // detect + describe: [exp table | bin angles | Gaussian weight] of the config last used ...
	std::vector<char> siftTablesHost;   // ... and the host block they were copied from (uploaded again only when the config changes)
	DevBuf dense;                   // cabi_dense.hip: the fast HOG's cell histograms, or the per-pixel values of standard HOG / dense SIFT, of the frames in flight
	DevBuf denseTables[2];          // [0] standard HOG: the block's pixel weights; [1] dense SIFT: [bin angles | Gaussian weight]; of the config last used ...
	std::vector<char> denseTablesHost[2];  // ... and the host blocks they were copied from
	DevBuf thresholdTaps;         // the Kernel1D_S32 Gaussian taps of the GrayU8 blurs, for thresholdTapsRadius (0: none yet)
	int thresholdTapsRadius = 0;
	AssocMfmaWork mfma;
	int assocExactOnly = -1;  // BHIP_ASSOC_EXACT=1 forces the exact VALU association kernels (parity cross-check)
	DevBuf describeQueue;     // slot counters of the k_describe launch in flight (BHIP_DESCRIBE_QUEUE_BYTES)
};
inline CtxScratch* scratchOf(bhip_ctx* ctx);

struct bhip_ctx_full : bhip_ctx {
	CtxScratch scratch;
};
inline CtxScratch* scratchOf(bhip_ctx* ctx) { return &static_cast<bhip_ctx_full*>(ctx)->scratch; }

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
HandleRegistry& registry();   // one definition (cabi.hip): every file sees the same registry

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
void releaseDevice(X* x) {
	if (!x->ctx) return;   // the context went first
	(void)hipSetDevice(x->ctx->device);
	(void)hipStreamSynchronize(x->ctx->stream);
	x->onRelease();
	static_cast<typename X::Device&>(*x) = typename X::Device();
	x->ctx = nullptr;
}
template <class X>
void orphanIfOn(void* child, bhip_ctx* ctx) {
	if (static_cast<X*>(child)->ctx == ctx) releaseDevice(static_cast<X*>(child));
}
// The create call of a child: holds the registry lock from the context's liveness check to the insert, so a concurrent bhip_ctx_destroy
// waits for it.  build(std::unique_ptr<X>&) does the type's own argument checks (a null `out` among them) and the construction.
template <class X, class Build>
int createChild(bhip_ctx* ctx, X** out, Build build) {
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
int destroyChild(X* x) {
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
int upload(bhip_ctx* ctx, T* dev, int pitch, const T* in, int start, int stride, int w, int h, hipStream_t st) {
	if (pitch == w && stride == w) BHIP_HIP(ctx, hipMemcpyAsync(dev, in + start, sizeof(T) * w * h, hipMemcpyHostToDevice, st));
	else BHIP_HIP(ctx, hipMemcpy2DAsync(dev, sizeof(T) * pitch, in + start, sizeof(T) * stride, sizeof(T) * w, h, hipMemcpyHostToDevice, st));
	return BHIP_OK;
}
template <class T>
int download(bhip_ctx* ctx, T* out, int start, int stride, const T* dev, int pitch, int w, int h, hipStream_t st) {
	if (pitch == w && stride == w) BHIP_HIP(ctx, hipMemcpyAsync(out + start, dev, sizeof(T) * w * h, hipMemcpyDeviceToHost, st));
	else BHIP_HIP(ctx, hipMemcpy2DAsync(out + start, sizeof(T) * stride, dev, sizeof(T) * pitch, sizeof(T) * w, h, hipMemcpyDeviceToHost, st));
	return BHIP_OK;
}

// Staging of a host-buffer export (see CtxScratch): stageIn reserves `slot` for one image shaped like `h` with rows `pitch` elements apart,
// uploads h into it unless `copy` is false (an output the implementation writes as a whole) and hands back the device view; stageOut
// enqueues the download.  The export synchronizes once after its last stageOut.
template <class T>
int stageIn(bhip_ctx* ctx, DevBuf& slot, HostImg<T> h, int pitch, DevImg<std::remove_const_t<T>>& dev, bool copy = true) {
	using E = std::remove_const_t<T>;
	BHIP_TRY(slot.reserve(ctx, (size_t)pitch * h.height * sizeof(E)));
	dev = bhip_img_over<E>(slot, pitch, h.width, h.height, 1);
	return copy ? upload<E>(ctx, dev.data, pitch, h.data, h.start, h.stride, h.width, h.height, ctx->stream) : BHIP_OK;
}
template <class T>
int stageOut(bhip_ctx* ctx, HostImg<T> h, DevImg<T> dev) {
	return download<T>(ctx, h.data, h.start, h.stride, dev.data, dev.stride, h.width, h.height, ctx->stream);
}
// pitch4(w): device rows 16-byte aligned so that the tiled ip kernels apply
inline int pitch4(int w) { return (w + 3) & ~3; }

// The usual host export: one input view, one output view.  After the context and image checks and the export's own argument check
// (argError: its message, nullptr when it passed) `in` is staged into in0 and `out` into out0 -- rows pitch4(width) apart when `pitched`,
// dense otherwise; `out` is uploaded too when `keepOut`, i.e. when the operation leaves some pixels as the caller had them -- then
// run(din, dout), the download and the synchronize.  When run fails, nothing is downloaded.
template <class TI, class TO, class Run>
int hostInOut(bhip_ctx* ctx, HostImg<const TI> in, HostImg<TO> out, bool pitched, bool keepOut, const char* argError, Run run) {
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
// host functions that one family calls in another
// ---------------------------------------------------------------------------------------------------------------
// cabi_detect.hip; the KLT tracker's spawn runs it on its corner intensity
int nonmaxDevice(bhip_ctx* ctx, DevImg<const float> img, int radius, float threshold, int border, int16_t* dev_xy, int cap, int* dev_n,
				 bool minimum = false);
// cabi_ip.hip, instantiated there for the types named: the KLT tracker's spawn (cornerImpl: float, int16_t) and process (pyramidImpl:
// float, uint8_t; PyrTraits: described with it), the BRIEF detect+describe object of cabi.hip (briefPatchOk)
template <class T>
int cornerImpl(bhip_ctx* ctx, bool weighted, int kind, int radius, float kappa, DevImg<const T> dx, DevImg<const T> dy, DevImg<float> intensity);
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
int pyramidImpl(bhip_ctx* ctx, const typename PyrTraits<T>::Kernel* kernel, int kw, const int* scales, int n, DevImg<const T> in, T* out,
				bool layer0Present = false);
bool briefPatchOk(const int32_t* samplePoints, int nSamples, int radius);
// cabi_ip.hip; the GrayF32 local thresholds (cabi_threshold.hip) blur with them
int gaussianImpl(bhip_ctx* ctx, double sigma, int radius, DevImg<const float> in, DevImg<float> out);

#pragma GCC visibility pop
