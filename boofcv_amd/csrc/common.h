// Internal declarations shared by the HIP translation units of libboofhip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>
#include <new>
#include <utility>
#include "../../include/boofhip.h"

#define BHIP_WAVE 64

// Parity cross-check hooks (BHIP_DETECT_UNFUSED, BHIP_ASSOC_EXACT, ...) select an alternative, equally exact execution plan; they are read
// from the environment on every call (no process-wide cache: contexts on different host threads may not share mutable statics).
// Timing-experiment switches (ablation, tile variants, stamps) exist only in -DBHIP_EXPERIMENTS builds (boofcv_amd/build.py --experiments),
// never in the shipped libboofhip.so.
static inline bool bhip_env_flag(const char* name) {
	const char* e = getenv(name);
	return e && e[0] == '1';
}
#ifdef BHIP_EXPERIMENTS
#define BHIP_ABLATE(P, bits) ((P).ablate & (bits))
#else
#define BHIP_ABLATE(P, bits) 0
#endif

// ---------------- owners of HIP resources ----------------
// Move-only; the destructor frees, and a move assignment swaps (the old resource leaves with the moved-from object).  Destructors never
// synchronize: the owner synchronizes before it drops device state, with the resource's device current.

// a stream or an event the library created
template <class H, hipError_t (*Destroy)(H)>
struct HipHandle {
	H h = nullptr;
	HipHandle() = default;
	HipHandle(HipHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
	HipHandle& operator=(HipHandle&& o) noexcept { std::swap(h, o.h); return *this; }
	~HipHandle() { if (h) (void)Destroy(h); }
	operator H() const { return h; }
};
using HipStream = HipHandle<hipStream_t, hipStreamDestroy>;
using HipEvent = HipHandle<hipEvent_t, hipEventDestroy>;

// grow-only page-locked host block
struct PinnedBuf {
	void* p = nullptr;
	size_t cap = 0;
	PinnedBuf() = default;
	PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
	PinnedBuf& operator=(PinnedBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
	~PinnedBuf() { if (p) (void)hipHostFree(p); }
	int reserve(bhip_ctx* ctx, size_t bytes);   // grows to exactly `bytes` (defined below DevBuf)
	template <class T> T* as() const { return (T*)p; }
};

// one bracketed kernel launch (profiling mode only)
struct ProfRecord {
	const char* tag;
	double algBytes;     // algorithmic HBM bytes of this launch, 0 when not an HBM-roofline kernel
	double algFlops;     // algorithmic flops / integer ops of this launch, 0 when not a compute-roofline kernel
	HipEvent start, stop;
};

struct bhip_ctx {
	int device = 0;
	hipStream_t stream = nullptr;   // ownedStream, or the caller's (bhip_ctx_create_on_stream)
	HipStream ownedStream;          // declared first: destroyed last
	std::string error;
	// small pinned staging buffer for count read-backs
	PinnedBuf hostScratch;
	// optional per-kernel HIP-event timing on the ctx stream (bhip_profile_*); every event of the ctx sits in one of the two lists
	bool profiling = false;
	std::vector<ProfRecord> profRecords;
	std::vector<HipEvent> eventPool;
	size_t integralLdsAttr = 0;   // largest dynamic-LDS size k_integral_fused has been configured for on this ctx's device
	int cuCount = 0;              // compute units of the device (sizes the persistent grid of k_describe)
};

// RAII bracket around one kernel launch: records a start/stop event pair on the ctx stream when profiling is on
struct ProfScope {
	bhip_ctx* ctx;
	int idx = -1;
	ProfScope(bhip_ctx* c, const char* tag, double algBytes = 0, double algFlops = 0);
	~ProfScope();
};

static inline int bhip_fail(bhip_ctx* ctx, int code, const std::string& msg) {
	if (ctx) ctx->error = msg;
	return code;
}

#define BHIP_HIP(ctx, expr)                                                                                                      \
	do {                                                                                                                         \
		hipError_t _e = (expr);                                                                                                  \
		if (_e != hipSuccess) return bhip_fail((ctx), _e == hipErrorOutOfMemory ? BHIP_ERR_NOMEM : BHIP_ERR_HIP,                 \
											   std::string(#expr) + ": " + hipGetErrorString(_e));                               \
	} while (0)

#define BHIP_TRY(expr)                 \
	do {                               \
		int _s = (expr);               \
		if (_s != BHIP_OK) return _s;  \
	} while (0)

// grow-only device buffer
struct DevBuf {
	void* p = nullptr;
	size_t cap = 0;
	DevBuf() = default;
	DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
	DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
	~DevBuf() { if (p) (void)hipFree(p); }
	int reserve(bhip_ctx* ctx, size_t bytes) {
		if (bytes <= cap) return BHIP_OK;
		if (p) { BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream)); BHIP_HIP(ctx, hipFree(p)); p = nullptr; cap = 0; }
		size_t want = bytes + bytes / 8;
		BHIP_HIP(ctx, hipMalloc(&p, want));
		cap = want;
		return BHIP_OK;
	}
	template <class T> T* as() const { return (T*)p; }
};

inline int PinnedBuf::reserve(bhip_ctx* ctx, size_t bytes) {
	if (bytes <= cap) return BHIP_OK;
	if (p) { BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipHostFree(p); p = nullptr; cap = 0; }
	if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return bhip_fail(ctx, BHIP_ERR_NOMEM, "page-locked staging buffer"); }
	cap = bytes;
	return BHIP_OK;
}

// work buffers of the MFMA association path (assoc_mfma.hip)
struct AssocMfmaWork {
	DevBuf Fs, Fd, nrmS, nrmD, probs, keys, best, args, cand, flags;   // probs: the problem table, then the block table
	PinnedBuf tables;            // page-locked staging copy of the problem and block tables; k_assoc_init reads it through its device address
	bool tablesInFlight = false; // a launch that reads `tables` has been issued and not been waited for since
	HipEvent flagsRead;          // recorded behind the flags read-back: the host waits for it alone, not for the result kernel after it
	int scaleHint = 1;           // q_h: the scale exponent the one-pass prep assumes; 1 = largest squared norm in [1, 4) (unit vectors)
};

// ---------------- image view passed to kernels ----------------
// Kernel-argument types only (they are in kernel signatures and *Params structs); `data` is typed float whatever the 32-bit element type is
struct ImgView {
	const float* data;   // base of image 0 (already offset by startIndex)
	long long imageStride;  // floats between images of a batch
	int stride;          // floats between rows
	int width, height;
};
struct ImgViewW {
	float* data;
	long long imageStride;
	int stride;
	int width, height;
};

// ---------------- typed view of a device image batch, passed between host functions ----------------
// `batch` images of width x height elements, imageStride elements apart, rows `stride` elements apart (all strides in elements of T).
// DevImg<const T> is the input form.  Host side only: the launchers unpack a view into their kernel's ImgView / *Params arguments.
template <class T>
struct DevImg {
	T* data;
	long long imageStride;
	int stride, width, height, batch;
	operator DevImg<const T>() const { return {data, imageStride, stride, width, height, batch}; }
};
// a launcher's kernel argument for a view of 32-bit elements (float, or the int32 of a GrayS32 integral image)
template <class T>
static inline ImgView bhip_kernel_view(DevImg<const T> v) {
	static_assert(sizeof(T) == 4, "ImgView carries 32-bit elements");
	return {reinterpret_cast<const float*>(v.data), v.imageStride, v.stride, v.width, v.height};
}
// `batch` images with rows `pitch` elements apart, packed from the start of `buf`
template <class T>
static inline DevImg<T> bhip_img_over(const DevBuf& buf, int pitch, int width, int height, int batch) {
	return {buf.as<T>(), (long long)pitch * height, pitch, width, height, batch};
}
// layer l of a pyramid batch laid out by bhip_pyramid_layout (dims, offs; `total` elements per frame): dense rows
template <class T>
static inline DevImg<T> bhip_pyr_layer(T* base, long long total, const int* dims, const long long* offs, int l, int batch) {
	return {base + offs[l], total, dims[2 * l], dims[2 * l], dims[2 * l + 1], batch};
}

// ---------------- detector structures ----------------
#define BHIP_MAX_OCTAVES 8
#define BHIP_MAX_LEVELS 8

struct KeyPoint {      // one detected interest point, as stored on the device
	double x, y, scale;
	unsigned int key;    // bit index in the per-image candidate bitmap == rank key (octave, level, blockY, blockX)
	unsigned int pad;
};

// tables for orientation + descriptor, resident in device memory
struct SurfTables {
	// orientation
	int oriStable;           // 1 sliding window, 0 average
	int oriRadius;           // sampleRadius
	int oriWidth;            // 2*radius+1
	int oriKernelWidth;      // ConfigOrientation.sampleWidth
	int oriHasWeights;
	double oriPeriod;        // samplePeriod
	double oriWindow;        // windowSize
	double oriRadiusToScale; // objectRadiusToScale
	const double* oriWeights;  // oriWidth^2
	// descriptor
	int stable;              // 1 DescribePointSurfMod, 0 DescribePointSurf
	int widthLargeGrid, widthSubRegion, widthSample, overLap;
	int dof;
	int radiusDescriptor;
	const double* weightSub;   // (sub+2*overlap)^2        (stable)
	const double* weightGrid;  // largeGrid^2              (stable)
	const double* weightFast;  // (largeGrid*sub)^2        (fast)
};

// host-side Gaussian tables (tables.cpp): product code, independent of oracle/
std::vector<double> bhip_gaussian2d_f64(double sigma, int radius);          // FactoryKernelGaussian.gaussian(2,true,64,sigma,radius)
std::vector<double> bhip_gaussian_width(double sigma, int width);           // FactoryKernelGaussian.gaussianWidth
std::vector<float> bhip_gaussian1d_f32(double sigma, int radius);           // FactoryKernelGaussian.gaussian(Kernel1D_F32,sigma,radius)
std::vector<int32_t> bhip_gaussian1d_s32(int radius);                       // FactoryKernelGaussian.gaussian(Kernel1D_S32,-1,radius)

// ---------------- kernel launchers (defined in the .hip files) ----------------
// An integral image is GrayF32 (from GrayF32 frames) or GrayS32 (from GrayU8 frames): the launchers that read one are templates over its
// element type T = float / int32_t (instantiated for these two where they are defined), which picks the kernel instantiation.
int bhip_launch_integral(bhip_ctx* ctx, DevImg<const float> in, DevImg<float> out);
// levels a fused octave writes out for the next octave (every second pixel, next octave's [image][slot][h][w] layout)
struct FusedExport {
	int n;
	int level[2];
	float* out;
	int w, h;
	long long imageStride;
	long long slotOffset[2];   // floats from an image's base to the slot's [h][w] plane (the consuming octave's level planes when it is written in place)
};
// where a stand-alone Hessian level comes from: computed, or copied from a level of the same kernel size one octave down
struct HessLevelSource {
	const float* src;        // nullptr: compute
	long long imageStride;   // floats between images at src
	int stride;              // floats between rows at src
	int step;                // 1: src already has this octave's layout, 2: take every second pixel
	int inPlace;             // src IS this level's output plane (the producer wrote it there): only the pixels that must be recomputed are touched
};
// level0: the octave's intensity planes, level l `levelStride` floats on; from == nullptr: all computed; skipMask: levels this launch does not produce
template <class T>
int bhip_launch_hessian(bhip_ctx* ctx, DevImg<const T> ii, int skip, int nlevels, const int* sizes, DevImg<float> level0, long long levelStride,
						const HessLevelSource* from, unsigned int skipMask);
// several octaves of one batch of integral images, in order (an octave may copy levels from the one before): the arguments of bhip_launch_hessian
struct HessOctave {
	int skip, nlevels;
	const int* sizes;
	DevImg<float> level0;
	long long levelStride;
	const HessLevelSource* from;
	unsigned int skipMask;
};
template <class T>
int bhip_launch_hessian_octaves(bhip_ctx* ctx, DevImg<const T> ii, int noct, const HessOctave* octs);

// colour SURF (see DescParams): the band integral images the descriptor is built from.  nBands == 0: grey SURF, nothing else is read
struct DescPlanar {
	const float* data;               // [image][band][H][W]
	long long imageStride, bandStride;
	int nBands;
};
struct DetectLevelParams {
	int skip, w, h;              // intensity image size
	int sizeLower, sizeMid, sizeUpper;  // kernel sizes of level-1, level, level+1
	int border;                  // ignoreBorder = size/(2*skip)
	int nbx, nby;                // blocks in the NMS region
	unsigned int bitBase;        // first bit of this (octave,level) in the per-image bitmap
};
// lower / mid / upper: three levels of one octave (one layout).  lower.data / upper.data == nullptr: that level is evaluated on demand from ii
template <class T>
int bhip_launch_nms_scalespace(bhip_ctx* ctx, DevImg<const float> lower, DevImg<const float> mid, DevImg<const float> upper, DetectLevelParams p, int radius,
							   float threshold, unsigned int* bitmap, int bitmapWords, KeyPoint* cand, int* candCount, int cap, bool listOnly,
							   DevImg<const T> ii);
// the same for n levels, of one octave or of several, in one launch per four levels (never the N-best list form)
struct NmsLevelArgs {
	DevImg<const float> lower, mid, upper;
	DetectLevelParams p;
};
template <class T>
int bhip_launch_nms_scalespace_levels(bhip_ctx* ctx, int n, const NmsLevelArgs* lv, int radius, float threshold, unsigned int* bitmap, int bitmapWords,
									  KeyPoint* cand, int* candCount, int cap, DevImg<const T> ii);
int bhip_launch_select_nbest(bhip_ctx* ctx, DevImg<const float> lower, DevImg<const float> mid, DevImg<const float> upper, DetectLevelParams p, int radius,
							 int target, const unsigned int* bitmap, const unsigned int* prefix, int bitmapWords, const KeyPoint* nms, int cap, float* keyBuf,
							 int* idxBuf, KeyPoint* out, int* levelStart, int* levelCount, int levelIndex, int nlv);
int bhip_launch_select_nbest_xy(bhip_ctx* ctx, DevImg<const float> img, const int16_t* xy, int n, int target, bool positive, float* key, int* idx, int16_t* out);
int bhip_launch_compact_levels(bhip_ctx* ctx, const KeyPoint* src, int cap, const int* levelStart, const int* levelCount, int nlv, int batch, KeyPoint* dst,
							   int* totals);
int bhip_launch_rank_scatter(bhip_ctx* ctx, const unsigned int* bitmap, int bitmapWords, unsigned int* wordPrefix, const KeyPoint* cand,
							 const int* candCount, int cap, int batch, KeyPoint* sorted);
int bhip_launch_word_prefix(bhip_ctx* ctx, const unsigned int* bitmap, int bitmapWords, int batch, unsigned int* wordPrefix, int* totals);

// describe.hip, detect.hip, associate.hip, assoc_mfma.hip, detect_fused.hip: what only the C ABI layer calls
// one slot of the describe stage's processing order (k_kp_tile_scatter): key point g of the compact list is key point `local` of image `img`
struct __attribute__((aligned(16))) KpOrder { int g, img, local, pad; };
#define BHIP_DESCRIBE_QUEUE_BYTES (8 * 128)   // k_describe's slot counters: one int per XCD chunk, each on a 128-byte line of its own
// ii: the grey integral images of the batch.  imageStart == nullptr: kps is a flat list for image `singleImage`; perm: optional processing order;
// queue: BHIP_DESCRIBE_QUEUE_BYTES of device memory that belong to this launch until it has finished (zeroed here, on the stream)
template <class T>
int bhip_launch_describe_ex(bhip_ctx* ctx, DevImg<const T> ii, const KeyPoint* kps, int cap, const int* imageStart, int singleImage, long long total,
							SurfTables t, const double* anglesIn, double* angles, double* desc, uint8_t* white, const KpOrder* perm, int* queue,
							DescPlanar planar);
int bhip_launch_kp_spatial_order(bhip_ctx* ctx, const KeyPoint* kps, int cap, const int* start, int batch, int maxCount, int W, int H, int* hist,
								 KpOrder* perm);
// per-split partial records of the association scans (associate.hip's VALU kernels and assoc_ham_mfma.hip write the same ones)
struct ColTop {
	double min1, min2;
	int idx1, pad;
};
struct RowBest {
	double best;
	int idx, pad;
};
int bhip_assoc_phase1_l2(bhip_ctx* ctx, const double* src, int nsLocal, int srcBegin, const double* dst, int nd, int dof, double maxErr, int sqrtScore,
						 int* pairs, double* fit, void* colTop, DevBuf& work);
int bhip_assoc_phase1_ham(bhip_ctx* ctx, const int32_t* src, int nsLocal, int srcBegin, const int32_t* dst, int nd, int words, double maxErr, int* pairs,
						  double* fit, void* colTop, DevBuf& work);
int bhip_assoc_phase2(bhip_ctx* ctx, const void* colAll, int nranks, int nd, int nsLocal, int srcBegin, int* pairs, double* fit);
int bhip_assoc_coltop_size();
// int8 MFMA Hamming path (assoc_ham_mfma.hip), called by associate.hip
int bhip_ham_expand(bhip_ctx* ctx, const int* D, long long rows, int words, unsigned char* bytes, int* pop);
int bhip_ham_mfma_splits(int nU, int nV);
int bhip_ham_mfma_scan(bhip_ctx* ctx, bool colMode, const unsigned char* Ub, const int* Up, int nU, const unsigned char* Vb, const int* Vp, int nV, int words,
						 int vBase, double maxErr, void* partial, int splits);
int bhip_assoc_hamming_batched(bhip_ctx* ctx, const int32_t* src, const int32_t* dst, int words, int count, const long long* srcOff, const int* ns,
							   const long long* dstOff, const int* nd, double maxErr, int backwards, int* pairs, double* fit, DevBuf& work);

int bhip_assoc_l2_mfma_batched(bhip_ctx* ctx, AssocMfmaWork& W, const double* dev_src, const double* dev_dst, int count, const long long* srcOff,
								 const int* ns, const long long* dstOff, const int* nd, double maxErr, int backwards, int* dev_pairs, double* dev_fit,
								 int* usedMfma);

bool bhip_fused_plan(int skip, int nlevels, const int* sizes, int radius, int* TX, int* TY, int* ldsBytes);
bool bhip_fused_is_fixed(int skip, int nlevels, const int* sizes, int radius);
template <class T>
int bhip_launch_detect_fused(bhip_ctx* ctx, DevImg<const T> ii, int skip, int nlevels, const int* sizes, int nmid, const DetectLevelParams* mids,
							 const int* midLevels, int radius, float threshold, unsigned int* bitmap, int bitmapWords, KeyPoint* cand, int* candCount,
							 int cap, const FusedExport* exp);

// ---------------- boofcv-ip front end (conv.hip, pyramid.hip, gradient.hip, corner.hip, brief.hip; the planar average and the GrayU8 integral
// image: integral.hip; what the units share: ip_dev.h) ----------------
// Images arrive as DevImg views.  Where the images of a call share one shape, width, height and batch are read from the first view; dx / dy
// pairs share one layout.
int bhip_launch_conv(bhip_ctx* ctx, bool vertical, bool normalized, const float* kernel, int kw, int koff, DevImg<const float> in, DevImg<float> out);
int bhip_launch_blur_fused(bhip_ctx* ctx, const float* kernel, int kw, DevImg<const float> in, DevImg<float> out, bool* done);
int bhip_launch_pyr_layer_fused(bhip_ctx* ctx, const float* kernel, int kw, DevImg<const float> in, DevImg<float> out, int skip, bool* done);
// ConvolveImageDownNormalized.horizontal / vertical: Kernel1D_F32 on GrayF32, or Kernel1D_S32 on GrayU8 -> GrayI8 (the integer pyramid's layer step)
int bhip_launch_conv_down(bhip_ctx* ctx, bool vertical, const float* kernel, int kw, DevImg<const float> in, DevImg<float> out, int skip);
int bhip_launch_conv_down(bhip_ctx* ctx, bool vertical, const int32_t* kernel, int kw, DevImg<const uint8_t> in, DevImg<uint8_t> out, int skip);
int bhip_launch_copy_images(bhip_ctx* ctx, DevImg<const float> in, DevImg<float> out);
int bhip_launch_copy_images(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<uint8_t> out);
int bhip_launch_planar_average(bhip_ctx* ctx, const float* bands, long long bandStride, int numBands, long long n, float* out);
// GradientSobel / GradientThree / GradientPrewitt (kind 0 / 1 / 2): GrayF32 -> GrayF32, GrayU8 -> GrayS16
int bhip_launch_gradient(bhip_ctx* ctx, int kind, DevImg<const float> in, DevImg<float> dx, DevImg<float> dy, int border);
int bhip_launch_gradient(bhip_ctx* ctx, int kind, DevImg<const uint8_t> in, DevImg<int16_t> dx, DevImg<int16_t> dy, int border);
int bhip_launch_grad_intensity(bhip_ctx* ctx, int kind, DevImg<const float> dx, DevImg<const float> dy, DevImg<float> out);
// box-window corner intensity.  F32: `scratch` holds three dense width x height float planes per image.  S16: fused, or through `scratch`
// (bhip_corner_box_s16_scratch bytes, 0: none) when the radius is beyond the fused block.
int bhip_launch_corner_intensity(bhip_ctx* ctx, int kind, int radius, float kappa, DevImg<const float> dx, DevImg<const float> dy, DevImg<float> intensity,
								 float* scratch);
size_t bhip_corner_box_s16_scratch(int radius, int width, int height, int batch);
int bhip_launch_corner_box_s16(bhip_ctx* ctx, int kind, int radius, float kappa, DevImg<const int16_t> dx, DevImg<const int16_t> dy, DevImg<float> intensity,
							   void* scratch);
// fused Gaussian-weighted corner intensity on F32 (ImplSsdCornerWeighted_F32) or S16 (ImplSsdCornerWeighted_S16) derivatives
int bhip_corner_weighted_max_radius();
int bhip_launch_corner_weighted(bhip_ctx* ctx, int kind, int radius, float kappa, DevImg<const float> dx, DevImg<const float> dy, DevImg<float> intensity);
int bhip_launch_corner_weighted(bhip_ctx* ctx, int kind, int radius, float kappa, DevImg<const int16_t> dx, DevImg<const int16_t> dy, DevImg<float> intensity);
// start == nullptr: n points on image 0.  Otherwise img.batch images and the device prefix `start` (batch + 1); maxCount = largest per-image count.
// patchOk: every sample point of the definition lies within [-radius, radius]^2 (checked on the host where the table is at hand), so the
// LDS-patch kernel may be used; otherwise the gather kernel runs
int bhip_launch_brief(bhip_ctx* ctx, DevImg<const float> img, int radius, int numPoints, const int* samplePoints, const int* compare, const double* xy, int n,
					  int* out, const int* start, int maxCount, int xyStride, long long xyImageStride, bool patchOk);
int bhip_launch_brief(bhip_ctx* ctx, DevImg<const uint8_t> img, int radius, int numPoints, const int* samplePoints, const int* compare, const double* xy, int n,
					  int* out, const int* start, int maxCount, int xyStride, long long xyImageStride, bool patchOk);
int bhip_launch_mean(bhip_ctx* ctx, bool vertical, DevImg<const float> in, DevImg<float> out, int radius);   // one direction of the mean blur, batched
// single images (batch 1)
int bhip_launch_conv2d(bhip_ctx* ctx, const float* kernel, int kw, int koff, DevImg<const float> in, DevImg<float> out);
int bhip_launch_median(bhip_ctx* ctx, DevImg<const float> in, DevImg<float> out, int radius);
int bhip_launch_integral_u8(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<int32_t> out);   // IntegralImageOps.transform(GrayU8, GrayS32)
// stand-alone strict block NMS over a batch (detect.hip): bitmap of accepted blocks + the pixel's position inside its block
int bhip_launch_nonmax_blocks(bhip_ctx* ctx, DevImg<const float> img, int radius, float threshold, int border, unsigned int* bitmap, int bitmapWords,
							  unsigned short* posInBlock, int nbx, int nby);
int bhip_launch_blocks_to_xy(bhip_ctx* ctx, const unsigned int* bitmap, const unsigned int* wordPrefix, int bitmapWords, const unsigned short* posInBlock,
							 int nbx, int nby, int batch, int radius, int border, int16_t* xy, int cap);
// the minima half (NonMaxBlockSearchStrict.Min): same outputs as bhip_launch_nonmax_blocks, into buffers of its own
int bhip_launch_nonmin_blocks(bhip_ctx* ctx, DevImg<const float> img, int radius, float threshold, int border, unsigned int* bitmap, int bitmapWords,
							  unsigned short* posInBlock, int nbx, int nby);

// ---------------- FAST corner detector (fast.hip) ----------------
template <class T> struct FastTol;   // ImplFastHelper_U8 / _F32: the type of pixelTol and of the pixel arithmetic
template <> struct FastTol<uint8_t> { using type = int; };
template <> struct FastTol<float> { using type = float; };
size_t bhip_fast_scratch(int width, int height, int batch);   // bytes of device scratch one bhip_launch_fast call needs
// FastCornerDetector.process(image, intensity) on every frame of a batch (inten.data == nullptr: process(image)).  maxFeatures: the
// reference's (int)(maxFeaturesFraction * width * height).  Frame b's dark / bright corners go to xyLow / xyHigh[b * cap ...] in raster
// order, their numbers to nLow / nHigh[b] (they may exceed cap: only the first cap pairs are written)
template <class T>
int bhip_launch_fast(bhip_ctx* ctx, DevImg<const T> img, typename FastTol<T>::type tol, int minContinuous, int maxFeatures, DevImg<float> inten, void* scratch,
					 int16_t* xyLow, int* nLow, int16_t* xyHigh, int* nHigh, int cap);

// ---------------- dense stereo disparity, SAD block matching (disparity.hip) ----------------
#define BHIP_DISP_MAX_RADIUS 7    // regionRadiusX / regionRadiusY the kernel's staged rows hold
#define BHIP_DISP_MAX_RANGE 256   // rangeDisparity the kernel's cost slab holds
// ConfigDisparityBM as the selector sees it: maxError = Integer.MAX_VALUE when the test is off, rtolTol < 0 and textureThr <= 0 likewise
struct DispBmParams {
	int minD, range, rx, ry;
	int maxError, rtolTol, textureThr;
};
size_t bhip_disparity_scratch(int width, int height, int batch);   // bytes of device scratch one bhip_launch_disparity_bm call needs
// DisparityScoreBM_S32 + SelectErrorWithChecks_S32.DispU8 (OutT = uint8_t) / SelectErrorSubpixel.S32_F32 (OutT = float) on every pair of a
// batch; the whole output view is written (rangeDisparity where the reference writes nothing).  The caller has validated c against the image.
template <class OutT>
int bhip_launch_disparity_bm(bhip_ctx* ctx, DevImg<const uint8_t> left, DevImg<const uint8_t> right, const DispBmParams& c, uint8_t* scratch, DevImg<OutT> out);

// ---------------- census transform (census.hip) and census block matching (disparity.hip) ----------------
#define BHIP_CENSUS_MAX_SAMPLES 64   // FilterCensusTransformSampleS64's own limit
#define BHIP_CENSUS_MAX_OFFSET 7     // |dx|, |dy| of a sample the kernel's halo holds
// a sample list as the kernel reads it: n and radius (the largest |dx|, |dy|) are those of the whole list, dx / dy the first 32 samples --
// `int bit` of sample_S64 is 0 from sample 32 on
struct CensusSamples {
	int n = 0, radius = 0;
	signed char dx[32] = {}, dy[32] = {};
};
// samplesXY = (x, y) pairs -> s and BHIP_OK; BHIP_ERR_INVALID: nSamples outside 0..64 or the list is missing; BHIP_ERR_UNSUPPORTED: an offset outside -7..7
int bhip_census_samples(const int* samplesXY, int nSamples, CensusSamples& s);
// the reference's sample list of a CensusVariants ordinal into samplesXY (room for 64 pairs) -> its length, -1: no such variant
int bhip_census_variant_list(int variant, int* samplesXY);
// OutT = uint8_t: dense3x3 (denseRadius 1); int32_t: dense5x5 (denseRadius 2), or with denseRadius 0 the low 32 bits of sample_S64's word;
// long long: sample_S64 (denseRadius 0).  REFLECT border; the whole output view is written.  Needs width, height >= radius + 1.
template <class OutT>
int bhip_launch_census(bhip_ctx* ctx, DevImg<const uint8_t> in, int denseRadius, const CensusSamples* s, DevImg<OutT> out);
// bytes of device scratch one bhip_launch_disparity_bm_census call needs: the right-to-left minima and the two census images
size_t bhip_disparity_census_scratch(int width, int height, int batch, int wordBytes);
// bhip_launch_disparity_bm with the Hamming distance of census words as the cost: wordBytes 1 (3x3), 4 (5x5) or 8 (the sample list s, matched
// on the low 32 bits of its words).  Census of both images into scratch, then the SAD entry's launches; no host synchronisation.
template <class OutT>
int bhip_launch_disparity_bm_census(bhip_ctx* ctx, DevImg<const uint8_t> left, DevImg<const uint8_t> right, const DispBmParams& c, int wordBytes,
									const CensusSamples* s, uint8_t* scratch, DevImg<OutT> out);
// FactoryStereoDisparity.blockMatchBest5: DisparityScoreBMBestFive_S32 with the same selectors (c.maxError holds the factory's 3 * rw * rh *
// maxPerPixelError), SAD and CENSUS; scratch as for the plain forms.  An image with no selector column (W - (4*rx+1) < minD) or no output row
// (H < 4*ry + 1) is filled with rangeDisparity.
template <class OutT>
int bhip_launch_disparity_bm5(bhip_ctx* ctx, DevImg<const uint8_t> left, DevImg<const uint8_t> right, const DispBmParams& c, uint8_t* scratch, DevImg<OutT> out);
template <class OutT>
int bhip_launch_disparity_bm5_census(bhip_ctx* ctx, DevImg<const uint8_t> left, DevImg<const uint8_t> right, const DispBmParams& c, int wordBytes,
									 const CensusSamples* s, uint8_t* scratch, DevImg<OutT> out);

// ---------------- image remap, ImageDistort (distort.hip) ----------------
// where the source coordinates of a destination pixel come from: model == 0, a device map of (x, y) pairs, dw*dh per image and mapImageStride
// floats from one image's map to the next (0: one map for the batch); otherwise BHIP_DISTORT_AFFINE / _HOMOGRAPHY with 6 / 9 coefficients
struct DistortCoords {
	int model;
	const float* map;
	long long mapImageStride;
	const float* coeff;   // host memory
};
struct DistortCrop {
	int x0, y0, x1, y1;
};
// ImageDistortBasic_SB / ImageDistortCache_SB apply on every image of a batch: the pixels of the crop of dst (assigned or skipped as renderAll
// says) and, when mask.data is not null, of the mask.  The caller has validated interp, border, the crop against dst and mask against dst.
template <class T>
int bhip_launch_distort(bhip_ctx* ctx, DevImg<const T> src, const DistortCoords& co, const DistortCrop& crop, int interp, int border, int renderAll, DevImg<T> dst,
						DevImg<uint8_t> mask);
// the map of a model, dw x dh entries, into device memory
int bhip_launch_distort_build_map(bhip_ctx* ctx, int model, const float* coeff, int dw, int dh, float* map);

// ---------------- stationary background models (background.hip; kernels: background_dev.h, background_gmm_*.hip) ----------------
#define BHIP_BG_MAX_BANDS 4
#define BHIP_BG_MAX_GAUSSIANS 8   // the mixture is a register array of this many slots at most
// what a bhip_bg was created for.  bands: 0 = a single-band Gray image (the reference's *_SB classes), 1..4 = a Planar image of that many bands
// (*_PL / *_MB); maxGaussians: GMM only
struct BgShape {
	int alg, bands, maxGaussians, width, height, streams;
};
// the fields of the three Java classes (those the algorithm does not have are unused)
struct BgConfig {
	float learnRate, threshold, initialVariance, minimumDifference;          // Basic / Gaussian
	float learningPeriod, decay, maxDistance, significantWeight;             // GMM (and initialVariance)
	int unknownValue;
};
// frames or masks of a batch of streams: element (stream, frame, band, y, x) at data[stream * streamStride + frame * frameStride +
// band * bandStride + y * stride + x]
template <class T>
struct BgFrames {
	T* data;
	long long streamStride, frameStride, bandStride;
	int stride, numFrames;
};
int bhip_bg_components(const BgShape& sh);   // float planes of one stream's model
double bhip_bg_bytes(const BgShape& sh, int pixelBytes, int numFrames, bool masks, bool segment);   // HBM bytes of one launch
// segment == false: updateBackground(frame_t[, mask_t]) for t = 0 .. numFrames-1 on every stream (m.data == nullptr: no masks).
// segment == true: segment(frame, mask) with the one frame of every stream.  state: device [streams][2] = {initialised, GMM common.unknownValue}
template <class T>
int bhip_launch_background(bhip_ctx* ctx, const BgShape& sh, const BgConfig& cfg, const BgFrames<const T>& f, const BgFrames<uint8_t>& m, float* model,
						   const int* state, bool segment);

// ---------------- template matching (template.hip; the match selection is in detect.hip next to the N-best selection) ----------------
size_t bhip_template_scratch(int batch);   // bytes of device scratch (the NCC template statistics) one bhip_launch_template_intensity call needs
// TemplateIntensityImage.process on every image of a batch, T = uint8_t / float; tpl.imageStride / mask.imageStride 0: shared by the batch,
// mask.data == nullptr: no mask.  The whole output view is written.  The caller has validated the sizes (tpl.width <= BHIP_TEMPLATE_MAX_WIDTH).
template <class T>
int bhip_launch_template_intensity(bhip_ctx* ctx, int score, DevImg<const T> img, DevImg<const T> tpl, DevImg<const T> mask, float* stats, DevImg<float> out);
// TemplateMatching.process after the extractor: image b selects from xy[b*cap ...], the first min(n[b], cap) pairs (n == nullptr: cap of them);
// key / idx: [batch][cap] work arrays
int bhip_launch_template_select(bhip_ctx* ctx, DevImg<const float> img, const int16_t* xy, const int* n, int cap, int maxMatches, bool maximize, float* key,
								int* idx, int16_t* outXY, float* outScore, int* outN);

// ---------------- pyramid KLT tracker (klt.hip) ----------------
#define BHIP_KLT_MAX_LAYERS 8
#define BHIP_KLT_MAX_RADIUS 7
#define BHIP_KLT_MAX_LEN ((2 * BHIP_KLT_MAX_RADIUS + 1) * (2 * BHIP_KLT_MAX_RADIUS + 1))

// image pyramid + derivative pyramids of `batch` frames: layer l of frame b starts at base + b * frameStride + off[l], rows stride[l] elements apart.
// TI / TD: pixel types of the image and of its derivatives -- GrayF32 / GrayF32 or GrayU8 / GrayS16
template <class TI, class TD>
struct KltPyrT {
	const TI* img;
	const TD* dx;   // nullptr when only tracking (PyramidKltTracker.setImage(image))
	const TD* dy;
	long long frameStride;
	long long off[BHIP_KLT_MAX_LAYERS];
	int w[BHIP_KLT_MAX_LAYERS], h[BHIP_KLT_MAX_LAYERS], stride[BHIP_KLT_MAX_LAYERS];
	float scale[BHIP_KLT_MAX_LAYERS];   // (float)image.getScale(layer)
	int numLayers;
	int frameW, frameH;                 // the input frame (PointTrackerKltPyramid's image.isInBounds)
};
using KltPyr = KltPyrT<float, float>;
using KltPyrU8 = KltPyrT<uint8_t, int16_t>;

// Track table of one tracker object.  Sequence b owns slots [0, cap); slot s of sequence b is entry g = b * cap + s of every per-track array
// (structure of arrays: the fields of neighbouring tracks are contiguous).  Lists hold slot numbers, in the reference's list order.
struct KltTab {
	int cap, batch, L, r, len;
	int *act, *drp, *spw, *freeL;          // [batch][cap]: active / dropped / spawned tracks, unused slots
	int *nAct, *nDrp, *nSpw, *nFree;       // [batch]
	long long* total;                      // [batch] totalFeatures
	long long* id;                         // featureId
	float *x, *y;                          // PyramidKltFeature.x,y == PointTrack position
	float *tx, *ty;                        // position found by track(), committed to x,y when the track survives the frame
	float* err;                            // KltTracker.getError() of the last layer whose error was computed
	int* fault;                            // KltTrackFault ordinal of the last track()
	int* keep;
	int* iters;                            // Lucas-Kanade iterations of the last track() | border-form iterations << 16 (bench figures)
	float *lx, *ly, *gxx, *gxy, *gyy;      // [L][batch * cap]: KltFeature x, y, Gxx, Gxy, Gyy of every layer
	float* tmpl;                           // [g][L][3][len]: desc, derivX, derivY (desc = NaN where the patch left the image)
};

int bhip_launch_klt_init(bhip_ctx* ctx, KltTab T, int firstSlot);   // slots firstSlot .. cap-1 of every sequence join its unused list (firstSlot 0: a fresh table)
int bhip_launch_klt_begin(bhip_ctx* ctx, KltTab T);                 // process(): dropped.clear() (their slots become unused), spawned.clear()
int bhip_launch_klt_track(bhip_ctx* ctx, KltPyr P, KltTab T, bhip_klt_cfg cfg, int maxActive);
// mode 0: process() -- tracks whose fault is SUCCESS and whose new centre is inside the frame are described at (tx,ty); keep = survives
// mode 1: the `count[b]` newest entries of sequence b's unused list are described at their x,y (spawnTracks); keep = the reference did not throw
// mode 3: the table entries count[0 .. maxCount) are described at their x,y (addTrack; entries < 0 are skipped)
// mode 2: every active track is described at its x,y (stage-level calls); keep = setDescription's result
int bhip_launch_klt_describe(bhip_ctx* ctx, KltPyr P, KltTab T, bhip_klt_cfg cfg, int mode, const int* count, int maxCount);
int bhip_launch_klt_track(bhip_ctx* ctx, KltPyrU8 P, KltTab T, bhip_klt_cfg cfg, int maxActive);
int bhip_launch_klt_describe(bhip_ctx* ctx, KltPyrU8 P, KltTab T, bhip_klt_cfg cfg, int mode, const int* count, int maxCount);
int bhip_launch_klt_compact(bhip_ctx* ctx, KltTab T, int toUnused);   // active := kept tracks in order; the others go to dropped (or straight to unused)
int bhip_launch_klt_mark_exclude(bhip_ctx* ctx, KltTab T, float scale0, DevImg<float> intensity, int maxActive);
int bhip_launch_klt_spawn_place(bhip_ctx* ctx, KltTab T, const int16_t* xy, int xyCap, const int* count, float scale0, int maxCount);
int bhip_launch_klt_spawn_commit(bhip_ctx* ctx, KltTab T, const int* count);
int bhip_launch_klt_add(bhip_ctx* ctx, KltTab T, const int* seq, const double* xy, int n, int frameW, int frameH, unsigned char* ok, int* list);
int bhip_launch_klt_match_drop(bhip_ctx* ctx, KltTab T, const int* seq, const long long* id, int n, unsigned char* ok, int maxActive);
int bhip_launch_klt_drop_all(bhip_ctx* ctx, KltTab T, int resetTotal);
int bhip_launch_klt_stats(bhip_ctx* ctx, KltTab T, unsigned long long* out);   // out[3] += tracks, iterations, border-form iterations of the last process()
int bhip_launch_klt_gather(bhip_ctx* ctx, KltTab T, int which, int seq, int n, long long* id, float* xy, int* fault, float* err);
int bhip_launch_klt_gather_templates(bhip_ctx* ctx, KltTab T, int which, int seq, int layer, int n, float* tmpl, float* G);

// ---------------- dense KLT optical flow (flow.hip; the generic track kernel is in klt.hip) ----------------
// one record per pixel, what DenseOpticalFlowKlt.process knows about a pixel's own track before checkNeighbors: the fault (KltTrackFault ordinal,
// BHIP_KLT_REFERENCE_THROWS, or BHIP_FLOW_NO_DESCRIPTION), and where it is BHIP_KLT_SUCCESS tracker.getError() and (feature.x - x, feature.y - y); 0 elsewhere
struct FlowRec {
	int fault;
	float error, dx, dy;
};
#define BHIP_FLOW_LANE_MAX_RADIUS 3   // the lane-per-pixel form keeps 3 (2r+1)^2 floats per lane in LDS
// one wave per pixel (any radius up to BHIP_KLT_MAX_RADIUS); P is the source pyramid with its gradient, dst the destination pyramid in the same layout
int bhip_launch_flow_track_wave(bhip_ctx* ctx, KltPyr P, const float* dst, int r, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats);
int bhip_launch_flow_track_wave(bhip_ctx* ctx, KltPyrU8 P, const uint8_t* dst, int r, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats);
// one lane per pixel, r <= BHIP_FLOW_LANE_MAX_RADIUS
int bhip_launch_flow_track_lane(bhip_ctx* ctx, KltPyr P, const float* dst, int r, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats);
int bhip_launch_flow_track_lane(bhip_ctx* ctx, KltPyrU8 P, const uint8_t* dst, int r, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats);
// checkNeighbors as an order-free reduction: flow[b][y][x] = (x, y) floats at flow.data + b * imageStride + y * stride + 2 * x (strides in floats)
int bhip_launch_flow_reduce(bhip_ctx* ctx, const FlowRec* rec, int r, DevImg<float> flow);

// ---------------- Horn-Schunck dense optical flow (hornschunck.hip) ----------------
#define BHIP_HS_TILE_W BHIP_FLOW_HS_TILE_WIDTH
#define BHIP_HS_TILE_H BHIP_FLOW_HS_TILE_HEIGHT
// computeDerivX / Y / T of HornSchunck_F32 (T = float) or HornSchunck_U8 (uint8_t; the GrayS16 values as floats) on every pair of a batch:
// deriv is dense [batch][3][height][width]
template <class T>
int bhip_launch_hs_derivatives(bhip_ctx* ctx, DevImg<const T> src, DevImg<const T> dst, float* deriv);
// n iterations (0 .. BHIP_FLOW_HS_MAX_FUSED) of findFlow in one launch.  in: the flow before, dense [batch][height][width] (x, y) pairs, nullptr = the
// zero flow; out: (x, y) of pixel (x, y) at out.data + b * imageStride + y * stride + 2 * x (out.width in pixels, strides in floats); in != out
int bhip_launch_hs_iterate(bhip_ctx* ctx, const float* deriv, const float* in, DevImg<float> out, float alpha2, int n);

// ---------------- SIFT detector: scale space, DoG extrema (sift.hip) ----------------
#define BHIP_SIFT_TILE_W BHIP_SIFT_LEVEL_TILE_WIDTH
#define BHIP_SIFT_TILE_H BHIP_SIFT_LEVEL_TILE_HEIGHT
#define BHIP_SIFT_FUSED_MAX_TAPS BHIP_SIFT_LEVEL_MAX_TAPS
// GConvertImage.convert(GrayU8, GrayF32); ImplPyramidOps.scaleImageUp with the EXTENDED bilinear interpolator (out is in * scale);
// ImplPyramidOps.scaleDown2 (out is in.width / 2 x in.height / 2); PixelMath.subtract (out = a - b).  Any strides, at most 65535 images
int bhip_launch_sift_u8_to_f32(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<float> out);
int bhip_launch_sift_scale_up(bhip_ctx* ctx, DevImg<const float> in, DevImg<float> out, int scale);
int bhip_launch_sift_scale_down2(bhip_ctx* ctx, DevImg<const float> in, DevImg<float> out);
int bhip_launch_sift_subtract(bhip_ctx* ctx, DevImg<const float> a, DevImg<const float> b, DevImg<float> out);
// One scale level in one launch: out = applyGaussian(in, kernel) and dog = out - in.  *done = false and nothing is queued when the shape is
// outside the fused form (kw even, < 3 or > BHIP_SIFT_FUSED_MAX_TAPS, a kernel as wide as the image in either direction, rows of `in` that
// are not 16-byte aligned): the caller then runs the two normalised passes and the subtract
int bhip_launch_sift_level(bhip_ctx* ctx, const float* kernel, int kw, DevImg<const float> in, DevImg<float> out, DevImg<float> dog, bool* done);
// What SiftDetector.detectFeatures does with the NonMaxLimiter list of one (octave, j) on every frame of a batch.  The list of frame b is its
// nMin[b] minima then its nMax[b] maxima ([batch][listCap] (x, y) pairs each), read through sel ([batch][2 * listCap] entry indices, the
// order QuickSelect left) and cut to maxFeatures when sel != nullptr.  Survivors are appended in list order behind count[b] records
struct SiftCandParams {
	const float *lower, *target, *upper;   // dog[j-1], dog[j], dog[j+1]
	long long imageStride;
	int stride, width, height, batch;
	const int16_t *xyMin, *xyMax;
	const int *nMin, *nMax;
	int listCap;
	const int* sel;
	int maxFeatures;
	double edgeThreshold, pixelScaleToInput, sigmaLower, sigmaTarget, sigmaUpper;
	int octave, j;
	double *x, *y, *scale;   // [batch][cap]
	uint8_t* white;          // [batch][cap]
	int16_t* where;          // [batch][cap][4]: octave, j, pixel x, pixel y
	int* count;              // [batch], advanced by the number of survivors (which may carry it beyond cap)
	int cap;
};
// bitmap, prefix: bhip_sift_cand_words(listCap) words per frame each; nPass: batch ints
static inline int bhip_sift_cand_words(int listCap) { return (2 * listCap + 255) / 256 * 8; }
int bhip_launch_sift_candidates(bhip_ctx* ctx, const SiftCandParams& P, unsigned int* bitmap, unsigned int* prefix, int* nPass);
// NonMaxLimiter's cut: where a frame's list is longer than maxFeatures, the restated sequential QuickSelect on keys -|value| (one wave per
// frame); sel and key are [batch][2 * listCap]
int bhip_launch_sift_select(bhip_ctx* ctx, const SiftCandParams& P, float* key, int* sel);

// ---------------- SIFT orientation and description (sift_describe.hip) ----------------
// What CompleteSift.handleDetection does with the detections of one (octave, j) on every frame of a batch.  The detections of frame b are
// detN[b] records of [batch][detCap] arrays in list order (bhip_launch_sift_candidates with count = detN, zero before it); the features go
// behind count[b] records of the [batch][cap] outputs, count[b] moves on by their number, and detN[b] is cleared for the next slice
struct SiftDescParams {
	const float* image;   // scale image j of the octave (not a DoG image)
	long long imageStride;
	int stride, width, height, batch;
	const double *detX, *detY, *detScale;   // ScalePoint x, y, scale: input pixels
	const uint8_t* detWhite;
	int* detN;
	int detCap;
	double pixelScaleToInput;
	// OrientationHistogramSift
	int histogramSize;
	double sigmaEnlarge, histAngleBin;
	const double* expTable;   // BHIP_CSIFT_EXP_TABLE samples of exp(-0.5 * i * 0.1)
	int* nAngles;             // [batch][detCap]
	int* angleOffset;         // [batch][detCap]: the exclusive scan of nAngles
	double* angles;           // [batch][detCap][BHIP_CSIFT_ANGLE_SLOTS]
	int* nFeat;               // [batch]
	// DescribePointSift
	int widthSubregion, widthGrid, numHistogramBins, dof;
	double sigmaToPixels, histogramBinWidth, maxDescriptorElementValue;
	const double* binAngle;       // k * histogramBinWidth, numHistogramBins of them
	const float* gaussianWeight;  // (widthSubregion * widthGrid)^2
	// the features
	double *x, *y, *scale, *orientation;   // [batch][cap]
	double* desc;                          // [batch][cap][dof]
	uint8_t* white;                        // [batch][cap]
	int* count;                            // [batch]
	int cap;
};
// generic: the describe kernel that takes any grid, also for the default one (BHIP_SIFT_DESCRIBE_GENERIC: parity cross-check of the two)
int bhip_launch_sift_describe(bhip_ctx* ctx, const SiftDescParams& P, bool generic);
// tables.cpp.  The BHIP_CSIFT_EXP_TABLE doubles of OrientationHistogramSift's approximateGauss, and DescribeSiftCommon.createGaussianWeightKernel:
// gaussian2D_F32(sigma, radius, odd = false, normalize = false) divided by its largest element, (2 * radius)^2 floats
std::vector<double> bhip_sift_exp_table();
std::vector<float> bhip_sift_gaussian_weight(double sigma, int radius);

// ---------------- dense descriptors: HOG and dense SIFT (dense.hip) ----------------
// The records of frame b: desc + b*cap*dof, xy + b*cap*2; only the first cap of a frame's `total` descriptors are written (`total` is the
// host's: the grid of a frame depends on its size alone)
struct DenseOut {
	double* desc;
	int32_t* xy;
	int cap;
};
struct DenseHogParams {
	int orientationBins, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, stepBlock;
	int cellRows, cellCols;   // fast variant: the cell grid of the frame
	int numX, numY, dof;      // descriptors per row / per column of the frame
};
struct DenseSiftParams {
	int widthSubregion, widthGrid, numHistogramBins, dof;
	double histogramBinWidth, maxDescriptorElementValue;
	int x0, y0, spanX, spanY;   // X0, Y0, X1 - X0, Y1 - Y0 of DescribeDenseSiftAlg.process
	int numX, numY;
};
// every count[b] = total
int bhip_launch_dense_count(bhip_ctx* ctx, int* count, int batch, int total);
// DescribeDenseHogFastAlg.computeCellHistograms: cells[batch][cellRows][cellCols][orientationBins]; T: float or uint8_t (converted, exact)
template <class T>
int bhip_launch_dense_hog_cells(bhip_ctx* ctx, DevImg<const T> in, const DenseHogParams& P, float* cells);
// computeDescriptor of every block: the copy into doubles and normalizeDescriptor(d, 0.2)
int bhip_launch_dense_hog_blocks(bhip_ctx* ctx, const DenseHogParams& P, const float* cells, int batch, DenseOut out);
// DescribeDenseHogAlg.computePixelFeatures, as far as it is shared by the blocks of a pixel: findex[batch][H][W] = orientation / angleBinSize and
// sumsq = dx*dx + dy*dy, both float (the magnitude is Math.sqrt of the widened sum)
template <class T>
int bhip_launch_dense_hog_pixels(bhip_ctx* ctx, DevImg<const T> in, int orientationBins, float* findex, float* sumsq);
// DescribeDenseHogAlg.process; weights: computeWeightBlockPixels, (cellsPerBlockY * pixelsPerCell) x (cellsPerBlockX * pixelsPerCell) doubles on the device
int bhip_launch_dense_hog_std(bhip_ctx* ctx, const DenseHogParams& P, const float* findex, const float* sumsq, const double* weights, int width, int height,
							  int batch, DenseOut out);
// DescribeDenseSiftAlg.precomputeAngles: angle[batch][H][W] double, magnitude float.  s16: T is uint8_t and the gradient is GradientThree's GrayS16
// one (b - a, read through getF); otherwise (a - b) * 0.5f
template <class T>
int bhip_launch_dense_sift_pixels(bhip_ctx* ctx, DevImg<const T> in, double* angle, float* magnitude);
// DescribeDenseSiftAlg.process; gaussianWeight, binAngle: on the device, as SiftDescParams'
int bhip_launch_dense_sift(bhip_ctx* ctx, const DenseSiftParams& P, const double* angle, const float* magnitude, const float* gaussianWeight, const double* binAngle,
						   int width, int height, int batch, DenseOut out);
// tables.cpp.  DescribeDenseHogAlg.computeWeightBlockPixels: rows x cols doubles
std::vector<double> bhip_dense_hog_weight_table(int rows, int cols);

// ---------------- thresholding, FactoryThresholdBinary, and the GrayU8 blurs (threshold.hip) ----------------
#define BHIP_THRESH_FUSED_MAX_RADIUS 16   // blur radius up to which a GrayU8 local threshold (and blur) runs as one launch out of LDS
// the compare of a pixel with its threshold: px <= thr (down), px > thr (up: fixed, local, min/max), !(px <= thr) (up: block mean, Otsu; differs on NaN)
enum { BHIP_CMP_LE = 0, BHIP_CMP_GT = 1, BHIP_CMP_NOT_LE = 2 };
// thr: the int or float threshold; imageThr != nullptr: one int threshold per image in device memory instead (GrayU8)
int bhip_launch_threshold_global(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<uint8_t> out, int thr, const int* imageThr, int mode);
int bhip_launch_threshold_global(bhip_ctx* ctx, DevImg<const float> in, DevImg<uint8_t> out, float thr, const int* imageThr, int mode);
// ImageStatistics.histogram(GrayU8, minValue, int[length]), length <= 256: hist[batch][length] += counts (zeroed by the caller); a value outside
// [minValue, minValue + length) is dropped
int bhip_launch_hist_u8(bhip_ctx* ctx, DevImg<const uint8_t> in, int* hist, int minValue = 0, int length = 256);
int bhip_launch_otsu_global(bhip_ctx* ctx, const int* hist, int batch, int totalPixels, double scale, int* thr);
template <class T>
int bhip_launch_local_compare(bhip_ctx* ctx, DevImg<const T> in, DevImg<const T> blur, DevImg<uint8_t> out, float scale, bool down);
// one direction of BlurImageOps.mean / gaussian on GrayU8; devTaps: 2*radius+1 Kernel1D_S32 taps in device memory, nullptr = the mean
int bhip_launch_blur_u8_pass(bhip_ctx* ctx, bool vertical, const int32_t* devTaps, int radius, DevImg<const uint8_t> in, DevImg<uint8_t> out);
// both directions, radius <= BHIP_THRESH_FUSED_MAX_RADIUS; hostTaps: the taps in host memory (nullptr = the mean); compare: `out` is the local
// threshold's 0/1 image instead of the blurred one
int bhip_launch_blur_u8_fused(bhip_ctx* ctx, const int32_t* hostTaps, int radius, DevImg<const uint8_t> in, DevImg<uint8_t> out, bool compare, float scale, bool down);
struct ThreshBlocks {
	int kind;                // BHIP_THRESHOLD_BLOCK_MIN_MAX / _MEAN / _OTSU
	int bw, bh, nbx, nby;    // ThresholdBlock.selectBlockSize and the stats grid
	int local, down, useOtsu2;
	double scale, minimumSpread, tuning;
};
size_t bhip_block_threshold_scratch(int kind, int nbx, int nby, int images);
// `chunk` images go through the three stages at a time; scratch: bhip_block_threshold_scratch(kind, nbx, nby, chunk) bytes
template <class T>
int bhip_launch_block_threshold(bhip_ctx* ctx, const ThreshBlocks& c, DevImg<const T> in, DevImg<uint8_t> out, void* scratch, int chunk);

// ---------------- BinaryImageOps: logic, morphology, label utilities (binary_ops.hip) and blob labelling (label.hip) ----------------
// iterations of erode / dilate that one launch applies inside an LDS tile (its halo); longer runs ping-pong between context scratch images
#define BHIP_MORPH_FUSED_MAX 4
// the neighbourhood operations one kernel serves: BHIP_MORPH_ERODE4 .. BHIP_MORPH_DILATE8 of the header, then these
#define BHIP_MORPH_EDGE4 4
#define BHIP_MORPH_EDGE8 5
#define BHIP_MORPH_REMOVE_POINT_NOISE 6
// op: BHIP_LOGIC_*; b == nullptr: invert(a).  out may be a or b
int bhip_launch_binary_logic(bhip_ctx* ctx, int op, DevImg<const uint8_t> a, const DevImg<const uint8_t>* b, DevImg<uint8_t> out);
// n iterations (1 .. BHIP_MORPH_FUSED_MAX) of a BHIP_MORPH_* operation in one launch; in and out must not overlap
int bhip_launch_binary_morph(bhip_ctx* ctx, int op, int outsideZero, int n, DevImg<const uint8_t> in, DevImg<uint8_t> out);
int bhip_launch_relabel(bhip_ctx* ctx, DevImg<int32_t> img, const int* devLabels, int numLabels);
int bhip_launch_label_to_binary(bhip_ctx* ctx, DevImg<const int32_t> in, DevImg<uint8_t> out, const uint8_t* devSelected, int numSelected);
size_t bhip_label_scratch(int width, int height, int images);
// width * height must fit an int and the image at most 65535 tiles of 32 rows high; scratch: bhip_label_scratch(width, height, in.batch) bytes
int bhip_launch_label_blobs(bhip_ctx* ctx, bool eight, DevImg<const uint8_t> in, DevImg<int32_t> out, int* devNumBlobs, void* scratch);

// ---------------- line detection: edge features (edge.hip), Hough transforms, relaxed block NMS, mean-shift peaks (hough.hip) ----------------
int bhip_launch_grad_intensity_abs_s16(bhip_ctx* ctx, DevImg<const int16_t> dx, DevImg<const int16_t> dy, DevImg<float> out);
// GradientToEdgeFeatures.nonMaxSuppressionCrude4 on float or int16_t derivatives; intensity and out must not overlap
template <class T>
int bhip_launch_edge_nonmax_crude4(bhip_ctx* ctx, DevImg<const float> intensity, DevImg<const T> dx, DevImg<const T> dy, DevImg<float> out);
// HoughTransformBinary.computeParameters with HoughParametersPolar: devCos / devSin are numBinsAngle floats, counts batch * numBinsAngle *
// numBinsRange ints of scratch, transform numBinsRange wide and numBinsAngle high.  width * height <= 2^24, batch and numBinsAngle <= 65535
int bhip_launch_hough_binary_polar(bhip_ctx* ctx, DevImg<const uint8_t> bin, const float* devCos, const float* devSin, int numBinsAngle, int numBinsRange, float rMax,
								   DevImg<float> transform, int* counts);
// HoughTransformGradient.transform with HoughParametersFootOfNorm (T: float or int16_t derivatives) on the images of the views: at most
// 65535, and images * width * height < 2^32 - 1.  The first `cap` edge pixels of an image (raster order) vote; devN[b] is their number, which
// may exceed cap.  scratch: bhip_hough_gradient_scratch(width, height, images, cap) bytes (0: the size could not be determined)
size_t bhip_hough_gradient_scratch(int width, int height, int images, int cap);
template <class T>
int bhip_launch_hough_gradient_foot(bhip_ctx* ctx, DevImg<const T> dx, DevImg<const T> dy, DevImg<const uint8_t> bin, DevImg<float> transform, int cap, int* devN,
									void* scratch);
// NonMaxBlock with NonMaxBlockSearchRelaxed.Max: one bit per pixel in block-raster order (zeroed bitmap of `words` words per image, more
// than nbx * nby * (radius+1)^2 bits); bhip_launch_word_prefix ranks them, bhip_launch_relaxed_to_xy writes the list
int bhip_launch_nonmax_relaxed(bhip_ctx* ctx, DevImg<const float> img, int radius, float threshold, int border, unsigned int* bitmap, int words, int nbx);
int bhip_launch_relaxed_to_xy(bhip_ctx* ctx, const unsigned int* bitmap, const unsigned int* wordPrefix, int words, int nbx, int batch, int radius, int border,
							  int16_t* xy, int cap);
// MeanShiftPeak.search from the first min(n[b], cap) integer peaks of every image (n == nullptr: cap of them); weights: device table of
// (2*radius+1)^2 floats, unused when radius <= 0 (no refinement).  peak [batch][cap][2], intensity [batch][cap]: the image at the integer peak
int bhip_launch_mean_shift_peak(bhip_ctx* ctx, DevImg<const float> img, const int16_t* xy, const int* n, int cap, int radius, int maxIterations, float convergenceTol,
								const float* weights, float* peak, float* intensity);

// ---------------- EnhanceImageOps: histogram equalisation, local equalisation, sharpen (enhance.hip; the histogram is k_hist_u8) ----------------
// EnhanceImageOps.equalize on `batch` histograms of `length` <= 256 bins in device memory
int bhip_launch_equalize_table(bhip_ctx* ctx, const int* hist, int length, int batch, int* transform);
// applyTransform; tableStride: ints between the tables of two images, 0 = one table for the batch.  A pixel >= length gives 0.  out may be in
int bhip_launch_apply_transform(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<uint8_t> out, const int* table, long long tableStride, int length);
// equalizeLocal as the rank of the centre pixel in its shifted window (enhance.hip): the direct count out of an LDS tile, which needs
// bhip_equalize_local_direct_fits, and the sliding histogram, any radius.  in and out must not overlap; at most 65535 images
bool bhip_equalize_local_direct_fits(int radius, int width, int height);
int bhip_launch_equalize_local_direct(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<uint8_t> out, int radius, int histogramLength);
int bhip_launch_equalize_local_sliding(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<uint8_t> out, int radius, int histogramLength);
// sharpen4 / sharpen8 (rule 4 / 8), T = uint8_t or float; in and out must not overlap
template <class T>
int bhip_launch_sharpen(bhip_ctx* ctx, int rule, DevImg<const T> in, DevImg<T> out);
