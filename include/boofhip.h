/*
 * boofhip.h -- C ABI of libboofhip.so, the MI355X (gfx950) provider for BoofCV's
 * detect -> describe -> associate hot path.
 *
 * This is the drop-in boundary: every entry point below is what a JNI shim for the reference would bind
 * (see INTEGRATION.md for the Java side).  Citations name the reference interface each function replaces;
 * abbreviations (paths under the reference tree):
 *   F: = main/boofcv-feature/src/main/java/boofcv/    I: = main/boofcv-ip/src/main/java/boofcv/
 *   T: = main/boofcv-types/src/main/java/boofcv/
 *
 * Conventions
 *  - plain C, no C++ or torch types; the caller owns every host buffer, the library owns device memory;
 *  - every function returns 0 (BHIP_OK) or a negative bhip_status and never throws or aborts;
 *    bhip_last_error(ctx) gives the message.  A Java shim turns a non-zero status into RuntimeException,
 *    which is the reference's own "override did not handle it, run the Java code" signal
 *    (I:alg/filter/convolve/BOverrideConvolveImage.java:53-62);
 *  - one bhip_ctx per host thread per device; calls on one ctx are serialised on one HIP stream
 *    (reference objects are not thread safe either: one instance per thread);
 *  - images are GrayF32: pixel (x,y) = data[startIndex + y*stride + x]  (T:struct/image/ImageBase.java:34-52),
 *    so sub-images (startIndex != 0, stride > width) work everywhere;
 *  - pointers named dev_* are device (HBM) addresses on the ctx's device; every other pointer is host memory;
 *  - there is no CPU fallback inside the library: without a usable GPU bhip_ctx_create fails;
 *  - handles may be destroyed in any order and more than once: bhip_ctx_destroy releases the device side of every bhip_surf created on
 *    that context (they become inert: every call on them returns BHIP_ERR_INVALID, bhip_surf_destroy then only frees the shell; the same
 *    holds for bhip_klt and bhip_klt_destroy, bhip_bg and bhip_bg_destroy), a
 *    pointer that is not a live handle is refused with BHIP_ERR_INVALID, and once the process is exiting the destroy calls do nothing
 *    (a finaliser that runs after the HIP runtime has shut down is harmless);
 *  - a context must not be destroyed while another thread is inside a call on it or on an object created on it.
 */
#ifndef BOOFHIP_H
#define BOOFHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
	BHIP_OK = 0,
	BHIP_ERR_INVALID = -1,     /* bad argument / shape (IllegalArgumentException in the reference) */
	BHIP_ERR_UNSUPPORTED = -2, /* configuration not implemented on the GPU: caller should use the Java path */
	BHIP_ERR_HIP = -3,         /* HIP runtime error (message has the hipError string) */
	BHIP_ERR_NOMEM = -4,
	BHIP_ERR_CAPACITY = -5     /* internal fixed-capacity list overflowed even after regrow */
} bhip_status;

typedef struct bhip_ctx bhip_ctx;
typedef struct bhip_surf bhip_surf;
typedef struct bhip_klt bhip_klt;   /* pyramid KLT point tracker; same handle rules as bhip_surf */
typedef struct bhip_bg bhip_bg;     /* stationary background models of a batch of streams; same handle rules as bhip_surf */

/* ---- configuration structs: same field names and defaults as the reference's Config* classes ---- */

/* F:abst/feature/detect/interest/ConfigFastHessian.java:33-70 */
typedef struct {
	float detectThreshold;     /* 1 */
	int extractRadius;         /* 2 */
	int maxFeaturesPerScale;   /* -1; > 0: SelectNBestFeatures per level (order = the restated ddogleg QuickSelect, unpinned vs the real jar) */
	int initialSampleSize;     /* 1 */
	int initialSize;           /* 9 */
	int numberScalesPerOctave; /* 4 */
	int numberOfOctaves;       /* 4 */
	int scaleStepSize;         /* 6 */
} bhip_fh_cfg;

/* F:abst/feature/describe/ConfigSurfDescribe.java:34-78 (Speed and Stability merged; useHaar=false only) */
typedef struct {
	int widthLargeGrid;    /* 4 */
	int widthSubRegion;    /* 5 */
	int widthSample;       /* 3 */
	double weightSigma;    /* Speed: 4.5 */
	int overLap;           /* Stability: 2 */
	double sigmaLargeGrid; /* Stability: 2.5 */
	double sigmaSubRegion; /* Stability: 2.5 */
} bhip_surf_cfg;

/* F:abst/feature/orientation/ConfigSlidingIntegral.java:34-54 (stable) /
 * ConfigAverageIntegral.java:34-51 (fast; windowSize ignored) */
typedef struct {
	double objectRadiusToScale; /* 1/BoofDefaults.SURF_SCALE_TO_RADIUS = 0.5 */
	double samplePeriod;        /* sliding 0.65, average 1 */
	double windowSize;          /* sliding pi/3 */
	int radius;                 /* sliding 8, average 6 */
	double weightSigma;         /* -1 */
	int sampleWidth;            /* 6 */
} bhip_ori_cfg;

/* F:alg/tracker/klt/KltConfig.java:32-49 */
typedef struct {
	int forbiddenBorder;    /* 0; not used by the reference either */
	float maxPerPixelError; /* 25 */
	int maxIterations;      /* 15 */
	float minDeterminant;   /* 0.001f */
	float minPositionDelta; /* 0.01f */
} bhip_klt_cfg;

/* F:factory/feature/disparity/ConfigDisparityBM.java:31-87 (errorType = SAD; subpixel is the choice between the _u8 and _f32 entry points) */
typedef struct {
	int minDisparity;        /* 0; must be >= 0 */
	int rangeDisparity;      /* 100; must be >= 1 */
	int regionRadiusX;       /* 3 */
	int regionRadiusY;       /* 3 */
	double maxPerPixelError; /* 0: the test is off (any value whose (int)(regionWidth*regionHeight*maxPerPixelError) is <= 0) */
	int validateRtoL;        /* 1; < 0: off */
	double texture;          /* 0.15; off when (int)(10000*texture) <= 0 */
} bhip_disparity_bm_cfg;

/* F:alg/tracker/klt/KltTrackFault.java:28-44 (ordinals).  BHIP_KLT_REFERENCE_THROWS: the position is one of the float round-off cases at the image
 * border where KltTracker.computeSubImageBounds / BilinearRectangle_F32.region throw IllegalArgumentException (in Java the exception leaves
 * PointTrackerKltPyramid.process); the library never reads outside the image, gives the track this fault and drops it. */
#define BHIP_KLT_SUCCESS 0
#define BHIP_KLT_DRIFTED 1
#define BHIP_KLT_OUT_OF_BOUNDS 2
#define BHIP_KLT_FAILED 3
#define BHIP_KLT_LARGE_ERROR 4
#define BHIP_KLT_REFERENCE_THROWS 5

void bhip_fh_cfg_default(bhip_fh_cfg* c);
void bhip_klt_cfg_default(bhip_klt_cfg* c);
void bhip_disparity_bm_cfg_default(bhip_disparity_bm_cfg* c);
void bhip_surf_cfg_default(bhip_surf_cfg* c);
void bhip_ori_cfg_default(bhip_ori_cfg* c, int stable);

/* ---- context ---- */
int bhip_ctx_create(int device, bhip_ctx** out);
/* same, but run on an existing hipStream_t (e.g. torch's current stream) instead of a private one */
int bhip_ctx_create_on_stream(int device, void* hip_stream, bhip_ctx** out);
int bhip_ctx_destroy(bhip_ctx* ctx);
int bhip_ctx_synchronize(bhip_ctx* ctx);
const char* bhip_last_error(bhip_ctx* ctx);
/* Page-locked ("pinned") host memory for the arrays a caller exchanges with the library -- what a JNI provider wraps in direct
 * ByteBuffers (NewDirectByteBuffer) for frames, fetched results and descriptor lists: copies to and from it are DMA transfers, copies
 * from ordinary (pageable) arrays go through the runtime's staging buffer.  Every entry point accepts either kind.  The block is not
 * tied to the context's lifetime; release it with bhip_host_free (a no-op for NULL and once process exit has begun). */
int bhip_host_alloc(bhip_ctx* ctx, long long bytes, uint8_t** host_mem);
int bhip_host_free(void* host_mem);
const char* bhip_version(void);
/* optional per-kernel timing with HIP events on the ctx stream (bench.py's live roofline numbers).  report writes one text line per
 * kernel tag, "tag launches total_ms algorithmic_bytes algorithmic_flops", and returns the buffer size it needs. */
int bhip_profile_enable(bhip_ctx* ctx, int on);
int bhip_profile_reset(bhip_ctx* ctx);
int bhip_profile_report(bhip_ctx* ctx, char* out, int cap);

/* ---- detect + describe: FactoryDetectDescribe.surfStable / surfFast -> DetectDescribePoint<GrayF32,BrightFeature>
 *      (F:factory/feature/detdesc/FactoryDetectDescribe.java:118-135,209-226; F:abst/feature/detdesc/DetectDescribePoint.java:32-46;
 *       F:abst/feature/detdesc/WrapDetectDescribeSurf.java:93-159).  NULL config = reference defaults. ---- */
#define BHIP_SURF_INITIAL_CAPACITY 8192   /* key-point lists start at this many entries per image and regrow; results do not depend on it */
int bhip_surf_create(bhip_ctx* ctx, const bhip_fh_cfg* fh, const bhip_surf_cfg* surf, const bhip_ori_cfg* ori, int stable, bhip_surf** out);
int bhip_surf_destroy(bhip_surf* s);
/* detect(T input) on a batch of host images (batch = 1 is the reference call).  Results are recycled by the next detect,
 * as in the reference (DetectDescribePoint.java:38-40). */
int bhip_surf_detect_f32(bhip_surf* s, const float* const* img, const int* startIndex, const int* stride, int width, int height, int batch);
/* same on a device-resident batch: image i starts at dev_images + i*imageStride floats, rows are `stride` floats apart.
 * Asynchronous on the ctx stream apart from one small count read-back: the call returns when the key points are counted (the frames have
 * been consumed by then), with the describe kernels still queued; counts are valid at once, every fetch waits for the results, device
 * views (bhip_surf_dev_view) and the resident associations are ordered behind them on the same stream. */
int bhip_surf_detect_dev_f32(bhip_surf* s, const float* dev_images, long long imageStride, int stride, int width, int height, int batch);
/* The same on GrayU8 frames: the integral images are GrayS32 (GIntegralImageOps.getIntegralType) and every stage runs on integer taps --
 * IntegralImageOps.transform(GrayU8, GrayS32), FastHessianFeatureDetector<GrayS32>, SparseIntegralGradient_NoBorder_I32 for the
 * orientation and the descriptor, convolveSparse(GrayS32) for the Laplacian sign.  Results through the same count / fetch calls;
 * bhip_surf_fetch_integral then returns the int32 words. */
int bhip_surf_detect_u8(bhip_surf* s, const uint8_t* const* img, const int* startIndex, const int* stride, int width, int height, int batch);
/* FactoryDetectDescribe.surfColorStable / surfColorFast (F:factory/feature/detdesc/FactoryDetectDescribe.java:154-176,246-268) on one
 * Planar<GrayF32> frame given as numBands band pointers of one shape: SurfPlanar_to_DetectDescribePoint.detect
 * (F:abst/feature/detdesc/SurfPlanar_to_DetectDescribePoint.java:62-77) = band average -> integral images of the average and of every band
 * -> Fast-Hessian on the average -> DetectDescribeSurfPlanar.describe (F:alg/feature/detdesc/DetectDescribeSurfPlanar.java:110-124;
 * orientation object radius = scale) -> DescribePointSurfPlanar.describe (F:alg/feature/describe/DescribePointSurfPlanar.java:100-114;
 * bands concatenated, normalised once; Laplacian sign from the average).  Results through bhip_surf_count / _fetch / _dev_view with
 * image = 0; bhip_surf_dof() then returns numBands * 64.  getRadius(i) of this wrapper is the scale itself (no factor 2). */
int bhip_surf_detect_planar_f32(bhip_surf* s, const float* const* bands, int numBands, int startIndex, int stride, int width, int height);
/* getNumberOfFeatures() of image `image` of the last detect */
int bhip_surf_count(bhip_surf* s, int image, int* n);
/* the same for every image of the last batch in one call: counts[i] for i < batch (capacity >= batch) */
int bhip_surf_counts(bhip_surf* s, int* counts, int capacity);
/* getLocation(i)/scale -> xy_scale[3n] ; getOrientation(i) -> angle[n] ; BrightFeature.white -> white[n] ;
 * getDescription(i).value -> desc[64n].  getRadius(i) = scale*2 (BoofDefaults.SURF_SCALE_TO_RADIUS).  Any pointer may be NULL. */
int bhip_surf_fetch(bhip_surf* s, int image, double* xy_scale, double* angle, uint8_t* white, double* desc);
/* the same for the WHOLE batch of the last detect in one set of copies: image i's slice starts at the exclusive prefix of the counts
 * (key point k of image i at index sum(count[0..i)) + k); arrays sized with bhip_surf_total */
int bhip_surf_fetch_all(bhip_surf* s, double* xy_scale, double* angle, uint8_t* white, double* desc);
/* AssociateDescription.associate() on descriptor lists that are still resident from the last detect of `s` (F:abst/feature/associate/
 * AssociateDescription.java:42-61 with lists a provider recognises as its own getDescription() objects): problem p associates image
 * srcImage[p] (source) with image dstImage[p] (destination), ScoreAssociateEuclideanSq_F64, same rules and results as bhip_assoc_l2_f64, no
 * descriptor upload.  pairs / fit: host arrays of bhip_surf_total entries; problem p's results start at the exclusive prefix of the counts
 * of srcImage[p] (an image may be the source of one problem per call); entries of images that are no source read -1 / 0.0. */
int bhip_assoc_l2_surf(bhip_surf* s, int count, const int* srcImage, const int* dstImage, double maxErr, int backwards, int* pairs, double* fit);

/* ---- Fast-Hessian + BRIEF as one DetectDescribePoint<T,TupleDesc_B>:
 *      FactoryDetectDescribe.fuseTogether(FactoryInterestPoint.fastHessian(fh), null, FactoryDescribeRegionPoint.brief(config, imageType))
 *      (F:factory/feature/detdesc/FactoryDetectDescribe.java:279-284; F:abst/feature/detdesc/DetectDescribeFusion.java:95-127;
 *       F:abst/feature/detect/interest/WrapFHtoInterestPoint.java:47-79; F:factory/feature/describe/FactoryDescribeRegionPoint.java:187-202;
 *       F:abst/feature/describe/WrapDescribeBrief.java:47-58; F:alg/feature/describe/DescribePointBrief.java:71-89), config.fixed = true.
 *      The definition (radius, numPoints, samplePoints, compare: FactoryBriefDefinition.gaussian2(new Random(123), radius, numPoints)) is
 *      generated on the Java side, as for bhip_brief_f32.  The object is a bhip_surf: detect with bhip_surf_detect_f32 / _dev_f32 / _u8 (GrayU8
 *      frames: GrayS32 integral image + ImplDescribeBinaryCompare_U8), read locations with bhip_surf_count / _total / _fetch (desc = NULL;
 *      getOrientation(i) is 0, getRadius(i) = scale*2), destroy with bhip_surf_destroy.  Every detected point is described (process() of the
 *      fixed BRIEF always returns true), in detector order; the words are taken from the frame itself (the reference blurs a copy it never
 *      reads), with the border rule of the image type (see bhip_brief_f32 / bhip_brief_u8). ---- */
int bhip_surf_create_brief(bhip_ctx* ctx, const bhip_fh_cfg* fh, int radius, int numPoints, const int32_t* samplePoints, const int32_t* compare,
						   bhip_surf** out);
/* getDescription(i).data (TupleDesc_B: ceil(numPoints/32) ints per feature, T:struct/feature/TupleDesc_B.java) of every feature of image
 * `image` of the last detect, or of the whole batch when image = -1 (image i's slice then starts at the exclusive prefix of the counts) */
int bhip_surf_fetch_brief(bhip_surf* s, int image, int32_t* words);
/* device view of the same words (valid until the next detect on s); *words = ints per feature */
int bhip_surf_dev_view_brief(bhip_surf* s, int image, const int32_t** dev_words, int* words, int* n);
/* AssociateDescription<TupleDesc_B>.associate() with ScoreAssociateHamming_B (F:alg/descriptor/DescriptorDistance.java:196-220) on the words still
 * resident from the last detect of a BRIEF object: contract of bhip_assoc_l2_surf, rules and results of bhip_assoc_hamming, no upload */
int bhip_assoc_hamming_surf(bhip_surf* s, int count, const int* srcImage, const int* dstImage, double maxErr, int backwards, int* pairs, double* fit);
/* device views of the same results (valid until the next detect): descriptors [n][dof] doubles, laplacian signs [n] bytes */
int bhip_surf_dev_view(bhip_surf* s, int image, const double** dev_desc, const double** dev_xy_scale, const uint8_t** dev_white, int* n);
int bhip_surf_dof(bhip_surf* s);
/* total key points over the whole batch of the last detect */
int bhip_surf_total(bhip_surf* s, long long* n);

/* stage-level entry points of the detector (used by the parity tests and by the BOverride nonmax hook) */
/* describe externally supplied points (x,y,scale) on the integral image of image `image` of the last detect:
 * WrapDetectDescribeSurf.computeDescriptors (:116-128) for a caller-provided foundPoints list */
int bhip_surf_describe_points(bhip_surf* s, int image, const double* xy_scale, int n, double* angle, uint8_t* white, double* desc);
/* copy the integral image of image `image` of the last detect to host (width*height floats, dense) */
int bhip_surf_fetch_integral(bhip_surf* s, int image, float* out);

/* GIntegralImageOps.transform -> ImplIntegralImageOps.transform(GrayF32,GrayF32) (I:alg/transform/ii/impl/ImplIntegralImageOps.java:42-66) */
int bhip_integral_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, float* out, int outStart, int outStride);
/* IntegralImageFeatureIntensity.hessian(GrayF32,skip,size,GrayF32) (F:alg/feature/detect/intensity/IntegralImageFeatureIntensity.java:43-56);
 * intensity is (width/skip) x (height/skip) */
int bhip_hessian_f32(bhip_ctx* ctx, const float* ii, int iiStart, int iiStride, int width, int height, int skip, int size, float* intensity,
					 int outStart, int outStride);
/* NonMaxSuppression.process for the strict block extractor built by FactoryFeatureExtractor.nonmax(ConfigExtract(radius,threshold,border,true))
 * (F:factory/feature/detect/extract/FactoryFeatureExtractor.java:63-102; F:alg/feature/detect/extract/NonMaxBlock.java:69-94).
 * Writes up to cap (x,y) int16 pairs in block-raster order (the USE_CONCURRENT=false order); *n is the number found. */
int bhip_nonmax_block_f32(bhip_ctx* ctx, const float* intensity, int start, int stride, int width, int height, int radius, float threshold,
						  int border, int16_t* xy, int cap, int* n);
/* NonMaxBlock.process with NonMaxBlockSearchStrict.Min / .Max / .MinMax (F:alg/feature/detect/extract/NonMaxBlock.java:69-94,
 * NonMaxBlockSearchStrict.java:56-79 Max, :97-139 Min, :141-194 MinMax, checkLocalMax / checkLocalMin :196-248), the extractor
 * FactoryFeatureExtractor.nonmax builds for a strict ConfigExtract with detectMinimums and / or detectMaximums.  A minimum is the first
 * smallest value of its (radius+1)^2 block, <= thresholdMin, != -Float.MAX_VALUE and strictly below every other pixel of its clipped
 * (2*radius+1)^2 window.  The factory sets thresholdMin = -config.threshold; here the two thresholds are separate, as in the wrapper.
 * Each list is written in block-raster order, up to cap pairs; *nMin / *nMax are the numbers found (0 for a side that is not detected).
 * The candidate lists of the interface are not used (NonMaxBlock ignores them). */
int bhip_nonmax_block_minmax_f32(bhip_ctx* ctx, const float* intensity, int start, int stride, int width, int height, int radius, float thresholdMin,
								 float thresholdMax, int border, int detectMin, int detectMax, int16_t* xyMin, int* nMin, int16_t* xyMax, int* nMax, int cap);
/* FastCornerDetector.process(image, intensity) (F:alg/feature/detect/intensity/FastCornerDetector.java:123-156; intensity == NULL:
 * process(image), :161-189) with the helper FactoryIntensityPointAlg.fast(pixelTol, minContinuous, GrayU8 / GrayF32) builds
 * (F:factory/feature/detect/intensity/FactoryIntensityPointAlg.java).  Circle: DiscretizedCircle.imageOffsets(3, stride)
 * (I:misc/DiscretizedCircle.java:39-77), 16 pixels.  Class: ImplFastCorner{9..12}_{U8,F32}.checkPixel, evaluated as the rule its decision
 * tree searches (GenericFastCorner.compareToNaiveDetection): minContinuous cyclically contiguous ring pixels all > centre + pixelTol
 * (bright, "high") or all < centre - pixelTol (dark, "low").  Score: ImplFastHelper_U8 / _F32.scoreLower / scoreUpper (:47-81): the sum of
 * the ring pixels beyond the bound minus centre * count; the F32 helper's sum is an `int` that truncates toward zero after every addition
 * (Java's (int): saturating, NaN -> 0), so the sign of an F32 score does not tell the polarity.
 * Rows 3 .. height-4 and columns 3 .. width-4 in raster order; after each row the detector stops once low + high >=
 * (int)(maxFeaturesFraction * width * height) (that row is kept whole).  xyLow / xyHigh receive up to cap (x,y) pairs each in raster order,
 * *nLow / *nHigh the numbers found (they may exceed cap).  width < 7 or height < 7: empty lists, zero intensity.
 * Validation: minContinuous 9..12 (ConfigFastCorner.checkValidity, F:abst/feature/detect/interest/ConfigFastCorner.java:31-64),
 * 0 < maxFeaturesFraction <= 1 (setMaxFeaturesFraction :195-199); otherwise BHIP_ERR_INVALID and nothing is written.
 * Deviations: a negative pixelTol is BHIP_ERR_INVALID (the trees define nothing sensible there); the intensity view is written as a whole,
 * 0 in the 3-pixel border and in the rows after an early stop, where the reference leaves what an earlier frame put there (its border is
 * 0 because BaseGeneralFeatureIntensity.init zeroes on a size change) -- the result of a freshly constructed reference detector. */
int bhip_fast_u8(bhip_ctx* ctx, const uint8_t* image, int start, int stride, int width, int height, int pixelTol, int minContinuous, double maxFeaturesFraction,
				 float* intensity, int iStart, int iStride, int16_t* xyLow, int* nLow, int16_t* xyHigh, int* nHigh, int cap);
int bhip_fast_f32(bhip_ctx* ctx, const float* image, int start, int stride, int width, int height, float pixelTol, int minContinuous, double maxFeaturesFraction,
				  float* intensity, int iStart, int iStride, int16_t* xyLow, int* nLow, int16_t* xyHigh, int* nHigh, int cap);
/* StereoDisparity.process(left, right) of FactoryStereoDisparity.blockMatch(ConfigDisparityBM, GrayU8.class, GrayU8.class | GrayF32.class) with
 * errorType = SAD (F:factory/feature/disparity/FactoryStereoDisparity.java:62-144,203-240): WrapDisparityBlockMatchRowFormat / WrapBaseBlockMatch
 * (F:abst/feature/disparity/WrapBaseBlockMatch.java:42-85) over DisparityScoreBM_S32 (F:alg/feature/disparity/block/score/DisparityScoreBM_S32.java:73-205)
 * with BlockRowScoreSad.U8 (block/BlockRowScore.java:96-138, BlockRowScoreSad.java:53-67) and the selector SelectErrorWithChecks_S32.DispU8
 * (block/select/SelectErrorWithChecks_S32.java:60-162,172-190; bhip_disparity_bm_u8_u8, subpixel = false) or SelectErrorSubpixel.S32_F32
 * (block/select/SelectErrorSubpixel.java:46-75; bhip_disparity_bm_u8_f32, subpixel = true).  cfg == NULL: the reference defaults.
 * With maxD = minDisparity + rangeDisparity, rw = 2*regionRadiusX+1, rh = 2*regionRadiusY+1, inv = rangeDisparity + 1:
 *   cost    for a row y in [ry, H-ry), a left block that starts at column c in [minDisparity, W-rw] and i in [0, lm), lm = min(c - minDisparity + 1,
 *           rangeDisparity) (maxDisparityAtColumnL2R): C(y,c,i) = sum over dy = -ry..ry, j < rw of |L[y+dy][c+j] - R[y+dy][c-minDisparity-i+j]|, an int
 *           (the reference's running sums are exact in integers).  The result goes to pixel (c + rx, y).
 *   best    the first i with the smallest cost (strict <), sBest its cost.
 *   error   maxError = (int)((rw*rh)*maxPerPixelError) in double; <= 0 turns the test off; sBest > maxError gives inv.
 *   R to L  only when not rejected and validateRtoL >= 0: k = c - best - minDisparity, n = min(W-rw, k+maxD) - k - minDisparity, rBest = the first
 *           minimum of C(y, k+minDisparity+j, j) over j = 0, then 1 <= j < n; |rBest - best| > validateRtoL gives inv.  As written in the reference,
 *           a search that the image clips leaves out the j whose left block would start at column W-rw.
 *   texture only when (int)(10000*texture) = thr > 0, not rejected and lm >= 3: second = the smallest C(y,c,i) over i in [0,best-1) and [best+2,lm),
 *           Integer.MAX_VALUE when there is none; 10000*(second-sBest) <= thr*sBest gives inv, both products Java ints that wrap (lm == 3 and
 *           best == 1: the wrapped product is negative and the pixel is rejected).
 *   store   U8: (byte)value.  F32: value <= 0 or value >= lm-1 (inv included) stores (float)value, otherwise value + (float)(c0-c2) /
 *           (float)(2*(c0-2*c1+c2)) with c0, c1, c2 the costs at value-1, value, value+1: one correctly rounded fp32 division and one fp32 addition.
 *   rest    rows < ry and >= H-ry, columns < rx+minDisparity and >= W-rx hold rangeDisparity, WrapBaseBlockMatch.getInvalidValue(), with which
 *           the wrapper fills a new disparity image -- not inv.  (TestWrapDisparityBlockMatchRowFormat.borderSetToInvalid asserts a value
 *           > rangeDisparity there and contradicts the main code, which is what is followed.)
 * Validation, BHIP_ERR_INVALID and nothing is written: minDisparity < 0, rangeDisparity < 1 (ConfigDisparityBM.checkValidity), a negative radius,
 * maxD > W - 2*regionRadiusX (DisparityBlockMatchRowFormat.process throws RuntimeException), an output of type U8 with inv > 254
 * (SelectDisparityWithChecksWta.configure), H < rh.
 * Deviations: H < rh is refused, where the reference indexes outside the image; the disparity view is written as a whole on every call,
 * rangeDisparity outside the region above, where the reference leaves what an earlier pair put there -- the result of a freshly constructed
 * reference object.
 * Limits: regionRadiusX, regionRadiusY <= 7 and rangeDisparity <= 256 (<= 253 for U8, by the validation); beyond them BHIP_ERR_UNSUPPORTED and
 * nothing is written.  errorType = CENSUS: bhip_disparity_bm_census_u8_u8 / _u8_f32.  blockMatchBest5: bhip_disparity_bm5_*.  NCC, SGM and the
 * GrayF32 / GrayU16 / GrayS16 inputs have no entry point. */
int bhip_disparity_bm_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart,
							int rStride, int width, int height, uint8_t* disp, int dStart, int dStride);
int bhip_disparity_bm_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart,
							 int rStride, int width, int height, float* disp, int dStart, int dStride);
/* ---- census transform: FilterImageInterface<GrayU8, GrayU8 | GrayS32 | GrayS64> of FactoryCensusTransform (census.hip) ---- */
typedef enum { BHIP_CENSUS_BLOCK_3_3 = 0, BHIP_CENSUS_BLOCK_5_5 = 1, BHIP_CENSUS_BLOCK_7_7 = 2, BHIP_CENSUS_BLOCK_9_7 = 3, BHIP_CENSUS_BLOCK_13_5 = 4,
			   BHIP_CENSUS_CIRCLE_9 = 5 } bhip_census_variant;   /* CensusVariants ordinals (I:factory/transform/census/CensusVariants.java) */
/* The reference's sample list of a variant, as (x, y) pairs into samplesXY[0 .. 2*cap) and its length into *n: CensusTransform.createBlockSamples(r),
 * createBlockSamples(rx, ry), createCircleSamples (I:alg/transform/census/CensusTransform.java:53-98) as FactoryCensusTransform.variant picks them
 * (I:factory/transform/census/FactoryCensusTransform.java:48-93).  Order: row-major over dy, then dx, without the centre.
 *   BLOCK_3_3   3x3, 8 samples (GrayU8 words)         BLOCK_9_7    blockDense(4,3): 9x7, 62 samples
 *   BLOCK_5_5   5x5, 24 samples (GrayS32 words)       BLOCK_13_5   blockDense(5,2): 11x5 despite its name, 54 samples
 *   BLOCK_7_7   7x7, 48 samples (GrayS64 words)       CIRCLE_9     56 samples, set(row-4, col-4): the loop's row is x
 * samplesXY == NULL: only *n is written.  BHIP_ERR_INVALID and nothing is written: no such variant, n == NULL, cap smaller than the list.  No
 * context: the lists exist once, here. */
int bhip_census_variant_samples(int variant, int* samplesXY, int cap, int* n);
/* FilterCensusTransformD33U8 / D55S32 / SampleS64.process(in, out) (I:abst/transform/census/) with the factory's border, CENSUS_BORDER = REFLECT:
 * CensusTransform.dense3x3 / dense5x5 / sample_S64 (I:alg/transform/census/CensusTransform.java:107-225) over ImplCensusTransformInner and
 * ImplCensusTransformBorder (I:alg/transform/census/impl/).  Facts read from those files:
 *   formula  the inner and the border code compute the same thing, so one rule covers the image: with c = in(x,y), bit i of out(x,y) is set iff
 *            in(reflect(x+dx_i), reflect(y+dy_i)) > c; reflect(k) = -k for k < 0, 2*len-2-k for k >= len (I:core/image/border/BorderIndex1D_Reflect.java:34-41).
 *   order    3x3 and 5x5: row-major over dy, then dx, without the centre; bit 0 is the first sample (8 and 24 bits).  The sample form: the list's order.
 *   S64      sample_S64 counts its bits in an int (`long census; int bit = 1; census |= bit; bit <<= 1`, inner :203-209, border :153-167): samples
 *            0..30 set bits 0..30, sample 31 ORs in 0x80000000 sign-extended and sets bits 31..63, samples 32 and up add nothing.  Every word is
 *            the sign extension of its low 32 bits.  This is reproduced bit for bit.
 *   size     one reflection must land inside: width, height >= radius + 1, radius = 1, 2, or the largest |dx|, |dy| of the whole list as
 *            sample_S64 computes it.
 * samplesXY: nSamples (x, y) pairs.  Validation, BHIP_ERR_INVALID and nothing is written: a bad view, nSamples < 0 or > 64
 * (FilterCensusTransformSampleS64's constructor), samplesXY == NULL with nSamples > 0, an image smaller than radius + 1 in either direction.
 * Limits, BHIP_ERR_UNSUPPORTED and nothing is written: a sample with |dx| or |dy| > 7.
 * Deviations: an image smaller than radius + 1 is refused, where the reference throws or writes outside the image; the output view is written
 * as a whole and must have the input's size (the reference reshapes it).  GrayU16 inputs and sample_IU16 have no entry point. */
int bhip_census_u8_u8(bhip_ctx* ctx, const uint8_t* in, int start, int stride, int width, int height, uint8_t* out, int oStart, int oStride);
int bhip_census_u8_s32(bhip_ctx* ctx, const uint8_t* in, int start, int stride, int width, int height, int32_t* out, int oStart, int oStride);
int bhip_census_sample_u8_s64(bhip_ctx* ctx, const int* samplesXY, int nSamples, const uint8_t* in, int start, int stride, int width, int height, long long* out,
							  int oStart, int oStride);
/* StereoDisparity.process(left, right) of FactoryStereoDisparity.blockMatch with errorType = CENSUS and configCensus.variant = `variant`
 * (F:factory/feature/disparity/FactoryStereoDisparity.java:85-102): WrapDisparityBlockMatchCensus (F:abst/feature/disparity/WrapDisparityBlockMatchCensus.java:32-80)
 * runs FactoryCensusTransform.variant(variant) on both images (bhip_census_*) and the block matching of bhip_disparity_bm_u8_u8 / _u8_f32 on the
 * census images, with BlockRowScoreCensus.U8 / S32 / S64 (F:alg/feature/disparity/block/BlockRowScoreCensus.java:39-85) as the row score:
 *   cost    C(y,c,i) = sum over dy = -ry..ry, j < rw of hamming(CL[y+dy][c+j] ^ CR[y+dy][c-minDisparity-i+j]), CL / CR the census images and hamming
 *           DescriptorDistance.hamming(int | long) (F:alg/descriptor/DescriptorDistance.java:213-224), the number of set bits.  Between two GrayS64
 *           words that is the number of differing bits among 0..30, plus 33 when their sample-31 bits differ (bits 31..63 are copies of it).
 *   rest    best, error, R to L, texture, store and the border value: exactly the rules of bhip_disparity_bm_u8_u8.  createDisparitySelect is called
 *           with the input image type, so the selector is the S32 one and maxError = (int)((rw*rh)*maxPerPixelError) counts differing bits.
 * cfg == NULL: the reference defaults (ConfigDisparityError.Census's default variant is BLOCK_5_5; here the variant is an argument).
 * Validation, BHIP_ERR_INVALID and nothing is written: that of bhip_disparity_bm_u8_u8, a variant outside 0..5, an image smaller than the variant's
 * radius + 1 in either direction (bhip_census_*).
 * Limits, BHIP_ERR_UNSUPPORTED and nothing is written: regionRadiusX, regionRadiusY <= 7, rangeDisparity <= 256 (<= 253 for U8 by the validation).
 * Deviations: those of bhip_disparity_bm_u8_u8 and of bhip_census_*; the census images are context scratch (getCLeft / getCRight of the
 * reference's wrapper: run bhip_census_* on the input).  blockMatchBest5: bhip_disparity_bm5_census_*.  NCC, SGM and the GrayF32 / GrayU16 / GrayS16
 * inputs have no entry point. */
int bhip_disparity_bm_census_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* left, int lStart, int lStride,
								   const uint8_t* right, int rStart, int rStride, int width, int height, uint8_t* disp, int dStart, int dStride);
int bhip_disparity_bm_census_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* left, int lStart, int lStride,
									const uint8_t* right, int rStart, int rStride, int width, int height, float* disp, int dStart, int dStride);
/* StereoDisparity.process(left, right) of FactoryStereoDisparity.blockMatchBest5(ConfigDisparityBMBest5, GrayU8.class, GrayU8.class | GrayF32.class)
 * (F:factory/feature/disparity/FactoryStereoDisparity.java:146-201): DisparityScoreBMBestFive_S32 (F:alg/feature/disparity/block/score/
 * DisparityScoreBMBestFive_S32.java:147-267) over the row scores and the selectors of bhip_disparity_bm_u8_u8 / _u8_f32 (SAD) and of
 * bhip_disparity_bm_census_u8_u8 / _u8_f32 (CENSUS, `variant` a CensusVariants ordinal).  ConfigDisparityBMBest5 adds no field to ConfigDisparityBM,
 * so cfg is a bhip_disparity_bm_cfg; cfg == NULL: the reference defaults.  With V(y,c,i) = the cost C(y,c,i) of bhip_disparity_bm_u8_u8 (the
 * sub-block that starts at column c, rows y-ry..y+ry), rx = regionRadiusX, ry = regionRadiusY, rw = 2*rx+1, rh = 2*ry+1:
 *   score   for a selector column col in [minDisparity, W-(4*rx+1)] and i in [0, lm), lm = min(col - minDisparity + 1, rangeDisparity):
 *           F(y,col,i) = V(y,col+rx,i) + the two smallest of { V(y-ry,col,i), V(y-ry,col+2*rx,i), V(y+ry,col,i), V(y+ry,col+2*rx,i) }
 *           (computeScoreFive's three compare() tests with SelectErrorWithChecks_S32.compare(a,b) = Integer.compare(-a,-b); ties give equal sums).
 *           The result goes to pixel (col + 2*rx, y).  F reaches 3*255*15*15 = 172125: an int, not 16 bits.
 *   select  best, error, R to L, texture and store: the rules of bhip_disparity_bm_u8_u8 on F, the selector configured with radius 2*rx
 *           (computeDisparity.configure(disparity, minDisparity, maxDisparity, radiusX*2)): region width 4*rx+1 in the R to L search,
 *           n = min(W-(4*rx+1), k+maxD) - k - minDisparity.
 *   error   maxError = (int)(rw*rh*maxPerPixelError*3) in double (FactoryStereoDisparity.java:159-162: three regions).
 *   rows    max(2*ry, 1) <= y < H-2*ry: computeFirstRow selects nothing and computeRemainingRows selects from image row max(rh, 4*ry) on, so
 *           with ry == 0 row 0 is never selected (plain block matching selects it in computeFirstRow).
 *   rest    every other pixel -- rows outside that range, columns < 2*rx+minDisparity and >= W-2*rx -- holds rangeDisparity.
 * Validation, BHIP_ERR_INVALID and nothing is written: everything bhip_disparity_bm_u8_u8 refuses, with the same tests --
 * minDisparity + rangeDisparity > W - 2*regionRadiusX (DisparityBlockMatchRowFormat.process tests radiusX, not 2*radiusX) and H < rh, where the
 * reference indexes outside the image; for the census forms also what bhip_disparity_bm_census_u8_u8 refuses.  Two shapes are legal and answer
 * BHIP_OK with the whole view set to rangeDisparity: rh <= H < 4*ry+1 (no output row), and W-(4*rx+1) < minDisparity (no selector column).
 * Limits, BHIP_ERR_UNSUPPORTED and nothing is written: regionRadiusX, regionRadiusY <= 7, rangeDisparity <= 256 (<= 253 for U8 by the validation).
 * Deviations: those of bhip_disparity_bm_u8_u8 (the view is written as a whole: the result of a freshly constructed reference object, single
 * threaded: BoofConcurrency.USE_CONCURRENT = false, one block over all rows) and, for the census forms, of bhip_disparity_bm_census_u8_u8. */
int bhip_disparity_bm5_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart,
							 int rStride, int width, int height, uint8_t* disp, int dStart, int dStride);
int bhip_disparity_bm5_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* left, int lStart, int lStride, const uint8_t* right, int rStart,
							  int rStride, int width, int height, float* disp, int dStart, int dStride);
int bhip_disparity_bm5_census_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* left, int lStart, int lStride,
									const uint8_t* right, int rStart, int rStride, int width, int height, uint8_t* disp, int dStart, int dStride);
int bhip_disparity_bm5_census_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* left, int lStart, int lStride,
									 const uint8_t* right, int rStart, int rStride, int width, int height, float* disp, int dStart, int dStride);
/* ---- image remap: ImageDistort<T,T>, GrayU8 -> GrayU8 and GrayF32 -> GrayF32 (distort.hip) ---- */
typedef enum { BHIP_INTERP_NEAREST_NEIGHBOR = 0, BHIP_INTERP_BILINEAR = 1, BHIP_INTERP_BICUBIC = 2, BHIP_INTERP_POLYNOMIAL4 = 3 } bhip_interp;   /* InterpolationType ordinals */
typedef enum { BHIP_BORDER_SKIP = 0, BHIP_BORDER_EXTENDED = 1, BHIP_BORDER_NORMALIZED = 2, BHIP_BORDER_REFLECT = 3, BHIP_BORDER_WRAP = 4, BHIP_BORDER_ZERO = 5 } bhip_border;   /* BorderType ordinals */
typedef enum { BHIP_DISTORT_AFFINE = 1, BHIP_DISTORT_HOMOGRAPHY = 2 } bhip_distort_model;
/* ImageDistort.apply(src, dst), apply(src, dst, mask) and apply(src, dst, x0, y0, x1, y1) of FactoryDistort.distortSB(cached, interp, type)
 * (I:factory/distort/FactoryDistort.java:96-122; callers I:alg/distort/DistortImageOps.java:70-145) with interp from
 * FactoryInterpolation.createPixelS(0, 255, NEAREST_NEIGHBOR | BILINEAR, ZERO | EXTENDED, type): ImageDistortCache_SB
 * (I:alg/distort/ImageDistortCache_SB.java:76-206) on a map the caller has filled with its PixelTransform, which is also what
 * ImageDistortBasic_SB (I:alg/distort/ImageDistortBasic_SB.java:56-135) computes with that transform.  Single-threaded reference results, bit
 * for bit (the library is built with -ffp-contract=off).
 * For every destination pixel (x, y) of the crop [x0,x1) x [y0,y1), with a source of sw x sh and (sx, sy) = map[y*dw + x]:
 *   inside   sx >= 0 && sx <= sw-1 && sy >= 0 && sy <= sh-1 (the int bounds converted to float).
 *   render   renderAll != 0: dst = assign(get(sx, sy)) for every pixel.  renderAll == 0 (what BorderType.SKIP becomes in
 *            DistortImageOps.distortSingle and RectifyImageOps.rectifyImage, with border EXTENDED): only the inside pixels are assigned, every
 *            other pixel of dst keeps what it held.
 *   mask     when not NULL, 1 for an inside pixel and 0 otherwise, for every pixel of the crop in both render modes.
 *   get      BILINEAR (ImplBilinearPixel_U8.java:48-90, ImplBilinearPixel_F32.java:48-90): when !(sx < 0 || sy < 0 || sx > sw-2 || sy > sh-2),
 *            xt = (int)sx, yt = (int)sy, ax = sx - xt, ay = sy - yt and the taps are pixels; otherwise xf = (float)floor(sx), xt = (int)xf,
 *            ax = sx - xf (same in y) and the taps come from the border.  val = (1-ax)*(1-ay)*p(xt,yt); val += ax*(1-ay)*p(xt+1,yt);
 *            val += ax*ay*p(xt+1,yt+1); val += (1-ax)*ay*p(xt,yt+1); each product left to right, in float.
 *            NEAREST_NEIGHBOR (NearestNeighborPixel_U8.java:56-72, NearestNeighborPixel_F32.java:56-72): pixel ((int)sx, (int)sy) when
 *            !(sx < 0 || sy < 0 || sx > sw-1 || sy > sh-1), otherwise the border at ((int)floor(sx), (int)floor(sy)).
 *   border   ZERO (ImageBorderValue, value 0): the pixel when in bounds, else 0.  EXTENDED (BorderIndex1D_Extend): each coordinate clamped
 *            to [0, n-1].
 *   assign   AssignPixelValue_SB.java:31-59: GrayF32 stores the float; GrayU8 stores (byte)value, Java's float -> int (toward zero, saturating,
 *            NaN -> 0) and then the low eight bits.
 * Domain: coordinates are finite with |v| <= 2^30.  For NaN, infinities and anything larger nothing outside the source view is read and
 * nothing outside the crop is written; the values stored for such pixels are unspecified.
 * Deviations: (1) ImageDistortCache_SB.renderAll indexes its map with the destination's array index (map[indexDst], :143), which is only
 * right for a destination with startIndex = 0 and stride = width; the library indexes the map by y*dw + x for every destination layout --
 * the same result for a dense destination, and what ImageDistortBasic_SB computes.  (2) Source and destination (and mask) must not overlap;
 * this is not detected.
 * BHIP_ERR_UNSUPPORTED and nothing is written: interp other than NEAREST_NEIGHBOR or BILINEAR; border other than ZERO or EXTENDED (REFLECT
 * and WRAP index outside the array in the reference for far coordinates, NORMALIZED is a different class).
 * BHIP_ERR_INVALID and nothing is written: an empty source or destination, a crop that is not inside the destination (0 <= x0 <= x1 <= dw,
 * 0 <= y0 <= y1 <= dh), a NULL map.
 * Host form: one image; map is dw*dh interleaved (x, y) float pairs in host memory; mask may be NULL (mStart, mStride then unread). */
int bhip_distort_map_u8(bhip_ctx* ctx, const uint8_t* src, int sStart, int sStride, int sw, int sh, const float* map, int dw, int dh, int x0, int y0, int x1,
						int y1, int interp, int border, int renderAll, uint8_t* dst, int dStart, int dStride, uint8_t* mask, int mStart, int mStride);
int bhip_distort_map_f32(bhip_ctx* ctx, const float* src, int sStart, int sStride, int sw, int sh, const float* map, int dw, int dh, int x0, int y0, int x1,
						 int y1, int interp, int border, int renderAll, float* dst, int dStart, int dStride, uint8_t* mask, int mStart, int mStride);
/* The host form with the coordinates computed from a model instead of read from a map: see bhip_distort_model_dev_u8 for the models, their
 * formulas and what they claim. */
int bhip_distort_model_u8(bhip_ctx* ctx, const uint8_t* src, int sStart, int sStride, int sw, int sh, int model, const float* coeff, int dw, int dh, int x0, int y0,
						  int x1, int y1, int interp, int border, int renderAll, uint8_t* dst, int dStart, int dStride, uint8_t* mask, int mStart, int mStride);
int bhip_distort_model_f32(bhip_ctx* ctx, const float* src, int sStart, int sStride, int sw, int sh, int model, const float* coeff, int dw, int dh, int x0, int y0,
						   int x1, int y1, int interp, int border, int renderAll, float* dst, int dStart, int dStride, uint8_t* mask, int mStart, int mStride);
/* SelectNBestFeatures.process(intensity, corners, positive) + getBestCorners() (F:alg/feature/detect/extract/SelectNBestFeatures.java:51-97):
 * n <= target copies the list; otherwise keys = -intensity (positive) or +intensity and org.ddogleg.sorting.QuickSelect.selectIndex(keys,
 * target, n, indexes) decides which `target` corners are kept and in which order.  ddogleg is not part of the reference tree: the routine
 * is the published Numerical Recipes `select` with an index array (see oracle/boof_oracle.hpp quickSelectIndex); the kept SET is pinned
 * (the N most intense, exact ties at the cut aside), the order is "parity unpinned".  xy / out_xy: (x,y) int16 pairs; out_xy holds
 * min(n, target) pairs.  Used by FastHessianFeatureDetector (maxFeaturesPerScale > 0) and GeneralFeatureDetector (maxFeatures > 0). */
int bhip_select_nbest_f32(bhip_ctx* ctx, const float* intensity, int start, int stride, int width, int height, const int16_t* xy, int n, int target,
						  int positive, int16_t* out_xy, int* out_n);
/* ---- template matching: TemplateMatchingIntensity / TemplateMatching of FactoryTemplateMatching.createIntensity / createMatcher (template.hip) ---- */
typedef enum { BHIP_TEMPLATE_SAD = 0, BHIP_TEMPLATE_SSE = 1, BHIP_TEMPLATE_NCC = 2, BHIP_TEMPLATE_CORRELATION = 3 } bhip_template_score;   /* TemplateScoreType ordinals */
#define BHIP_TEMPLATE_MAX_WIDTH 160          /* template columns the kernel's staged rows hold; the template height is not limited */
#define BHIP_TEMPLATE_MAX_CANDIDATES 65536   /* candidates per image bhip_template_select_f32 / _dev_f32 take */
/* TemplateMatchingIntensity.setInputImage(image); process(template) / process(template, mask); getIntensity() of
 * FactoryTemplateMatching.createIntensity(SUM_ABSOLUTE_DIFFERENCE | SUM_SQUARE_ERROR | NCC, GrayU8.class | GrayF32.class)
 * (F:factory/feature/detect/template/FactoryTemplateMatching.java:47-99): TemplateIntensityImage
 * (F:alg/feature/detect/template/TemplateIntensityImage.java:56-125) over TemplateSumAbsoluteDifference (TemplateSumAbsoluteDifference.java:46-128),
 * TemplateSumSquaredError (TemplateSumSquaredError.java:46-144) or TemplateNCC (TemplateNCC.java:54-274).  mask == NULL: process(template).
 * Single-threaded reference results, bit for bit (the library is built with -ffp-contract=off; divide and sqrt are correctly rounded).
 * The image is W x H, the template tw x th: w = W-tw+1, h = H-th+1, bx0 = tw/2, by0 = th/2, bx1 = tw-bx0, by1 = th-by0.
 *   intensity[y+by0][x+bx0] = evaluate(x, y) for x < w, y < h; every other pixel of the W x H intensity image is 0.
 * evaluate(x, y) compares I = image[y+j][x+i] with T = template[j][i] (and m = mask[j][i]) for j < th (outer loop), i < tw (inner loop); fp32
 * operations are separate (no fused multiply-add), `total` is a float that starts at 0:
 *   SAD  GrayU8:  int rowTotal = sum_i |I-T|, masked sum_i m*|I-T|; total += rowTotal (int to float, then the fp32 add), row by row.
 *        GrayF32: float rowTotal += |I-T|, masked rowTotal += m*|I-T|, in order; total += rowTotal.
 *   SSE  div = 255.0f*255.0f.  GrayU8: int rowTotal = sum_i e*e with e = I-T, masked sum_i m*e*e in Java int arithmetic (it wraps at 32 bits);
 *        total += rowTotal/div.  GrayF32: float rowTotal += e*e, masked rowTotal += (m*e)*e; total += rowTotal/div.
 *   NCC  area = (float)(tw*th).  Once per template, in order: templateMean = (sum of T)/area, templateSigma = (float)sqrt((sum of
 *        (T-templateMean)^2)/area).  Per pixel the image sum comes first (GrayU8: int imageSum, imageMean = imageSum/area; GrayF32: a sequential
 *        float sum, then /= area); a second pass accumulates, with diff = I-imageMean, imageSigma += diff*diff and top += diff*(T-templateMean),
 *        masked top += (m*diff)*(T-templateMean) -- the mask enters nothing else; imageSigma = (float)sqrt(imageSigma/area); the result is
 *        top/(EPS + imageSigma*templateSigma).  EPS = UtilEjml.F_EPS; EJML is not part of the reference tree: the library uses (float)2^-21,
 *        EJML's definition -- "parity unpinned" against the jar.
 * isMaximize(): NCC true, SAD and SSE false.  isBorderProcessed(): false.
 * Deviation: the masked process(template, mask) of the reference does not fill the border, which keeps what an earlier call left there; the
 * library writes the whole intensity view on every call, 0 in the border (the result of a freshly constructed object).
 * BHIP_ERR_UNSUPPORTED and nothing is written: score CORRELATION (TemplateCorrelationFFT); tw > BHIP_TEMPLATE_MAX_WIDTH (160).
 * BHIP_ERR_INVALID and nothing is written: an unknown score; an empty image or template; a template larger than the image (the reference
 * indexes outside its arrays); a mask whose size is not the template's.
 * Domain: inputs are finite.  With NaN / Inf nothing outside the views is read or written; the values are unspecified.
 * Image, template, mask and intensity must not overlap (not detected).  Host form: one image; start / stride in elements. */
int bhip_template_intensity_u8(bhip_ctx* ctx, int score, const uint8_t* image, int iStart, int iStride, int width, int height, const uint8_t* templ, int tStart,
							   int tStride, int tWidth, int tHeight, const uint8_t* mask, int mStart, int mStride, int mWidth, int mHeight, float* intensity, int oStart,
							   int oStride);
int bhip_template_intensity_f32(bhip_ctx* ctx, int score, const float* image, int iStart, int iStride, int width, int height, const float* templ, int tStart,
								int tStride, int tWidth, int tHeight, const float* mask, int mStart, int mStride, int mWidth, int mHeight, float* intensity, int oStart,
								int oStride);
/* The selection of TemplateMatching.process() (F:alg/feature/detect/template/TemplateMatching.java:117-176) after the non-maximum suppression:
 * `intensity` is the sub-image [bx0, bx0+w) x [by0, by0+h) of the template intensity, xy the n candidates the extractor found in it (the
 * maxima of bhip_nonmax_block_f32 for NCC, the minima of bhip_nonmax_block_minmax_f32 for SAD / SSE; radius 2 unless setMinimumSeparation,
 * threshold -Float.MAX_VALUE, border 0).  scores[i] = sgn*intensity(xy[i]) with sgn = -1 when maximize and +1 otherwise, N = min(maxMatches, n),
 * QuickSelect.selectIndex(scores, N, n, indexes) -- also when N == n: the list is permuted, there is no shortcut -- then match i is
 * out_xy[i] = xy[indexes[i]] (the template's top-left corner) with out_score[i] = -scores[indexes[i]], the score of that candidate: the
 * intensity for NCC, minus the intensity for SAD / SSE (the reference's own TestTemplateMatching pins a match's score to its candidate's
 * intensity; the restated routine permutes the key array it is given, so the score is read from the keys as they were before it ran).
 * *out_n = N; n == 0 gives no matches.  The routine is the restated one of bhip_select_nbest_f32: the kept set is pinned, the order is
 * "parity unpinned" against the ddogleg jar.
 * BHIP_ERR_INVALID: a candidate outside the view, n or maxMatches < 0.  BHIP_ERR_UNSUPPORTED: n > BHIP_TEMPLATE_MAX_CANDIDATES (65536). */
int bhip_template_select_f32(bhip_ctx* ctx, const float* intensity, int start, int stride, int width, int height, const int16_t* xy, int n, int maxMatches,
							 int maximize, int16_t* out_xy, float* out_score, int* out_n);
/* FastHessianFeatureDetector.detect(ii) (F:alg/feature/detect/interest/FastHessianFeatureDetector.java:156-188) on a host integral image */
int bhip_fh_detect_f32(bhip_ctx* ctx, const bhip_fh_cfg* cfg, const float* ii, int iiStart, int iiStride, int width, int height, double* xy_scale,
					   int cap, int* n);

/* ---- association: FactoryAssociation.greedy(score,maxErr,backwards) -> AssociateDescription
 *      (F:factory/feature/associate/FactoryAssociation.java:51-65; F:alg/feature/associate/AssociateGreedy.java:65-118;
 *       F:abst/feature/associate/WrapAssociateGreedy.java:73-93).  pairs[i] = dst index or -1, fit[i] = AssociateGreedyBase.fitQuality. ---- */
/* ScoreAssociateEuclideanSq_F64 (DescriptorDistance.euclideanSq, F:alg/descriptor/DescriptorDistance.java:55-64); sqrtScore!=0 gives
 * ScoreAssociateEuclidean_F64 (:36-46) */
int bhip_assoc_l2_f64(bhip_ctx* ctx, const double* src, int ns, const double* dst, int nd, int dof, double maxErr, int backwards, int sqrtScore,
					  int* pairs, double* fit);
/* ScoreAssociateHamming_B (DescriptorDistance.hamming, :196-220) on TupleDesc_B.data words */
int bhip_assoc_hamming(bhip_ctx* ctx, const int32_t* src, int ns, const int32_t* dst, int nd, int words, double maxErr, int backwards, int* pairs,
					   double* fit);
/* device-resident forms (async on the ctx stream; outputs are device arrays) */
int bhip_assoc_l2_dev(bhip_ctx* ctx, const double* dev_src, int ns, const double* dev_dst, int nd, int dof, double maxErr, int backwards,
					  int sqrtScore, int* dev_pairs, double* dev_fit);
int bhip_assoc_hamming_dev(bhip_ctx* ctx, const int32_t* dev_src, int ns, const int32_t* dev_dst, int nd, int words, double maxErr, int backwards,
						   int* dev_pairs, double* dev_fit);
/* batched device form: `count` independent (src,dst) problems in one launch sequence.  Problem p uses rows
 * [srcOff[p], srcOff[p]+ns[p]) of dev_src and [dstOff[p], dstOff[p]+nd[p]) of dev_dst (host arrays of offsets/sizes);
 * pairs/fit are written at the source row offsets. */
int bhip_assoc_l2_dev_batched(bhip_ctx* ctx, const double* dev_src, const double* dev_dst, int dof, int count, const long long* srcOff,
							  const int* ns, const long long* dstOff, const int* nd, double maxErr, int backwards, int* dev_pairs, double* dev_fit);
/* the same for ScoreAssociateHamming_B word lists (`words` ints per row): the consecutive-frame problems of a batch of BRIEF frames */
int bhip_assoc_hamming_dev_batched(bhip_ctx* ctx, const int32_t* dev_src, const int32_t* dev_dst, int words, int count, const long long* srcOff,
								   const int* ns, const long long* dstOff, const int* nd, double maxErr, int backwards, int* dev_pairs, double* dev_fit);

/* sharded association: this rank owns source rows [srcBegin, srcBegin+nsLocal) of a global problem with nsGlobal rows and the
 * whole destination set.  Phase 1 computes the local forward matches and, per destination column, the local column top-2
 * (min1, argmin1 as GLOBAL source index, min2) into dev_colTop (nd records of {double min1; double min2; int idx1; int pad}).
 * The caller all-gathers dev_colTop across ranks (RCCL, e.g. torch.distributed.all_gather_into_tensor) into nranks*nd records;
 * phase 2 merges them and applies the strict column-minimum rule to the local rows. */
int bhip_assoc_l2_shard_phase1(bhip_ctx* ctx, const double* dev_src, int nsLocal, int srcBegin, const double* dev_dst, int nd, int dof,
							   double maxErr, int* dev_pairs, double* dev_fit, void* dev_colTop);
int bhip_assoc_hamming_shard_phase1(bhip_ctx* ctx, const int32_t* dev_src, int nsLocal, int srcBegin, const int32_t* dev_dst, int nd, int words,
									double maxErr, int* dev_pairs, double* dev_fit, void* dev_colTop);
int bhip_assoc_shard_phase2(bhip_ctx* ctx, const void* dev_colTopAll, int nranks, int nd, int nsLocal, int srcBegin, int* dev_pairs,
							double* dev_fit);
int bhip_assoc_coltop_bytes(void); /* sizeof one column record */

/* ---- boofcv-ip front end behind the BOverride* hooks ---- */
/* BOverrideConvolveImage.horizontal/vertical (I:alg/filter/convolve/BOverrideConvolveImage.java:37-51) = ConvolveImageNoBorder
 * (I:alg/filter/convolve/ConvolveImageNoBorder.java:53-77): border pixels of out are left untouched */
int bhip_conv_h_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, int kernelOffset, const float* in, int inStart, int inStride, int width,
					int height, float* out, int outStart, int outStride);
int bhip_conv_v_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, int kernelOffset, const float* in, int inStart, int inStride, int width,
					int height, float* out, int outStart, int outStride);
/* BOverrideConvolveImageNormalized.horizontal/vertical (I:alg/filter/convolve/BOverrideConvolveImageNormalized.java:38-52) =
 * ConvolveImageNormalized.horizontal/vertical (I:alg/filter/convolve/ConvolveImageNormalized.java:48-93) */
int bhip_conv_norm_h_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, int kernelOffset, const float* in, int inStart, int inStride,
						 int width, int height, float* out, int outStart, int outStride);
int bhip_conv_norm_v_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, int kernelOffset, const float* in, int inStart, int inStride,
						 int width, int height, float* out, int outStart, int outStride);
/* BOverrideBlurImageOps.gaussian (I:alg/filter/blur/BOverrideBlurImageOps.java:38,48-49) = BlurImageOps.gaussian(GrayF32,out,sigma,radius,storage)
 * (I:alg/filter/blur/BlurImageOps.java:406-425), sigmaX==sigmaY / radiusX==radiusY form */
int bhip_gaussian_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, double sigma, int radius, float* out,
					  int outStart, int outStride);
/* BOverrideConvolveImage.convolve target: ConvolveImageNoBorder.convolve(Kernel2D_F32, GrayF32, GrayF32)
 * (I:alg/filter/convolve/ConvolveImageNoBorder.java:79-90; unrolled widths 3..11 sum every kernel row from 0 and add the row sums,
 * I:alg/filter/convolve/noborder/ConvolveImageUnrolled_SB_F32_F32.java:592-644; otherwise ConvolveImageStandard_SB.java:106-134).
 * kernel = kernelWidth x kernelWidth values, row-major; the frame of `out` is left untouched. */
int bhip_conv2d_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, int kernelOffset, const float* in, int inStart, int inStride, int width,
					int height, float* out, int outStart, int outStride);
/* BOverrideBlurImageOps.mean target: BlurImageOps.mean(GrayF32, out, radiusX, radiusY, storage) (I:alg/filter/blur/BlurImageOps.java:359-376)
 * = ConvolveImageMean.horizontal then vertical (I:alg/filter/convolve/ConvolveImageMean.java:55-101): float running sums in the
 * single-threaded order of ImplConvolveMean (I:alg/filter/convolve/noborder/ImplConvolveMean.java:281-357), re-normalised border. */
int bhip_mean_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, int radiusX, int radiusY, float* out,
				  int outStart, int outStride);
/* BOverrideBlurImageOps.median target: BlurImageOps.median(GrayF32, out, radius) (I:alg/filter/blur/BlurImageOps.java:752-765) =
 * ImplMedianSortNaive.process (I:alg/filter/blur/impl/ImplMedianSortNaive.java:97-135): the (count/2)-th order statistic of the clipped window */
int bhip_median_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, int radius, float* out, int outStart,
					int outStride);
/* GradientSobel.process(GrayF32,derivX,derivY,border) (I:alg/filter/derivative/GradientSobel.java:158-173);
 * border: 0 = null (frame untouched), 1 = ImageBorderValue(0), 2 = BorderType.EXTENDED (BoofDefaults.DERIV_BORDER_TYPE, what
 * FactoryDerivative.sobel passes: I:abst/filter/derivative/ImageGradient_SB.java:39-66): every frame pixel is kernelDerivX/Y_F32 on the
 * index-clamped image, summed as ConvolveJustBorder_General_SB.convolve does (I:alg/filter/convolve/border/ConvolveJustBorder_General_SB.java:110-174).
 * bhip_sobel_u8_s16 accepts 2 as well (see there); the three-tap gradients of both types answer BHIP_ERR_UNSUPPORTED to 2. */
int bhip_sobel_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, float* dx, float* dy, int outStart,
				   int outStride, int border);
/* GradientThree.process(GrayF32,...) -> GradientThree_Standard.process (I:alg/filter/derivative/impl/GradientThree_Standard.java:40-62) */
int bhip_three_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, float* dx, float* dy, int outStart,
				   int outStride, int border);
/* ConvolveImageDownNormalized.horizontal/vertical (I:alg/filter/convolve/ConvolveImageDownNormalized.java:53-86): every skip-th pixel
 * along the filtered axis, kernel re-normalised where it overlaps the border (ConvolveDownNormalized_JustBorder.java:43-139), plain
 * sum inside (ConvolveDownNoBorderUnrolled_F32_F32 / ConvolveDownNoBorderStandard), naive form when kernelWidth >= width.  `out` is
 * outWidth x outHeight and must satisfy ConvolveImageDownNoBorder.checkParametersH/V (:160-176); pixels the reference does not write
 * keep the caller's values.  BHIP_ERR_INVALID where the reference throws. */
int bhip_conv_down_norm_h_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, const float* in, int inStart, int inStride, int width, int height,
							  float* out, int outStart, int outStride, int outWidth, int outHeight, int skip);
int bhip_conv_down_norm_v_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, const float* in, int inStart, int inStride, int width, int height,
							  float* out, int outStart, int outStride, int outWidth, int outHeight, int skip);
/* PyramidDiscreteSampleBlur (I:alg/transform/pyramid/PyramidDiscreteSampleBlur.java:68-126).  bhip_pyramid_layout is
 * ImagePyramidBase.initialize + checkScales (T:struct/pyramid/ImagePyramidBase.java:73-112): dims[2i],dims[2i+1] = width,height of layer i,
 * offsets[i] = first float of layer i in the packed output (layers dense, stride = layer width), *totalFloats = floats per frame.
 * bhip_pyramid_f32 = process(input) for one host image; bhip_pyramid_dev_f32 runs `batch` device-resident frames (frame b of the
 * output starts at dev_out + b * totalFloats) without leaving the stream.  The 1-D kernel is FactoryPyramid.discreteGaussian's
 * FactoryKernelGaussian.gaussian(Kernel1D_F32, sigma, radius) (I:factory/transform/pyramid/FactoryPyramid.java:53-61), built by the caller. */
/* FactoryKernelGaussian.gaussian(Kernel1D_F32.class, sigma, radius) (I:factory/filter/kernel/FactoryKernelGaussian.java:120-153): host-only
 * helper for callers outside the JVM.  Returns the kernel width, or -(needed width) when capacity is too small / out is NULL. */
int bhip_gaussian_kernel1d_f32(double sigma, int radius, float* out, int capacity);
int bhip_pyramid_layout(int width, int height, const int* scales, int numLayers, int* dims, long long* offsets, long long* totalFloats);
int bhip_pyramid_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, const int* scales, int numLayers, const float* in, int inStart,
					 int inStride, int width, int height, float* out);
int bhip_pyramid_dev_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, const int* scales, int numLayers, const float* dev_in,
						 long long inImageStride, int inStride, int width, int height, int batch, float* dev_out);
/* The same on GrayU8: ConvolveImageDownNormalized.horizontal/vertical(Kernel1D_S32, GrayU8, GrayI8, skip)
 * (I:alg/filter/convolve/ConvolveImageDownNormalized.java:109-137).  Interior (byte)((total + divisor/2) / divisor) with divisor =
 * kernel.computeSum() (ConvolveDownNoBorderStandard.java:329-394, ConvolveDownNoBorderUnrolled_U8_I8_Div), border (byte)((total + weight/2) / weight)
 * over the taps inside the image (ConvolveDownNormalized_JustBorder.java:262-358), naive form when kernelWidth >= width
 * (ConvolveDownNormalizedNaive.java:133-187); Java's truncating int division for any S32 kernel.  BHIP_ERR_INVALID where the reference throws
 * (also a kernel that sums to 0: ArithmeticException). */
int bhip_conv_down_norm_h_u8(bhip_ctx* ctx, const int32_t* kernel, int kernelWidth, const uint8_t* in, int inStart, int inStride, int width, int height,
							 uint8_t* out, int outStart, int outStride, int outWidth, int outHeight, int skip);
int bhip_conv_down_norm_v_u8(bhip_ctx* ctx, const int32_t* kernel, int kernelWidth, const uint8_t* in, int inStart, int inStride, int width, int height,
							 uint8_t* out, int outStart, int outStride, int outWidth, int outHeight, int skip);
/* PyramidDiscreteSampleBlur<GrayU8> (I:alg/transform/pyramid/PyramidDiscreteSampleBlur.java:67-124): bhip_pyramid_f32 / bhip_pyramid_dev_f32 on
 * bytes, with the layout of bhip_pyramid_layout counted in elements.  The kernel is FactoryKernelGaussian.gaussian(Kernel1D_S32, -1, radius)
 * (bhip_gaussian_kernel1d_s32), built by the caller; the image between the two passes of a layer is a GrayU8. */
int bhip_pyramid_u8(bhip_ctx* ctx, const int32_t* kernel, int kernelWidth, const int* scales, int numLayers, const uint8_t* in, int inStart,
					int inStride, int width, int height, uint8_t* out);
int bhip_pyramid_dev_u8(bhip_ctx* ctx, const int32_t* kernel, int kernelWidth, const int* scales, int numLayers, const uint8_t* dev_in,
						long long inImageStride, int inStride, int width, int height, int batch, uint8_t* dev_out);
/* FactoryIntensityPointAlg.shiTomasi(radius, false, GrayF32) / harris(radius, kappa, false, GrayF32)
 * (F:factory/feature/detect/intensity/FactoryIntensityPointAlg.java:91-160) -> GradientCornerIntensity.process(derivX, derivY, intensity)
 * = ImplSsdCorner_F32 (F:alg/feature/detect/intensity/impl/ImplSsdCorner_F32.java:62-196, ImplSsdCornerBox.java:36-51) with
 * ShiTomasiCorner_F32 (kind 0) or HarrisCorner_F32 (kind 1): box-window running sums of dx*dx, dx*dy, dy*dy in the reference's
 * single-threaded order (bit-exact), intensity 0 inside the border of `radius` pixels.  derivX / derivY share startIndex and stride.
 * Together with bhip_sobel_f32 and bhip_nonmax_block_f32 this is GeneralFeatureDetector.process for maxFeatures <= 0
 * (F:alg/feature/detect/interest/GeneralFeatureDetector.java:118-160). */
int bhip_corner_intensity_f32(bhip_ctx* ctx, int kind, int radius, float kappa, const float* derivX, const float* derivY, int dStart, int dStride,
							  int width, int height, float* intensity, int iStart, int iStride);
/* GrayU8 -> GrayS16 gradients: GradientSobel.process(GrayU8, GrayS16, GrayS16, border) (I:alg/filter/derivative/GradientSobel.java:110-124 ->
 * impl/GradientSobel_Outer.java:76- process_sub) and GradientThree.process(GrayU8, ...) (I:alg/filter/derivative/GradientThree.java:86-101 ->
 * impl/GradientThree_Standard.java:67-88).  Integer arithmetic stored as (short).  border: 0 = null (frame untouched), 1 = ImageBorderValue(0)
 * (ConvolveJustBorder_General_SB with kernelDerivX/Y_I32, DerivativeHelperFunctions.processBorderHorizontal/Vertical with kernelDeriv_I32),
 * 2 (bhip_sobel_u8_s16 only) = BorderType.EXTENDED, ImageBorder1D_S32 over BorderIndex1D_Extend: the nine-tap kernelDerivX/Y_I32 sum on the
 * index-clamped image, what FactoryDerivative.sobel(GrayU8, GrayS16) passes.  dx and dy share outStart / outStride. */
int bhip_sobel_u8_s16(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int16_t* dx, int16_t* dy, int outStart,
					  int outStride, int border);
int bhip_three_u8_s16(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int16_t* dx, int16_t* dy, int outStart,
					  int outStride, int border);
/* FactoryIntensityPointAlg.shiTomasi(radius, weighted, GrayS16) / harris(radius, kappa, weighted, GrayS16)
 * (F:factory/feature/detect/intensity/FactoryIntensityPointAlg.java:91-160) -> GradientCornerIntensity<GrayS16>.process.
 * weighted 0: ImplSsdCorner_S16 (F:alg/feature/detect/intensity/impl/ImplSsdCorner_S16.java:63-198) with ShiTomasiCorner_S32 (kind 0) or
 * HarrisCorner_S32 (kind 1): int32 box-window sums (wrapping as Java int), intensity 0 inside the border of `radius` pixels; 2r+1 <= width, height.
 * weighted 1: ImplSsdCornerWeighted_S16 (F:alg/feature/detect/intensity/impl/ImplSsdCornerWeighted_S16.java:50-108): products, then
 * ConvolveImageNormalized.horizontal / vertical (Kernel1D_S32) with FactoryKernelGaussian.gaussian(Kernel1D_S32, -1, radius), score on every
 * pixel; radius 1 .. 15, BHIP_ERR_UNSUPPORTED above (output untouched).  derivX / derivY share startIndex and stride. */
int bhip_corner_intensity_s16(bhip_ctx* ctx, int kind, int radius, float kappa, int weighted, const int16_t* derivX, const int16_t* derivY, int dStart,
							  int dStride, int width, int height, float* intensity, int iStart, int iStride);
/* FactoryIntensityPointAlg.shiTomasi(radius, true, GrayF32) / harris(radius, kappa, true, GrayF32) -> ImplSsdCornerWeighted_F32
 * (F:alg/feature/detect/intensity/impl/ImplSsdCornerWeighted_F32.java:46-104): products, ConvolveImageNormalized.horizontal / vertical
 * (I:alg/filter/convolve/ConvolveImageNormalized.java:48-93) with FactoryKernelGaussian.gaussian(Kernel1D_F32, -1, radius), score on every
 * pixel.  radius 1 .. 15, BHIP_ERR_UNSUPPORTED above (output untouched). */
int bhip_corner_intensity_weighted_f32(bhip_ctx* ctx, int kind, int radius, float kappa, const float* derivX, const float* derivY, int dStart, int dStride,
									   int width, int height, float* intensity, int iStart, int iStride);
/* FactoryKernelGaussian.gaussian(Kernel1D_S32.class, -1, radius) (I:factory/filter/kernel/FactoryKernelGaussian.java:120-160, KernelMath.convert
 * :556-620): host-only, same contract as bhip_gaussian_kernel1d_f32; -1 for radius <= 0 (the reference throws). */
int bhip_gaussian_kernel1d_s32(int radius, int32_t* out, int capacity);
/* Integer image variants at stage level.
 * bhip_integral_u8_s32: IntegralImageOps.transform(GrayU8, GrayS32) (I:alg/transform/ii/impl/ImplIntegralImageOps.java:94-118).
 * bhip_hessian_s32: IntegralImageFeatureIntensity.hessian(GrayS32, skip, size, GrayF32) (F:alg/feature/detect/intensity/impl/
 *   ImplIntegralImageFeatureIntensity.java:245-390): integer box sums, converted to float where the Java code assigns them to a float.
 * bhip_brief_u8: DescribePointBrief on GrayU8 = ImplDescribeBinaryCompare_U8 (F:alg/feature/describe/impl/ImplDescribeBinaryCompare_U8.java:47-101;
 *   its border form shifts the word for every pair, the F32 class only for pairs inside the image). */
int bhip_integral_u8_s32(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int32_t* out, int outStart, int outStride);
int bhip_hessian_s32(bhip_ctx* ctx, const int32_t* ii, int iiStart, int iiStride, int width, int height, int skip, int size, float* out, int outStart,
					 int outStride);
/* FastHessianFeatureDetector<GrayS32>.detect(integral) (F:alg/feature/detect/interest/FastHessianFeatureDetector.java:156-188 on the integral image
 * of a GrayU8 frame): same outputs as bhip_fh_detect_f32 */
int bhip_fh_detect_s32(bhip_ctx* ctx, const bhip_fh_cfg* cfg, const int32_t* ii, int iiStart, int iiStride, int width, int height,
					   double* xy_scale, int cap, int* n);
int bhip_brief_u8(bhip_ctx* ctx, const uint8_t* img, int start, int stride, int width, int height, int radius, int numPoints,
				  const int32_t* samplePoints, const int32_t* compare, const double* xy, int n, int32_t* out);
/* DescribePointBrief.process for n points on one image (F:alg/feature/describe/DescribePointBrief.java:73-89;
 * F:alg/feature/describe/impl/ImplDescribeBinaryCompare_F32.java:47-101).  The definition (samplePoints[numPoints][2], compare[numPoints][2])
 * is supplied by the caller: FactoryBriefDefinition.gaussian2 depends on java.util.Random + StrictMath and is generated on the Java side. */
int bhip_brief_f32(bhip_ctx* ctx, const float* img, int start, int stride, int width, int height, int radius, int numPoints,
				   const int32_t* samplePoints, const int32_t* compare, const double* xy, int n, int32_t* out);

/* ---- device-resident, batched forms of the boofcv-ip front end (BASELINE config 5: pyramid -> gradient -> non-max -> SURF on a 4K stream that
 *      never leaves HBM).  Image b of a batch starts imageStride floats after image 0, rows are `stride` floats apart; calls are asynchronous on
 *      the ctx stream.  Same kernels and arithmetic as the host-buffer entry points above (each cites the same reference function). ---- */
/* ConvolveImageNoBorder.horizontal / vertical (I:alg/filter/convolve/ConvolveImageNoBorder.java:53-77): frame of dev_out untouched */
int bhip_conv_h_dev_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, int kernelOffset, const float* dev_in, long long inImageStride, int inStride,
						int width, int height, int batch, float* dev_out, long long outImageStride, int outStride);
int bhip_conv_v_dev_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, int kernelOffset, const float* dev_in, long long inImageStride, int inStride,
						int width, int height, int batch, float* dev_out, long long outImageStride, int outStride);
/* ConvolveImageNormalized.horizontal / vertical (I:alg/filter/convolve/ConvolveImageNormalized.java:48-93) */
int bhip_conv_norm_h_dev_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, int kernelOffset, const float* dev_in, long long inImageStride, int inStride,
							 int width, int height, int batch, float* dev_out, long long outImageStride, int outStride);
int bhip_conv_norm_v_dev_f32(bhip_ctx* ctx, const float* kernel, int kernelWidth, int kernelOffset, const float* dev_in, long long inImageStride, int inStride,
							 int width, int height, int batch, float* dev_out, long long outImageStride, int outStride);
/* BlurImageOps.gaussian(GrayF32, out, sigma, radius, storage) (I:alg/filter/blur/BlurImageOps.java:406-425); `storage` is library scratch */
int bhip_gaussian_dev_f32(bhip_ctx* ctx, const float* dev_in, long long inImageStride, int inStride, int width, int height, int batch, double sigma, int radius,
						  float* dev_out, long long outImageStride, int outStride);
/* GradientSobel.process (I:alg/filter/derivative/GradientSobel.java:158-173) / GradientThree.process -> GradientThree_Standard
 * (I:alg/filter/derivative/impl/GradientThree_Standard.java:40-62); dx and dy share outImageStride / outStride; border as in bhip_sobel_f32 */
int bhip_sobel_dev_f32(bhip_ctx* ctx, const float* dev_in, long long inImageStride, int inStride, int width, int height, int batch, float* dev_dx, float* dev_dy,
					   long long outImageStride, int outStride, int border);
int bhip_three_dev_f32(bhip_ctx* ctx, const float* dev_in, long long inImageStride, int inStride, int width, int height, int batch, float* dev_dx, float* dev_dy,
					   long long outImageStride, int outStride, int border);
/* Gradient magnitude images: kind 0 = GradientToEdgeFeatures.intensityE, (float)Math.sqrt(dx*dx + dy*dy); kind 1 = intensityAbs, |dx| + |dy|
 * (F:alg/feature/detect/edge/GradientToEdgeFeatures.java:61-95 -> impl/ImplGradientToEdgeFeatures.java:40-85); kind 2 = dx*dx + dy*dy, the
 * |grad|^2 image BASELINE config 5 runs the non-max suppression on (the products and the sum of intensityE without the root) */
int bhip_gradient_intensity_dev_f32(bhip_ctx* ctx, int kind, const float* dev_dx, const float* dev_dy, long long dImageStride, int dStride, int width,
									int height, int batch, float* dev_out, long long outImageStride, int outStride);
/* NonMaxBlock.process, strict rule (F:alg/feature/detect/extract/NonMaxBlock.java:69-94; NonMaxBlockSearchStrict.java:56-79,196-221) on every image of
 * a batch: image b's maxima go to dev_xy[b*cap ...] as (x,y) int16 pairs in block-raster order, their number to dev_n[b] (it may exceed cap;
 * only the first cap pairs are written) */
int bhip_nonmax_block_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long imageStride, int stride, int width, int height, int batch, int radius,
							  float threshold, int border, int16_t* dev_xy, int cap, int* dev_n);
/* bhip_nonmax_block_minmax_f32 on every image of a batch: image b's lists go to dev_xyMin / dev_xyMax[b*cap ...], their lengths to dev_nMin /
 * dev_nMax[b] (a length may exceed cap; only the first cap pairs are written).  No host synchronisation. */
int bhip_nonmax_block_minmax_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long imageStride, int stride, int width, int height, int batch, int radius,
									 float thresholdMin, float thresholdMax, int border, int detectMin, int detectMax, int16_t* dev_xyMin, int* dev_nMin,
									 int16_t* dev_xyMax, int* dev_nMax, int cap);
/* bhip_fast_u8 / bhip_fast_f32 on a batch of device frames (strides in elements; any byte alignment of a GrayU8 view).  dev_intensity == NULL:
 * process(image).  Frame b writes dev_xyLow / dev_xyHigh[b*cap ...] and dev_nLow / dev_nHigh[b]; a count may exceed cap, only the first cap
 * pairs are written.  Classification, row counts with the early stop, and the ordered lists are queued without a host synchronisation. */
int bhip_fast_dev_u8(bhip_ctx* ctx, const uint8_t* dev_img, long long imageStride, int stride, int width, int height, int batch, int pixelTol, int minContinuous,
					 double maxFeaturesFraction, float* dev_intensity, long long iImageStride, int iStride, int16_t* dev_xyLow, int* dev_nLow, int16_t* dev_xyHigh,
					 int* dev_nHigh, int cap);
int bhip_fast_dev_f32(bhip_ctx* ctx, const float* dev_img, long long imageStride, int stride, int width, int height, int batch, float pixelTol, int minContinuous,
					  double maxFeaturesFraction, float* dev_intensity, long long iImageStride, int iStride, int16_t* dev_xyLow, int* dev_nLow, int16_t* dev_xyHigh,
					  int* dev_nHigh, int cap);
/* bhip_disparity_bm_u8_u8 / bhip_disparity_bm_u8_f32 on a batch of device pairs (strides in elements; any byte alignment of a GrayU8 view): pair b is
 * dev_left + b*lImageStride, dev_right + b*rImageStride and writes dev_disp + b*dImageStride, the whole width x height view and nothing outside it.
 * Cost and selection run in two launches (right-to-left minima into one byte per pixel of context scratch, then selection) without a host
 * synchronisation. */
int bhip_disparity_bm_dev_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride,
								const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, uint8_t* dev_disp,
								long long dImageStride, int dStride);
int bhip_disparity_bm_dev_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride,
								 const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, float* dev_disp,
								 long long dImageStride, int dStride);
/* bhip_census_u8_u8 / bhip_census_u8_s32 / bhip_census_sample_u8_s64 on a batch of device images (strides in elements; any byte alignment and stride
 * of the GrayU8 view): image b is dev_in + b*iImageStride and writes dev_out + b*oImageStride, the whole width x height view and nothing outside it.
 * One launch: a tile of 64 x 16 pixels and its halo are staged in LDS with the reflected indices resolved, one lane per output pixel.  samplesXY is
 * host memory (the list travels in the kernel arguments).  No host synchronisation. */
int bhip_census_dev_u8_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long iImageStride, int iStride, int width, int height, int batch, uint8_t* dev_out,
						  long long oImageStride, int oStride);
int bhip_census_dev_u8_s32(bhip_ctx* ctx, const uint8_t* dev_in, long long iImageStride, int iStride, int width, int height, int batch, int32_t* dev_out,
						   long long oImageStride, int oStride);
int bhip_census_sample_dev_u8_s64(bhip_ctx* ctx, const int* samplesXY, int nSamples, const uint8_t* dev_in, long long iImageStride, int iStride, int width,
								  int height, int batch, long long* dev_out, long long oImageStride, int oStride);
/* bhip_disparity_bm_census_u8_u8 / _u8_f32 on a batch of device pairs (strides in elements; any byte alignment of a GrayU8 view): pair b is
 * dev_left + b*lImageStride, dev_right + b*rImageStride and writes dev_disp + b*dImageStride, the whole width x height view and nothing outside it.
 * Two stages without a host synchronisation: the census of both images into context scratch (1 byte per pixel for BLOCK_3_3, 4 for BLOCK_5_5 and --
 * the low words, which carry all the information -- for the GrayS64 variants), then the launches of bhip_disparity_bm_dev_u8_u8 on the census images. */
int bhip_disparity_bm_census_dev_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* dev_left, long long lImageStride, int lStride,
									   const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, uint8_t* dev_disp,
									   long long dImageStride, int dStride);
int bhip_disparity_bm_census_dev_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* dev_left, long long lImageStride, int lStride,
										const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, float* dev_disp,
										long long dImageStride, int dStride);
/* bhip_disparity_bm5_u8_u8 / _u8_f32 / _census_u8_u8 / _census_u8_f32 on a batch of device pairs (strides in elements; any byte alignment of a GrayU8
 * view): pair b is dev_left + b*lImageStride, dev_right + b*rImageStride and writes dev_disp + b*dImageStride, the whole width x height view and
 * nothing outside it.  The census forms first write the census images into context scratch, as bhip_disparity_bm_census_dev_u8_u8 does.  Then
 * three launches without a host synchronisation: the fill, the right-to-left minima of F (one byte per pixel of context scratch), the selection.
 * No cost volume leaves the chip: a workgroup keeps the three rows of sub-block sums it needs in LDS. */
int bhip_disparity_bm5_dev_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride,
								 const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, uint8_t* dev_disp,
								 long long dImageStride, int dStride);
int bhip_disparity_bm5_dev_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, const uint8_t* dev_left, long long lImageStride, int lStride,
								  const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, float* dev_disp,
								  long long dImageStride, int dStride);
int bhip_disparity_bm5_census_dev_u8_u8(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* dev_left, long long lImageStride, int lStride,
										const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, uint8_t* dev_disp,
										long long dImageStride, int dStride);
int bhip_disparity_bm5_census_dev_u8_f32(bhip_ctx* ctx, const bhip_disparity_bm_cfg* cfg, int variant, const uint8_t* dev_left, long long lImageStride, int lStride,
										 const uint8_t* dev_right, long long rImageStride, int rStride, int width, int height, int batch, float* dev_disp,
										 long long dImageStride, int dStride);
/* bhip_template_intensity_u8 / _f32 on a batch of device images (strides in elements; any byte alignment of a GrayU8 view): image b is
 * dev_image + b*iImageStride and writes dev_intensity + b*oImageStride, the whole width x height view and nothing outside it.  tImageStride /
 * mImageStride 0: one template / mask shared by the batch; otherwise image b is matched against dev_templ + b*tImageStride (and
 * dev_mask + b*mImageStride).  dev_mask == NULL: no mask.  No host synchronisation. */
int bhip_template_intensity_dev_u8(bhip_ctx* ctx, int score, const uint8_t* dev_image, long long iImageStride, int iStride, int width, int height, int batch,
								   const uint8_t* dev_templ, long long tImageStride, int tStride, int tWidth, int tHeight, const uint8_t* dev_mask,
								   long long mImageStride, int mStride, int mWidth, int mHeight, float* dev_intensity, long long oImageStride, int oStride);
int bhip_template_intensity_dev_f32(bhip_ctx* ctx, int score, const float* dev_image, long long iImageStride, int iStride, int width, int height, int batch,
									const float* dev_templ, long long tImageStride, int tStride, int tWidth, int tHeight, const float* dev_mask,
									long long mImageStride, int mStride, int mWidth, int mHeight, float* dev_intensity, long long oImageStride, int oStride);
/* bhip_template_select_f32 on every image of a batch: image b's candidates are dev_xy[b*cap ...], the first min(dev_n[b], cap) of them (the
 * lists and counts of bhip_nonmax_block_dev_f32 / bhip_nonmax_block_minmax_dev_f32: a list the extractor cut at cap is selected from as it
 * is); its matches go to dev_out_xy[b*maxMatches ...] and dev_out_score[b*maxMatches ...], their number to dev_out_n[b].  A candidate outside
 * the view reads as intensity 0.  One wave per image runs the sequential routine on one lane, as for the N best per scale.
 * BHIP_ERR_UNSUPPORTED: cap > BHIP_TEMPLATE_MAX_CANDIDATES (65536).  No host synchronisation. */
int bhip_template_select_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long imageStride, int stride, int width, int height, int batch,
								 const int16_t* dev_xy, const int* dev_n, int cap, int maxMatches, int maximize, int16_t* dev_out_xy, float* dev_out_score,
								 int* dev_out_n);
/* bhip_distort_map_u8 / _f32 on a batch of device images (strides in elements; any byte alignment of a GrayU8 view): image b reads
 * dev_src + b*sImageStride (sw x sh) and the map dev_map + b*mapImageStride (dw*dh interleaved float (x, y) pairs, dense; mapImageStride in
 * floats, 0 = one map shared by the batch, the usual case of one map per camera), and writes the crop of dev_dst + b*dImageStride (dw x dh)
 * and, when dev_mask is not NULL, of dev_mask + b*mImageStride.  One launch, no host synchronisation. */
int bhip_distort_map_dev_u8(bhip_ctx* ctx, const uint8_t* dev_src, long long sImageStride, int sStride, int sw, int sh, int batch, const float* dev_map,
							long long mapImageStride, int dw, int dh, int x0, int y0, int x1, int y1, int interp, int border, int renderAll, uint8_t* dev_dst,
							long long dImageStride, int dStride, uint8_t* dev_mask, long long mImageStride, int mStride);
int bhip_distort_map_dev_f32(bhip_ctx* ctx, const float* dev_src, long long sImageStride, int sStride, int sw, int sh, int batch, const float* dev_map,
							 long long mapImageStride, int dw, int dh, int x0, int y0, int x1, int y1, int interp, int border, int renderAll, float* dev_dst,
							 long long dImageStride, int dStride, uint8_t* dev_mask, long long mImageStride, int mStride);
/* The same with the coordinates computed in the kernel from `coeff` (host memory, passed by value to the kernel) instead of read from a map:
 * ImageDistortBasic_SB with PixelTransformAffine_F32 / PixelTransformHomography_F32 (I:alg/distort/PixelTransformAffine_F32.java,
 * PixelTransformHomography_F32.java).  With x, y converted from int to float first and every sum left to right, in float:
 *   BHIP_DISTORT_AFFINE      coeff = a11 a12 a21 a22 tx ty:     sx = tx + a11*x + a12*y,  sy = ty + a21*x + a22*y
 *   BHIP_DISTORT_HOMOGRAPHY  coeff = a11 .. a33, row-major:    z = a31*x + a32*y + a33,  sx = (a11*x + a12*y + a13)/z,  sy = (a21*x + a22*y + a23)/z
 *                            (correctly rounded divisions)
 * These formulas are the library's definition.  They restate georegression's AffinePointOps_F32.transform and HomographyPointOps_F32.transform,
 * whose source is not part of the reference tree, so their order of operations is unconfirmed: a Java caller who needs bit equality with
 * ImageDistortBasic_SB fills a map with its own transform and uses the map form.  The result is, bit for bit, the map form on the map
 * bhip_distort_build_map writes.  BHIP_ERR_INVALID: a model other than the two, a NULL coeff. */
int bhip_distort_model_dev_u8(bhip_ctx* ctx, const uint8_t* dev_src, long long sImageStride, int sStride, int sw, int sh, int batch, int model, const float* coeff,
							  int dw, int dh, int x0, int y0, int x1, int y1, int interp, int border, int renderAll, uint8_t* dev_dst, long long dImageStride,
							  int dStride, uint8_t* dev_mask, long long mImageStride, int mStride);
int bhip_distort_model_dev_f32(bhip_ctx* ctx, const float* dev_src, long long sImageStride, int sStride, int sw, int sh, int batch, int model, const float* coeff,
							   int dw, int dh, int x0, int y0, int x1, int y1, int interp, int border, int renderAll, float* dev_dst, long long dImageStride,
							   int dStride, uint8_t* dev_mask, long long mImageStride, int mStride);
/* The map of a model: dev_map[2*(y*dw + x)], [.. + 1] = (sx, sy) of the formulas above for 0 <= x < dw, 0 <= y < dh (what
 * ImageDistortCache_SB.init, I:alg/distort/ImageDistortCache_SB.java:111-134, computes on the host).  No host synchronisation. */
int bhip_distort_build_map(bhip_ctx* ctx, int model, const float* coeff, int dw, int dh, float* dev_map);
/* GradientCornerIntensity.process (see bhip_corner_intensity_f32) on a batch; derivX / derivY share dImageStride / dStride */
int bhip_corner_intensity_dev_f32(bhip_ctx* ctx, int kind, int radius, float kappa, const float* dev_dx, const float* dev_dy, long long dImageStride,
								  int dStride, int width, int height, int batch, float* dev_intensity, long long iImageStride, int iStride);
/* bhip_sobel_u8_s16 / bhip_three_u8_s16 on a batch (element strides: bytes in, shorts out); dx and dy share outImageStride / outStride */
int bhip_sobel_dev_u8_s16(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int16_t* dev_dx,
						  int16_t* dev_dy, long long outImageStride, int outStride, int border);
int bhip_three_dev_u8_s16(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int16_t* dev_dx,
						  int16_t* dev_dy, long long outImageStride, int outStride, int border);
/* bhip_corner_intensity_s16 / bhip_corner_intensity_weighted_f32 on a batch; derivX / derivY share dImageStride / dStride */
int bhip_corner_intensity_dev_s16(bhip_ctx* ctx, int kind, int radius, float kappa, int weighted, const int16_t* dev_dx, const int16_t* dev_dy,
								  long long dImageStride, int dStride, int width, int height, int batch, float* dev_intensity, long long iImageStride, int iStride);
int bhip_corner_intensity_weighted_dev_f32(bhip_ctx* ctx, int kind, int radius, float kappa, const float* dev_dx, const float* dev_dy, long long dImageStride,
										   int dStride, int width, int height, int batch, float* dev_intensity, long long iImageStride, int iStride);
/* DescribePointBrief.process (see bhip_brief_f32) for the points of a batch: image b owns points [start[b], start[b+1]) of dev_xy ((x,y) doubles;
 * `start` is a host array of batch+1 entries); point p's words go to dev_out[p * ceil(numPoints/32) ...] */
int bhip_brief_dev_f32(bhip_ctx* ctx, const float* dev_img, long long imageStride, int stride, int width, int height, int batch, int radius, int numPoints,
					   const int32_t* samplePoints, const int32_t* compare, const double* dev_xy, const int* start, int32_t* dev_out);

/* ---- pyramid KLT point tracker: FactoryPointTracker.klt(PkltConfig, ConfigGeneralDetector, GrayF32, GrayF32) -> PointTrackerKltPyramid
 *      (G:factory/feature/tracker/FactoryPointTracker.java:120-145,534-541; G:abst/feature/tracker/PointTrackerKltPyramid.java:139-348;
 *       F:alg/tracker/klt/PyramidKltTracker.java:58-151; F:alg/tracker/klt/KltTracker.java:147-495; I:alg/interpolate/impl/BilinearRectangle_F32.java:64-172;
 *       G: = main/boofcv-geo/src/main/java/boofcv/).  One object tracks `batch` independent image sequences of one shape; batch = 1 is the
 *      reference object.  Pyramid = FactoryPyramid.discreteGaussian(scales, -1, 2), gradient = GradientSobel with BorderType.EXTENDED, corners =
 *      Shi-Tomasi radius 1 unweighted + strict NonMaxBlock(detectRadius, detectThreshold, detectBorder), all on the device.  Every value is the
 *      single-threaded Java arithmetic bit for bit.  Deviations: BHIP_KLT_REFERENCE_THROWS (above); positions are reported as the float
 *      PyramidKltFeature.x,y (PointTrack holds the same numbers as doubles, and the caller's doubles after addTrack); a track added by
 *      bhip_klt_add_tracks has featureId -1 (the reference leaves whatever the recycled PointTrack held); a track that process() drops after a
 *      successful track() (centre outside the frame, or setDescription false) keeps fault BHIP_KLT_SUCCESS.  templateRadius 1..7, numLayers 1..8,
 *      maxIterations >= 1, otherwise BHIP_ERR_UNSUPPORTED. ---- */
#define BHIP_KLT_INITIAL_CAPACITY 1024   /* track lists start at this many entries per sequence and regrow; results do not depend on it */
int bhip_klt_create(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int templateRadius, const int* scales, int numLayers, int detectRadius, float detectThreshold,
					int detectBorder, int width, int height, int batch, bhip_klt** out);
int bhip_klt_destroy(bhip_klt* k);
/* process(image) for every sequence: frame b starts at dev_frames + b * imageStride, rows `stride` floats apart.  Pyramid, gradient, track,
 * re-describe and the list update are queued on the ctx stream without a host synchronisation. */
int bhip_klt_process_dev_f32(bhip_klt* k, const float* dev_frames, long long imageStride, int stride);
/* the same for host frames (one pointer per sequence) */
int bhip_klt_process_f32(bhip_klt* k, const float* const* img, const int* startIndex, const int* stride);
/* spawnTracks() for every sequence with ConfigGeneralDetector.maxFeatures <= 0; maxFeatures > 0 (SelectNBestFeatures) is BHIP_ERR_UNSUPPORTED here.
 * New tracks follow the block-raster order of bhip_nonmax_block_dev_f32.  One small count read-back. */
int bhip_klt_spawn(bhip_klt* k, int maxFeatures);
/* the second half of spawnTracks() for corners the caller found itself (GeneralFeatureDetector with maxFeatures > 0 composed from
 * bhip_klt_fetch_layer, the corner entry points and bhip_select_nbest_f32): sequence b gets count[b] candidates, xy[(b * capacity + i) * 2] in
 * layer-0 pixels, in detector order */
int bhip_klt_spawn_points(bhip_klt* k, const int16_t* xy, const int* count, int capacity);
/* addTrack(x, y) on sequence seq[i], in call order; ok[i] = 0 where the reference returns null */
int bhip_klt_add_tracks(bhip_klt* k, const int* seq, const double* xy, int n, uint8_t* ok);
/* dropTrack of the active track with that featureId (the first one in list order); ok (may be NULL): the reference's boolean */
int bhip_klt_drop_tracks(bhip_klt* k, const int* seq, const long long* featureId, int n, uint8_t* ok);
int bhip_klt_drop_all(bhip_klt* k);
int bhip_klt_reset(bhip_klt* k);
/* sizes of getActiveTracks / getNewTracks / getDroppedTracks of every sequence ([batch] each; any pointer may be NULL) */
int bhip_klt_counts(bhip_klt* k, int* active, int* spawned, int* dropped);
/* one list of sequence seq (which: 0 active, 1 spawned, 2 dropped) in the reference's list order: featureId[n], xy[2n], fault[n] (last
 * track() result), error[n] (KltTracker.getError() of the last layer of this track whose error was computed).  Any pointer may be NULL. */
int bhip_klt_fetch(bhip_klt* k, int which, int seq, long long* featureId, float* xy, int* fault, float* error);
/* what PyramidKltFeature.desc[layer] holds for the tracks of one list of sequence seq, in list order: tmpl[n][3][(2r+1)^2] = KltFeature.desc,
 * derivX, derivY (F:alg/tracker/klt/KltFeature.java; desc = NaN outside the image, the derivative templates 0 there), G[n][3] = Gxx, Gyy, Gxy.
 * Either pointer may be NULL.  For tests and for callers that re-use descriptions; either pixel type. */
int bhip_klt_fetch_templates(bhip_klt* k, int which, int seq, int layer, float* tmpl, float* G);
/* figures of the last process() over all sequences: tracks that went through track(), Lucas-Kanade iterations they took, and how many of those
 * took the border form (computeGandE_border) */
int bhip_klt_stats(bhip_klt* k, long long* tracks, long long* iterations, long long* borderIterations);
/* layer `layer` of sequence seq of the last process(): which 0 = image pyramid, 1 = derivX, 2 = derivY; dense, bhip_pyramid_layout's dims */
int bhip_klt_fetch_layer(bhip_klt* k, int seq, int layer, int which, float* out);
/* for callers that stay on the device: sequence b's active slots are dev_activeSlots[b * slotsPerSequence + i], i < dev_activeCount[b]; slot s of
 * sequence b is entry b * slotsPerSequence + s of dev_x / dev_y / dev_featureId.  Layer l of frame b of the pyramid / derivative buffers starts at
 * b * floatsPerFrame + offsets[l] of bhip_pyramid_layout.  Valid until the next spawn or add (the table may regrow). */
int bhip_klt_dev_view(bhip_klt* k, const int** dev_activeSlots, const int** dev_activeCount, const float** dev_x, const float** dev_y,
					  const long long** dev_featureId, const float** dev_pyramid, const float** dev_derivX, const float** dev_derivY, int* slotsPerSequence,
					  long long* floatsPerFrame);
/* stage level, host buffers, one image: KltTracker.setDescription (:147-240) for n features of radius `radius` at xy[2n] on (image, derivX, derivY) of
 * one shape; image and derivatives each with their own startIndex / stride.  desc / derivX / derivY templates [n][(2r+1)^2] (desc = NaN outside the
 * image; the derivative templates read 0 there, the reference leaves them stale), G[3n] = Gxx, Gyy, Gxy, ok[n] = the boolean
 * (2 = BHIP_KLT_REFERENCE_THROWS). */
int bhip_klt_set_description_f32(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const float* image, int imgStart, int imgStride, const float* derivX,
								 const float* derivY, int dStart, int dStride, int width, int height, const float* xy, int n, float* desc, float* descX,
								 float* descY, float* G, uint8_t* ok);
/* KltTracker.track (:251-325): xy[2n] in / out (moved also when a fault is returned, as in the reference), fault[n], error[n] (written where
 * computeError ran: SUCCESS and LARGE_ERROR) */
int bhip_klt_track_f32(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const float* image, int imgStart, int imgStride, int width, int height,
					   const float* desc, const float* descX, const float* descY, const float* G, float* xy, int n, int* fault, float* error);

/* ---- the same tracker on GrayU8 frames: FactoryPointTracker.klt(PkltConfig, ConfigGeneralDetector, GrayU8, GrayS16)
 *      (G:factory/feature/tracker/FactoryPointTracker.java:120-145; derivType = GImageDerivativeOps.getDerivativeType(GrayU8) = GrayS16).
 *      Pyramid = PyramidDiscreteSampleBlur<GrayU8> with Kernel1D_S32 [1,4,7,4,1] (bhip_pyramid_dev_u8), gradient = GradientSobel.process(GrayU8,
 *      GrayS16, GrayS16, EXTENDED) (I:alg/filter/derivative/GradientSobel.java:110-124), interpolation = BilinearRectangle_U8 / _S16
 *      (I:alg/interpolate/impl/BilinearRectangle_U8.java:65-173, BilinearRectangle_S16.java:66-168: the F32 expression on taps converted to
 *      float), corners = ImplSsdCorner_S16 + ShiTomasiCorner_S32 (bhip_corner_intensity_dev_s16).  KltTracker / PyramidKltTracker and the lists
 *      are type independent, so spawn, spawn_points, add, drop, counts, fetch, stats, reset and destroy are the calls above on either kind of
 *      handle.  A handle answers BHIP_ERR_INVALID to the process / fetch_layer / dev_view calls of the other pixel type. ---- */
int bhip_klt_create_u8(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int templateRadius, const int* scales, int numLayers, int detectRadius, float detectThreshold,
					   int detectBorder, int width, int height, int batch, bhip_klt** out);
/* process(GrayU8) for every sequence: strides in bytes (= elements).  The frames are copied into layer 0, so dev_frames may be reused once the
 * call has been queued on the stream. */
int bhip_klt_process_dev_u8(bhip_klt* k, const uint8_t* dev_frames, long long imageStride, int stride);
/* the same for host frames (one pointer per sequence); with scale[0] == 1 they are uploaded straight into layer 0 */
int bhip_klt_process_u8(bhip_klt* k, const uint8_t* const* img, const int* startIndex, const int* stride);
/* layer `layer` of sequence seq of the last process(): the GrayU8 image pyramid, and derivX (which 1) / derivY (which 2) as GrayS16 */
int bhip_klt_fetch_layer_u8(bhip_klt* k, int seq, int layer, uint8_t* out);
int bhip_klt_fetch_layer_s16(bhip_klt* k, int seq, int layer, int which, int16_t* out);
/* bhip_klt_dev_view for a GrayU8 tracker: layer l of frame b starts at b * elementsPerFrame + offsets[l] elements of each buffer */
int bhip_klt_dev_view_u8(bhip_klt* k, const int** dev_activeSlots, const int** dev_activeCount, const float** dev_x, const float** dev_y,
						 const long long** dev_featureId, const uint8_t** dev_pyramid, const int16_t** dev_derivX, const int16_t** dev_derivY,
						 int* slotsPerSequence, long long* elementsPerFrame);
/* bhip_klt_set_description_f32 / bhip_klt_track_f32 on a GrayU8 image with GrayS16 derivatives (KltTracker<GrayU8, GrayS16> with
 * BilinearRectangle_U8 / _S16); templates, G, positions, faults and errors are float as there */
int bhip_klt_set_description_u8(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const uint8_t* image, int imgStart, int imgStride, const int16_t* derivX,
								const int16_t* derivY, int dStart, int dStride, int width, int height, const float* xy, int n, float* desc, float* descX,
								float* descY, float* G, uint8_t* ok);
int bhip_klt_track_u8(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const uint8_t* image, int imgStart, int imgStride, int width, int height,
					  const float* desc, const float* descX, const float* descY, const float* G, float* xy, int n, int* fault, float* error);

/* ---- stationary background models: FactoryBackgroundModel.stationaryBasic / stationaryGaussian / stationaryGmm (background.hip) ----
 * BackgroundStationaryBasic_SB / _PL      F:alg/background/stationary/BackgroundStationaryBasic_SB.java:58-123, BackgroundStationaryBasic_PL.java:66-142
 * BackgroundStationaryGaussian_SB / _PL   F:alg/background/stationary/BackgroundStationaryGaussian_SB.java:58-142, BackgroundStationaryGaussian_PL.java:72-180
 * BackgroundStationaryGmm_SB / _MB        F:alg/background/stationary/BackgroundStationaryGmm.java:48-78, BackgroundStationaryGmm_SB.java:50-100,
 *                                         BackgroundStationaryGmm_MB.java:54-105, F:alg/background/BackgroundGmmCommon.java:78-375
 * factory and configs                     F:factory/background/FactoryBackgroundModel.java:47-64,112-141,193-225, ConfigBackground*.java
 *
 * A bhip_bg holds `streams` independent models of one algorithm for frames of one type and shape, resident on the device: stream s is one
 * Java object.  Frames are GrayU8 / GrayF32 (family GRAY, bands ignored: the *_SB classes) or Planar<GrayU8> / Planar<GrayF32> of 1..4 bands
 * (family PLANAR: the *_PL / *_MB classes, also for one band).  Model planes and masks equal the single-threaded Java results bit for bit:
 * plain IEEE fp32 evaluated left to right without fused multiply-add, the one double accumulator of Basic_PL.segment, denormal variances kept
 * (ConfigBackgroundGaussian.initialVariance is Float.MIN_VALUE), 0/0 = NaN and x/0 = +Inf in Gaussian.segment as in Java.
 *
 * Rules taken from the reference:
 *  - updateBackground(frame, mask) is update, then segment, for Basic and Gaussian (F:alg/background/BackgroundModelStationary.java:48-51);
 *    GMM writes updateMixture's return value;
 *  - a stream's first Basic / Gaussian update after creation or bhip_bg_reset initialises it (GConvertImage.convert; Gaussian: the variance
 *    planes are filled with initialVariance); a GMM stream starts from the zeroed model; an uninitialised stream segments to unknownValue;
 *  - BackgroundStationaryGaussian tests `background.width == 1` for "not initialised", so a Gaussian model of width 1 never leaves that state:
 *    every update initialises it again and every mask is unknownValue.  Reproduced;
 *  - BackgroundGmmCommon.unknownValue is refreshed only inside segment(): a GMM update that creates a pixel's first Gaussian writes the
 *    unknown value that the stream's last segment() on an initialised model installed, 0 before any.  Kept per stream, untouched by
 *    bhip_bg_reset (the Java object keeps it too);
 *  - bhip_bg_create_* is the factory call: config.checkValidity(), the constructor and the factory's setters.  stationaryBasic does not forward
 *    config.unknownValue (it stays 0 until bhip_bg_set_unknown_value); stationaryGmm installs the config's maxDistance (3) and
 *    significantWeight (0.01f) over the constructor's 3*3 and min(0.2f, 100/learningPeriod).  The setters validate nothing, as in Java, except
 *    bhip_bg_set_unknown_value (0..255).
 * Deviations and limits:
 *  - width, height and the stream count are fixed at creation; the reference's re-initialisation when the frame size changes and its
 *    InputSanityCheck exceptions belong to the caller (the Python and Java classes create a new handle);
 *  - a mask is written, never reshaped; frames and masks must not overlap;
 *  - BHIP_ERR_UNSUPPORTED: numberOfGaussian > 8 (1..8 are compiled: the mixture lives in registers), more than 4 bands, family INTERLEAVED,
 *    pixel types other than U8 / F32;
 *  - BHIP_ERR_INVALID, nothing written: what checkValidity and the constructors reject (learnRate outside [0,1], threshold <= 0,
 *    initialVariance <= 0, minimumDifference < 0, learningPeriod <= 0, decayCoefient < 0, numberOfGaussian outside 1..255, an unknownValue
 *    outside 0..255 as in BackgroundModel.setUnknownValue), a NULL Basic or
 *    Gaussian config (threshold has no default), bands outside 1.. for PLANAR, sizes < 1, a view with stride < width, numFrames < 1, a call of
 *    the other pixel type, a setter the algorithm does not have, a stream index out of range. */
typedef enum { BHIP_BG_BASIC = 0, BHIP_BG_GAUSSIAN = 1, BHIP_BG_GMM = 2 } bhip_bg_algorithm;
typedef enum { BHIP_IMAGE_GRAY = 0, BHIP_IMAGE_PLANAR = 1, BHIP_IMAGE_INTERLEAVED = 2 } bhip_image_family;   /* ImageType.Family */
typedef enum { BHIP_PIXEL_U8 = 0, BHIP_PIXEL_F32 = 1 } bhip_pixel_type;
/* F:factory/background/ConfigBackgroundBasic.java */
typedef struct {
	float learnRate;      /* 0.05f */
	float threshold;      /* no default in Java: 0 here, which bhip_bg_create_basic refuses */
	int unknownValue;     /* 0; not forwarded by stationaryBasic */
} bhip_bg_basic_cfg;
/* F:factory/background/ConfigBackgroundGaussian.java */
typedef struct {
	float learnRate;          /* 0.05f */
	float threshold;          /* no default in Java: 0 here, which bhip_bg_create_gaussian refuses */
	float initialVariance;    /* Float.MIN_VALUE, the smallest denormal */
	float minimumDifference;  /* 0 */
	int unknownValue;         /* 0 */
} bhip_bg_gaussian_cfg;
/* F:factory/background/ConfigBackgroundGmm.java */
typedef struct {
	float learningPeriod;     /* 1000 */
	float initialVariance;    /* 400 */
	float decayCoefient;      /* 0.005f */
	float maxDistance;        /* 3 */
	int numberOfGaussian;     /* 5 */
	float significantWeight;  /* 0.01f */
	int unknownValue;         /* 0 */
} bhip_bg_gmm_cfg;
void bhip_bg_basic_cfg_default(bhip_bg_basic_cfg* c);
void bhip_bg_gaussian_cfg_default(bhip_bg_gaussian_cfg* c);
void bhip_bg_gmm_cfg_default(bhip_bg_gmm_cfg* c);
/* family / pixelType: bhip_image_family / bhip_pixel_type; bands: the Planar image's, ignored for GRAY.  cfg NULL: the defaults (GMM only) */
int bhip_bg_create_basic(bhip_ctx* ctx, const bhip_bg_basic_cfg* cfg, int family, int pixelType, int bands, int width, int height, int streams, bhip_bg** out);
int bhip_bg_create_gaussian(bhip_ctx* ctx, const bhip_bg_gaussian_cfg* cfg, int family, int pixelType, int bands, int width, int height, int streams, bhip_bg** out);
int bhip_bg_create_gmm(bhip_ctx* ctx, const bhip_bg_gmm_cfg* cfg, int family, int pixelType, int bands, int width, int height, int streams, bhip_bg** out);
int bhip_bg_destroy(bhip_bg* bg);
/* BackgroundModel.reset() of stream `stream`, or of every stream when stream < 0 */
int bhip_bg_reset(bhip_bg* bg, int stream);
/* BackgroundModel.setUnknownValue and the setters of BackgroundAlgorithmBasic / BackgroundAlgorithmGaussian / BackgroundAlgorithmGmm, for
 * every stream.  setLearningPeriod: learningRate = 1.0f / period */
int bhip_bg_set_unknown_value(bhip_bg* bg, int unknownValue);
int bhip_bg_set_threshold(bhip_bg* bg, float threshold);                   /* Basic, Gaussian */
int bhip_bg_set_learn_rate(bhip_bg* bg, float learnRate);                  /* Basic, Gaussian */
int bhip_bg_set_initial_variance(bhip_bg* bg, float initialVariance);      /* Gaussian, GMM */
int bhip_bg_set_minimum_difference(bhip_bg* bg, float minimumDifference);  /* Gaussian */
int bhip_bg_set_learning_period(bhip_bg* bg, float period);                /* GMM */
int bhip_bg_set_significant_weight(bhip_bg* bg, float significantWeight);  /* GMM */
int bhip_bg_set_max_distance(bhip_bg* bg, float maxDistance);              /* GMM */
/* GMM: installs BackgroundGmmCommon.unknownValue of every stream, as a segment() on an initialised model would.  For a caller that replaces a
 * handle (another frame size) and has to carry the Java object's stale value over */
int bhip_bg_set_common_unknown_value(bhip_bg* bg, int unknownValue);
/* updateBackground(frame_t) (dev_masks NULL) or updateBackground(frame_t, mask_t) for t = 0 .. numFrames-1, in order, on every stream, in one
 * launch that keeps each pixel's model in registers.  Pixel (x, y) of band b of frame t of stream s is
 * dev_frames[s*streamStride + t*frameStride + b*bandStride + y*stride + x], mask pixel dev_masks[s*mStreamStride + t*mFrameStride + y*mStride + x]
 * (strides in elements, any byte alignment).  No host synchronisation. */
int bhip_bg_update_dev_u8(bhip_bg* bg, const uint8_t* dev_frames, long long streamStride, long long frameStride, long long bandStride, int stride, int numFrames,
						  uint8_t* dev_masks, long long mStreamStride, long long mFrameStride, int mStride);
int bhip_bg_update_dev_f32(bhip_bg* bg, const float* dev_frames, long long streamStride, long long frameStride, long long bandStride, int stride, int numFrames,
						   uint8_t* dev_masks, long long mStreamStride, long long mFrameStride, int mStride);
/* segment(frame, mask) with one frame per stream; the model is not changed */
int bhip_bg_segment_dev_u8(bhip_bg* bg, const uint8_t* dev_frames, long long streamStride, long long bandStride, int stride, uint8_t* dev_masks,
						   long long mStreamStride, int mStride);
int bhip_bg_segment_dev_f32(bhip_bg* bg, const float* dev_frames, long long streamStride, long long bandStride, int stride, uint8_t* dev_masks,
							long long mStreamStride, int mStride);
/* the same on host buffers (the first element at frames[start] / masks[mStart]): staged, run through the _dev forms, synchronised */
int bhip_bg_update_u8(bhip_bg* bg, const uint8_t* frames, long long start, long long streamStride, long long frameStride, long long bandStride, int stride,
					  int numFrames, uint8_t* masks, long long mStart, long long mStreamStride, long long mFrameStride, int mStride);
int bhip_bg_update_f32(bhip_bg* bg, const float* frames, long long start, long long streamStride, long long frameStride, long long bandStride, int stride,
					   int numFrames, uint8_t* masks, long long mStart, long long mStreamStride, long long mFrameStride, int mStride);
int bhip_bg_segment_u8(bhip_bg* bg, const uint8_t* frames, long long start, long long streamStride, long long bandStride, int stride, uint8_t* masks,
					   long long mStart, long long mStreamStride, int mStride);
int bhip_bg_segment_f32(bhip_bg* bg, const float* frames, long long start, long long streamStride, long long bandStride, int stride, uint8_t* masks,
						long long mStart, long long mStreamStride, int mStride);
/* The model of one stream in the reference's layout, width*height*components floats (bhip_bg_model_floats):
 *   Basic     `bands` GrayF32 planes [band][y][x]                     (getBackground())
 *   Gaussian  Planar<GrayF32>(2*bands): plane 2b the mean, 2b+1 the variance of band b
 *   GMM       common.model.data[y][x*modelStride + g*(2+bands) + k], k = 0 weight, 1 variance, 2.. the means; modelStride = numberOfGaussian*(2+bands)
 * BHIP_ERR_INVALID when the stream is not initialised (the reference's model is then 0 x 0 or 1 x 1).  bhip_bg_store_model is the inverse and
 * leaves the stream initialised. */
int bhip_bg_model_floats(bhip_bg* bg, long long* floats);
int bhip_bg_fetch_model(bhip_bg* bg, int stream, float* model);
int bhip_bg_store_model(bhip_bg* bg, int stream, const float* model);

/* ---------------------------------------------------------------------------------------------------------------
 * Dense KLT optical flow: DenseOpticalFlow.process(source, destination, flow) of FactoryDenseOpticalFlow.flowKlt(PkltConfig, radius, GrayF32 | GrayU8,
 * GrayF32 | GrayS16) (F:factory/flow/FactoryDenseOpticalFlow.java:61-82): FlowKlt_to_DenseOpticalFlow.process (F:abst/flow/FlowKlt_to_DenseOpticalFlow.java:76-86)
 * builds FactoryPyramid.discreteGaussian(scales, -1, 2, true) of both frames and the FactoryDerivative.sobel gradient (BorderType.EXTENDED; GrayU8 ->
 * GrayS16) of every source layer, then DenseOpticalFlowKlt.process (F:alg/flow/DenseOpticalFlowKlt.java:62-131): for every pixel (x, y) in raster order
 * feature.setPosition(x, y), PyramidKltTracker.setDescription on the source pyramid (F:alg/tracker/klt/PyramidKltTracker.java:58-71), track on the
 * destination pyramid (:113-151); on SUCCESS score = tracker.getError(), the pixel's slot is set to (score * 0.7f, flow = (feature.x - x, feature.y - y))
 * and checkNeighbors offers (score, flow) to every slot of the (2*radius+1)^2 window clipped to the image: a slot takes it when its score is greater, or
 * equal with flowX^2 + flowY^2 strictly smaller than its own.  `radius` is the template radius of the tracker and the radius of that window.  The
 * raster-order pass is computed as a reduction per slot ("Dense KLT optical flow"); every value equals the single-threaded Java arithmetic
 * bit for bit.  cfg == NULL: KltConfig's defaults.
 *   flow    pixel (x, y) of pair b is the two floats (x, y) at dev_flow[b*fImageStride + y*fStride + 2*x] (strides in floats, fStride >= 2*width);
 *           an invalid pixel (ImageFlow.D.markInvalid) is (NaN, 0)
 *   tracks  NULL, or [batch][height][width] records {int fault; float error, dx, dy} (16 bytes, dense) of every pixel's own track: fault is a
 *           BHIP_KLT_* value or BHIP_FLOW_NO_DESCRIPTION (setDescription returned false); error and (dx, dy) are tracker.getError() and the flow
 *           where fault is BHIP_KLT_SUCCESS, 0 elsewhere
 *   form    which track kernel runs: BHIP_FLOW_FORM_AUTO (lane per pixel for radius <= 3, else wave per pixel), BHIP_FLOW_FORM_LANE (radius <= 3 only),
 *           BHIP_FLOW_FORM_WAVE (any radius); the results are the same bit for bit
 * Validation, BHIP_ERR_INVALID and nothing is written: radius < 1, numLayers < 1, scales[0] != 1, a scale smaller than the layer below or not a multiple
 * of it (ImagePyramidBase.checkScales, PyramidDiscrete.setScaleFactors), non-positive sizes, strides smaller than a row, an unknown form.
 * Deviations: a pixel whose track reaches one of the positions where the reference throws (BHIP_KLT_REFERENCE_THROWS) counts as a failed track; y of
 * an invalid pixel is 0, the result for a freshly constructed ImageFlow, where the reference keeps what the caller's ImageFlow held (a caller that has
 * to reproduce that merges the kept y values, as the Python mirror does).
 * Limits, BHIP_ERR_UNSUPPORTED and nothing is written: radius > 7, numLayers > 8, maxIterations < 1, batch > 65535, BHIP_FLOW_FORM_LANE with radius > 3.
 * The _dev forms do not synchronise; scratch (pyramids, gradients, records) belongs to the context. */
#define BHIP_FLOW_NO_DESCRIPTION 6
#define BHIP_FLOW_FORM_AUTO 0
#define BHIP_FLOW_FORM_LANE 1
#define BHIP_FLOW_FORM_WAVE 2
int bhip_flow_klt_dev_f32(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, const float* dev_src, long long sImageStride,
						  int sStride, const float* dev_dst, long long dImageStride, int dStride, int width, int height, int batch, float* dev_flow,
						  long long fImageStride, int fStride, void* dev_tracks, int form);
int bhip_flow_klt_dev_u8(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, const uint8_t* dev_src, long long sImageStride,
						 int sStride, const uint8_t* dev_dst, long long dImageStride, int dStride, int width, int height, int batch, float* dev_flow,
						 long long fImageStride, int fStride, void* dev_tracks, int form);
/* the same on one pair of host images: pixel (x, y) at src[sStart + y*sStride + x], its flow at flow[fStart + y*fStride + 2*x]; staged, run through the
 * _dev form (BHIP_FLOW_FORM_AUTO), synchronised */
int bhip_flow_klt_f32(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, const float* src, int sStart, int sStride,
					  const float* dst, int dStart, int dStride, int width, int height, float* flow, int fStart, int fStride);
int bhip_flow_klt_u8(bhip_ctx* ctx, const bhip_klt_cfg* cfg, int radius, const int* scales, int numLayers, const uint8_t* src, int sStart, int sStride,
					 const uint8_t* dst, int dStart, int dStride, int width, int height, float* flow, int fStart, int fStride);
/* pixels tracked and Lucas-Kanade iterations run by the last bhip_flow_klt_* call on this context (synchronises) */
int bhip_flow_klt_stats(bhip_ctx* ctx, long long* pixels, long long* iterations);

/* ---------------------------------------------------------------------------------------------------------------
 * Horn-Schunck dense optical flow: DenseOpticalFlow.process(source, destination, flow) of FactoryDenseOpticalFlow.hornSchunck(ConfigHornSchunck,
 * GrayF32 | GrayU8) (F:factory/flow/FactoryDenseOpticalFlow.java:122-138): HornSchunck_to_DenseOpticalFlow over HornSchunck_F32 / HornSchunck_U8
 * (F:alg/flow/HornSchunck.java:92-191, HornSchunck_F32.java:36-175, HornSchunck_U8.java:38-177).  process computes derivX, derivY, derivT of the
 * pair (GrayU8: in int, GrayS16) and runs numIterations Jacobi iterations from the zero flow (resetOutput is true and has no setter): with w =
 * width-1, h = height-1, A = source, B = destination,
 *   derivX  x < w, y < h: 0.25f*(d0+d1+d2+d3), the x forward differences of A row y, A row y+1, B row y, B row y+1; y == h: 0.5f*(d0+d1) of A, B; x == w: 0
 *   derivY  x < w, y < h: 0.25f*(d0+d1+d2+d3), the y forward differences of A column x, A column x+1, B column x, B column x+1; x == w, y < h:
 *           0.5f*(d0+d1) of A, B; y == h: 0
 *   derivT  0.25f*(d0+d1+d2+d3), dk = B - A at (x,y), (x+1,y), (x,y+1), (x+1,y+1) with the coordinates clamped to the image
 *   GrayU8  the same taps in int, (..)/4 and (..)/2 truncating toward zero
 *   every iteration, for every pixel from the flow of the iteration before (x and y clamped to the image, getExtend):
 *           u = 0.1666667f*(f0+f1+f2+f3) + 0.08333333f*(f4+f5+f6+f7) over left, right, up, down, up-left, up-right, down-left, down-right, v alike;
 *           r = (dx*u + dy*v + dt)/(alpha2 + dx*dx + dy*dy), alpha2 = alpha*alpha in float; flow = (u - dx*r, v - dy*r)
 * IEEE fp32, nothing contracted, the division correctly rounded: every float equals the single-threaded Java result bit for bit (alpha = 0 on a
 * flat patch gives 0/0 = NaN, which spreads one pixel per iteration, as in Java).  numIterations <= 0 gives the zero flow, as the Java loop does.
 *   flow    pixel (x, y) of pair b is the two floats (x, y) at dev_flow[b*fImageStride + y*fStride + 2*x] (strides in floats, fStride >= 2*width)
 *   deriv   NULL, or dense [batch][3][height][width] float32 that receives derivX, derivY, derivT (the GrayS16 values of GrayU8 pairs as floats)
 *   itersPerLaunch  iterations one kernel launch runs on a BHIP_FLOW_HS_TILE_WIDTH x BHIP_FLOW_HS_TILE_HEIGHT tile out of LDS ("Horn-Schunck dense
 *           optical flow"): 0 = the library's choice, 1 .. BHIP_FLOW_HS_MAX_FUSED forces the depth; the results are the same bit for bit
 * Validation, BHIP_ERR_INVALID and nothing is written: non-positive sizes, strides smaller than a row, null images, itersPerLaunch outside
 * 0 .. BHIP_FLOW_HS_MAX_FUSED.
 * Deviations: derivY(w, h) is never written by the reference and keeps what the reused array held: it is 0 here, the value of a freshly
 * constructed instance; HornSchunck_F32.computeDerivT :114 indexes image1 with image2.stride in its fourth tap: image1's pixel (x+1, y+1) is read
 * here whatever the two strides are; the flow has the size of the images (the Java indexes past a smaller one; the mirrors refuse another size).
 * Limits, BHIP_ERR_UNSUPPORTED and nothing is written: batch > 65535, width or height > 1048576, width * height > 2^28.
 * The _dev forms do not synchronise; scratch (the derivatives when deriv is NULL, two flow images when there is more than one launch) belongs to
 * the context. */
#define BHIP_FLOW_HS_MAX_FUSED 8
#define BHIP_FLOW_HS_TILE_WIDTH 112
#define BHIP_FLOW_HS_TILE_HEIGHT 48
int bhip_flow_hs_dev_f32(bhip_ctx* ctx, float alpha, int numIterations, const float* dev_src, long long sImageStride, int sStride, const float* dev_dst,
						 long long dImageStride, int dStride, int width, int height, int batch, float* dev_flow, long long fImageStride, int fStride,
						 float* dev_deriv, int itersPerLaunch);
int bhip_flow_hs_dev_u8(bhip_ctx* ctx, float alpha, int numIterations, const uint8_t* dev_src, long long sImageStride, int sStride, const uint8_t* dev_dst,
						long long dImageStride, int dStride, int width, int height, int batch, float* dev_flow, long long fImageStride, int fStride,
						float* dev_deriv, int itersPerLaunch);
/* the same on one pair of host images: pixel (x, y) at src[sStart + y*sStride + x], its flow at flow[fStart + y*fStride + 2*x]; staged, run through the
 * _dev form (itersPerLaunch 0, no deriv), synchronised */
int bhip_flow_hs_f32(bhip_ctx* ctx, float alpha, int numIterations, const float* src, int sStart, int sStride, const float* dst, int dStart, int dStride,
					 int width, int height, float* flow, int fStart, int fStride);
int bhip_flow_hs_u8(bhip_ctx* ctx, float alpha, int numIterations, const uint8_t* src, int sStart, int sStride, const uint8_t* dst, int dStart, int dStride,
					int width, int height, float* flow, int fStart, int fStride);

/* ---- thresholding: FactoryThresholdBinary.threshold(ConfigThreshold, GrayU8 | GrayF32) -> InputToBinary.process (threshold.hip),
 *      I:factory/filter/binary/FactoryThresholdBinary.java:318-372; the provider seam is I:factory/filter/binary/BOverrideFactoryThresholdBinary.java.
 *      The output is the GrayU8 0/1 image, bit for bit the single-threaded Java result.
 *   FIXED           GlobalFixedBinaryFilter -> ImplThresholdImageOps.threshold (I:alg/filter/binary/impl/ImplThresholdImageOps.java:46-134); GrayU8
 *                   compares with (int)fixedThreshold, GrayF32 with (float)fixedThreshold
 *   GLOBAL_OTSU     GrayU8 with minPixelValue 0 and maxPixelValue 255: GlobalBinaryFilter.process (I:abst/filter/binary/GlobalBinaryFilter.java:57-88)
 *                   on GThresholdImageOps.computeOtsu (I:alg/filter/binary/GThresholdImageOps.java:56-142), histogram and threshold on the device
 *   LOCAL_MEAN      ImplThresholdImageOps.localMean (:226-270 GrayU8, :424-468 GrayF32) on BlurImageOps.mean
 *   LOCAL_GAUSSIAN  ImplThresholdImageOps.localGaussian (:272-323, :470-520) on BlurImageOps.gaussian(.., -1, radius, ..)
 *   BLOCK_MIN_MAX   ThresholdBlock (I:alg/filter/binary/ThresholdBlock.java:90-170) with impl/ThresholdBlockMinMax_U8 / _F32
 *   BLOCK_MEAN      ThresholdBlock with impl/ThresholdBlockMean_U8 / _F32 (GrayF32: the block sum runs in raster order, as there)
 *   BLOCK_OTSU      GrayU8: ThresholdBlockOtsu.java:73-145 with ComputeOtsu.java:71-170 (useOtsu2, tuning, scale)
 * The local radius is ConfigLength.computeI(min(width, height)) / 2 (T:struct/ConfigLength.java:74-84), the requested block width computeI of the same.
 * BHIP_ERR_UNSUPPORTED and nothing is written: GLOBAL_ENTROPY, GLOBAL_LI, GLOBAL_HUANG, LOCAL_OTSU, LOCAL_SAVOLA, LOCAL_NICK; GLOBAL_OTSU and
 * BLOCK_OTSU on GrayF32 (InputToBinarySwitch's conversion in the reference); GLOBAL_OTSU with another pixel range; a GrayF32 local threshold
 * whose blur kernel is wider than 255 taps (the limit of bhip_mean_f32 / bhip_gaussian_f32).
 * BHIP_ERR_INVALID and nothing is written, where the reference throws: an unknown type, a local radius <= 0, a requested block width <= 0,
 * empty images, strides smaller than a row.
 * Fields mirror ConfigThreshold (I:factory/filter/binary/ConfigThreshold.java:30-86), ConfigThresholdBlockMinMax and ConfigThresholdLocalOtsu;
 * widthLength / widthFraction are ConfigLength.length / fraction (fraction < 0: a fixed length). */
#define BHIP_THRESHOLD_FIXED 0 /* ThresholdType ordinals (I:factory/filter/binary/ThresholdType.java:28-109) */
#define BHIP_THRESHOLD_GLOBAL_ENTROPY 1
#define BHIP_THRESHOLD_GLOBAL_OTSU 2
#define BHIP_THRESHOLD_GLOBAL_LI 3
#define BHIP_THRESHOLD_GLOBAL_HUANG 4
#define BHIP_THRESHOLD_LOCAL_GAUSSIAN 5
#define BHIP_THRESHOLD_LOCAL_MEAN 6
#define BHIP_THRESHOLD_LOCAL_OTSU 7
#define BHIP_THRESHOLD_BLOCK_MIN_MAX 8
#define BHIP_THRESHOLD_BLOCK_MEAN 9
#define BHIP_THRESHOLD_BLOCK_OTSU 10
#define BHIP_THRESHOLD_LOCAL_SAVOLA 11
#define BHIP_THRESHOLD_LOCAL_NICK 12
typedef struct bhip_threshold_cfg {
	int type;                     /* BHIP_THRESHOLD_* */
	double fixedThreshold;        /* FIXED */
	double scale;                 /* 1.0; 0.95 for the local and block types (ConfigThreshold.local) */
	int down;                     /* 1 */
	double widthLength;           /* 11 */
	double widthFraction;         /* -1 */
	int minPixelValue;            /* 0 */
	int maxPixelValue;            /* 255 */
	int thresholdFromLocalBlocks; /* 1 */
	double minimumSpread;         /* 10 (ConfigThresholdBlockMinMax) */
	int useOtsu2;                 /* 1 (ConfigThresholdLocalOtsu) */
	double tuning;                /* 0 */
} bhip_threshold_cfg;
/* ConfigThreshold.fixed(0) / global(type) / local(type, 11) (ConfigThreshold.java:88-133); BHIP_ERR_INVALID for a type outside the list */
int bhip_threshold_cfg_default(int type, bhip_threshold_cfg* cfg);
/* ThresholdBlock.selectBlockSize (ThresholdBlock.java:112-127); the stats grid is (width / blockWidth) x (height / blockHeight) and the last
 * block of a direction takes the remainder.  BHIP_ERR_INVALID: non-positive sizes or requestedWidth.  Host only. */
int bhip_threshold_block_size(int width, int height, int requestedWidth, int* blockWidth, int* blockHeight);
/* batch images at dev_in + b*inImageStride -> dev_out + b*outImageStride (strides in elements, any alignment).  The whole width x height view of
 * every output image is written and nothing outside it.  Asynchronous on the context's stream, no host synchronisation; scratch belongs to the
 * context.  GrayU8 local thresholds run as one launch out of LDS up to radius 16, beyond it (and for kernels wider than the image) as two blur
 * passes and a compare. */
int bhip_threshold_dev_u8(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height,
						  int batch, uint8_t* dev_out, long long outImageStride, int outStride);
int bhip_threshold_dev_f32(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, const float* dev_in, long long inImageStride, int inStride, int width, int height,
						   int batch, uint8_t* dev_out, long long outImageStride, int outStride);
/* the same on one host image view: staged, run through the _dev form, synchronised */
int bhip_threshold_u8(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out,
					  int outStart, int outStride);
int bhip_threshold_f32(bhip_ctx* ctx, const bhip_threshold_cfg* cfg, const float* in, int inStart, int inStride, int width, int height, uint8_t* out,
					   int outStart, int outStride);
/* BOverrideBlurImageOps.mean / gaussian targets for GrayU8: BlurImageOps.mean(GrayU8, .., radiusX, radiusY, ..) (I:alg/filter/blur/BlurImageOps.java:75-92:
 * ConvolveImageMean.horizontal then .vertical with a GrayU8 image between them, I:alg/filter/convolve/ConvolveImageMean.java:168-215) and
 * BlurImageOps.gaussian(GrayU8, .., -1, radius, ..) (:122-141: the Kernel1D_S32 of bhip_gaussian_kernel1d_s32 through
 * ConvolveImageNormalized.horizontal / vertical).  Every pixel is (total + weight/2) / weight over the taps inside the image, any radius >= 1;
 * BHIP_ERR_INVALID for a radius <= 0 ("Radius must be > 0").  The _dev forms are batched and do not synchronise. */
int bhip_mean_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int radiusX, int radiusY, uint8_t* out, int outStart,
				 int outStride);
int bhip_gaussian_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int radius, uint8_t* out, int outStart, int outStride);
int bhip_mean_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int radiusX, int radiusY,
					 uint8_t* dev_out, long long outImageStride, int outStride);
int bhip_gaussian_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int radius,
						 uint8_t* dev_out, long long outImageStride, int outStride);

/* ---- binary images: BinaryImageOps (I:alg/filter/binary/BinaryImageOps.java) on GrayU8 0/1 images and GrayS32 label images
 *      (binary_ops.hip, label.hip).  There is no BOverride hook for BinaryImageOps in the reference: integration/java/boofcv/hip/BinaryImageOpsHip.java
 *      is a provider class with the same static signatures.
 * The _dev forms take batch images at dev_x + b*xImageStride (strides in elements, any alignment), write the whole width x height view of every
 * output image and nothing outside it, are asynchronous on the context's stream without host synchronisation, and keep their scratch in the
 * context.  The forms without _dev take one host image view each: staged, run through the _dev form, synchronised.
 * Results equal the single-threaded Java results bit for bit on images that hold only 0 and 1.  Other byte values: the logic operations still
 * follow the reference's tests (== 1, == 0, !=); the neighbourhood operations give an unspecified result inside the view (the reference sums
 * raw signed bytes in its inner loops and unsigned get() values on the frame; here every byte counts as unsigned).
 * Not provided: thin (BinaryThinning), the contour point lists of contour / contourExternal, labelToClusters, clusterToBinary, image types other
 * than GrayU8 / GrayS32.
 * BHIP_ERR_INVALID and nothing is written: empty images, strides smaller than a row, an unknown op or rule, erode4 with numTimes <= 0
 * ("numTimes must be >= 1"), overlapping input and output of a neighbourhood operation.  BHIP_ERR_UNSUPPORTED: more than 65535 images in a
 * batch; for the labelling, width * height beyond an int32 index or more than 2097120 rows. */
#define BHIP_LOGIC_AND 0 /* ImplBinaryImageOps.logicAnd: a == 1 && a == b */
#define BHIP_LOGIC_OR 1  /* a == 1 || b == 1 */
#define BHIP_LOGIC_XOR 2 /* a != b */
/* BinaryImageOps.logicAnd / logicOr / logicXor (:69-125, impl/ImplBinaryImageOps.java:30-78).  dev_out may be dev_a or dev_b (the same view). */
int bhip_binary_logic_dev_u8(bhip_ctx* ctx, int op, const uint8_t* dev_a, long long aImageStride, int aStride, const uint8_t* dev_b, long long bImageStride,
							 int bStride, int width, int height, int batch, uint8_t* dev_out, long long outImageStride, int outStride);
int bhip_binary_logic_u8(bhip_ctx* ctx, int op, const uint8_t* a, int aStart, int aStride, const uint8_t* b, int bStart, int bStride, int width, int height,
						 uint8_t* out, int outStart, int outStride);
/* BinaryImageOps.invert (:134-145, ImplBinaryImageOps.java:80-93): in == 0 ? 1 : 0.  dev_out may be dev_in. */
int bhip_binary_invert_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, uint8_t* dev_out,
							  long long outImageStride, int outStride);
int bhip_binary_invert_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart, int outStride);
/* BinaryImageOps.erode4 / dilate4 / erode8 / dilate8(input, numTimes, output) (:158-361): impl/ImplBinaryInnerOps.java for 1 <= x < width-1,
 * 1 <= y < height-1, then impl/ImplBinaryBorderOps.java in its loop order (every x: top, bottom; every y: left, right -- the last write stands,
 * which is what widths and heights of 1 and 2 and the corners come out of).  The value outside the image is 0 for erode4, dilate4 and dilate8
 * and 1 for erode8 (ImplBinaryBorderOps.java:105), at every iteration.  erode4 refuses numTimes <= 0; the other three apply the operation once
 * for numTimes <= 1.  Up to 4 iterations run in one launch inside an LDS tile with a halo; more repeat such launches between two scratch images.
 * Input and output must not overlap. */
#define BHIP_MORPH_ERODE4 0
#define BHIP_MORPH_DILATE4 1
#define BHIP_MORPH_ERODE8 2
#define BHIP_MORPH_DILATE8 3
int bhip_binary_morph_dev_u8(bhip_ctx* ctx, int op, int numTimes, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch,
							 uint8_t* dev_out, long long outImageStride, int outStride);
int bhip_binary_morph_u8(bhip_ctx* ctx, int op, int numTimes, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart,
						 int outStride);
/* BinaryImageOps.edge4 / edge8(input, output, outsideZero) (:258-269, :378-389); rule: BHIP_CONNECT_*.  outsideZero != 0: the frame is a copy of
 * the input (ImplBinaryBorderOps.edge_outside0), otherwise the value outside the image is 1.  Input and output must not overlap. */
#define BHIP_CONNECT_FOUR 4 /* ConnectRule.FOUR (T:struct/ConnectRule.java) */
#define BHIP_CONNECT_EIGHT 8
int bhip_binary_edge_dev_u8(bhip_ctx* ctx, int rule, int outsideZero, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch,
							uint8_t* dev_out, long long outImageStride, int outStride);
int bhip_binary_edge_u8(bhip_ctx* ctx, int rule, int outsideZero, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart,
						int outStride);
/* BinaryImageOps.removePointNoise (:400-411): 8-neighbour total < 2 -> 0, > 6 -> 1, else the input; outside is 0 and the frame rows and columns
 * have no "> 6" branch (ImplBinaryBorderOps.java:297-339).  Input and output must not overlap. */
int bhip_binary_remove_point_noise_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch,
										  uint8_t* dev_out, long long outImageStride, int outStride);
int bhip_binary_remove_point_noise_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart, int outStride);
/* The labelled image and getContours().size of BinaryImageOps.contour(input, rule, output) (:457-469, LinearContourLabelChang2004.process :96-152):
 * a pixel equal to 1 is foreground, background gets 0, blobs are numbered 1..N per image in the raster order of their first pixel, and N goes to
 * dev_numBlobs[b].  The contour point lists are not produced.  Parity holds for images of 0 and 1: on other values the reference scans and
 * traces with != 1 but tests the pixel below with == 0 (step 2), so it is not the connected components of the 1s there; this is.  Union-find with the smallest linear index as root, then a raster-order rank of
 * the roots: six launches, no workgroup waits for another.  Scratch: 4 bytes per pixel plus 4 per row, for at most 256 MiB of images at a time. */
int bhip_label_blobs_dev_u8_s32(bhip_ctx* ctx, int rule, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch,
								int32_t* dev_out, long long outImageStride, int outStride, int* dev_numBlobs);
int bhip_label_blobs_u8_s32(bhip_ctx* ctx, int rule, const uint8_t* in, int inStart, int inStride, int width, int height, int32_t* out, int outStart, int outStride,
							int* numBlobs);
/* BinaryImageOps.relabel(GrayS32, int[] labels) in place (:509-515): pixel = labels[pixel].  Deviation: a pixel outside [0, numLabels) is left
 * unchanged (the reference throws ArrayIndexOutOfBoundsException; the device form cannot report it without a synchronisation). */
int bhip_relabel_dev_s32(bhip_ctx* ctx, int32_t* dev_img, long long imageStride, int stride, int width, int height, int batch, const int* dev_labels, int numLabels);
int bhip_relabel_s32(bhip_ctx* ctx, int32_t* img, int start, int stride, int width, int height, const int* labels, int numLabels);
/* BinaryImageOps.labelToBinary(GrayS32, GrayU8) (:524-534: pixel != 0) when selected is null, else labelToBinary(GrayS32, GrayU8, boolean[]
 * selectedBlobs) (:545-557: selectedBlobs[pixel]) with one byte per entry, non-zero = true.  Deviation: a pixel outside [0, numSelected) gives 0
 * (the reference throws). */
int bhip_label_to_binary_dev_s32_u8(bhip_ctx* ctx, const int32_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, uint8_t* dev_out,
									long long outImageStride, int outStride, const uint8_t* dev_selected, int numSelected);
int bhip_label_to_binary_s32_u8(bhip_ctx* ctx, const int32_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart, int outStride,
								const uint8_t* selected, int numSelected);

/* ---- line detection: the stages of FactoryDetectLine.houghLinePolar(ConfigHoughBinary, ...) and houghLineFoot(ConfigHoughGradient, ...)
 *      (F:factory/feature/detect/line/FactoryDetectLine.java:90-163; hough.hip, edge.hip, the Prewitt form of the gradient kernels in gradient.hip).
 *      The parity target is the single-threaded classes.  There is no BOverride hook for them: integration/java/boofcv/hip/HoughLinesHip.java is
 *      a provider class.  The _dev forms take batch images at dev_x + b*xImageStride (strides in elements), write the whole view of every output
 *      image and nothing outside it, are asynchronous on the context's stream without host synchronisation, and keep their scratch in the
 *      context.  Every argument check comes before anything is queued: a refused call writes nothing.  BHIP_ERR_UNSUPPORTED: more than 65535
 *      images in a batch or rows in an image.  Not provided: houghLinePolar(ConfigHoughGradient, ...), houghLineFootSub, lineRansac, GrayS32
 *      derivatives, Planar / interleaved images; the candidates list of HoughTransformGradient (the block extractor ignores it). */
/* GradientPrewitt.process (I:alg/filter/derivative/GradientPrewitt.java:80-142): GradientPrewitt_Shared.process inside
 * (impl/GradientPrewitt_Shared.java:34-67 GrayU8 -> GrayS16, :104-137 GrayF32), ConvolveJustBorder_General_SB.convolve with
 * kernelDerivX/Y on the frame.  border: 0 = null (frame untouched), 1 = ImageBorderValue(0), 2 = BorderType.EXTENDED (the default of
 * FactoryDerivative.prewitt).  dx and dy share their start and strides. */
int bhip_prewitt_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, float* dx, float* dy, int outStart, int outStride,
					 int border);
int bhip_prewitt_u8_s16(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int16_t* dx, int16_t* dy, int outStart,
						int outStride, int border);
int bhip_prewitt_dev_f32(bhip_ctx* ctx, const float* dev_in, long long inImageStride, int inStride, int width, int height, int batch, float* dev_dx, float* dev_dy,
						 long long outImageStride, int outStride, int border);
int bhip_prewitt_dev_u8_s16(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int16_t* dev_dx,
							int16_t* dev_dy, long long outImageStride, int outStride, int border);
/* GradientToEdgeFeatures.intensityAbs(GrayS16, GrayS16, GrayF32) (F:alg/feature/detect/edge/impl/ImplGradientToEdgeFeatures.java:151-169):
 * |dx| + |dy| in int, stored as float (the GrayF32 form is bhip_gradient_intensity_dev_f32 with kind 1) */
int bhip_gradient_intensity_abs_dev_s16(bhip_ctx* ctx, const int16_t* dev_dx, const int16_t* dev_dy, long long dImageStride, int dStride, int width, int height,
										int batch, float* dev_out, long long outImageStride, int outStride);
/* GradientToEdgeFeatures.nonMaxSuppressionCrude4 (F:alg/feature/detect/edge/GradientToEdgeFeatures.java:143-157, 248-262 ->
 * impl/ImplEdgeNonMaxSuppressionCrude.java inner4 :50-115, border4 :155-242): the step is (+1 where the derivative is > 0, else -1) in x and
 * y; out = 0 where the intensity one step back or one step forward is greater, else the intensity; outside the image the intensity is 0.
 * BHIP_ERR_INVALID when intensity and out overlap. */
int bhip_edge_nonmax_crude4_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long iImageStride, int iStride, const float* dev_dx, const float* dev_dy,
									long long dImageStride, int dStride, int width, int height, int batch, float* dev_out, long long outImageStride, int outStride);
int bhip_edge_nonmax_crude4_dev_s16(bhip_ctx* ctx, const float* dev_intensity, long long iImageStride, int iStride, const int16_t* dev_dx, const int16_t* dev_dy,
									long long dImageStride, int dStride, int width, int height, int batch, float* dev_out, long long outImageStride, int outStride);
/* HoughParametersPolar.initialize (F:alg/feature/detect/line/HoughParametersPolar.java:54-60): *rMax = (float)Math.sqrt(originX^2 + originY^2)
 * with Java's int products, *numBinsRange = (int)Math.ceil(rMax / rangeResolution).  The transform is numBinsRange wide, numBinsAngle high.
 * Either output may be NULL.  BHIP_ERR_INVALID: width or height <= 0. */
int bhip_hough_polar_bins(int width, int height, double rangeResolution, int* numBinsRange, float* rMax);
/* HoughTransformBinary.computeParameters (F:alg/feature/detect/line/HoughTransformBinary.java:124-135) with HoughParametersPolar.parameterize
 * (HoughParametersPolar.java:97-114) after the fill with 0: every pixel != 0 adds 1 to one cell in each of the numBinsAngle rows, at
 * col = (int)Math.floor(p * w2 / r_max) + w2 with p = x*c[i] + y*s[i] summed in float and widened, the rest in double.  cosTable / sinTable
 * are the numBinsAngle floats of CachedSineCosine_F32(0, (float)Math.PI, numBinsAngle) (georegression; host arrays, the caller builds them).
 * The Java linear index i*stride + col is kept: col == numBinsRange lands in the next row's first cell.  Deviation: an index outside the
 * transform is dropped where Java throws ArrayIndexOutOfBoundsException.  Counted in int32 and converted, which equals Java's float++.
 * BHIP_ERR_UNSUPPORTED: width * height > 2^24 (float++ stops counting there), numBinsAngle > 65535, numBinsAngle * numBinsRange > 2^28.
 * BHIP_ERR_INVALID: numBinsAngle <= 0, numBinsRange <= 0 (bhip_hough_polar_bins), a transform view of another size. */
int bhip_hough_binary_polar_dev_u8(bhip_ctx* ctx, const uint8_t* dev_binary, long long imageStride, int stride, int width, int height, int batch,
								   double rangeResolution, int numBinsAngle, const float* cosTable, const float* sinTable, float* dev_transform,
								   long long tImageStride, int tStride, int tWidth, int tHeight);
int bhip_hough_binary_polar_u8(bhip_ctx* ctx, const uint8_t* binary, int start, int stride, int width, int height, double rangeResolution, int numBinsAngle,
							   const float* cosTable, const float* sinTable, float* transform, int tStart, int tStride, int tWidth, int tHeight);
/* HoughTransformGradient.transform(derivX, derivY, binary) up to the transform image (F:alg/feature/detect/line/HoughTransformGradient.java:
 * 114-123, transform :238-252, parameterize :184-202, addParameters :204-213) with HoughParametersFootOfNorm.parameterize
 * (HoughParametersFootOfNorm.java:76-85), on GrayF32 or GrayS16 derivatives of any source (Prewitt, Sobel, ...).  The transform has the
 * image's size.  Java's float-to-int rules are kept (NaN -> 0, saturation, x0+1 wrapping, truncation toward zero, so a parameter in (-1, 0)
 * gives x0 = 0 and a negative weight).  A cell is the float sum of its contributions in the order Java adds them -- edge pixels in raster
 * order, within a pixel (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1) -- started from 0; no float atomics (records, a stable sort by cell, one
 * lane per cell).  cap: the edge pixels per image that vote, in raster order (width * height: always all of them); dev_n[b] is image b's
 * number of edge pixels and may exceed cap.  Scratch: 64 bytes per possible vote plus the sort's, for at most 1 GiB of images at a time.
 * BHIP_ERR_UNSUPPORTED: width * height beyond 2^31 - 2.  BHIP_ERR_INVALID: cap < 0, a null count. */
int bhip_hough_gradient_foot_dev_f32(bhip_ctx* ctx, const float* dev_dx, const float* dev_dy, long long dImageStride, int dStride, const uint8_t* dev_binary,
									 long long bImageStride, int bStride, int width, int height, int batch, float* dev_transform, long long tImageStride,
									 int tStride, int cap, int* dev_n);
int bhip_hough_gradient_foot_dev_s16(bhip_ctx* ctx, const int16_t* dev_dx, const int16_t* dev_dy, long long dImageStride, int dStride, const uint8_t* dev_binary,
									 long long bImageStride, int bStride, int width, int height, int batch, float* dev_transform, long long tImageStride,
									 int tStride, int cap, int* dev_n);
/* NonMaxBlock.process with NonMaxBlockSearchRelaxed.Max (F:alg/feature/detect/extract/NonMaxBlock.java:69-94, NonMaxBlockSearchRelaxed.java:69-98,
 * checkLocalMax :227-251), the extractor FactoryFeatureExtractor.nonmax builds for ConfigExtract(radius, threshold, border, false).  Its quirks
 * are kept: a pixel equal to the threshold is a peak, all equal maxima of a block are tested in raster order within the block, checkLocalMax
 * rejects only on > over the clipped window, nothing is reported when the peak value is Float.MAX_VALUE.  Output as bhip_nonmax_block_dev_f32:
 * (x,y) int16 pairs in block-raster order, image b's at dev_xy[b*cap ...], their number in dev_n[b] (it may exceed cap; only the first cap
 * pairs are written).  BHIP_ERR_UNSUPPORTED: an image side of 32768 or more. */
int bhip_nonmax_block_relaxed_dev_f32(bhip_ctx* ctx, const float* dev_intensity, long long imageStride, int stride, int width, int height, int batch, int radius,
									  float threshold, int border, int16_t* dev_xy, int cap, int* dev_n);
int bhip_nonmax_block_relaxed_f32(bhip_ctx* ctx, const float* intensity, int start, int stride, int width, int height, int radius, float threshold, int border,
								  int16_t* xy, int cap, int* n);
/* MeanShiftPeak.search(x, y) (F:alg/feature/detect/peak/MeanShiftPeak.java:103-160) from the first min(dev_n[b], cap) integer peaks
 * dev_xy[b*cap ...] of every image, as HoughTransformGradient.extractLines runs it (:151): bilinear GrayF32 interpolation with the ZERO border
 * (I:alg/interpolate/impl/ImplBilinearPixel_F32.java:48-90), the isInFastBounds choice per iteration, the three sums as sequential float chains
 * in the reference's order, one lane per peak.  weights: the (2*radius+1)^2 floats of the WeightPixel_F32 kernel, row-major (host array;
 * WeightPixelGaussian_F32 for the detector).  radius <= 0: no refinement (weights may be NULL).  dev_peak[(b*cap+i)*2 ...] = (peakX, peakY),
 * dev_intensity[b*cap+i] = the image at the integer peak (0 for a peak outside the image).  dev_n == NULL: cap peaks in every image. */
int bhip_mean_shift_peak_dev_f32(bhip_ctx* ctx, const float* dev_image, long long imageStride, int stride, int width, int height, int batch, const int16_t* dev_xy,
								 const int* dev_n, int cap, int radius, int maxIterations, float convergenceTol, const float* weights, float* dev_peak,
								 float* dev_intensity);

/* ---- image enhancement: EnhanceImageOps (I:alg/enhance/EnhanceImageOps.java) and the histogram it starts from, on GrayU8 (sharpen also on
 *      GrayF32) images (enhance.hip; the histogram kernel is threshold.hip's).  There is no BOverride hook for EnhanceImageOps in the reference:
 *      integration/java/boofcv/hip/EnhanceImageOpsHip.java is a provider class with the same static signatures.
 * The _dev forms take batch images at dev_x + b*xImageStride (strides in elements, any alignment), write the whole width x height view of every
 * output image and nothing outside it, are asynchronous on the context's stream without host synchronisation and need no scratch.  The forms
 * without _dev take one host image view each: staged, run through the same implementation, synchronised.  All of the GrayU8 arithmetic is
 * integer, and the GrayF32 sharpen keeps Java's evaluation order without fused multiply-add: results equal the single-threaded Java results
 * bit for bit.
 * Not provided: the GrayU16 / GrayS8 / GrayS16 / GrayS32 forms of applyTransform and equalizeLocal.
 * BHIP_ERR_INVALID and nothing is written: empty images, strides smaller than a row, a length or histogramLength outside 1 .. 256, a minValue
 * outside 0 .. 255, a negative radius, an unknown path or rule, overlapping input and output of equalizeLocal or sharpen.
 * BHIP_ERR_UNSUPPORTED: more than 65535 images in a batch, an equalizeLocal radius beyond 255, a forced path that cannot run the call. */
/* ImageStatistics.histogram(GrayU8 input, int minValue, int[] histogram) (I:alg/misc/ImageStatistics.java:299-306,
 * impl/ImplImageStatistics.java:206-221) with histogram.length = length <= 256: image b's counts go to dev_histogram[b*length ...], which is
 * cleared first as Arrays.fill does.  Deviation: a pixel outside [minValue, minValue + length) is dropped (the reference throws
 * ArrayIndexOutOfBoundsException). */
int bhip_histogram_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int minValue, int length,
						  int* dev_histogram);
int bhip_histogram_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int minValue, int length, int* histogram);
/* EnhanceImageOps.equalize(histogram, transform) (:65-77) on `batch` histograms of `length` <= 256 ints in device memory:
 * transform[i] = ((histogram[0] + .. + histogram[i]) * (length - 1)) / sum in Java's int arithmetic.  dev_transform may be dev_histogram.
 * Deviation: a histogram whose sum is 0 gives a table of zeros (the reference throws ArithmeticException). */
int bhip_equalize_table_dev(bhip_ctx* ctx, const int* dev_histogram, int length, int batch, int* dev_transform);
/* EnhanceImageOps.applyTransform(GrayU8, int[] transform, GrayU8) (:86-94, impl/ImplEnhanceHistogram.java:42-53): out = (byte)transform[in].
 * Image b reads the `length` ints at dev_transform + b*transformStride (transformStride 0: one table for the batch, `length`: the layout
 * bhip_equalize_table_dev writes).  dev_out may be dev_in (the same view).  Deviation: a pixel >= length gives 0 (the reference throws). */
int bhip_apply_transform_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch,
								const int* dev_transform, long long transformStride, int length, uint8_t* dev_out, long long outImageStride, int outStride);
int bhip_apply_transform_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, const int* transform, int length, uint8_t* out,
							int outStart, int outStride);
/* EnhanceImageOps.equalizeLocal(GrayU8 input, radius, GrayU8 output, histogramLength, workArrays) (:176-232).  The reference's three branches --
 * equalizeLocalInner + two equalizeLocalRow + two equalizeLocalCol (impl/ImplEnhanceHistogram.java:175-401) when both sides are >= 2*radius+1,
 * the whole-image histogram when both are smaller, equalizeLocalNaive (:111-170) otherwise -- are one rule: with w = 2*radius+1,
 * x0 = max(0, min(x - radius, width - w)), x1 = min(width, x0 + w) and the same in y,
 * out(x,y) = (byte)((number of pixels in [x0,x1) x [y0,y1) with a value <= in(x,y)) * (histogramLength - 1) / ((x1-x0) * (y1-y0))).
 * path: BHIP_EQLOCAL_DIRECT counts the window out of an LDS tile (it needs (64 + 2*radius) x (16 + 2*radius) bytes, each clipped to the image
 * side, within 64 KiB), BHIP_EQLOCAL_SLIDING slides a 256-bin histogram along runs of a row (any radius, at most 65535 rows), BHIP_EQLOCAL_AUTO
 * picks by radius; the three give the same image.  0 <= radius <= 255, 1 <= histogramLength <= 256; input and output must not overlap.
 * Deviation: a pixel >= histogramLength is ranked like any other (the reference throws ArrayIndexOutOfBoundsException). */
#define BHIP_EQLOCAL_AUTO 0
#define BHIP_EQLOCAL_DIRECT 1
#define BHIP_EQLOCAL_SLIDING 2
int bhip_equalize_local_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int radius,
							   int histogramLength, int path, uint8_t* dev_out, long long outImageStride, int outStride);
int bhip_equalize_local_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int radius, int histogramLength, int path,
						   uint8_t* out, int outStart, int outStride);
/* EnhanceImageOps.sharpen4 / sharpen8 (:307-371; rule 4 or 8): impl/ImplEnhanceFilter.java sharpenInner4 / 8 (:43-64, :120-141, :197-226,
 * :321-350) for 1 <= x < width-1, 1 <= y < height-1 -- 5*c - (((l + r) + u) + d), 9*c - (the eight neighbours in raster order) -- then
 * sharpenBorder4 / 8 (:66-118, :143-195, :228-319, :352-443) through the clamping safeGet (:448-475) in its loop order (every x: top, bottom;
 * every y in 1 .. height-2: left, right -- the last write stands, which is what sides of 1 and 2 and the corners come out of), clamped to
 * [0, 255] as `if (a > 255) a = 255; else if (a < 0) a = 0`.  GrayF32 keeps the order of the additions and uses no fused multiply-add.
 * Input and output must not overlap. */
int bhip_sharpen_dev_u8(bhip_ctx* ctx, int rule, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, uint8_t* dev_out,
						long long outImageStride, int outStride);
int bhip_sharpen_dev_f32(bhip_ctx* ctx, int rule, const float* dev_in, long long inImageStride, int inStride, int width, int height, int batch, float* dev_out,
						 long long outImageStride, int outStride);
int bhip_sharpen_u8(bhip_ctx* ctx, int rule, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart, int outStride);
int bhip_sharpen_f32(bhip_ctx* ctx, int rule, const float* in, int inStart, int inStride, int width, int height, float* out, int outStart, int outStride);

/* ---- SIFT detector: scale space and DoG extrema.  FactoryInterestPoint.sift (F:factory/feature/detect/interest/FactoryInterestPoint.java:133-148):
 *      WrapSiftDetector (F:abst/feature/detect/interest/WrapSiftDetector.java:38-60) over SiftDetector (F:alg/feature/detect/interest/SiftDetector.java:
 *      119-331), SiftScaleSpace (F:alg/feature/detect/interest/SiftScaleSpace.java:102-270) and NonMaxLimiter
 *      (F:abst/feature/detect/extract/NonMaxLimiter.java:49-84) with FactoryFeatureExtractor.nonmax(ConfigExtract).  Orientation and description
 *      (OrientationHistogramSift, DescribePointSift, CompleteSift): the bhip_csift_* section below. ----
 * Every scale image, DoG image and detection equals the single-threaded Java result bit for bit: the border-normalised separable Gaussian
 * convolutions (the arithmetic of bhip_conv_norm_h / _v, naive form included), a float subtraction, the strict block min / max non-maximum
 * suppression with ignoreBorder 1, the 3x3x3 comparison, the edge test in double on three sparse float convolutions with an EXTENDED border, and
 * polyPeak.  levelK, computeSigmaScale and pixelScaleCurrentToInput are the host's pow: unpinned against Java's Math.pow.  With
 * maxFeaturesPerScale > 0 the list of a scale that is longer is cut by the project's restatement of QuickSelect.select on keys -|value|: the
 * order it leaves is unpinned against the ddogleg jar, the kept set is pinned whenever no two |value| around the cut are equal.
 * A scale level (octave[i] = blur(octave[i-1]), dog[i-1] = octave[i] - octave[i-1]) runs as one launch on BHIP_SIFT_LEVEL_TILE_WIDTH x
 * BHIP_SIFT_LEVEL_TILE_HEIGHT tiles for odd kernels of 3 .. BHIP_SIFT_LEVEL_MAX_TAPS taps narrower than the image both ways over 16-byte aligned
 * rows, and as the two normalised passes plus a subtract otherwise; BHIP_SIFT_TWO_PASS=1 in the environment forces the latter (same results).
 * BHIP_ERR_INVALID and nothing is written, where the reference throws: lastOctave <= firstOctave, numScales < 1, edgeR < 1 (detect), an
 * extractor with extractIgnoreBorder != 1, without minima or maxima, or with extractRadius < 1 (detect), sigma0 <= 0, empty images (an octave
 * of no pixels included), strides smaller than a row, cap < 0.
 * BHIP_ERR_UNSUPPORTED and nothing is written: an octave image wider or taller than 32767 (the lists are Point2D_I16), a blur kernel beyond 255
 * taps, more than 65535 frames, extractUseStrictRule == 0 (the relaxed rule). */
#define BHIP_SIFT_LEVEL_TILE_WIDTH 64
#define BHIP_SIFT_LEVEL_TILE_HEIGHT 64
#define BHIP_SIFT_LEVEL_MAX_TAPS 27
/* (a struct tag and a typedef of it: the form boofcv_amd/_header.py reads as Header.declared) */
struct bhip_sift_cfg {
	int firstOctave;          /* ConfigSiftScaleSpace: 0 */
	int lastOctave;           /* 5 */
	int numScales;            /* 3 */
	double sigma0;            /* (double)2.75f; SiftScaleSpace takes a double */
	int extractRadius;        /* ConfigSiftDetector.extract = ConfigExtract(2, 0, 1, true, true, true): radius 2 */
	float extractThreshold;   /* 0 (thresholdMax = threshold, thresholdMin = -threshold) */
	int extractIgnoreBorder;  /* 1 */
	int extractUseStrictRule; /* 1 */
	int extractDetectMin;     /* 1 */
	int extractDetectMax;     /* 1 */
	int maxFeaturesPerScale;  /* 0: no limit */
	double edgeR;             /* 10 */
};
typedef struct bhip_sift_cfg bhip_sift_cfg;
/* new ConfigSiftScaleSpace() (F:abst/feature/describe/ConfigSiftScaleSpace.java) and new ConfigSiftDetector()
 * (F:abst/feature/detect/interest/ConfigSiftDetector.java) */
int bhip_sift_cfg_default(bhip_sift_cfg* cfg);
/* Host only: the octaves SiftScaleSpace.initialize / computeNextOctave (:170-212) compute for a width x height frame.  Returns their number (>= 1)
 * or a BHIP_ERR_* code; dims receives (width, height) of the first min(number, cap) octaves, octave firstOctave first.  A frame's scale images
 * take *scaleFloats floats: octave after octave, numScales+3 dense images of plane = (w*h + 3) & ~3 floats each; its DoG images *dogFloats
 * floats in the same way with numScales+2 images per octave.  dims, scaleFloats and dogFloats may be NULL. */
int bhip_sift_layout(const bhip_sift_cfg* cfg, int width, int height, int* dims, int cap, long long* scaleFloats, long long* dogFloats);
/* The scale space of `batch` device frames at dev_in + b*imageStride (rows `stride` elements apart, any alignment): frame b's images go to
 * dev_scale + b * scaleFloats and dev_dog + b * dogFloats in the layout of bhip_sift_layout (the padding floats of a plane are not written).  The
 * _u8 form converts as GConvertImage.convert does (& 0xFF to float) on the device.  Asynchronous on the context's stream, no host synchronisation. */
int bhip_sift_scale_space_dev_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const float* dev_in, long long imageStride, int stride, int width, int height,
								  int batch, float* dev_scale, float* dev_dog);
int bhip_sift_scale_space_dev_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const uint8_t* dev_in, long long imageStride, int stride, int width, int height,
								 int batch, float* dev_scale, float* dev_dog);
/* SiftDetector.process on every frame, one octave at a time in context scratch.  Frame b's detections, in the reference's order, go to
 * dev_x / dev_y / dev_scale + b*cap (ScalePoint x, y, scale), dev_white + b*cap (ScalePoint.white as 0 / 1) and dev_where + b*cap*4 (octave, the
 * DoG index j, and the pixel (x, y) in that octave where the extremum was found); dev_count[b] is their number, which may exceed cap: only the
 * first cap records are written.  No host synchronisation between the first launch and the last. */
int bhip_sift_detect_dev_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const float* dev_in, long long imageStride, int stride, int width, int height, int batch,
							 double* dev_x, double* dev_y, double* dev_scale, uint8_t* dev_white, int16_t* dev_where, int* dev_count, int cap);
int bhip_sift_detect_dev_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const uint8_t* dev_in, long long imageStride, int stride, int width, int height, int batch,
							double* dev_x, double* dev_y, double* dev_scale, uint8_t* dev_white, int16_t* dev_where, int* dev_count, int cap);
/* the same on one host image view: staged, run through the _dev forms, synchronised.  scale / dog: scaleFloats / dogFloats floats (written as a
 * whole, the padding floats of a plane as 0); x, y, scale, white: cap elements, where: 4 * cap; *count as dev_count. */
int bhip_sift_scale_space_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const float* in, int start, int stride, int width, int height, float* scale, float* dog);
int bhip_sift_scale_space_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const uint8_t* in, int start, int stride, int width, int height, float* scale, float* dog);
int bhip_sift_detect_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const float* in, int start, int stride, int width, int height, double* x, double* y,
						 double* scale, uint8_t* white, int16_t* where, int* count, int cap);
int bhip_sift_detect_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const uint8_t* in, int start, int stride, int width, int height, double* x, double* y,
						double* scale, uint8_t* white, int16_t* where, int* count, int cap);

/* ---- SIFT detect + describe: FactoryDetectDescribe.sift(ConfigCompleteSift) (F:factory/feature/detdesc/FactoryDetectDescribe.java:72-96):
 *      DetectDescribe_CompleteSift (F:abst/feature/detdesc/DetectDescribe_CompleteSift.java) over CompleteSift
 *      (F:alg/feature/detdesc/CompleteSift.java:89-134), OrientationHistogramSift (F:alg/feature/orientation/OrientationHistogramSift.java:135-309)
 *      and DescribePointSift / DescribeSiftCommon (F:alg/feature/describe/DescribePointSift.java:105-165, DescribeSiftCommon.java:60-131). ----
 * The detector is the one above (bhip_sift_cfg, bit for bit).  For every detection of (octave, j), on scale image j of the octave with
 * GradientThree's EXTENDED-border gradient: the orientation histograms (every bin the reference's ordered double sum), the peaks, the angles,
 * and one feature per angle: the 128-element (widthGrid^2 * numHistogramBins) descriptor, normalised twice.  Discrete results -- the number of
 * angles of every detection, hence the count and order of features; x, y, scale, white -- equal the single-threaded Java result exactly.
 * Angles and descriptor elements differ from it by the last ulp of atan2 / sin / cos alone (Java's, the host's and the device library's are
 * three implementations): where an argument of atan2 is zero the results the Java specification fixes are selected explicitly, so samples
 * on a bin edge are binned as in Java.  Host decisions, unpinned against Java's Math.exp / Math.sqrt: the exp table of the orientation
 * weight and the Gaussian weight of the descriptor (bhip_csift_weights returns both).  UtilAngle.domain2PI / dist / bound are georegression's,
 * restated from their contract.
 * BHIP_ERR_INVALID and nothing is written, beyond the detector's: histogramSize < 3, sigmaEnlarge, sigmaToPixels, weightingSigmaFraction or
 * maxDescriptorElementValue not > 0, widthSubregion, widthGrid or numHistogramBins < 1, widthSubregion * widthGrid odd (the reference indexes
 * its weight kernel out of range), cap < 0.
 * BHIP_ERR_UNSUPPORTED and nothing is written, beyond the detector's: histogramSize > BHIP_CSIFT_MAX_HISTOGRAM, widthSubregion * widthGrid >
 * BHIP_CSIFT_MAX_SAMPLE_WIDTH, a descriptor of more than BHIP_CSIFT_MAX_DOF elements (the kernels' LDS).  The orientation window has no limit:
 * r = ceil(sigma * sigmaEnlarge) is walked in chunks whatever its size.
 * BHIP_SIFT_DESCRIBE_GENERIC=1 in the environment runs the default grid (4, 4, 8) through the describe kernel that takes any grid (same results). */
#define BHIP_CSIFT_EXP_TABLE 160
#define BHIP_CSIFT_ANGLE_SLOTS 3
#define BHIP_CSIFT_MAX_HISTOGRAM 256
#define BHIP_CSIFT_MAX_SAMPLE_WIDTH 48
#define BHIP_CSIFT_MAX_DOF 2048
/* (the typedef, then the struct: the form boofcv_amd/_header.py reads as Header.forward) */
typedef struct bhip_csift_cfg bhip_csift_cfg;
struct bhip_csift_cfg {
	int histogramSize;                /* ConfigSiftOrientation: 36 */
	double sigmaEnlarge;              /* 2.0 (createPaper: 1.5) */
	int widthSubregion;               /* ConfigSiftDescribe: 4 */
	int widthGrid;                    /* 4 */
	int numHistogramBins;             /* 8 */
	double sigmaToPixels;             /* 1.0 */
	double weightingSigmaFraction;    /* 0.5 */
	double maxDescriptorElementValue; /* 0.2 */
};
/* new ConfigSiftOrientation() (F:abst/feature/orientation/ConfigSiftOrientation.java) and new ConfigSiftDescribe()
 * (F:abst/feature/describe/ConfigSiftDescribe.java) */
int bhip_csift_cfg_default(bhip_csift_cfg* desc);
/* Host only: DescribeSiftCommon.getDescriptorLength, or a BHIP_ERR_* code for a config the calls below refuse. */
int bhip_csift_dof(const bhip_csift_cfg* desc);
/* Host only: the tables the kernels are given.  expTable: BHIP_CSIFT_EXP_TABLE doubles, exp(-0.5 * i * 0.1); gaussianWeight:
 * (widthSubregion * widthGrid)^2 floats, DescribeSiftCommon.gaussianWeight.  Either may be NULL. */
int bhip_csift_weights(const bhip_csift_cfg* desc, double* expTable, float* gaussianWeight);
/* CompleteSift.process on every frame, one octave at a time in context scratch.  Frame b's features, in the reference's order (detection
 * order, then the order of the angle list), go to dev_x / dev_y / dev_scale / dev_orientation + b*cap (the ScalePoint and the angle),
 * dev_white + b*cap and dev_desc + b*cap*dof (dof doubles per feature: the layout bhip_assoc_l2_dev and bhip_assoc_l2_dev_batched read);
 * dev_count[b] is their number, exact also where it exceeds cap: only the first cap records are written.  No host synchronisation between
 * the first launch and the last. */
int bhip_csift_dev_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const bhip_csift_cfg* desc, const float* dev_in, long long imageStride, int stride, int width,
					   int height, int batch, double* dev_x, double* dev_y, double* dev_scale, double* dev_orientation, uint8_t* dev_white, double* dev_desc,
					   int* dev_count, int cap);
int bhip_csift_dev_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const bhip_csift_cfg* desc, const uint8_t* dev_in, long long imageStride, int stride, int width,
					  int height, int batch, double* dev_x, double* dev_y, double* dev_scale, double* dev_orientation, uint8_t* dev_white, double* dev_desc,
					  int* dev_count, int cap);
/* the same on one host image view: staged, run through the _dev forms, synchronised.  x, y, scale, orientation, white: cap elements; descriptors:
 * cap * dof doubles; *count as dev_count. */
int bhip_csift_f32(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const bhip_csift_cfg* desc, const float* in, int start, int stride, int width, int height, double* x,
				   double* y, double* scale, double* orientation, uint8_t* white, double* descriptors, int* count, int cap);
int bhip_csift_u8(bhip_ctx* ctx, const bhip_sift_cfg* cfg, const bhip_csift_cfg* desc, const uint8_t* in, int start, int stride, int width, int height, double* x,
				  double* y, double* scale, double* orientation, uint8_t* white, double* descriptors, int* count, int cap);

/* ---- Dense descriptors: FactoryDescribeImageDense.hog(ConfigDenseHoG, imageType), both variants, and FactoryDescribeImageDense.sift(ConfigDenseSift,
 *      imageType) (F:factory/feature/dense/FactoryDescribeImageDense.java:108-165) on single-band GrayF32 / GrayU8 frames: DescribeDenseHogFastAlg
 *      (F:alg/feature/dense/DescribeDenseHogFastAlg.java:80-215), DescribeDenseHogAlg (F:alg/feature/dense/DescribeDenseHogAlg.java:121-339) and
 *      DescribeDenseSiftAlg (F:alg/feature/dense/DescribeDenseSiftAlg.java:120-198) with DescribeSiftCommon.  The configuration values are plain
 *      arguments: ConfigDenseHoG (9, 8, 3, 3, 1, fastVariant = 1) and ConfigSiftDescribe (4, 4, 8, 0.5, 0.2; sigmaToPixels is not used) with
 *      DenseSampling (6, 6). ----
 * The gradient is GradientThree with the EXTENDED border.  HOG on GrayU8 converts to GrayF32 first (DescribeImageDense_Convert, exact);
 * dense SIFT on GrayU8 takes the GrayS16 gradient, which in this reference is b - a with no divisor (kernel -1 0 1), read through getF.
 * Counts, locations and their order equal the single-threaded Java result exactly.  HOG: every operation between the pixels and the
 * descriptor is IEEE-specified except the one Math.atan of a pixel, whose double result is narrowed to float at once: the fast variant's float
 * cell histograms and the descriptors of both variants equal Java's bit for bit wherever the host's / device's / Java's atan narrow to the same
 * float.  Dense SIFT: Math.atan2 stays a double (where an argument is zero the results the Java specification fixes are selected), so descriptor
 * elements differ from Java's by its last ulp.  Every ordered sum -- a cell's bin in pixel raster order; a standard-HOG element over the cells of
 * the block in row-major order, their pixels in raster order and a pixel's adds as written (a contribution with a zero spatial weight adds +0.0
 * and is skipped); a SIFT element over the window's samples in raster order; both L2 sums in index order -- is taken in that order by one lane.
 * UtilAngle.atanSafe / domain2PI / dist (georegression) and UtilGaussian.computePDF (ddogleg) are restated from their contract, unpinned.
 * Locations: HOG, the block's top-left pixel (BaseDenseHog.getLocations; DescribeImageDenseHoG.process adds half the region afterwards); dense
 * SIFT, the window's centre.
 * BHIP_ERR_INVALID and nothing is written, where the reference throws or divides by zero: stepBlock <= 0; orientationBins, pixelsPerCell,
 * cellsPerBlockX / Y, widthSubregion, widthGrid, numHistogramBins < 1; periods, weightingSigmaFraction, maxDescriptorElementValue not > 0;
 * widthSubregion * widthGrid odd (the reference indexes its weight kernel out of range); empty images, strides smaller than a row, cap < 0, a
 * cell-histogram output with the standard variant; dense SIFT with one row of descriptors (numY == 1), or with one column (numX == 1) and at
 * least one row: the reference divides by numX - 1 in int arithmetic.
 * BHIP_ERR_UNSUPPORTED and nothing is written: a descriptor of more than BHIP_DENSE_MAX_DOF elements, more than BHIP_DENSE_MAX_BINS orientation /
 * histogram bins, pixelsPerCell > BHIP_DENSE_MAX_CELL, a dense-SIFT window wider than BHIP_DENSE_MAX_SAMPLE_WIDTH samples, more than 65535 frames, more
 * than 65535 image rows, a grid whose count or whose (X1 - X0) * (numX - 1) is beyond int.
 * An image too small for one block or window gives count 0.
 * BHIP_DENSE_SIFT_GENERIC=1 in the environment runs the default grid (4, 4, 8) through the kernel that takes any grid (same results). */
#define BHIP_DENSE_MAX_DOF 2048
#define BHIP_DENSE_MAX_BINS 64
#define BHIP_DENSE_MAX_CELL 32
#define BHIP_DENSE_MAX_SAMPLE_WIDTH 48
/* Host only: the grid of a width x height frame.  Returns the number of descriptors (>= 0) or a BHIP_ERR_* code; *perRow descriptors in a row of
 * the grid, *perCol rows, *dof elements per descriptor, and xy receives (x, y) of the first min(number, cap) descriptors in row-major order.  Any
 * of the pointers may be NULL. */
int bhip_dense_hog_layout(int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant, int width, int height,
						  int* perRow, int* perCol, int* dof, int32_t* xy, int cap);
int bhip_dense_sift_layout(int widthSubregion, int widthGrid, int numHistogramBins, double periodX, double periodY, int width, int height, int* perRow, int* perCol,
						   int* dof, int32_t* xy, int cap);
/* Host only: DescribeDenseHogAlg.computeWeightBlockPixels, (cellsPerBlockY * pixelsPerCell) rows of (cellsPerBlockX * pixelsPerCell) doubles.  Returns
 * their number or a BHIP_ERR_* code; weights may be NULL. */
int bhip_dense_hog_weights(int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, double* weights);
/* Every frame of a device batch at dev_in + b*imageStride (rows `stride` elements apart, any alignment).  Frame b's descriptors, in the
 * reference's row-major order, go to dev_desc + b*cap*dof (dof doubles each: the layout bhip_assoc_l2_dev and bhip_assoc_l2_dev_batched read) and
 * their locations to dev_xy + b*cap*2; dev_count[b] is their number, which may exceed cap: only the first cap records are written.  dev_cells,
 * fast variant only and optional (NULL): the cell histograms, [batch][height / pixelsPerCell][width / pixelsPerCell][orientationBins] floats.
 * The per-pixel values and cell histograms live in context scratch; a batch whose scratch would exceed 256 MiB runs as several groups of frames.
 * Asynchronous on the context's stream, no host synchronisation (the weight tables are uploaded, with one, when the configuration changes). */
int bhip_dense_hog_dev_f32(bhip_ctx* ctx, int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant,
						   const float* dev_in, long long imageStride, int stride, int width, int height, int batch, double* dev_desc, int32_t* dev_xy, int* dev_count,
						   int cap, float* dev_cells);
int bhip_dense_hog_dev_u8(bhip_ctx* ctx, int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant,
						  const uint8_t* dev_in, long long imageStride, int stride, int width, int height, int batch, double* dev_desc, int32_t* dev_xy, int* dev_count,
						  int cap, float* dev_cells);
int bhip_dense_sift_dev_f32(bhip_ctx* ctx, int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue,
							double periodX, double periodY, const float* dev_in, long long imageStride, int stride, int width, int height, int batch, double* dev_desc,
							int32_t* dev_xy, int* dev_count, int cap);
int bhip_dense_sift_dev_u8(bhip_ctx* ctx, int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue,
						   double periodX, double periodY, const uint8_t* dev_in, long long imageStride, int stride, int width, int height, int batch, double* dev_desc,
						   int32_t* dev_xy, int* dev_count, int cap);
/* the same on one host image view: staged, run through the _dev forms, synchronised.  descriptors: cap * dof doubles; xy: cap * 2; *count as
 * dev_count; cells (fast variant, may be NULL): (height / pixelsPerCell) * (width / pixelsPerCell) * orientationBins floats. */
int bhip_dense_hog_f32(bhip_ctx* ctx, int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant, const float* in,
					   int start, int stride, int width, int height, double* descriptors, int32_t* xy, int* count, int cap, float* cells);
int bhip_dense_hog_u8(bhip_ctx* ctx, int orientationBins, int pixelsPerCell, int cellsPerBlockX, int cellsPerBlockY, int stepBlock, int fastVariant, const uint8_t* in,
					  int start, int stride, int width, int height, double* descriptors, int32_t* xy, int* count, int cap, float* cells);
int bhip_dense_sift_f32(bhip_ctx* ctx, int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue,
						double periodX, double periodY, const float* in, int start, int stride, int width, int height, double* descriptors, int32_t* xy, int* count,
						int cap);
int bhip_dense_sift_u8(bhip_ctx* ctx, int widthSubregion, int widthGrid, int numHistogramBins, double weightingSigmaFraction, double maxDescriptorElementValue,
					   double periodX, double periodY, const uint8_t* in, int start, int stride, int width, int height, double* descriptors, int32_t* xy, int* count,
					   int cap);

#ifdef __cplusplus
}
#endif
#endif /* BOOFHIP_H */
