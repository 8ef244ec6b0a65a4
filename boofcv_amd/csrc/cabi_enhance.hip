// ---------------------------------------------------------------------------------------------------------------
// EnhanceImageOps on the C boundary: the histogram, the equalize table, applyTransform, equalizeLocal and sharpen4 / sharpen8
// (enhance.hip; the histogram kernel is threshold.hip's).  Every argument check comes before anything touches the device, so a refused
// call writes nothing.  The _dev exports run on the caller's views, asynchronous on the ctx stream; the host exports stage their views and
// run the same implementation with batch 1.
// ---------------------------------------------------------------------------------------------------------------
#include "cabi.h"

// Radius from which BHIP_EQLOCAL_AUTO takes the sliding form; below it the direct one, wherever its tile fits LDS.  Measured on 16 1080p
// frames (scripts/bench_enhance.py -> profiles/bench_enhance.jsonl): the direct form is the faster one at every swept radius up to 64
// (line "equalizeLocal_r64_summary": direct 24.8 ms, sliding 30.5 ms per batch), the sliding one from 80 on (line
// "equalizeLocal_r80_summary": direct 41.8 ms, sliding 37.0 ms).  No radius between 64 and 80 was measured; the direct form grows with
// (2r+1)^2 and the sliding one with r, which puts the tie near 76.
#define BHIP_EQLOCAL_SLIDING_MIN_RADIUS 80

// the bytes two views span, for the overlap test (an image stride may be negative: the first image is then the highest)
template <class T>
static bool overlaps(DevImg<const T> a, DevImg<const T> b) {
	auto span = [](DevImg<const T> v, uintptr_t& lo, uintptr_t& hi) {
		const long long back = v.imageStride < 0 ? (long long)(v.batch - 1) * -v.imageStride : 0;
		const long long fwd = v.imageStride > 0 ? (long long)(v.batch - 1) * v.imageStride : 0;
		lo = (uintptr_t)v.data - (uintptr_t)back * sizeof(T);
		hi = (uintptr_t)v.data + (uintptr_t)(fwd + (long long)(v.height - 1) * v.stride + v.width) * sizeof(T);
	};
	uintptr_t alo, ahi, blo, bhi;
	span(a, alo, ahi);
	span(b, blo, bhi);
	return alo < bhi && blo < ahi;
}

// BHIP_OK, or the refusal of an equalizeLocal call's own arguments (the same for the device and the host form)
static int eqLocalArgs(bhip_ctx* ctx, int radius, int histogramLength, int path, int width, int height) {
	if (radius < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "equalizeLocal: radius must be >= 0");
	if (histogramLength < 1 || histogramLength > 256) return bhip_fail(ctx, BHIP_ERR_INVALID, "equalizeLocal: histogramLength must be in 1 .. 256");
	if (path != BHIP_EQLOCAL_AUTO && path != BHIP_EQLOCAL_DIRECT && path != BHIP_EQLOCAL_SLIDING) return bhip_fail(ctx, BHIP_ERR_INVALID, "equalizeLocal: unknown path");
	if (radius > 255) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "equalizeLocal: radius beyond 255");
	if (height > 65535 * 16) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "equalizeLocal: more than 1048560 rows");
	if (path == BHIP_EQLOCAL_DIRECT && !bhip_equalize_local_direct_fits(radius, width, height))
		return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "equalizeLocal: the direct form's tile does not fit LDS at this radius");
	if (path == BHIP_EQLOCAL_SLIDING && height > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "equalizeLocal: the sliding form takes at most 65535 rows");
	return BHIP_OK;
}
static int eqLocalImpl(bhip_ctx* ctx, int radius, int histogramLength, int path, DevImg<const uint8_t> in, DevImg<uint8_t> out) {
	bool sliding = path == BHIP_EQLOCAL_SLIDING;
	if (path == BHIP_EQLOCAL_AUTO)
		sliding = (radius >= BHIP_EQLOCAL_SLIDING_MIN_RADIUS && in.height <= 65535) || !bhip_equalize_local_direct_fits(radius, in.width, in.height);
	return sliding ? bhip_launch_equalize_local_sliding(ctx, in, out, radius, histogramLength) : bhip_launch_equalize_local_direct(ctx, in, out, radius, histogramLength);
}
static const char* histArgError(int minValue, int length) {
	if (length < 1 || length > 256) return "histogram: length must be in 1 .. 256";
	if (minValue < 0 || minValue > 255) return "histogram: minValue must be in 0 .. 255";
	return nullptr;
}
static const char* ruleArgError(int rule) { return rule == 4 || rule == 8 ? nullptr : "sharpen: rule must be 4 or 8"; }

template <class T>
static int sharpenDev(bhip_ctx* ctx, int rule, DevImg<const T> in, DevImg<T> out) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	if (const char* e = ruleArgError(rule)) return bhip_fail(ctx, BHIP_ERR_INVALID, e);
	if (in.batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	if (in.height > 65535 * 4) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "sharpen: more than 262140 rows");
	if (overlaps<T>(in, out)) return bhip_fail(ctx, BHIP_ERR_INVALID, "input and output of sharpen must not overlap");
	return bhip_launch_sharpen<T>(ctx, rule, in, out);
}
template <class T>
static int sharpenHost(bhip_ctx* ctx, int rule, HostImg<const T> in, HostImg<T> out) {
	const char* e = ruleArgError(rule);
	if (!e && in.height > 65535 * 4) e = "sharpen: more than 262140 rows";
	return hostInOut<T, T>(ctx, in, out, false, false, e, [&](DevImg<T> din, DevImg<T> dout) { return bhip_launch_sharpen<T>(ctx, rule, DevImg<const T>(din), dout); });
}

extern "C" {

int bhip_histogram_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int minValue, int length,
						  int* dev_histogram) {
	const DevImg<const uint8_t> in{dev_in, inImageStride, inStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	if (!dev_histogram) return bhip_fail(ctx, BHIP_ERR_INVALID, "null histogram");
	if (const char* e = histArgError(minValue, length)) return bhip_fail(ctx, BHIP_ERR_INVALID, e);
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	BHIP_HIP(ctx, hipMemsetAsync(dev_histogram, 0, (size_t)batch * length * sizeof(int), ctx->stream));
	return bhip_launch_hist_u8(ctx, in, dev_histogram, minValue, length);
}
int bhip_histogram_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int minValue, int length, int* histogram) {
	const HostImg<const uint8_t> hin{in, inStart, inStride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	if (!histogram) return bhip_fail(ctx, BHIP_ERR_INVALID, "null histogram");
	if (const char* e = histArgError(minValue, length)) return bhip_fail(ctx, BHIP_ERR_INVALID, e);
	CtxScratch* sc = scratchOf(ctx);
	DevImg<uint8_t> din;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	BHIP_TRY(sc->enhance.reserve(ctx, 256 * sizeof(int)));
	int* h = sc->enhance.as<int>();
	BHIP_HIP(ctx, hipMemsetAsync(h, 0, (size_t)length * sizeof(int), ctx->stream));
	BHIP_TRY(bhip_launch_hist_u8(ctx, DevImg<const uint8_t>(din), h, minValue, length));
	BHIP_HIP(ctx, hipMemcpyAsync(histogram, h, (size_t)length * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}
int bhip_equalize_table_dev(bhip_ctx* ctx, const int* dev_histogram, int length, int batch, int* dev_transform) {
	CHECK_CTX(ctx);
	if (!dev_histogram || !dev_transform) return bhip_fail(ctx, BHIP_ERR_INVALID, "null table");
	if (length < 1 || length > 256) return bhip_fail(ctx, BHIP_ERR_INVALID, "equalize: length must be in 1 .. 256");
	if (batch < 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "equalize: batch must be >= 1");
	return bhip_launch_equalize_table(ctx, dev_histogram, length, batch, dev_transform);
}
int bhip_apply_transform_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch,
								const int* dev_transform, long long transformStride, int length, uint8_t* dev_out, long long outImageStride, int outStride) {
	const DevImg<const uint8_t> in{dev_in, inImageStride, inStride, width, height, batch};
	const DevImg<uint8_t> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	if (!dev_transform || length < 1 || length > 256 || transformStride < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "applyTransform: bad table");
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	return bhip_launch_apply_transform(ctx, in, out, dev_transform, transformStride, length);
}
int bhip_apply_transform_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, const int* transform, int length, uint8_t* out,
							int outStart, int outStride) {
	return hostInOut<uint8_t, uint8_t>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, false, false,
									   !transform || length < 1 || length > 256 ? "applyTransform: bad table" : nullptr, [&](DevImg<uint8_t> din, DevImg<uint8_t> dout) {
										   DevBuf& buf = scratchOf(ctx)->enhance;
										   BHIP_TRY(buf.reserve(ctx, 256 * sizeof(int)));
										   BHIP_HIP(ctx, hipMemcpyAsync(buf.p, transform, (size_t)length * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
										   return bhip_launch_apply_transform(ctx, DevImg<const uint8_t>(din), dout, buf.as<int>(), 0, length);
									   });
}

int bhip_equalize_local_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int radius,
							   int histogramLength, int path, uint8_t* dev_out, long long outImageStride, int outStride) {
	const DevImg<const uint8_t> in{dev_in, inImageStride, inStride, width, height, batch};
	const DevImg<uint8_t> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	BHIP_TRY(eqLocalArgs(ctx, radius, histogramLength, path, width, height));
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	if (overlaps<uint8_t>(in, out)) return bhip_fail(ctx, BHIP_ERR_INVALID, "input and output of equalizeLocal must not overlap");
	return eqLocalImpl(ctx, radius, histogramLength, path, in, out);
}
int bhip_equalize_local_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int radius, int histogramLength, int path,
						   uint8_t* out, int outStart, int outStride) {
	const HostImg<const uint8_t> hin{in, inStart, inStride, width, height};
	const HostImg<uint8_t> hout{out, outStart, outStride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	CHECK_IMG(ctx, hout);
	BHIP_TRY(eqLocalArgs(ctx, radius, histogramLength, path, width, height));
	return hostInOut<uint8_t, uint8_t>(ctx, hin, hout, false, false, nullptr, [&](DevImg<uint8_t> din, DevImg<uint8_t> dout) {
		return eqLocalImpl(ctx, radius, histogramLength, path, DevImg<const uint8_t>(din), dout);
	});
}

int bhip_sharpen_dev_u8(bhip_ctx* ctx, int rule, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, uint8_t* dev_out,
						long long outImageStride, int outStride) {
	return sharpenDev<uint8_t>(ctx, rule, {dev_in, inImageStride, inStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_sharpen_dev_f32(bhip_ctx* ctx, int rule, const float* dev_in, long long inImageStride, int inStride, int width, int height, int batch, float* dev_out,
						 long long outImageStride, int outStride) {
	return sharpenDev<float>(ctx, rule, {dev_in, inImageStride, inStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_sharpen_u8(bhip_ctx* ctx, int rule, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart, int outStride) {
	return sharpenHost<uint8_t>(ctx, rule, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height});
}
int bhip_sharpen_f32(bhip_ctx* ctx, int rule, const float* in, int inStart, int inStride, int width, int height, float* out, int outStart, int outStride) {
	return sharpenHost<float>(ctx, rule, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height});
}

}  // extern "C"
