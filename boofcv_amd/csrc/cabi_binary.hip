// ---------------------------------------------------------------------------------------------------------------
// BinaryImageOps on the C boundary: the logic operations, erode / dilate / edge / removePointNoise, the labelled image of contour(), relabel
// and labelToBinary (binary_ops.hip, label.hip).  Every argument check comes before anything touches the device, so a refused call writes
// nothing.  The _dev exports run on the caller's views, asynchronous on the ctx stream; the host exports stage their views and run the same
// implementation with batch 1.
// ---------------------------------------------------------------------------------------------------------------
#include "cabi.h"

// the bytes a view spans, for the overlap test of the neighbourhood operations
static bool overlaps(DevImg<const uint8_t> a, DevImg<const uint8_t> b) {
	auto span = [](DevImg<const uint8_t> v, uintptr_t& lo, uintptr_t& hi) {   // an image stride may be negative: the first image is then the highest
		const long long back = v.imageStride < 0 ? (long long)(v.batch - 1) * -v.imageStride : 0;
		const long long fwd = v.imageStride > 0 ? (long long)(v.batch - 1) * v.imageStride : 0;
		lo = (uintptr_t)v.data - (uintptr_t)back;
		hi = (uintptr_t)v.data + (uintptr_t)(fwd + (long long)(v.height - 1) * v.stride + v.width);
	};
	uintptr_t alo, ahi, blo, bhi;
	span(a, alo, ahi);
	span(b, blo, bhi);
	return alo < bhi && blo < ahi;
}

// op: BHIP_MORPH_* of common.h; n: iterations (>= 1).  Up to BHIP_MORPH_FUSED_MAX iterations are one launch; beyond that the launches
// alternate between the two scratch images and the last one writes `out`.
static int morphImpl(bhip_ctx* ctx, int op, int outsideZero, int n, DevImg<const uint8_t> in, DevImg<uint8_t> out) {
	if (n <= BHIP_MORPH_FUSED_MAX) return bhip_launch_binary_morph(ctx, op, outsideZero, n, in, out);
	DevBuf& buf = scratchOf(ctx)->binary;
	const size_t plane = (size_t)in.width * in.height * in.batch;
	BHIP_TRY(buf.reserve(ctx, 2 * plane));
	DevImg<uint8_t> tmp[2] = {bhip_img_over<uint8_t>(buf, in.width, in.width, in.height, in.batch), bhip_img_over<uint8_t>(buf, in.width, in.width, in.height, in.batch)};
	tmp[1].data += plane;
	DevImg<const uint8_t> src = in;
	int which = 0;
	while (n > 0) {
		const int step = std::min(n, BHIP_MORPH_FUSED_MAX);
		n -= step;
		const DevImg<uint8_t> dst = n == 0 ? out : tmp[which];
		BHIP_TRY(bhip_launch_binary_morph(ctx, op, outsideZero, step, src, dst));
		src = dst;
		which ^= 1;
	}
	return BHIP_OK;
}
// the checks of a neighbourhood operation on device views; numTimes is turned into the iteration count
static const char* morphArgError(int op, int& numTimes) {
	if (op < BHIP_MORPH_ERODE4 || op > BHIP_MORPH_DILATE8) return "unknown morphology operation";
	if (op == BHIP_MORPH_ERODE4 && numTimes <= 0) return "numTimes must be >= 1";
	if (numTimes < 1) numTimes = 1;
	return nullptr;
}
static const char* ruleArgError(int rule) { return rule == BHIP_CONNECT_FOUR || rule == BHIP_CONNECT_EIGHT ? nullptr : "Connectivity rule must be 4 or 8"; }

static int neighbourDev(bhip_ctx* ctx, int op, int outsideZero, int n, const char* argError, DevImg<const uint8_t> in, DevImg<uint8_t> out) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	if (argError) return bhip_fail(ctx, BHIP_ERR_INVALID, argError);
	if (in.batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	if (overlaps(in, out)) return bhip_fail(ctx, BHIP_ERR_INVALID, "input and output of a neighbourhood operation must not overlap");
	return morphImpl(ctx, op, outsideZero, n, in, out);
}
static int neighbourHost(bhip_ctx* ctx, int op, int outsideZero, int n, const char* argError, HostImg<const uint8_t> in, HostImg<uint8_t> out) {
	return hostInOut<uint8_t, uint8_t>(ctx, in, out, false, false, argError,
									   [&](DevImg<uint8_t> din, DevImg<uint8_t> dout) { return morphImpl(ctx, op, outsideZero, n, DevImg<const uint8_t>(din), dout); });
}

static int labelImpl(bhip_ctx* ctx, int rule, DevImg<const uint8_t> in, DevImg<int32_t> out, int* devNumBlobs) {
	if ((long long)in.width * in.height > 2147483647LL) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "width * height beyond an int32 index");
	if (in.height > 65535 * 32) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 2097120 rows");
	// parent[] is 4 bytes per pixel: at most 256 MiB of images at a time
	const size_t perImage = bhip_label_scratch(in.width, in.height, 1);
	const int chunk = (int)std::max<size_t>(1, std::min<size_t>(in.batch, ((size_t)256 << 20) / perImage));
	DevBuf& buf = scratchOf(ctx)->label;
	BHIP_TRY(buf.reserve(ctx, perImage * chunk));
	for (int b0 = 0; b0 < in.batch; b0 += chunk) {
		DevImg<const uint8_t> i = in;
		DevImg<int32_t> o = out;
		i.data += (long long)b0 * in.imageStride;
		o.data += (long long)b0 * out.imageStride;
		i.batch = o.batch = std::min(chunk, in.batch - b0);
		BHIP_TRY(bhip_launch_label_blobs(ctx, rule == BHIP_CONNECT_EIGHT, i, o, devNumBlobs + b0, buf.p));
	}
	return BHIP_OK;
}

// a host lookup table in device memory (binaryTable); the upload is ordered on the ctx stream before the launch that reads it
template <class T>
static int uploadTable(bhip_ctx* ctx, const T* table, int n, const T** dev) {
	DevBuf& buf = scratchOf(ctx)->binaryTable;
	BHIP_TRY(buf.reserve(ctx, std::max<size_t>(16, (size_t)std::max(n, 0) * sizeof(T))));
	if (n > 0) BHIP_HIP(ctx, hipMemcpyAsync(buf.p, table, (size_t)n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
	*dev = buf.as<T>();
	return BHIP_OK;
}

extern "C" {

int bhip_binary_logic_dev_u8(bhip_ctx* ctx, int op, const uint8_t* dev_a, long long aImageStride, int aStride, const uint8_t* dev_b, long long bImageStride,
							 int bStride, int width, int height, int batch, uint8_t* dev_out, long long outImageStride, int outStride) {
	const DevImg<const uint8_t> a{dev_a, aImageStride, aStride, width, height, batch}, b{dev_b, bImageStride, bStride, width, height, batch};
	const DevImg<uint8_t> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, a);
	CHECK_IMG(ctx, b);
	CHECK_IMG(ctx, out);
	if (op < BHIP_LOGIC_AND || op > BHIP_LOGIC_XOR) return bhip_fail(ctx, BHIP_ERR_INVALID, "unknown logic operation");
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	return bhip_launch_binary_logic(ctx, op, a, &b, out);
}
int bhip_binary_logic_u8(bhip_ctx* ctx, int op, const uint8_t* a, int aStart, int aStride, const uint8_t* b, int bStart, int bStride, int width, int height,
						 uint8_t* out, int outStart, int outStride) {
	const HostImg<const uint8_t> ha{a, aStart, aStride, width, height}, hb{b, bStart, bStride, width, height};
	const HostImg<uint8_t> ho{out, outStart, outStride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, ha);
	CHECK_IMG(ctx, hb);
	CHECK_IMG(ctx, ho);
	if (op < BHIP_LOGIC_AND || op > BHIP_LOGIC_XOR) return bhip_fail(ctx, BHIP_ERR_INVALID, "unknown logic operation");
	CtxScratch* sc = scratchOf(ctx);
	DevImg<uint8_t> da, db, dout;
	BHIP_TRY(stageIn(ctx, sc->in0, ha, width, da));
	BHIP_TRY(stageIn(ctx, sc->in1, hb, width, db));
	BHIP_TRY(stageIn(ctx, sc->out0, ho, width, dout, false));
	const DevImg<const uint8_t> cb = db;
	BHIP_TRY(bhip_launch_binary_logic(ctx, op, da, &cb, dout));
	BHIP_TRY(stageOut(ctx, ho, dout));
	return bhip_ctx_synchronize(ctx);
}
int bhip_binary_invert_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, uint8_t* dev_out,
							  long long outImageStride, int outStride) {
	const DevImg<const uint8_t> in{dev_in, inImageStride, inStride, width, height, batch};
	const DevImg<uint8_t> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	return bhip_launch_binary_logic(ctx, 0, in, nullptr, out);
}
int bhip_binary_invert_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart, int outStride) {
	return hostInOut<uint8_t, uint8_t>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, false, false, nullptr,
									   [&](DevImg<uint8_t> din, DevImg<uint8_t> dout) { return bhip_launch_binary_logic(ctx, 0, DevImg<const uint8_t>(din), nullptr, dout); });
}

int bhip_binary_morph_dev_u8(bhip_ctx* ctx, int op, int numTimes, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch,
							 uint8_t* dev_out, long long outImageStride, int outStride) {
	const char* e = morphArgError(op, numTimes);
	return neighbourDev(ctx, op, 0, numTimes, e, {dev_in, inImageStride, inStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_binary_morph_u8(bhip_ctx* ctx, int op, int numTimes, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart,
						 int outStride) {
	const char* e = morphArgError(op, numTimes);
	return neighbourHost(ctx, op, 0, numTimes, e, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height});
}
int bhip_binary_edge_dev_u8(bhip_ctx* ctx, int rule, int outsideZero, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch,
							uint8_t* dev_out, long long outImageStride, int outStride) {
	return neighbourDev(ctx, rule == BHIP_CONNECT_FOUR ? BHIP_MORPH_EDGE4 : BHIP_MORPH_EDGE8, outsideZero, 1, ruleArgError(rule),
						{dev_in, inImageStride, inStride, width, height, batch}, {dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_binary_edge_u8(bhip_ctx* ctx, int rule, int outsideZero, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart,
						int outStride) {
	return neighbourHost(ctx, rule == BHIP_CONNECT_FOUR ? BHIP_MORPH_EDGE4 : BHIP_MORPH_EDGE8, outsideZero, 1, ruleArgError(rule), {in, inStart, inStride, width, height},
						 {out, outStart, outStride, width, height});
}
int bhip_binary_remove_point_noise_dev_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch,
										  uint8_t* dev_out, long long outImageStride, int outStride) {
	return neighbourDev(ctx, BHIP_MORPH_REMOVE_POINT_NOISE, 0, 1, nullptr, {dev_in, inImageStride, inStride, width, height, batch},
						{dev_out, outImageStride, outStride, width, height, batch});
}
int bhip_binary_remove_point_noise_u8(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart, int outStride) {
	return neighbourHost(ctx, BHIP_MORPH_REMOVE_POINT_NOISE, 0, 1, nullptr, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height});
}

int bhip_label_blobs_dev_u8_s32(bhip_ctx* ctx, int rule, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch,
								int32_t* dev_out, long long outImageStride, int outStride, int* dev_numBlobs) {
	const DevImg<const uint8_t> in{dev_in, inImageStride, inStride, width, height, batch};
	const DevImg<int32_t> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	if (!dev_numBlobs) return bhip_fail(ctx, BHIP_ERR_INVALID, "null blob count");
	if (const char* e = ruleArgError(rule)) return bhip_fail(ctx, BHIP_ERR_INVALID, e);
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	return labelImpl(ctx, rule, in, out, dev_numBlobs);
}
int bhip_label_blobs_u8_s32(bhip_ctx* ctx, int rule, const uint8_t* in, int inStart, int inStride, int width, int height, int32_t* out, int outStart, int outStride,
							int* numBlobs) {
	const HostImg<const uint8_t> hin{in, inStart, inStride, width, height};
	const HostImg<int32_t> hout{out, outStart, outStride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	CHECK_IMG(ctx, hout);
	if (!numBlobs) return bhip_fail(ctx, BHIP_ERR_INVALID, "null blob count");
	if (const char* e = ruleArgError(rule)) return bhip_fail(ctx, BHIP_ERR_INVALID, e);
	CtxScratch* sc = scratchOf(ctx);
	DevImg<uint8_t> din;
	DevImg<int32_t> dout;
	BHIP_TRY(stageIn(ctx, sc->in0, hin, width, din));
	BHIP_TRY(stageIn(ctx, sc->out0, hout, width, dout, false));
	BHIP_TRY(sc->binaryTable.reserve(ctx, 16));   // the count
	BHIP_TRY(labelImpl(ctx, rule, DevImg<const uint8_t>(din), dout, sc->binaryTable.as<int>()));
	BHIP_TRY(stageOut(ctx, hout, dout));
	BHIP_HIP(ctx, hipMemcpyAsync(numBlobs, sc->binaryTable.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

int bhip_relabel_dev_s32(bhip_ctx* ctx, int32_t* dev_img, long long imageStride, int stride, int width, int height, int batch, const int* dev_labels, int numLabels) {
	const DevImg<int32_t> img{dev_img, imageStride, stride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, img);
	if (numLabels < 0 || (numLabels > 0 && !dev_labels)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad label table");
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	return bhip_launch_relabel(ctx, img, dev_labels, numLabels);
}
int bhip_relabel_s32(bhip_ctx* ctx, int32_t* img, int start, int stride, int width, int height, const int* labels, int numLabels) {
	const HostImg<int32_t> h{img, start, stride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, h);
	if (numLabels < 0 || (numLabels > 0 && !labels)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad label table");
	DevImg<int32_t> d;
	BHIP_TRY(stageIn(ctx, scratchOf(ctx)->out0, h, width, d));
	const int* table;
	BHIP_TRY(uploadTable<int>(ctx, labels, numLabels, &table));
	BHIP_TRY(bhip_launch_relabel(ctx, d, table, numLabels));
	BHIP_TRY(stageOut(ctx, h, d));
	return bhip_ctx_synchronize(ctx);
}
int bhip_label_to_binary_dev_s32_u8(bhip_ctx* ctx, const int32_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, uint8_t* dev_out,
									long long outImageStride, int outStride, const uint8_t* dev_selected, int numSelected) {
	const DevImg<const int32_t> in{dev_in, inImageStride, inStride, width, height, batch};
	const DevImg<uint8_t> out{dev_out, outImageStride, outStride, width, height, batch};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	if (numSelected < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad selection table");
	if (batch > 65535) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "more than 65535 images in a batch");
	return bhip_launch_label_to_binary(ctx, in, out, dev_selected, numSelected);
}
int bhip_label_to_binary_s32_u8(bhip_ctx* ctx, const int32_t* in, int inStart, int inStride, int width, int height, uint8_t* out, int outStart, int outStride,
								const uint8_t* selected, int numSelected) {
	return hostInOut<int32_t, uint8_t>(ctx, {in, inStart, inStride, width, height}, {out, outStart, outStride, width, height}, false, false,
									   numSelected < 0 ? "bad selection table" : nullptr, [&](DevImg<int32_t> din, DevImg<uint8_t> dout) {
										   const uint8_t* table = nullptr;
										   if (selected) BHIP_TRY(uploadTable<uint8_t>(ctx, selected, numSelected, &table));
										   return bhip_launch_label_to_binary(ctx, DevImg<const int32_t>(din), dout, table, numSelected);
									   });
}

}  // extern "C"
