// ---------------------------------------------------------------------------------------------------------------
// boofcv-ip front end.  Most operations have a host-buffer export (the caller's image view) and a device-batched _dev export (BASELINE
// config 5: pyramid -> gradient -> NMS -> SURF on a 4K stream without leaving HBM).  Both run one implementation -- a launcher of conv.hip, pyramid.hip, gradient.hip, corner.hip or brief.hip, or
// an xxxImpl around several -- on DevImg views of device images, asynchronous on the ctx stream.  The _dev export wraps the caller's
// pointers into views and calls it after its argument checks.  The host export checks its HostImg views, stages them (stageIn / hostInOut:
// rows pitch4(width) apart where the tiled kernels apply, dense otherwise), calls it with batch 1, downloads and synchronizes; when the
// implementation fails, nothing is downloaded.
// ---------------------------------------------------------------------------------------------------------------
#include "cabi.h"

// BlurImageOps.gaussian: one fused pass, or a horizontal pass into the library's `storage` and a vertical pass into `out`
int gaussianImpl(bhip_ctx* ctx, double sigma, int radius, DevImg<const float> in, DevImg<float> out) {
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
int cornerImpl(bhip_ctx* ctx, bool weighted, int kind, int radius, float kappa, DevImg<const T> dx, DevImg<const T> dy, DevImg<float> intensity) {
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
template int cornerImpl<float>(bhip_ctx*, bool, int, int, float, DevImg<const float>, DevImg<const float>, DevImg<float>);
template int cornerImpl<int16_t>(bhip_ctx*, bool, int, int, float, DevImg<const int16_t>, DevImg<const int16_t>, DevImg<float>);

// every sample point the pairs use lies within [-radius, radius]^2: the LDS-patch BRIEF kernel may be used (brief.hip, k_brief_patch)
bool briefPatchOk(const int32_t* samplePoints, int nSamples, int radius) {
	for (int i = 0; i < 2 * nSamples; i++)
		if (samplePoints[i] < -radius || samplePoints[i] > radius) return false;
	return radius >= 0 && radius <= 40;
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

static bool gradBorderOk(int kind, int border) { return border == 0 || border == 1 || (border == 2 && kind != 1); }   // 2 = BorderType.EXTENDED: GradientSobel and GradientPrewitt

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
template <class T>
int pyramidImpl(bhip_ctx* ctx, const typename PyrTraits<T>::Kernel* kernel, int kw, const int* scales, int n, DevImg<const T> in, T* out,
					   bool layer0Present) {
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
template int pyramidImpl<float>(bhip_ctx*, const float*, int, const int*, int, DevImg<const float>, float*, bool);
template int pyramidImpl<uint8_t>(bhip_ctx*, const int32_t*, int, const int*, int, DevImg<const uint8_t>, uint8_t*, bool);

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

int bhip_prewitt_f32(bhip_ctx* ctx, const float* in, int inStart, int inStride, int width, int height, float* dx, float* dy, int outStart, int outStride,
					 int border) {
	return gradHost<float, float>(ctx, 2, {in, inStart, inStride, width, height}, {dx, outStart, outStride, width, height}, {dy, outStart, outStride, width, height}, border);
}
int bhip_prewitt_u8_s16(bhip_ctx* ctx, const uint8_t* in, int inStart, int inStride, int width, int height, int16_t* dx, int16_t* dy, int outStart,
						int outStride, int border) {
	return gradHost<uint8_t, int16_t>(ctx, 2, {in, inStart, inStride, width, height}, {dx, outStart, outStride, width, height}, {dy, outStart, outStride, width, height}, border);
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

int bhip_prewitt_dev_f32(bhip_ctx* ctx, const float* dev_in, long long inImageStride, int inStride, int width, int height, int batch, float* dev_dx, float* dev_dy,
						 long long outImageStride, int outStride, int border) {
	return gradDev<float, float>(ctx, 2, {dev_in, inImageStride, inStride, width, height, batch}, {dev_dx, outImageStride, outStride, width, height, batch},
								 {dev_dy, outImageStride, outStride, width, height, batch}, border);
}
int bhip_prewitt_dev_u8_s16(bhip_ctx* ctx, const uint8_t* dev_in, long long inImageStride, int inStride, int width, int height, int batch, int16_t* dev_dx,
							int16_t* dev_dy, long long outImageStride, int outStride, int border) {
	return gradDev<uint8_t, int16_t>(ctx, 2, {dev_in, inImageStride, inStride, width, height, batch}, {dev_dx, outImageStride, outStride, width, height, batch},
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
