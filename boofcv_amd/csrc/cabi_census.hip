// C ABI, census transform (census.hip): FilterImageInterface.process of FactoryCensusTransform.variant / blockDense on GrayU8 images.
#include "cabi.h"

// what one call computes: the dense 3x3 / 5x5 block (denseRadius 1 / 2) or a sample list
struct CensusForm {
	int denseRadius = 0;
	CensusSamples s;
	int radius() const { return denseRadius ? denseRadius : s.radius; }
};

// the checks every form shares, before anything is staged or launched (include/boofhip.h)
static int censusForm(bhip_ctx* ctx, int denseRadius, const int* samplesXY, int nSamples, int width, int height, CensusForm& f) {
	f.denseRadius = denseRadius;
	if (!denseRadius) {
		const int st = bhip_census_samples(samplesXY, nSamples, f.s);
		if (st == BHIP_ERR_UNSUPPORTED) return bhip_fail(ctx, st, "census on the GPU: sample offsets within -7 .. 7");
		if (st != BHIP_OK) return bhip_fail(ctx, st, "At most 64 sample points for now. size = " + std::to_string(nSamples));
	}
	if (width < f.radius() + 1 || height < f.radius() + 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "the image is smaller than the census region's radius + 1");
	return BHIP_OK;
}

template <class OutT>
static int censusDev(bhip_ctx* ctx, int denseRadius, const int* samplesXY, int nSamples, const uint8_t* dev_in, long long iImageStride, int iStride, int width,
					 int height, int batch, OutT* dev_out, long long oImageStride, int oStride) {
	CHECK_CTX(ctx);
	const DevImg<const uint8_t> in{dev_in, iImageStride, iStride, width, height, batch};
	const DevImg<OutT> out{dev_out, oImageStride, oStride, width, height, batch};
	CHECK_IMG(ctx, in);
	CHECK_IMG(ctx, out);
	CensusForm f;
	BHIP_TRY(censusForm(ctx, denseRadius, samplesXY, nSamples, width, height, f));
	return bhip_launch_census<OutT>(ctx, in, f.denseRadius, denseRadius ? nullptr : &f.s, out);
}

template <class OutT>
static int censusHost(bhip_ctx* ctx, int denseRadius, const int* samplesXY, int nSamples, const uint8_t* in, int start, int stride, int width, int height,
					  OutT* out, int oStart, int oStride) {
	const HostImg<const uint8_t> hi{in, start, stride, width, height};
	const HostImg<OutT> ho{out, oStart, oStride, width, height};
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hi);
	CHECK_IMG(ctx, ho);
	CensusForm f;
	BHIP_TRY(censusForm(ctx, denseRadius, samplesXY, nSamples, width, height, f));
	CtxScratch* sc = scratchOf(ctx);
	DevImg<uint8_t> din;
	DevImg<OutT> dout;
	BHIP_TRY(stageIn(ctx, sc->in0, hi, width, din));
	BHIP_TRY(stageIn(ctx, sc->out0, ho, width, dout, false));
	BHIP_TRY(bhip_launch_census<OutT>(ctx, din, f.denseRadius, denseRadius ? nullptr : &f.s, dout));
	BHIP_TRY(stageOut(ctx, ho, dout));
	return bhip_ctx_synchronize(ctx);
}

extern "C" {

int bhip_census_variant_samples(int variant, int* samplesXY, int cap, int* n) {
	int xy[2 * BHIP_CENSUS_MAX_SAMPLES];
	const int len = bhip_census_variant_list(variant, xy);
	if (len < 0 || !n || (samplesXY && cap < len)) return BHIP_ERR_INVALID;
	if (samplesXY) memcpy(samplesXY, xy, sizeof(int) * 2 * len);
	*n = len;
	return BHIP_OK;
}

int bhip_census_u8_u8(bhip_ctx* ctx, const uint8_t* in, int start, int stride, int width, int height, uint8_t* out, int oStart, int oStride) {
	return censusHost<uint8_t>(ctx, 1, nullptr, 0, in, start, stride, width, height, out, oStart, oStride);
}
int bhip_census_u8_s32(bhip_ctx* ctx, const uint8_t* in, int start, int stride, int width, int height, int32_t* out, int oStart, int oStride) {
	return censusHost<int32_t>(ctx, 2, nullptr, 0, in, start, stride, width, height, out, oStart, oStride);
}
int bhip_census_sample_u8_s64(bhip_ctx* ctx, const int* samplesXY, int nSamples, const uint8_t* in, int start, int stride, int width, int height, long long* out,
							  int oStart, int oStride) {
	return censusHost<long long>(ctx, 0, samplesXY, nSamples, in, start, stride, width, height, out, oStart, oStride);
}
int bhip_census_dev_u8_u8(bhip_ctx* ctx, const uint8_t* dev_in, long long iImageStride, int iStride, int width, int height, int batch, uint8_t* dev_out,
						  long long oImageStride, int oStride) {
	return censusDev<uint8_t>(ctx, 1, nullptr, 0, dev_in, iImageStride, iStride, width, height, batch, dev_out, oImageStride, oStride);
}
int bhip_census_dev_u8_s32(bhip_ctx* ctx, const uint8_t* dev_in, long long iImageStride, int iStride, int width, int height, int batch, int32_t* dev_out,
						   long long oImageStride, int oStride) {
	return censusDev<int32_t>(ctx, 2, nullptr, 0, dev_in, iImageStride, iStride, width, height, batch, dev_out, oImageStride, oStride);
}
int bhip_census_sample_dev_u8_s64(bhip_ctx* ctx, const int* samplesXY, int nSamples, const uint8_t* dev_in, long long iImageStride, int iStride, int width,
								  int height, int batch, long long* dev_out, long long oImageStride, int oStride) {
	return censusDev<long long>(ctx, 0, samplesXY, nSamples, dev_in, iImageStride, iStride, width, height, batch, dev_out, oImageStride, oStride);
}

}   // extern "C"
