// Census transform of GrayU8 images: FactoryCensusTransform.variant / blockDense, the front end of census block matching (disparity.hip).
//
// Reference (I: = main/boofcv-ip/src/main/java/boofcv/):
//   CensusTransform.dense3x3 / dense5x5 / sample_S64, createBlockSamples / createCircleSamples   I:alg/transform/census/CensusTransform.java:53-225
//   ImplCensusTransformInner, ImplCensusTransformBorder (regionNxN, sample_S64)                   I:alg/transform/census/impl/
//   FactoryCensusTransform (CENSUS_BORDER = REFLECT), CensusVariants                              I:factory/transform/census/
//   BorderIndex1D_Reflect                                                                         I:core/image/border/BorderIndex1D_Reflect.java:34-41
//
// One formula for every pixel (the reference's inner and border code compute the same thing): with c = in(x, y), bit i of the word is set iff
// in(reflect(x + dx_i), reflect(y + dy_i)) > c, reflect(k) = -k for k < 0 and 2*len - 2 - k for k >= len.  The dense forms take their samples
// row-major over dy, then dx, without the centre; bit 0 is the first sample.
// The S64 form counts its bits in a Java int (`long census; int bit = 1; census |= bit; bit <<= 1`): samples 0..30 set bits 0..30, sample 31
// ORs in 0x80000000 sign-extended and so sets bits 31..63, samples 32 and up add nothing.  A word is the sign extension of its low 32 bits,
// which is all the kernel computes: it reads the first 32 samples only.
// The image must hold one reflection: W, H >= radius + 1 with radius the largest |dx|, |dy| of all samples (the caller checks).
//
// Tile: a workgroup of 256 owns 64 x 16 output pixels (CENSUS_TW x CENSUS_TH).  It stages the tile plus a halo of (rx, ry) input bytes in LDS,
// the reflected index resolved per staged byte, so every load is a byte inside the view at any alignment and stride.  A lane owns one column
// and four rows (ty, ty + 4, ..), reads the centre and the samples from LDS (consecutive lanes read consecutive bytes: four lanes share a
// bank word, no conflicts) and builds the word in a register; a wave stores 64 consecutive elements of one output row.
// LDS: 30 rows x 80 B = 2400 B per workgroup; occupancy is bounded by waves, not LDS.  HBM traffic: 1 B read, 1 / 4 / 8 B written per pixel.
#include "common.h"

#define CENSUS_TW 64
#define CENSUS_TH 16
#define CENSUS_PITCH 80   // CENSUS_TW + 2 * BHIP_CENSUS_MAX_OFFSET, rounded up to dwords
#define CENSUS_ROWS (CENSUS_TH + 2 * BHIP_CENSUS_MAX_OFFSET)

struct CensusKernelParams {
	const uint8_t* in;
	long long iImageStride;
	int iStride, w, h;
	void* out;
	long long oImageStride;
	int oStride;
	int rx, ry;        // halo of the sample list (the dense forms know theirs)
	int n;             // samples the kernel reads, <= 32
	int off[32];       // dy * CENSUS_PITCH + dx of sample i
};

// BorderIndex1D_Reflect, then clamped: tile positions past the image's own halo are staged but never read
__device__ __forceinline__ int censusReflect(int k, int len) {
	const int r = k < 0 ? -k : k >= len ? 2 * len - 2 - k : k;
	return min(max(r, 0), len - 1);
}

// R > 0: the dense (2R+1)^2 block, unrolled; R == 0: the sample list of P
template <int R, class OutT>
__global__ __launch_bounds__(256) void k_census(CensusKernelParams P) {
	__shared__ __attribute__((aligned(16))) uint8_t tile[CENSUS_ROWS * CENSUS_PITCH];
	const int rx = R ? R : P.rx, ry = R ? R : P.ry;
	const int x0 = blockIdx.x * CENSUS_TW, y0 = blockIdx.y * CENSUS_TH;
	const uint8_t* img = P.in + (long long)blockIdx.z * P.iImageStride;
	const int cols = CENSUS_TW + 2 * rx, rows = CENSUS_TH + 2 * ry;
	// one staged byte per lane and pass, indexed over rows of the constant pitch (a division by a constant; cols of its 80 slots are live)
	for (int s = threadIdx.x; s < rows * CENSUS_PITCH; s += 256) {
		const int r = s / CENSUS_PITCH, k = s - r * CENSUS_PITCH;
		if (k >= cols) continue;
		const int yy = censusReflect(y0 - ry + r, P.h), xx = censusReflect(x0 - rx + k, P.w);
		tile[s] = img[(long long)yy * P.iStride + xx];
	}
	__syncthreads();
	const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
	const int x = x0 + tx;
	if (x >= P.w) return;
	OutT* out = (OutT*)P.out + (long long)blockIdx.z * P.oImageStride + x;
#pragma unroll
	for (int j = 0; j < CENSUS_TH / 4; j++) {
		const int yl = ty + 4 * j, y = y0 + yl;
		if (y >= P.h) break;
		const uint8_t* cp = tile + (yl + ry) * CENSUS_PITCH + tx + rx;
		const unsigned int c = *cp;
		unsigned int word = 0;
		if constexpr (R > 0) {
			int bit = 0;
#pragma unroll
			for (int dy = -R; dy <= R; dy++)
#pragma unroll
				for (int dx = -R; dx <= R; dx++)
					if (dx != 0 || dy != 0) word |= (unsigned int)(cp[dy * CENSUS_PITCH + dx] > c) << bit++;
		} else {
			for (int i = 0; i < P.n; i++) word |= (unsigned int)(cp[P.off[i]] > c) << i;
		}
		if constexpr (sizeof(OutT) == 8) out[(long long)y * P.oStride] = (OutT)(int)word;   // `census |= bit` with an int bit: sign extension
		else out[(long long)y * P.oStride] = (OutT)word;
	}
}

int bhip_census_samples(const int* samplesXY, int nSamples, CensusSamples& s) {
	if (nSamples < 0 || nSamples > BHIP_CENSUS_MAX_SAMPLES || (nSamples > 0 && !samplesXY)) return BHIP_ERR_INVALID;
	s = CensusSamples();
	s.n = nSamples;
	for (int i = 0; i < nSamples; i++) {
		const int dx = samplesXY[2 * i], dy = samplesXY[2 * i + 1];
		if (dx < -BHIP_CENSUS_MAX_OFFSET || dx > BHIP_CENSUS_MAX_OFFSET || dy < -BHIP_CENSUS_MAX_OFFSET || dy > BHIP_CENSUS_MAX_OFFSET) return BHIP_ERR_UNSUPPORTED;
		s.radius = std::max(s.radius, std::max(abs(dx), abs(dy)));
		if (i < 32) {
			s.dx[i] = (signed char)dx;
			s.dy[i] = (signed char)dy;
		}
	}
	return BHIP_OK;
}

int bhip_census_variant_list(int variant, int* samplesXY) {
	int n = 0;
	auto block = [&](int rx, int ry) {   // CensusTransform.createBlockSamples
		for (int y = -ry; y <= ry; y++)
			for (int x = -rx; x <= rx; x++)
				if (x != 0 || y != 0) { samplesXY[2 * n] = x; samplesXY[2 * n + 1] = y; n++; }
	};
	switch (variant) {
		case BHIP_CENSUS_BLOCK_3_3: block(1, 1); break;
		case BHIP_CENSUS_BLOCK_5_5: block(2, 2); break;
		case BHIP_CENSUS_BLOCK_7_7: block(3, 3); break;
		case BHIP_CENSUS_BLOCK_9_7: block(4, 3); break;
		case BHIP_CENSUS_BLOCK_13_5: block(5, 2); break;
		case BHIP_CENSUS_CIRCLE_9:   // CensusTransform.createCircleSamples: set(row - 4, col - 4), the loop's row is x
			for (int row = 0; row < 9; row++) {
				const int col0 = row <= 4 ? std::max(0, 3 - row) : row - 5, col1 = 9 - col0;
				for (int col = col0; col < col1; col++)
					if (row != 4 || col != 4) { samplesXY[2 * n] = row - 4; samplesXY[2 * n + 1] = col - 4; n++; }
			}
			break;
		default: return -1;
	}
	return n;
}

template <class OutT>
int bhip_launch_census(bhip_ctx* ctx, DevImg<const uint8_t> in, int denseRadius, const CensusSamples* s, DevImg<OutT> out) {
	const int w = in.width, h = in.height, batch = in.batch;
	if (batch <= 0 || w <= 0 || h <= 0) return BHIP_OK;
	// GrayU8: the 3x3 block; GrayS32: the 5x5 block, or the low words of a sample list (census block matching); GrayS64: a sample list
	const bool form = sizeof(OutT) == 1 ? denseRadius == 1 : sizeof(OutT) == 4 ? denseRadius == 2 || (denseRadius == 0 && s) : denseRadius == 0 && s;
	const int radius = denseRadius ? denseRadius : s ? s->radius : 0;
	if (!form || w < radius + 1 || h < radius + 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "bhip_launch_census: outside the kernel's limits");
	CensusKernelParams P{in.data, in.imageStride, in.stride, w, h, out.data, out.imageStride, out.stride, 0, 0, 0, {}};
	if (!denseRadius) {
		P.n = std::min(s->n, 32);
		for (int i = 0; i < P.n; i++) {
			P.off[i] = s->dy[i] * CENSUS_PITCH + s->dx[i];
			P.rx = std::max(P.rx, abs((int)s->dx[i]));
			P.ry = std::max(P.ry, abs((int)s->dy[i]));
		}
	}
	const dim3 grid((w + CENSUS_TW - 1) / CENSUS_TW, (h + CENSUS_TH - 1) / CENSUS_TH, batch);
	const double px = (double)w * h * batch;
	ProfScope ps(ctx, sizeof(OutT) == 1 ? "k_census_u8" : sizeof(OutT) == 4 ? "k_census_s32" : "k_census_s64", (1.0 + sizeof(OutT)) * px);
	if constexpr (sizeof(OutT) == 1) {
		hipLaunchKernelGGL((k_census<1, uint8_t>), grid, dim3(256), 0, ctx->stream, P);
	} else if constexpr (sizeof(OutT) == 4) {
		if (denseRadius) hipLaunchKernelGGL((k_census<2, int32_t>), grid, dim3(256), 0, ctx->stream, P);
		else hipLaunchKernelGGL((k_census<0, int32_t>), grid, dim3(256), 0, ctx->stream, P);
	} else {
		hipLaunchKernelGGL((k_census<0, long long>), grid, dim3(256), 0, ctx->stream, P);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_census(bhip_ctx*, DevImg<const uint8_t>, int, const CensusSamples*, DevImg<uint8_t>);
template int bhip_launch_census(bhip_ctx*, DevImg<const uint8_t>, int, const CensusSamples*, DevImg<int32_t>);
template int bhip_launch_census(bhip_ctx*, DevImg<const uint8_t>, int, const CensusSamples*, DevImg<long long>);
