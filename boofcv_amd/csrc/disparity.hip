// Dense stereo disparity by SAD block matching on GrayU8 pairs: FactoryStereoDisparity.blockMatch(ConfigDisparityBM, GrayU8, GrayU8 | GrayF32), errorType = SAD.
//
// Reference (F: = main/boofcv-feature/src/main/java/boofcv/):
//   DisparityBlockMatchRowFormat.process              F:alg/feature/disparity/DisparityBlockMatchRowFormat.java:95-107
//   DisparityScoreBM_S32 (running row / column sums)  F:alg/feature/disparity/block/score/DisparityScoreBM_S32.java:73-205
//   BlockRowScore.ArrayS32.scoreRow, BlockRowScoreSad.U8   F:alg/feature/disparity/block/BlockRowScore.java:96-138, BlockRowScoreSad.java:53-67
//   SelectErrorWithChecks_S32.process / selectRightToLeft  F:alg/feature/disparity/block/select/SelectErrorWithChecks_S32.java:73-162
//   SelectErrorWithChecks_S32.DispU8.setDisparity     :172-190        SelectErrorSubpixel.S32_F32.setDisparity   SelectErrorSubpixel.java:46-75
//   WrapBaseBlockMatch.process (the fill value)       F:abst/feature/disparity/WrapBaseBlockMatch.java:42-85
//
// With rw = 2*rx+1, rh = 2*ry+1 the cost of the left block that starts at column c against the right block that starts at c - minD - i is
//   C(y,c,i) = sum_{dy=-ry..ry} sum_{j<rw} |L[y+dy][c+j] - R[y+dy][c-minD-i+j]|        (int; integers make the reference's running sums exact)
// for i < lm = min(c - minD + 1, range); the result goes to pixel (c + rx, y).  Selection, checks and the sub-pixel rule: include/boofhip.h.
//
// Two stages, separable in the code: the cost stage (dispCostRow, the per-pixel cost is the template parameter Cost) fills a slab
// V[anchor column][disparity] of one output row in LDS; the selection stage (dispFirstMin, dispSecondMin, dispChecks) reduces the slab.  k_disparity_bm runs both, in two
// launches per batch and no host synchronisation:
//   RTOL = true    anchor = right block at column k, moving = left block at k + minD + j: rBest(k) = first minimum over j, one byte per
//                  pixel into the context's scratch image (skipped when validateRtoL < 0);
//   RTOL = false   anchor = left block at column c, moving = right block at c - minD - i: first minimum, maxError, the right-to-left test
//                  (rBest(c - best - minD) from the scratch image), texture, then the U8 or sub-pixel F32 store.
// k_disparity_border writes rangeDisparity into the pixels the reference never writes.
//
// Tile: a workgroup of 256 owns DISP_TW = 64 anchor columns x DISP_TH = 16 output rows of one pair.  It stages the rows it needs once
// (anchor: 64 + rw - 1 bytes, moving: + range - 1 more; pixels outside the image are zero and only feed costs that are never selected) and
// slides the vertical sum down the band: V += H(new row) - H(old row), where the horizontal box sum H runs along the columns in a register.
// In the cost stage a thread owns one disparity (and a column segment when range <= 128): the anchor byte is a broadcast, the moving bytes
// and the slab entries of a wave are consecutive.  In the selection stage four lanes share a column; a slab row is 258 u16 = 129 dwords,
// odd, so the 16 columns of a wave fall into different banks.  Costs fit 16 bits: 255 * 15 * 15 = 57375.  First minimum = minimum of
// (cost << 9 | disparity).
// LDS: slab 64 * 258 * 2 = 33024 B, staged rows 30 * (80 + 336) = 12480 B; 45504 B per workgroup, three workgroups per CU.
//
// Deviations from the reference (include/boofhip.h): the output view is written as a whole on every call (the result of a freshly constructed
// reference object); height < rh is refused.  Limits: rx, ry <= 7, rangeDisparity <= 256.
#include "common.h"

#define DISP_TW 64       // anchor columns per workgroup
#define DISP_TH 16       // output rows per workgroup
#define DISP_VPITCH 258  // u16 per slab row (BHIP_DISP_MAX_RANGE + 2: an odd number of dwords)
#define DISP_APITCH 80   // DISP_TW + 2 * BHIP_DISP_MAX_RADIUS, rounded up to dwords
#define DISP_MPITCH 336  // DISP_TW + 2 * BHIP_DISP_MAX_RADIUS + BHIP_DISP_MAX_RANGE - 1, rounded up to dwords
#define DISP_ROWS (DISP_TH + 2 * BHIP_DISP_MAX_RADIUS)

// BlockRowScoreSad.U8: acc + |a - b| of two pixels (one v_sad_u8: the upper three bytes of a and b are zero)
struct DispCostSad {
	static __device__ __forceinline__ int add(int acc, unsigned int a, unsigned int b) { return (int)__builtin_amdgcn_sad_u8(a, b, (unsigned int)acc); }
};

struct DispKernelParams {
	const uint8_t* left;
	const uint8_t* right;
	long long lImageStride, rImageStride;
	int lStride, rStride, w, h;
	DispBmParams c;
	uint8_t* rtol;   // [batch][h][w]: rBest of the right block that starts at column x, rows ry .. h-ry-1
	void* out;
	long long oImageStride;
	int oStride;
};

// Rows y0 .. y0+rows-1, columns x0 .. x0+count-1 of a GrayU8 view into dst (row pitch `pitch`, column x0 at dst[0]); the caller has zeroed dst,
// columns outside the image stay zero.  A row segment starts at any byte address: it is read as the aligned dwords that lie inside it and
// byte by byte at its head and tail, never a byte outside the view.
__device__ __forceinline__ void dispStage(uint8_t* dst, int pitch, const uint8_t* img, int stride, int w, int y0, int rows, int x0, int count) {
	const int xs = max(x0, 0), xe = min(x0 + count, w);
	const int len = xe - xs;
	if (len <= 0) return;
	const int slots = (len + 3) / 4 + 1;
	for (int s = threadIdx.x; s < rows * slots; s += 256) {
		const int r = s / slots, k = s - r * slots;
		const uint8_t* a = img + (long long)(y0 + r) * stride + xs;
		const int o = 4 * k - (int)((uintptr_t)a & 3);   // the slot's first byte, relative to the segment
		if (o >= len) continue;
		uint8_t* d = dst + r * pitch + (xs - x0);
		if (o >= 0 && o + 4 <= len) {
			const unsigned int v = *(const unsigned int*)(a + o);
			d[o] = (uint8_t)v;
			d[o + 1] = (uint8_t)(v >> 8);
			d[o + 2] = (uint8_t)(v >> 16);
			d[o + 3] = (uint8_t)(v >> 24);
		} else {
#pragma unroll
			for (int j = 0; j < 4; j++)
				if (o + j >= 0 && o + j < len) d[o + j] = a[o + j];
		}
	}
}

// Cost stage, one staged row pair into the slab entries (columns c0 .. c0+cs-1, disparity s) of the calling thread:
// v[col] += H(an, mn)(col) - H(ao, mo)(col), H(col) = sum_{j<rw} cost(a[col + j], m[col + j]); HASOLD = false adds only.
template <class Cost, bool HASOLD>
__device__ __forceinline__ void dispCostRow(unsigned short* v, const uint8_t* an, const uint8_t* mn, const uint8_t* ao, const uint8_t* mo, int c0, int cs, int rw) {
	int hsum = 0;
	for (int j = 0; j < rw; j++) {
		const int x = c0 + j;
		hsum = Cost::add(hsum, an[x], mn[x]);
		if constexpr (HASOLD) hsum -= Cost::add(0, ao[x], mo[x]);
	}
	*v = (unsigned short)(*v + hsum);
	for (int col = c0 + 1; col < c0 + cs; col++) {
		const int x0 = col - 1, x1 = col + rw - 1;
		hsum = Cost::add(hsum, an[x1], mn[x1]) - Cost::add(0, an[x0], mn[x0]);
		if constexpr (HASOLD) hsum += Cost::add(0, ao[x0], mo[x0]) - Cost::add(0, ao[x1], mo[x1]);
		v += DISP_VPITCH;
		*v = (unsigned short)(*v + hsum);
	}
}

// Selection stage, four lanes (q = 0..3) per slab row vc: the first minimum of vc[0 .. lm-1] as (cost << 9 | index); every lane gets it.
__device__ __forceinline__ unsigned int dispFirstMin(const unsigned short* vc, int lm, int q) {
	unsigned int key = 0xFFFFFFFFu;
	for (int i = q; i < lm; i += 4) key = min(key, ((unsigned int)vc[i] << 9) | (unsigned int)i);
	key = min(key, (unsigned int)__shfl_xor((int)key, 1, 64));
	key = min(key, (unsigned int)__shfl_xor((int)key, 2, 64));
	return key;
}
// the smallest cost outside best-1 .. best+1 (Integer.MAX_VALUE when there is none); `on` is uniform over the four lanes
__device__ __forceinline__ int dispSecondMin(const unsigned short* vc, int lm, int q, int best, bool on) {
	int second = 2147483647;
	if (on)
		for (int i = q; i < lm; i += 4)
			if (i < best - 1 || i > best + 1) second = min(second, (int)vc[i]);
	second = min(second, __shfl_xor(second, 1, 64));
	second = min(second, __shfl_xor(second, 2, 64));
	return second;
}

// SelectErrorWithChecks_S32.process for one left block column (lane q == 0 of its four): returns the disparity or `inv`
__device__ __forceinline__ int dispChecks(const DispBmParams& c, int best, int sBest, int second, int lm, int rBest) {
	const int inv = c.range + 1;
	int d = best;
	if (sBest > c.maxError) {
		d = inv;
	} else if (c.rtolTol >= 0) {
		if (abs(rBest - best) > c.rtolTol) d = inv;
	}
	if (c.textureThr > 0 && d != inv && lm >= 3) {
		// Java int products, which wrap: evaluated in unsigned arithmetic and read back as two's complement
		const unsigned int lhs = 10000u * (unsigned int)(second - sBest), rhs = (unsigned int)c.textureThr * (unsigned int)sBest;
		if ((int)lhs <= (int)rhs) d = inv;
	}
	return d;
}

template <class Cost, bool RTOL, class OutT>
__global__ __launch_bounds__(256) void k_disparity_bm(DispKernelParams P) {
	__shared__ __attribute__((aligned(16))) unsigned short V[DISP_TW * DISP_VPITCH];
	__shared__ __attribute__((aligned(16))) uint8_t sa[DISP_ROWS * DISP_APITCH];
	__shared__ __attribute__((aligned(16))) uint8_t sm[DISP_ROWS * DISP_MPITCH];
	const DispBmParams& c = P.c;
	const int w = P.w, h = P.h, S = c.range, rw = 2 * c.rx + 1, rh = 2 * c.ry + 1;
	const long long b = blockIdx.z;
	const uint8_t* L = P.left + b * P.lImageStride;
	const uint8_t* R = P.right + b * P.rImageStride;
	const int a0 = (RTOL ? 0 : c.minD) + blockIdx.x * DISP_TW;   // block start column of the tile's first anchor
	const int yb0 = c.ry + blockIdx.y * DISP_TH, yb1 = min(yb0 + DISP_TH, h - c.ry);
	const int nrows = yb1 - yb0 + 2 * c.ry;                       // staged image rows yb0 - ry ..
	const int acount = DISP_TW + rw - 1, mcount = acount + S - 1;
	const int m0 = RTOL ? a0 + c.minD : a0 - c.minD - (S - 1);    // image column of sm[0]
	for (int i = threadIdx.x; i < DISP_ROWS * DISP_APITCH / 4; i += 256) ((unsigned int*)sa)[i] = 0u;
	for (int i = threadIdx.x; i < DISP_ROWS * DISP_MPITCH / 4; i += 256) ((unsigned int*)sm)[i] = 0u;
	__syncthreads();
	dispStage(sa, DISP_APITCH, RTOL ? R : L, RTOL ? P.rStride : P.lStride, w, yb0 - c.ry, nrows, a0, acount);
	dispStage(sm, DISP_MPITCH, RTOL ? L : R, RTOL ? P.lStride : P.rStride, w, yb0 - c.ry, nrows, m0, mcount);
	__syncthreads();
	// cost stage: thread = (column segment, disparity s); the moving pixel of anchor column x is sm[x + mofs]
	const int sp = S <= 64 ? 64 : S <= 128 ? 128 : 256;
	const int s = threadIdx.x & (sp - 1), seg = threadIdx.x / sp, cs = DISP_TW * sp / 256;
	const int mofs = RTOL ? s : S - 1 - s;
	unsigned short* vmine = V + seg * cs * DISP_VPITCH + s;
	// selection stage: thread = (column, quarter)
	const int col = threadIdx.x >> 2, q = threadIdx.x & 3;
	const int x = a0 + col;
	const unsigned short* vc = V + col * DISP_VPITCH;
	int lm = 0;   // disparities to search; 0: no block starts here
	if constexpr (RTOL) {
		if (x <= w - rw - c.minD) lm = max(min(w - rw, x + c.minD + S) - x - c.minD, 1);   // selectRightToLeft: j = 0, then 1 <= j < localMax
	} else {
		if (x <= w - rw) lm = min(x - c.minD + 1, S);                                         // maxDisparityAtColumnL2R
	}
	for (int y = yb0; y < yb1; y++) {
		const int r0 = y - yb0;   // staged index of image row y - ry
		if (s < S) {
			if (y == yb0) {
				for (int k = 0; k < cs; k++) vmine[k * DISP_VPITCH] = 0;
				for (int d = 0; d < rh; d++)
					dispCostRow<Cost, false>(vmine, sa + (r0 + d) * DISP_APITCH, sm + (r0 + d) * DISP_MPITCH + mofs, nullptr, nullptr, seg * cs, cs, rw);
			} else {
				dispCostRow<Cost, true>(vmine, sa + (r0 + rh - 1) * DISP_APITCH, sm + (r0 + rh - 1) * DISP_MPITCH + mofs, sa + (r0 - 1) * DISP_APITCH,
										sm + (r0 - 1) * DISP_MPITCH + mofs, seg * cs, cs, rw);
			}
		}
		__syncthreads();
		const unsigned int key = dispFirstMin(vc, lm, q);
		const int best = (int)(key & 511u), sBest = (int)(key >> 9);
		if constexpr (RTOL) {
			if (lm > 0 && q == 0) P.rtol[(b * h + y) * w + x] = (uint8_t)best;
		} else {
			const int second = dispSecondMin(vc, lm, q, best, c.textureThr > 0 && lm >= 3);
			if (lm > 0 && q == 0) {
				int rBest = 0;
				if (c.rtolTol >= 0 && sBest <= c.maxError) rBest = P.rtol[(b * h + y) * w + (x - best - c.minD)];
				const int d = dispChecks(c, best, sBest, second, lm, rBest);
				OutT* o = (OutT*)P.out + b * P.oImageStride + (long long)y * P.oStride + (x + c.rx);
				if constexpr (sizeof(OutT) == 1) {
					*o = (OutT)d;   // (byte)value
				} else {
					float f = (float)d;
					if (d > 0 && d < lm - 1) {   // the rejection value range + 1 is >= lm - 1
						const int c0 = vc[d - 1], c1 = vc[d], c2 = vc[d + 1];
						const float offset = (float)(c0 - c2) / (float)(2 * (c0 - 2 * c1 + c2));   // > 0: c1 is the first strict minimum
						f = (float)d + offset;
					}
					*o = f;
				}
			}
		}
		__syncthreads();
	}
}

// rows < y0 and >= y1, columns < x0 and >= x1: the pixels DisparityScoreBM_S32 never writes
template <class OutT>
__global__ __launch_bounds__(256) void k_disparity_border(OutT* out, long long imageStride, int stride, int w, int h, int x0, int x1, int y0, int y1, OutT value) {
	const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (x >= w || y >= h) return;
	if (x < x0 || x >= x1 || y < y0 || y >= y1) out[(long long)blockIdx.z * imageStride + (long long)y * stride + x] = value;
}

size_t bhip_disparity_scratch(int width, int height, int batch) { return (size_t)width * height * batch; }

template <class OutT>
int bhip_launch_disparity_bm(bhip_ctx* ctx, DevImg<const uint8_t> left, DevImg<const uint8_t> right, const DispBmParams& c, uint8_t* scratch, DevImg<OutT> out) {
	const int w = left.width, h = left.height, batch = left.batch;
	const int rw = 2 * c.rx + 1, rh = 2 * c.ry + 1;
	if (batch <= 0 || w <= 0 || h <= 0) return BHIP_OK;
	if (c.rx < 0 || c.ry < 0 || c.rx > BHIP_DISP_MAX_RADIUS || c.ry > BHIP_DISP_MAX_RADIUS || c.range < 1 || c.range > BHIP_DISP_MAX_RANGE || c.minD < 0 ||
		c.minD + c.range > w - 2 * c.rx || h < rh)
		return bhip_fail(ctx, BHIP_ERR_INVALID, "bhip_launch_disparity_bm: outside the kernel's limits");
	DispKernelParams P{left.data, right.data, left.imageStride, right.imageStride, left.stride, right.stride, w, h, c, scratch, out.data, out.imageStride, out.stride};
	const dim3 grid((w - rw - c.minD + 1 + DISP_TW - 1) / DISP_TW, (h - 2 * c.ry + DISP_TH - 1) / DISP_TH, batch);
	const double px = (double)w * h * batch, ops = px * c.range;
	{
		ProfScope ps(ctx, "k_disparity_border", 0);
		hipLaunchKernelGGL(k_disparity_border<OutT>, dim3((w + 63) / 64, (h + 3) / 4, batch), dim3(256), 0, ctx->stream, out.data, out.imageStride, out.stride, w, h,
						   c.rx + c.minD, w - c.rx, c.ry, h - c.ry, (OutT)c.range);
	}
	if (c.rtolTol >= 0) {
		ProfScope ps(ctx, "k_disparity_rtol", 3.0 * px, ops);
		hipLaunchKernelGGL((k_disparity_bm<DispCostSad, true, uint8_t>), grid, dim3(256), 0, ctx->stream, P);
	}
	{
		ProfScope ps(ctx, sizeof(OutT) == 1 ? "k_disparity_bm_u8" : "k_disparity_bm_f32", (2.0 + sizeof(OutT) + (c.rtolTol >= 0 ? 1.0 : 0.0)) * px, ops);
		hipLaunchKernelGGL((k_disparity_bm<DispCostSad, false, OutT>), grid, dim3(256), 0, ctx->stream, P);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_disparity_bm(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, const DispBmParams&, uint8_t*, DevImg<uint8_t>);
template int bhip_launch_disparity_bm(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, const DispBmParams&, uint8_t*, DevImg<float>);
