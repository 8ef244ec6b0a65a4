// Dense stereo disparity by block matching on GrayU8 pairs: FactoryStereoDisparity.blockMatch(ConfigDisparityBM, GrayU8, GrayU8 | GrayF32), errorType = SAD
// on the pair itself, errorType = CENSUS on the census images of the pair (census.hip).  FactoryStereoDisparity.blockMatchBest5, the five-region
// form of both: k_disparity_bm5 in the second half of this file, on the same stages.
//
// Reference (F: = main/boofcv-feature/src/main/java/boofcv/):
//   DisparityBlockMatchRowFormat.process              F:alg/feature/disparity/DisparityBlockMatchRowFormat.java:95-107
//   DisparityScoreBM_S32 (running row / column sums)  F:alg/feature/disparity/block/score/DisparityScoreBM_S32.java:73-205
//   BlockRowScore.ArrayS32.scoreRow, BlockRowScoreSad.U8   F:alg/feature/disparity/block/BlockRowScore.java:96-138, BlockRowScoreSad.java:53-67
//   SelectErrorWithChecks_S32.process / selectRightToLeft  F:alg/feature/disparity/block/select/SelectErrorWithChecks_S32.java:73-162
//   SelectErrorWithChecks_S32.DispU8.setDisparity     :172-190        SelectErrorSubpixel.S32_F32.setDisparity   SelectErrorSubpixel.java:46-75
//   WrapBaseBlockMatch.process (the fill value)       F:abst/feature/disparity/WrapBaseBlockMatch.java:42-85
//   BlockRowScoreCensus.U8 / S32 / S64 (CENSUS)       F:alg/feature/disparity/block/BlockRowScoreCensus.java:39-85; DescriptorDistance.hamming   F:alg/descriptor/DescriptorDistance.java:213-224
//   WrapDisparityBlockMatchCensus._process            F:abst/feature/disparity/WrapDisparityBlockMatchCensus.java:55-63
//
// With rw = 2*rx+1, rh = 2*ry+1 the cost of the left block that starts at column c against the right block that starts at c - minD - i is
//   C(y,c,i) = sum_{dy=-ry..ry} sum_{j<rw} |L[y+dy][c+j] - R[y+dy][c-minD-i+j]|        (int; integers make the reference's running sums exact)
// for i < lm = min(c - minD + 1, range); the result goes to pixel (c + rx, y).  Selection, checks and the sub-pixel rule: include/boofhip.h.
// CENSUS: L and R are the census images and |a - b| is hamming(a ^ b); everything after the cost is the same code (the reference builds the
// same DisparityScoreBM_S32 and S32 selector on the census images).
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
// Census words (the Cost's Elem): the staged rows hold words instead of pixels, the slab is the same (costs <= 64 * 15 * 15 = 14400).
//   BLOCK_3_3, GrayU8 words    1-byte elements: the SAD geometry and budget, 45504 B, three workgroups per CU.
//   BLOCK_5_5, GrayS32 words   4-byte elements.  30 staged rows would take 30 * 416 * 4 = 49920 B + the slab = 82944 B: one workgroup per CU
//                              (160 KiB).  The band is cut to DISP_ROWS_W32 = 22 staged rows instead, 22 - 2*ry output rows per workgroup (16 at
//                              the default ry = 3, 8 at ry = 7): 22 * 416 * 4 = 36608 B + 33024 B = 69632 B, two workgroups per CU.  The price
//                              is the first row of a band, which sums rh rows where a later row adds one and drops one: (rh + 2 * (th - 1)) / th
//                              row costs per output row, 2.3 at ry = 3 as for SAD, 3.6 at ry = 7 (SAD: 2.8).
//   GrayS64 words              folded to their low 32 bits, which carry all the information (census.hip: a word is the sign extension of its
//                              low word): the census stage writes 4-byte words, the cost is popc(x) + 32 * (x >> 31) -- bits 0..30 count once,
//                              bit 31 stands for the 33 bits 31..63 -- and the geometry is that of GrayS32.  8-byte elements would need
//                              22 * 416 * 8 + 33024 = 106240 B, one workgroup per CU, and twice the scratch traffic for nothing.
// The SAD instantiations compile to the instructions they had before the cost became a type with an element (checked on the assembly).
//
// Deviations from the reference (include/boofhip.h): the output view is written as a whole on every call (the result of a freshly constructed
// reference object); height < rh is refused.  Limits: rx, ry <= 7, rangeDisparity <= 256.  CENSUS: the census images are context scratch.
#include "common.h"

#define DISP_TW 64       // anchor columns per workgroup
#define DISP_TH 16       // output rows per workgroup
#define DISP_VPITCH 258  // u16 per slab row (BHIP_DISP_MAX_RANGE + 2: an odd number of dwords)
#define DISP_APITCH 80   // DISP_TW + 2 * BHIP_DISP_MAX_RADIUS, rounded up to dwords
#define DISP_MPITCH 336  // DISP_TW + 2 * BHIP_DISP_MAX_RADIUS + BHIP_DISP_MAX_RANGE - 1, rounded up to dwords
#define DISP_ROWS (DISP_TH + 2 * BHIP_DISP_MAX_RADIUS)

#define DISP_ROWS_W32 22  // staged rows of a cost with 32-bit elements: 22 - 2 * ry output rows per workgroup (16 at the default radius 3, 8 at radius 7)

// A cost: Elem, the staged element; ROWS, the staged rows per workgroup (DISP_ROWS: the fixed DISP_TH output rows; fewer: ROWS - 2 * ry output rows);
// add(acc, a, b) = acc + the cost of two elements.
// BlockRowScoreSad.U8: acc + |a - b| of two pixels (one v_sad_u8: the upper three bytes of a and b are zero)
struct DispCostSad {
	using Elem = uint8_t;
	static constexpr int ROWS = DISP_ROWS;
	static __device__ __forceinline__ int add(int acc, unsigned int a, unsigned int b) { return (int)__builtin_amdgcn_sad_u8(a, b, (unsigned int)acc); }
};
// BlockRowScoreCensus.U8 / S32: acc + DescriptorDistance.hamming(a ^ b) of two census words (3x3: 8 bits, 5x5: 24 bits)
struct DispCostCensus8 {
	using Elem = uint8_t;
	static constexpr int ROWS = DISP_ROWS;
	static __device__ __forceinline__ int add(int acc, unsigned int a, unsigned int b) { return acc + __popc(a ^ b); }
};
struct DispCostCensus32 {
	using Elem = uint32_t;
	static constexpr int ROWS = DISP_ROWS_W32;
	static __device__ __forceinline__ int add(int acc, unsigned int a, unsigned int b) { return acc + __popc(a ^ b); }
};
// BlockRowScoreCensus.S64 on the low 32 bits of the words: a GrayS64 census word is the sign extension of its low word (census.hip), so
// hamming(long) of the xor is the bits that differ among 0..30, plus 33 (bits 31..63) when the sample-31 bits differ: popc(x) + 32 * bit 31
struct DispCostCensus64 {
	using Elem = uint32_t;
	static constexpr int ROWS = DISP_ROWS_W32;
	static __device__ __forceinline__ int add(int acc, unsigned int a, unsigned int b) {
		const unsigned int x = a ^ b;
		return acc + __popc(x) + (int)((x >> 31) << 5);
	}
};
// output rows per workgroup
template <class Cost>
__host__ __device__ __forceinline__ int dispTileRows(int ry) {
	if constexpr (Cost::ROWS == DISP_ROWS) return DISP_TH;
	else return Cost::ROWS - 2 * ry;
}

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

// The same for a dense, aligned image of 32-bit census words (context scratch): one element per load
__device__ __forceinline__ void dispStage(uint32_t* dst, int pitch, const uint32_t* img, int stride, int w, int y0, int rows, int x0, int count) {
	const int xs = max(x0, 0), xe = min(x0 + count, w);
	const int len = xe - xs;
	if (len <= 0) return;
	for (int s = threadIdx.x; s < rows * len; s += 256) {
		const int r = s / len, k = s - r * len;
		dst[r * pitch + (xs - x0) + k] = img[(long long)(y0 + r) * stride + xs + k];
	}
}

// Cost stage, one staged row pair into the slab entries (columns c0 .. c0+cs-1, disparity s) of the calling thread:
// v[col] += H(an, mn)(col) - H(ao, mo)(col), H(col) = sum_{j<rw} cost(a[col + j], m[col + j]); HASOLD = false adds only.  VPITCH: u16 per slab row.
template <class Cost, bool HASOLD, int VPITCH = DISP_VPITCH>
__device__ __forceinline__ void dispCostRow(unsigned short* v, const typename Cost::Elem* an, const typename Cost::Elem* mn, const typename Cost::Elem* ao,
											const typename Cost::Elem* mo, int c0, int cs, int rw) {
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
		v += VPITCH;
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
	using Elem = typename Cost::Elem;
	__shared__ __attribute__((aligned(16))) Elem sa[Cost::ROWS * DISP_APITCH];
	__shared__ __attribute__((aligned(16))) Elem sm[Cost::ROWS * DISP_MPITCH];
	const DispBmParams& c = P.c;
	const int w = P.w, h = P.h, S = c.range, rw = 2 * c.rx + 1, rh = 2 * c.ry + 1;
	const long long b = blockIdx.z;
	const Elem* L = (const Elem*)P.left + b * P.lImageStride;
	const Elem* R = (const Elem*)P.right + b * P.rImageStride;
	const int a0 = (RTOL ? 0 : c.minD) + blockIdx.x * DISP_TW;   // block start column of the tile's first anchor
	const int th = dispTileRows<Cost>(c.ry);
	const int yb0 = c.ry + blockIdx.y * th, yb1 = min(yb0 + th, h - c.ry);
	const int nrows = yb1 - yb0 + 2 * c.ry;                       // staged image rows yb0 - ry ..
	const int acount = DISP_TW + rw - 1, mcount = acount + S - 1;
	const int m0 = RTOL ? a0 + c.minD : a0 - c.minD - (S - 1);    // image column of sm[0]
	for (int i = threadIdx.x; i < Cost::ROWS * DISP_APITCH * (int)sizeof(Elem) / 4; i += 256) ((unsigned int*)sa)[i] = 0u;
	for (int i = threadIdx.x; i < Cost::ROWS * DISP_MPITCH * (int)sizeof(Elem) / 4; i += 256) ((unsigned int*)sm)[i] = 0u;
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

// the launches of one batch on images of Cost::Elem (the GrayU8 pair, or its two census images): border fill, right-to-left minima, selection
template <class Cost, class OutT>
static int dispLaunch(bhip_ctx* ctx, const char* what, DevImg<const typename Cost::Elem> left, DevImg<const typename Cost::Elem> right, const DispBmParams& c,
					  uint8_t* rtol, DevImg<OutT> out) {
	const int w = left.width, h = left.height, batch = left.batch;
	const int rw = 2 * c.rx + 1, rh = 2 * c.ry + 1;
	if (batch <= 0 || w <= 0 || h <= 0) return BHIP_OK;
	if (c.rx < 0 || c.ry < 0 || c.rx > BHIP_DISP_MAX_RADIUS || c.ry > BHIP_DISP_MAX_RADIUS || c.range < 1 || c.range > BHIP_DISP_MAX_RANGE || c.minD < 0 ||
		c.minD + c.range > w - 2 * c.rx || h < rh)
		return bhip_fail(ctx, BHIP_ERR_INVALID, std::string(what) + ": outside the kernel's limits");
	DispKernelParams P{(const uint8_t*)left.data, (const uint8_t*)right.data, left.imageStride, right.imageStride, left.stride, right.stride, w, h, c, rtol,
					   out.data, out.imageStride, out.stride};
	const int th = dispTileRows<Cost>(c.ry);
	const dim3 grid((w - rw - c.minD + 1 + DISP_TW - 1) / DISP_TW, (h - 2 * c.ry + th - 1) / th, batch);
	const double px = (double)w * h * batch, ops = px * c.range, eb = sizeof(typename Cost::Elem);
	{
		ProfScope ps(ctx, "k_disparity_border", 0);
		hipLaunchKernelGGL(k_disparity_border<OutT>, dim3((w + 63) / 64, (h + 3) / 4, batch), dim3(256), 0, ctx->stream, out.data, out.imageStride, out.stride, w, h,
						   c.rx + c.minD, w - c.rx, c.ry, h - c.ry, (OutT)c.range);
	}
	if (c.rtolTol >= 0) {
		ProfScope ps(ctx, "k_disparity_rtol", (2.0 * eb + 1.0) * px, ops);
		hipLaunchKernelGGL((k_disparity_bm<Cost, true, uint8_t>), grid, dim3(256), 0, ctx->stream, P);
	}
	{
		ProfScope ps(ctx, sizeof(OutT) == 1 ? "k_disparity_bm_u8" : "k_disparity_bm_f32", (2.0 * eb + sizeof(OutT) + (c.rtolTol >= 0 ? 1.0 : 0.0)) * px, ops);
		hipLaunchKernelGGL((k_disparity_bm<Cost, false, OutT>), grid, dim3(256), 0, ctx->stream, P);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

template <class OutT>
int bhip_launch_disparity_bm(bhip_ctx* ctx, DevImg<const uint8_t> left, DevImg<const uint8_t> right, const DispBmParams& c, uint8_t* scratch, DevImg<OutT> out) {
	return dispLaunch<DispCostSad, OutT>(ctx, "bhip_launch_disparity_bm", left, right, c, scratch, out);
}
template int bhip_launch_disparity_bm(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, const DispBmParams&, uint8_t*, DevImg<uint8_t>);
template int bhip_launch_disparity_bm(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, const DispBmParams&, uint8_t*, DevImg<float>);

// scratch of the census form: [right-to-left minima, one byte per pixel, rounded up to 16 B][census of the left images][census of the right images],
// the census images dense, in 1-byte (3x3) or 4-byte (5x5; the low words of a sample list) elements
static size_t dispCensusRtolBytes(int width, int height, int batch) { return ((size_t)width * height * batch + 15) & ~(size_t)15; }
size_t bhip_disparity_census_scratch(int width, int height, int batch, int wordBytes) {
	return dispCensusRtolBytes(width, height, batch) + 2 * (size_t)width * height * batch * (wordBytes == 1 ? 1 : 4);
}

template <class Cost, class OutT>
static int disp5Launch(bhip_ctx* ctx, const char* what, DevImg<const typename Cost::Elem> left, DevImg<const typename Cost::Elem> right, const DispBmParams& c,
					   uint8_t* rtol, DevImg<OutT> out);

// FIVE: the five-region launches (blockMatchBest5) on the census images instead of the plain ones
template <class Cost, class OutT, bool FIVE = false>
static int dispCensus(bhip_ctx* ctx, DevImg<const uint8_t> left, DevImg<const uint8_t> right, const DispBmParams& c, int denseRadius, const CensusSamples* s,
					  uint8_t* scratch, DevImg<OutT> out) {
	using Elem = typename Cost::Elem;
	using Word = std::conditional_t<sizeof(Elem) == 1, uint8_t, int32_t>;   // what bhip_launch_census writes
	const int w = left.width, h = left.height, batch = left.batch;
	Elem* cl = (Elem*)(scratch + dispCensusRtolBytes(w, h, batch));
	Elem* cr = cl + (size_t)w * h * batch;
	const DevImg<Elem> dl{cl, (long long)w * h, w, w, h, batch}, dr{cr, (long long)w * h, w, w, h, batch};
	BHIP_TRY(bhip_launch_census<Word>(ctx, left, denseRadius, s, DevImg<Word>{(Word*)cl, dl.imageStride, w, w, h, batch}));
	BHIP_TRY(bhip_launch_census<Word>(ctx, right, denseRadius, s, DevImg<Word>{(Word*)cr, dr.imageStride, w, w, h, batch}));
	if constexpr (FIVE) return disp5Launch<Cost, OutT>(ctx, "bhip_launch_disparity_bm5_census", dl, dr, c, scratch, out);
	else return dispLaunch<Cost, OutT>(ctx, "bhip_launch_disparity_bm_census", dl, dr, c, scratch, out);
}

template <class OutT>
int bhip_launch_disparity_bm_census(bhip_ctx* ctx, DevImg<const uint8_t> left, DevImg<const uint8_t> right, const DispBmParams& c, int wordBytes,
									const CensusSamples* s, uint8_t* scratch, DevImg<OutT> out) {
	if (wordBytes == 1) return dispCensus<DispCostCensus8, OutT>(ctx, left, right, c, 1, nullptr, scratch, out);
	if (wordBytes == 4) return dispCensus<DispCostCensus32, OutT>(ctx, left, right, c, 2, nullptr, scratch, out);
	if (wordBytes == 8 && s) return dispCensus<DispCostCensus64, OutT>(ctx, left, right, c, 0, s, scratch, out);
	return bhip_fail(ctx, BHIP_ERR_INVALID, "bhip_launch_disparity_bm_census: no such census word");
}
template int bhip_launch_disparity_bm_census(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, const DispBmParams&, int, const CensusSamples*, uint8_t*,
											 DevImg<uint8_t>);
template int bhip_launch_disparity_bm_census(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, const DispBmParams&, int, const CensusSamples*, uint8_t*,
											 DevImg<float>);

// ---------------- five-region block matching: FactoryStereoDisparity.blockMatchBest5 ----------------
// Reference:
//   FactoryStereoDisparity.blockMatchBest5            F:factory/feature/disparity/FactoryStereoDisparity.java:146-201 (maxError * 3)
//   DisparityScoreBMBestFive_S32                      F:alg/feature/disparity/block/score/DisparityScoreBMBestFive_S32.java:147-267
//   DisparityBlockMatchBestFive (border 2 * radius)   F:alg/feature/disparity/DisparityBlockMatchBestFive.java
// With V(y, c, i) the sub-block cost C above, the score of selector column col (pixel col + 2*rx, row y) at disparity minD + i is
//   F(y, col, i) = V(y, col+rx, i) + the two smallest of { V(y-ry, col, i), V(y-ry, col+2rx, i), V(y+ry, col, i), V(y+ry, col+2rx, i) }
// (computeScoreFive's three compare() branches, compare(a, b) = Integer.compare(-a, -b)), and the selector is the S32 selector of plain block
// matching configured with radius 2*rx: columns minD .. W-(4rx+1), region width 4rx+1 in selectRightToLeft.  Output rows are
// max(2ry, 1) .. H-2ry-1: computeFirstRow selects nothing and computeRemainingRows starts at image row rh, so with ry = 0 row 0 is never
// selected (plain block matching selects it in computeFirstRow).  On the right-anchored slab Vr(k, j) = V(k + minD + j, j) a shift of col by rx
// at a fixed disparity is a shift of k by rx, so the right-to-left pass has the same five-region shape.
//
// k_disparity_bm5: a workgroup of 256 owns DISP5_TW = 32 selector columns x th output rows of one pair and keeps three u16 slabs in LDS, top =
// V(y-ry), mid = V(y), bottom = V(y+ry), each TW + 2*rx anchor columns by `range` entries.  Each slab slides down the band with
// V += H(entering row) - H(leaving row): six dispCostRow calls per output row where plain block matching has two, on th + 4*ry staged rows.
// The selection stage evaluates F from five LDS reads, in 32 bits (F <= 3 * 57375 = 172125 does not fit u16; F << 9 | i needs 27 bits), for the
// first minimum, the second minimum and the three scores of the sub-pixel fit.  Eight lanes share a column; a slab row is RC + 8 u16 = 68 or 132
// dwords, 4 mod 32, so the 8 columns x 4 dwords a wave reads fall into 32 different banks.  RC, the slab's disparity capacity, is a template
// parameter (128 or 256): the default range of 100 then runs three workgroups per CU where the full slab allows one.
//   LDS per workgroup                          RC = 128 (range <= 128)                          RC = 256
//   1-byte elements (SAD, census 3x3)          3*46*272 + 44*(60+188)   = 48448 B, 3 per CU     3*46*528 + 44*(60+316)   =  89408 B, 1 per CU
//   4-byte elements (census 5x5, S64)          3*46*272 + 32*(60+188)*4 = 69280 B, 2 per CU     3*46*528 + 32*(60+316)*4 = 120992 B, 1 per CU
// 1-byte elements: th = DISP5_TH = 16, 16 + 4*ry <= 44 staged rows.  4-byte elements: DISP5_ROWS_W32 = 32 staged rows, th = 32 - 4*ry output
// rows (20 at the default ry = 3, 4 at ry = 7).
#define DISP5_TW 32                                           // selector columns per workgroup
#define DISP5_TH 16                                           // output rows per workgroup, 1-byte elements
#define DISP5_COLS (DISP5_TW + 2 * BHIP_DISP_MAX_RADIUS)      // anchor columns of a slab
#define DISP5_APITCH (DISP5_TW + 4 * BHIP_DISP_MAX_RADIUS)    // staged anchor elements per row: TW + 2*rx + rw - 1
#define DISP5_ROWS (DISP5_TH + 4 * BHIP_DISP_MAX_RADIUS)      // staged rows, 1-byte elements
#define DISP5_ROWS_W32 32                                     // staged rows, 4-byte elements: 32 - 4 * ry output rows per workgroup
#define DISP5_LPC (256 / DISP5_TW)                            // lanes per selector column

template <class Cost>
__host__ __device__ __forceinline__ int disp5TileRows(int ry) {
	if constexpr (sizeof(typename Cost::Elem) == 1) return DISP5_TH;
	else return DISP5_ROWS_W32 - 4 * ry;
}
// first output row: DisparityScoreBMBestFive_S32 selects from image row max(rh, 4*ry) on
__host__ __device__ __forceinline__ int disp5FirstRow(int ry) { return ry ? 2 * ry : 1; }

// the five-region score of one selector column: slab rows of top / bottom at col and col + 2*rx, of mid at col + rx
struct Disp5Score {
	const unsigned short *t0, *t1, *m, *b0, *b1;
	__device__ __forceinline__ int operator()(int i) const {
		const int v0 = t0[i], v1 = t1[i], v2 = b0[i], v3 = b1[i];
		const int lo01 = min(v0, v1), hi01 = max(v0, v1), lo23 = min(v2, v3), hi23 = max(v2, v3);
		return (int)m[i] + min(lo01, lo23) + min(max(lo01, lo23), min(hi01, hi23));   // the two smallest of four
	}
};
// dispFirstMin / dispSecondMin on F, DISP5_LPC lanes (q) per column
__device__ __forceinline__ unsigned int disp5FirstMin(const Disp5Score& F, int lm, int q) {
	unsigned int key = 0xFFFFFFFFu;
	for (int i = q; i < lm; i += DISP5_LPC) key = min(key, ((unsigned int)F(i) << 9) | (unsigned int)i);
#pragma unroll
	for (int m = 1; m < DISP5_LPC; m <<= 1) key = min(key, (unsigned int)__shfl_xor((int)key, m, 64));
	return key;
}
__device__ __forceinline__ int disp5SecondMin(const Disp5Score& F, int lm, int q, int best, bool on) {
	int second = 2147483647;
	if (on)
		for (int i = q; i < lm; i += DISP5_LPC)
			if (i < best - 1 || i > best + 1) second = min(second, F(i));
#pragma unroll
	for (int m = 1; m < DISP5_LPC; m <<= 1) second = min(second, __shfl_xor(second, m, 64));
	return second;
}

template <class Cost, int RC, bool RTOL, class OutT>
__global__ __launch_bounds__(256) void k_disparity_bm5(DispKernelParams P) {
	using Elem = typename Cost::Elem;
	constexpr int VP = RC + 8, MP = DISP5_APITCH + RC, ROWS = sizeof(Elem) == 1 ? DISP5_ROWS : DISP5_ROWS_W32, SLAB = DISP5_COLS * VP;
	__shared__ __attribute__((aligned(16))) unsigned short V[3 * SLAB];   // top, mid, bottom
	__shared__ __attribute__((aligned(16))) Elem sa[ROWS * DISP5_APITCH];
	__shared__ __attribute__((aligned(16))) Elem sm[ROWS * MP];
	const DispBmParams& c = P.c;
	const int w = P.w, h = P.h, S = c.range, rx = c.rx, ry = c.ry, rw = 2 * rx + 1, rh = 2 * ry + 1, rw5 = 4 * rx + 1;
	const long long b = blockIdx.z;
	const Elem* L = (const Elem*)P.left + b * P.lImageStride;
	const Elem* R = (const Elem*)P.right + b * P.rImageStride;
	const int nc = DISP5_TW + 2 * rx;                                 // anchor columns of the slabs
	const int a0 = (RTOL ? 0 : c.minD) + blockIdx.x * DISP5_TW;       // the tile's first selector column = block start column of its first anchor
	const int th = disp5TileRows<Cost>(ry);
	const int yb0 = disp5FirstRow(ry) + blockIdx.y * th, yb1 = min(yb0 + th, h - 2 * ry);
	const int nrows = yb1 - yb0 + 4 * ry;                             // staged image rows yb0 - 2*ry ..
	const int acount = nc + rw - 1, mcount = acount + S - 1;
	const int m0 = RTOL ? a0 + c.minD : a0 - c.minD - (S - 1);        // image column of sm[0]
	for (int i = threadIdx.x; i < ROWS * DISP5_APITCH * (int)sizeof(Elem) / 4; i += 256) ((unsigned int*)sa)[i] = 0u;
	for (int i = threadIdx.x; i < ROWS * MP * (int)sizeof(Elem) / 4; i += 256) ((unsigned int*)sm)[i] = 0u;
	__syncthreads();
	dispStage(sa, DISP5_APITCH, RTOL ? R : L, RTOL ? P.rStride : P.lStride, w, yb0 - 2 * ry, nrows, a0, acount);
	dispStage(sm, MP, RTOL ? L : R, RTOL ? P.lStride : P.rStride, w, yb0 - 2 * ry, nrows, m0, mcount);
	__syncthreads();
	// cost stage: thread = (column segment, disparity s)
	const int sp = S <= 64 ? 64 : S <= 128 ? 128 : 256;
	const int s = threadIdx.x & (sp - 1), seg = threadIdx.x / sp, cs = (nc * sp + 255) / 256;
	const int cb = seg * cs, cn = min(cs, nc - cb);                   // this thread's anchor columns cb .. cb + cn - 1
	const int mofs = RTOL ? s : S - 1 - s;
	unsigned short* vt = V + cb * VP + s;
	unsigned short* vm = vt + SLAB;
	unsigned short* vb = vm + SLAB;
	// selection stage: thread = (selector column, lane q of DISP5_LPC)
	const int col = threadIdx.x / DISP5_LPC, q = threadIdx.x % DISP5_LPC;
	const int x = a0 + col;
	const Disp5Score F{V + col * VP, V + (col + 2 * rx) * VP, V + SLAB + (col + rx) * VP, V + 2 * SLAB + col * VP, V + 2 * SLAB + (col + 2 * rx) * VP};
	int lm = 0;   // disparities to search; 0: no selector column here
	if constexpr (RTOL) {
		if (x <= w - rw5 - c.minD) lm = max(min(w - rw5, x + c.minD + S) - x - c.minD, 1);   // selectRightToLeft, region width 4*rx + 1
	} else {
		if (x <= w - rw5) lm = min(x - c.minD + 1, S);                                         // maxDisparityAtColumnL2R
	}
	for (int y = yb0; y < yb1; y++) {
		const int r0 = y - yb0;   // staged index of image row y - 2*ry: top = rows r0 .. r0+2ry, mid = r0+ry .. r0+3ry, bottom = r0+2ry .. r0+4ry
		if (s < S && cn > 0) {
			if (y == yb0) {
				for (int k = 0; k < cn; k++) vt[k * VP] = vm[k * VP] = vb[k * VP] = 0;
				for (int d = 0; d < rh; d++) {
					dispCostRow<Cost, false, VP>(vt, sa + (r0 + d) * DISP5_APITCH, sm + (r0 + d) * MP + mofs, nullptr, nullptr, cb, cn, rw);
					dispCostRow<Cost, false, VP>(vm, sa + (r0 + ry + d) * DISP5_APITCH, sm + (r0 + ry + d) * MP + mofs, nullptr, nullptr, cb, cn, rw);
					dispCostRow<Cost, false, VP>(vb, sa + (r0 + 2 * ry + d) * DISP5_APITCH, sm + (r0 + 2 * ry + d) * MP + mofs, nullptr, nullptr, cb, cn, rw);
				}
			} else {
				const int nt = r0 + 2 * ry, ot = r0 - 1;   // entering and leaving row of top; mid: + ry; bottom: + 2*ry
				dispCostRow<Cost, true, VP>(vt, sa + nt * DISP5_APITCH, sm + nt * MP + mofs, sa + ot * DISP5_APITCH, sm + ot * MP + mofs, cb, cn, rw);
				dispCostRow<Cost, true, VP>(vm, sa + (nt + ry) * DISP5_APITCH, sm + (nt + ry) * MP + mofs, sa + (ot + ry) * DISP5_APITCH,
											sm + (ot + ry) * MP + mofs, cb, cn, rw);
				dispCostRow<Cost, true, VP>(vb, sa + (nt + 2 * ry) * DISP5_APITCH, sm + (nt + 2 * ry) * MP + mofs, sa + (ot + 2 * ry) * DISP5_APITCH,
											sm + (ot + 2 * ry) * MP + mofs, cb, cn, rw);
			}
		}
		__syncthreads();
		const unsigned int key = disp5FirstMin(F, lm, q);
		const int best = (int)(key & 511u), sBest = (int)(key >> 9);
		if constexpr (RTOL) {
			if (lm > 0 && q == 0) P.rtol[(b * h + y) * w + x] = (uint8_t)best;
		} else {
			const int second = disp5SecondMin(F, lm, q, best, c.textureThr > 0 && lm >= 3);
			if (lm > 0 && q == 0) {
				int rBest = 0;
				if (c.rtolTol >= 0 && sBest <= c.maxError) rBest = P.rtol[(b * h + y) * w + (x - best - c.minD)];
				const int d = dispChecks(c, best, sBest, second, lm, rBest);
				OutT* o = (OutT*)P.out + b * P.oImageStride + (long long)y * P.oStride + (x + 2 * rx);
				if constexpr (sizeof(OutT) == 1) {
					*o = (OutT)d;   // (byte)value
				} else {
					float f = (float)d;
					if (d > 0 && d < lm - 1) {   // the rejection value range + 1 is >= lm - 1
						const int c0 = F(d - 1), c1 = F(d), c2 = F(d + 1);
						const float offset = (float)(c0 - c2) / (float)(2 * (c0 - 2 * c1 + c2));
						f = (float)d + offset;
					}
					*o = f;
				}
			}
		}
		__syncthreads();
	}
}

// the launches of one batch: border fill (the whole view where no selector column or output row exists), right-to-left minima, selection
template <class Cost, int RC, class OutT>
static int disp5LaunchRC(bhip_ctx* ctx, DevImg<const typename Cost::Elem> left, DevImg<const typename Cost::Elem> right, const DispBmParams& c, uint8_t* rtol,
						 DevImg<OutT> out) {
	const int w = left.width, h = left.height, batch = left.batch;
	const int y0 = disp5FirstRow(c.ry), y1 = h - 2 * c.ry, ncol = w - (4 * c.rx + 1) - c.minD + 1;
	DispKernelParams P{(const uint8_t*)left.data, (const uint8_t*)right.data, left.imageStride, right.imageStride, left.stride, right.stride, w, h, c, rtol,
					   out.data, out.imageStride, out.stride};
	const double px = (double)w * h * batch, ops = 3.0 * px * c.range, eb = sizeof(typename Cost::Elem);
	{
		ProfScope ps(ctx, "k_disparity_border", 0);
		hipLaunchKernelGGL(k_disparity_border<OutT>, dim3((w + 63) / 64, (h + 3) / 4, batch), dim3(256), 0, ctx->stream, out.data, out.imageStride, out.stride, w, h,
						   2 * c.rx + c.minD, w - 2 * c.rx, y0, y1, (OutT)c.range);
	}
	if (ncol > 0 && y1 > y0) {
		const int th = disp5TileRows<Cost>(c.ry);
		const dim3 grid((ncol + DISP5_TW - 1) / DISP5_TW, (y1 - y0 + th - 1) / th, batch);
		if (c.rtolTol >= 0) {
			ProfScope ps(ctx, "k_disparity_bm5_rtol", (2.0 * eb + 1.0) * px, ops);
			hipLaunchKernelGGL((k_disparity_bm5<Cost, RC, true, uint8_t>), grid, dim3(256), 0, ctx->stream, P);
		}
		{
			ProfScope ps(ctx, sizeof(OutT) == 1 ? "k_disparity_bm5_u8" : "k_disparity_bm5_f32", (2.0 * eb + sizeof(OutT) + (c.rtolTol >= 0 ? 1.0 : 0.0)) * px, ops);
			hipLaunchKernelGGL((k_disparity_bm5<Cost, RC, false, OutT>), grid, dim3(256), 0, ctx->stream, P);
		}
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

template <class Cost, class OutT>
static int disp5Launch(bhip_ctx* ctx, const char* what, DevImg<const typename Cost::Elem> left, DevImg<const typename Cost::Elem> right, const DispBmParams& c,
					   uint8_t* rtol, DevImg<OutT> out) {
	const int w = left.width, h = left.height, batch = left.batch;
	if (batch <= 0 || w <= 0 || h <= 0) return BHIP_OK;
	if (c.rx < 0 || c.ry < 0 || c.rx > BHIP_DISP_MAX_RADIUS || c.ry > BHIP_DISP_MAX_RADIUS || c.range < 1 || c.range > BHIP_DISP_MAX_RANGE || c.minD < 0 ||
		c.minD + c.range > w - 2 * c.rx || h < 2 * c.ry + 1)
		return bhip_fail(ctx, BHIP_ERR_INVALID, std::string(what) + ": outside the kernel's limits");
	if (c.range <= 128) return disp5LaunchRC<Cost, 128, OutT>(ctx, left, right, c, rtol, out);
	return disp5LaunchRC<Cost, 256, OutT>(ctx, left, right, c, rtol, out);
}

template <class OutT>
int bhip_launch_disparity_bm5(bhip_ctx* ctx, DevImg<const uint8_t> left, DevImg<const uint8_t> right, const DispBmParams& c, uint8_t* scratch, DevImg<OutT> out) {
	return disp5Launch<DispCostSad, OutT>(ctx, "bhip_launch_disparity_bm5", left, right, c, scratch, out);
}
template int bhip_launch_disparity_bm5(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, const DispBmParams&, uint8_t*, DevImg<uint8_t>);
template int bhip_launch_disparity_bm5(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, const DispBmParams&, uint8_t*, DevImg<float>);

template <class OutT>
int bhip_launch_disparity_bm5_census(bhip_ctx* ctx, DevImg<const uint8_t> left, DevImg<const uint8_t> right, const DispBmParams& c, int wordBytes,
									 const CensusSamples* s, uint8_t* scratch, DevImg<OutT> out) {
	if (wordBytes == 1) return dispCensus<DispCostCensus8, OutT, true>(ctx, left, right, c, 1, nullptr, scratch, out);
	if (wordBytes == 4) return dispCensus<DispCostCensus32, OutT, true>(ctx, left, right, c, 2, nullptr, scratch, out);
	if (wordBytes == 8 && s) return dispCensus<DispCostCensus64, OutT, true>(ctx, left, right, c, 0, s, scratch, out);
	return bhip_fail(ctx, BHIP_ERR_INVALID, "bhip_launch_disparity_bm5_census: no such census word");
}
template int bhip_launch_disparity_bm5_census(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, const DispBmParams&, int, const CensusSamples*, uint8_t*,
											  DevImg<uint8_t>);
template int bhip_launch_disparity_bm5_census(bhip_ctx*, DevImg<const uint8_t>, DevImg<const uint8_t>, const DispBmParams&, int, const CensusSamples*, uint8_t*,
											  DevImg<float>);
