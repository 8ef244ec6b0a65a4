// K6 (MFMA path): batched greedy L2 association whose results are bit-identical to the reference's fp64 sequential scores.
//
// Reference: AssociateGreedy.associate  F:alg/feature/associate/AssociateGreedy.java:65-118 with
//            DescriptorDistance.euclideanSq  F:alg/descriptor/DescriptorDistance.java:55-64  (SURVEY hard part 3)
//
// The matrix cores only FILTER: they find, for every row and every column, the short list of pairs that can attain the exact minimum; the
// listed pairs (about 1.15 per row / column on SURF descriptors) are then re-scored with the reference's sequential fp64 loop and the
// reference's rules are applied to those exact values.  Because the filter only needs a rigorous error bound, not accuracy, it runs in
// fp16 (v_mfma_f32_32x32x16_f16, 16x the fp32 matrix rate) on descriptors scaled by one power of two 2^-q per call so that the largest
// squared norm lies in [1/16, 1).  q is not measured first: the prep kernel converts with the exponent q_h the previous call measured
// (AssocMfmaWork::scaleHint; 1 at first, the exponent of unit vectors) while it forms the norms, and the host accepts the run iff the
// largest norm M it read back is 0 or 4^(q_h - 2) <= M < 4^q_h.  Otherwise the call is repeated once with the measured q (largest scaled
// norm in [1/4, 1)) through k_assoc_norms + k_assoc_half.  The result does not depend on which q was used: the filter only selects.
//     a^ = fl16(2^-q a),  n_a = |2^-q a|^2 (fp32, rounded up) = hi + lo (two fp16),
//     d~(i,j) = 1 + n_a + n_b - 2 <a^_i, b^_j> -- ONE K = 80 contraction: the row holds [-2 a^ | hi lo 1 1 1 | 0...], the column [b^ | 1 1 hi lo 1 | 0...]
//   (the constant 1 keeps every score a positive float, so minima are unsigned-integer minima of the bit patterns: v_min3_u32, no NaN
//    canonicalisation, LDS / global atomicMin on the raw bits)
// Error bound (u = 2^-11, s = 2^-25 fp16 subnormal half-spacing, |a'|,|b'| < 1 after scaling; products of fp16 are exact in fp32):
//     input rounding   2[(2u + u^2)|a'||b'| + 8s(1+u)(|a'|+|b'|) + 64 s^2]   <= 9.78e-4 (n_a + n_b) + 1e-6     (double rounding f64->f32->f16: + 2^-24 rel.)
//     norm split       2^-22 (n_a + n_b) + 2^-24 ;  norm round-up 4 * 2^-24 (n_a + n_b)
//     fp32 accumulate  85 additions, <= 2^-23 relative each even if truncating: 2^-16 (1 + n_a + n_b + 2|a'||b'|) <= 2^-15 (n_a + n_b) + 1.6e-5
//   =>  |d~ - 1 - d'| <= eps(i,j) = C16 (n_a + n_b) + ABS16,   C16 = 1.03e-3,  ABS16 = 2e-5   (d' = 2^-2q d, the exact scaled distance)
//   The bound asks only for |a'|, |b'| < 1, i.e. a largest scaled norm below 1; how far below does not enter.  Line by line: input rounding
//   splits into a part proportional to |a'||b'| <= (n_a + n_b) / 2 and the subnormal part, absolute once |a'| + |b'| < 2 (32 s < 1e-6);
//   norm split and round-up are relative to n_a + n_b, the 2^-24 covers hi or lo falling into the fp16 subnormals whatever the size of n;
//   the accumulation term is relative to 1 + n_a + n_b + 2|a'||b'| and its absolute part 2^-16 < 1.6e-5 comes from the constant 1 alone.
//   A largest scaled norm in [1/16, 1/4) therefore keeps eps valid; it only lets the absolute terms weigh up to four times more against
//   the scores, i.e. a slightly longer candidate list.  The padding "norm" BIG16 likewise needs real norms < 1 and nothing else.
// Pass 1 reduces d~ to per-row and per-column minima.  Pass 2 recomputes the tiles (same instructions, same bits) and lists every pair with
//     d~(i,j) <= rowmin~(i) + band(i)   /   d~(i,j) <= colmin~(j) + band(j),     band = 2 (C16 (n + max n) + ABS16)   (>= 2 eps)
// The true row arg-min (and every exact tie of it) and the true column minimum (and every exact tie) are provably inside those lists and
// everything outside is strictly larger than the list's best.  Exact re-score + the reference's rules:
//   forward : smallest exact score, largest destination index among exact ties, inclusive maxFitError
//   backward: (i -> m) survives iff i is the only row attaining the exact minimum of column m
// Degenerate inputs (candidate list overflow, e.g. many near-equal descriptors; non-finite values) fall back to the exact VALU kernels.
//
// Layout: one 144-byte row per descriptor = 9 chunks of 8 halves (64 values + [hi lo 1 1 1 0 0 0]).  A workgroup keeps ONE column strip of
// a problem (<= 384 destination rows, fragment order) in LDS and walks its row range in wave tiles of 64 rows (two A tiles in VGPRs, the
// next tile's chunks requested one tile ahead): 20 MFMAs per 64-column step, every B fragment read from LDS feeds two of them, no barrier
// and no global traffic inside the sweep.  The norms ride in the contraction, so the epilogue is one v_min3_u32 per two scores (pass 1) or
// one compare per score (pass 2).  Column minima of the strip accumulate in LDS over all row tiles; row minima of a tile are reduced with
// DPP exchanges and meet the other strips in a global atomicMin.
// Bound: MFMA (fp16 matrix rate); algorithmic flops per pass = 2 * Ns * Nd * 64.
#include "common.h"
#include <cfloat>
#include <cmath>
#include <cstring>
#include <algorithm>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

struct AssocProblem {
	int srcOff, ns, dstOff, nd;   // rows in the src / dst descriptor buffers
	int rowBase, colBase;         // compact offsets into the per-row / per-column work arrays
};
struct AssocBlock {
	int p, row0, row1, col0, col1;   // rows [row0, row1) x columns [col0, col1) of problem p
};
struct AssocCand {
	int p, i, j, pad;
	double score;
};

#define C16 1.03e-3f
#define ABS16 2.0e-5f
#define BIG16 60000.0f     // "norm" of a row / column that does not exist: its scores can never pass a threshold (real norms are < 1)
#define ROW_CHUNKS 9       // uint4 per stored row

// LDS writes of one lane visible to the other lanes of the same wave (lock-step wave: only the memory counter has to drain)
__device__ __forceinline__ void waveSyncLds() {
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// q with max norm * 2^-2q in [1/4, 1)  (0 when there is no positive norm)
__host__ __device__ __forceinline__ int scaleExp(float maxN) {
	if (!(maxN > 0.0f)) return 0;
	int e;
	(void)frexpf(maxN, &e);
	return (e + 1) >> 1;
}
// a run scaled with 2^-q is usable: max norm * 2^-2q in [1/16, 1), or no positive norm at all.  maxN = m 2^e with m in [1/2, 1), so
// 4^(q-2) <= maxN < 4^q is 2q - 3 <= e <= 2q (integers only: the host and the device decide alike)
__host__ __device__ __forceinline__ bool scaleHolds(float maxN, int q) {
	if (!(maxN > 0.0f)) return true;
	int e;
	(void)frexpf(maxN, &e);
	return e >= 2 * q - 3 && e <= 2 * q;
}
// the filter's run is not to be used: a non-finite value, more listed pairs than the list holds, or a scale that does not fit the norms
// flags: [0] non-finite seen, [1] max norm (float bits), [2] number of listed pairs, [3] scale exponent q of this run
__host__ __device__ __forceinline__ bool assocDegenerate(const int* flags, int cap) {
	float maxN;
	memcpy(&maxN, &flags[1], 4);
	return flags[0] != 0 || flags[2] > cap || !scaleHolds(maxN, flags[3]);
}

// ---- squared norms (fp32, rounded up); flags[0] = non-finite seen, flags[1] = max norm (float bits, non-negative) ----
// 16 lanes per row, 4 consecutive values (two 16-byte loads) per lane; a lane group takes PREP_ROWS rows with all their loads in flight
#define PREP_ROWS 8
__global__ __launch_bounds__(256) void k_assoc_norms(const double* __restrict__ D, long long rows, float* __restrict__ nrm, int* __restrict__ flags) {
	const long long row0 = (((long long)blockIdx.x * 256 + threadIdx.x) >> 4) * PREP_ROWS;
	const int part = threadIdx.x & 15;
	if (row0 >= rows) return;   // whole 16-lane groups leave together
	double2 v0[PREP_ROWS], v1[PREP_ROWS];
#pragma unroll
	for (int q = 0; q < PREP_ROWS; q++) {
		const long long row = min(row0 + q, rows - 1);
		const double2* src = (const double2*)(D + row * 64 + 4 * part);
		v0[q] = src[0]; v1[q] = src[1];
	}
#pragma unroll
	for (int q = 0; q < PREP_ROWS; q++) {
		double s = (v0[q].x * v0[q].x + v0[q].y * v0[q].y) + (v1[q].x * v1[q].x + v1[q].y * v1[q].y);
#pragma unroll
		for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
		if (part == 0 && row0 + q < rows) {
			const float n = (float)s;
			const float nUp = n * (1.0f + 4.0f * 5.9604644775390625e-08f);   // rounded up: a band computed from it can only grow
			nrm[row0 + q] = nUp;
			// one hot word for the whole launch: only touch it when this row actually raises the maximum (a handful of times per launch)
			if (!(s < 1e30)) atomicOr(&flags[0], 1);  // NaN, Inf or absurdly large: use the exact path
			else if (__float_as_int(nUp) > __hip_atomic_load(&flags[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&flags[1], __float_as_int(nUp));
		}
	}
}

// ---- fp64 -> scaled fp16 rows [64 values | hi lo 1 1 1 0 0 0]; nrm is rescaled in place ----
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_assoc_half(const double* __restrict__ D, long long rows, float* __restrict__ nrm, int* __restrict__ flags,
													  _Float16* __restrict__ Hrow) {
	const long long row0 = (((long long)blockIdx.x * 256 + threadIdx.x) >> 4) * PREP_ROWS;
	const int part = threadIdx.x & 15;
	if (row0 >= rows) return;
	const int q_ = scaleExp(__int_as_float(flags[1]));
	if (blockIdx.x == 0 && threadIdx.x == 0) flags[3] = q_;   // the exponent of this run, for pass 2 and the validity checks
	double2 v0[PREP_ROWS], v1[PREP_ROWS];
#pragma unroll
	for (int q = 0; q < PREP_ROWS; q++) {
		const long long row = min(row0 + q, rows - 1);
		const double2* src = (const double2*)(D + row * 64 + 4 * part);
		v0[q] = src[0]; v1[q] = src[1];
	}
#pragma unroll
	for (int q = 0; q < PREP_ROWS; q++) {
		const long long row = row0 + q;
		if (row >= rows) break;
		_Float16* out = Hrow + row * (ROW_CHUNKS * 8);
		const h16x4 hv = {(_Float16)(float)ldexp(v0[q].x, -q_), (_Float16)(float)ldexp(v0[q].y, -q_), (_Float16)(float)ldexp(v1[q].x, -q_),
						  (_Float16)(float)ldexp(v1[q].y, -q_)};
		*(h16x4*)(out + 4 * part) = hv;
		if (part == 0) {
			const float n = ldexpf(nrm[row], -2 * q_);
			const _Float16 hi = (_Float16)n;
			const _Float16 lo = (_Float16)(n - (float)hi);
			const h16x8 e = {hi, lo, (_Float16)1.0f, (_Float16)1.0f, (_Float16)1.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
			*(h16x8*)(out + 64) = e;
			nrm[row] = n;
		}
	}
}

// ---- both steps in one pass over the descriptors, with the scale exponent q_h assumed instead of measured (flags[3], set by k_assoc_init);
// same loads, same norm expression and shuffle order as k_assoc_norms, same conversion as k_assoc_half: with q_h = q the rows, the norms
// and the flags are the bits those two kernels write.  Whether q_h fitted is decided afterwards from flags[1] (scaleHolds) ----
__global__ __launch_bounds__(256) void k_assoc_prep_hinted(const double* __restrict__ D, long long rows, int q_, float* __restrict__ nrm, int* __restrict__ flags,
															 _Float16* __restrict__ Hrow) {
	const long long row0 = (((long long)blockIdx.x * 256 + threadIdx.x) >> 4) * PREP_ROWS;
	const int part = threadIdx.x & 15;
	if (row0 >= rows) return;   // whole 16-lane groups leave together
	double2 v0[PREP_ROWS], v1[PREP_ROWS];
#pragma unroll
	for (int q = 0; q < PREP_ROWS; q++) {
		const long long row = min(row0 + q, rows - 1);
		const double2* src = (const double2*)(D + row * 64 + 4 * part);
		v0[q] = src[0]; v1[q] = src[1];
	}
#pragma unroll
	for (int q = 0; q < PREP_ROWS; q++) {
		double s = (v0[q].x * v0[q].x + v0[q].y * v0[q].y) + (v1[q].x * v1[q].x + v1[q].y * v1[q].y);
#pragma unroll
		for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
		const long long row = row0 + q;
		if (row >= rows) continue;   // the group's lanes agree (the shuffles above are done)
		_Float16* out = Hrow + row * (ROW_CHUNKS * 8);
		const h16x4 hv = {(_Float16)(float)ldexp(v0[q].x, -q_), (_Float16)(float)ldexp(v0[q].y, -q_), (_Float16)(float)ldexp(v1[q].x, -q_),
						  (_Float16)(float)ldexp(v1[q].y, -q_)};
		*(h16x4*)(out + 4 * part) = hv;
		if (part == 0) {
			const float nRaw = (float)s;
			const float nUp = nRaw * (1.0f + 4.0f * 5.9604644775390625e-08f);   // rounded up: a band computed from it can only grow
			if (!(s < 1e30)) atomicOr(&flags[0], 1);  // NaN, Inf or absurdly large: use the exact path
			else if (__float_as_int(nUp) > __hip_atomic_load(&flags[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&flags[1], __float_as_int(nUp));
			const float n = ldexpf(nUp, -2 * q_);
			const _Float16 hi = (_Float16)n;
			const _Float16 lo = (_Float16)(n - (float)hi);
			const h16x8 e = {hi, lo, (_Float16)1.0f, (_Float16)1.0f, (_Float16)1.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
			*(h16x8*)(out + 64) = e;
			nrm[row] = n;
		}
	}
}

// ---- the constants every call starts from, one launch: minima keys and exact minima at "+infinity", arg-max slots at -1, the column tie
// counts at 0 (args = [rowArg | colArg | colCnt]) and the flags words ([3] = the scale exponent the prep kernel is given, 0 otherwise) ----
// It also brings the problem and block tables over: tabSrc is the page-locked staging block itself, read through its device address, so no
// copy command stands in the stream (one costs the stream about 18 us, whatever memory it reads from); tabWords = 0: they are in place
__global__ __launch_bounds__(256) void k_assoc_init(unsigned int* __restrict__ keys, unsigned long long* __restrict__ best, int* __restrict__ args, long long nk,
													  long long colTotal, int* __restrict__ flags, int q_, const uint4* __restrict__ tabSrc, uint4* __restrict__ tabDst,
													  long long tabWords) {
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i < tabWords) tabDst[i] = tabSrc[i];
	if (i < 16) flags[i] = i == 3 ? q_ : 0;
	if (i >= nk) return;
	keys[i] = 0xFFFFFFFFu;
	best[i] = ~0ull;
	args[i] = -1;
	if (i < colTotal) args[nk + i] = 0;
}

struct MfmaArgs {
	const uint4* Hs;   // 9 chunks per row
	const uint4* Hd;
	const AssocProblem* probs;
	const AssocBlock* blocks;
	unsigned int* rowKey;
	unsigned int* colKey;
	const float* nrmS;   // scaled norms (pass 2 forms its thresholds from them, the minima keys and the largest norm)
	const float* nrmD;
	const int* flags;
	AssocCand* cand;
	int* counter;    // number of listed pairs
	int cap;
#ifdef BHIP_EXPERIMENTS
	int ablate;      // timing experiments only (BHIP_ASSOC_ABLATE): 1 no MFMA, 2 no per-step epilogue, 4 no A-fragment loads, 16 no row-minimum atomics, 32 no column-minimum flush
#endif
};

#define CAND_LDS 256   // per-wave staging slots in LDS (flushed between row tiles when half full; a 64-row tile lists about 25 pairs per strip)

// One list for both directions: a pair listed for its row also updates its column's exact minimum and vice versa, which is harmless (every
// listed pair is a real pair, and every pair that can attain a row / column minimum is listed).  Hits are rare per lane, so a hit lane
// appends with one LDS atomic; the wave flushes its staging area once, with ONE atomicAdd on the global counter (a single contended word
// sustains only ~88 atomics/us, MI355X_MICROARCH.md).  Entries that do not fit the staging area go to the global list directly.
// The staging area is full (a wave tile with several times the usual number of hits): straight to the global list.  Out of line: never on
// the hot path, and its 64-bit addressing must not cost the sweep registers.
__device__ __noinline__ void candSlow(AssocCand* cand, int* counter, int cap, int p, int rr, int col) {
	const int g = atomicAdd(counter, 1);
	if (g < cap) { AssocCand c; c.p = p; c.i = rr; c.j = col; c.pad = 0; c.score = 0; cand[g] = c; }
}
// one hit lane = one LDS atomic + one 8-byte LDS store.  Inlined at every accumulator register so that the pointers stay LDS pointers
// (ds_add_rtn / ds_write; as an out-of-line function it went through flat atomics and a full wait at entry: 0.08 ms of pass 2)
__device__ __forceinline__ void candAdd(const MfmaArgs& A, int2* buf, int* cnt, bool hit, int p, int rr, int col) {
	if (hit) {
		const int pos = atomicAdd(cnt, 1);
		if (pos < CAND_LDS) buf[pos] = make_int2(rr, col);
		else candSlow(A.cand, A.counter, A.cap, p, rr, col);
	}
}
__device__ __forceinline__ void candFlush(const MfmaArgs& A, const int2* buf, const int* cnt, int p, int lane) {
	waveSyncLds();
	const int n = min(*cnt, CAND_LDS);
	if (n == 0) return;
	int base = 0;
	if (lane == 0) base = atomicAdd(A.counter, n);
	base = __builtin_amdgcn_readfirstlane(base);
	for (int k = lane; k < n; k += 64) {
		if (base + k < A.cap) {
			const int2 v = buf[k];
			AssocCand c; c.p = p; c.i = v.x; c.j = v.y; c.pad = 0; c.score = 0;
			A.cand[base + k] = c;
		}
	}
}

__device__ __forceinline__ h16x8 asHalf8(uint4 v) { return __builtin_bit_cast(h16x8, v); }
__device__ __forceinline__ uint4 extChunk(float n0, float n1, float n2, float n3) {   // [n0 n1 n2 n3 1 0 0 0] as halves
	const h16x8 h = {(_Float16)n0, (_Float16)n1, (_Float16)n2, (_Float16)n3, (_Float16)1.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
	return __builtin_bit_cast(uint4, h);
}

// B-stationary: a workgroup stages ONE column strip of a problem (<= STRIP_COLS destination rows, fragment order, 5.3 KB per 32 columns)
// in LDS and then walks its row range in wave tiles of 64 rows -- no barrier and no global traffic inside the sweep except the A fragments
// of the next tile.  The column minima of the strip accumulate in LDS over all row tiles and leave with one atomic per column.
// BHIP_ASSOC_PEEL: the sweep's single last column tile of an odd tile count is a step of its own, so that the steps with two tiles have no
// branch between their MFMAs and no accumulator set-up (pass 1 0.274 -> 0.256 ms, pass 2 0.442 -> 0.419 ms at 256 x 2150 key points;
// DESIGN.md, "association: one-pass prep").  -DBHIP_ASSOC_PEEL=0 (BHIP_EXP_DEFS of build.py) builds the single loop for A/B runs.
#ifndef BHIP_ASSOC_PEEL
#define BHIP_ASSOC_PEEL 1
#endif
#define STRIP_COLS 384
#define STRIP_TILES (STRIP_COLS / 32)
template <int PASS>
__global__ __launch_bounds__(256, 2) void k_assoc_mfma(MfmaArgs A) {
	// B tiles: [tile][chunk * 33 + column]; chunk 8 = [1 1 hi lo 1 ..], chunk 9 = zeros (k = 72..79, read by the upper half-wave)
	__shared__ uint4 tileB[STRIP_TILES][10 * 33];
	__shared__ unsigned int colLds[STRIP_COLS];       // PASS 1: column minima over this block's rows ; PASS 2: column thresholds (float bits)
	__shared__ float rowThrLds[PASS == 2 ? 4 : 1][64];   // PASS 2: thresholds of the wave's current 64 rows
	__shared__ int2 candLds[PASS == 2 ? 4 : 1][PASS == 2 ? CAND_LDS : 1];
	__shared__ int candCnt[4];
	const AssocBlock B = A.blocks[blockIdx.x];
	if (B.col0 >= B.col1) return;   // padding entry of the block table
	const AssocProblem P = A.probs[B.p];
	const int tid = threadIdx.x;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
	const int r = lane & 31, h = lane >> 5;
	const int ncol = B.col1 - B.col0;
	const int ntile = (ncol + 31) >> 5;
	int2* candBuf = candLds[PASS == 2 ? wave : 0];
	int* candN = &candCnt[wave];
	if (lane == 0) *candN = 0;

	// ---- stage the strip: consecutive threads fetch consecutive 16-byte chunks of a destination row (9 per row), four requests per
	// thread in flight before the first LDS store ----
	for (int g0 = tid; g0 < ntile * 32 * ROW_CHUNKS; g0 += 4 * 256) {
		uint4 v[4];
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const int g = g0 + 256 * q;
			const int cl = g / ROW_CHUNKS, ch = g - cl * ROW_CHUNKS;
			if (g < ntile * 32 * ROW_CHUNKS && cl < ncol) {
				v[q] = A.Hd[(long long)(P.dstOff + B.col0 + cl) * ROW_CHUNKS + ch];
				if (ch == 8) { const unsigned int x = v[q].x; v[q].x = v[q].y; v[q].y = x; }   // [hi lo | 1 1 | 1 ..] -> [1 1 | hi lo | 1 ..]
			} else {
				v[q] = ch == 8 ? extChunk(1.0f, 1.0f, BIG16, 0.0f) : make_uint4(0, 0, 0, 0);   // a column that does not exist scores > BIG16
			}
		}
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const int g = g0 + 256 * q;
			const int cl = g / ROW_CHUNKS, ch = g - cl * ROW_CHUNKS;
			if (g < ntile * 32 * ROW_CHUNKS) tileB[cl >> 5][ch * 33 + (cl & 31)] = v[q];
		}
	}
	for (int g = tid; g < ntile * 32; g += 256) tileB[g >> 5][9 * 33 + (g & 31)] = make_uint4(0, 0, 0, 0);
	// PASS 2: thr = min~ + band, band = 2 (C16 (norm + maxNorm) + ABS16) in scaled units; min~ still carries the +1 of the scores
	float maxN = 0.0f;
	if (PASS == 2) maxN = ldexpf(__int_as_float(A.flags[1]), -2 * A.flags[3]);
	for (int c = tid; c < ntile * 32; c += 256) {
		unsigned int v = 0xFFFFFFFFu;
		if (PASS == 2) {
			float thr = -INFINITY;
			if (c < ncol) {
				const float band = 2.0f * (C16 * (A.nrmD[P.dstOff + B.col0 + c] + maxN) + ABS16);
				thr = __uint_as_float(A.colKey[P.colBase + B.col0 + c]) + band;
			}
			v = __float_as_uint(thr);
		}
		colLds[c] = v;
	}
	__syncthreads();

	// ---- row tiles of this block's row range, 64 rows per wave and turn ----
	// A fragments: tile t, row rowT + 32 t + r; MFMA s (k = 16 s + 8 h ..) reads chunk 2 s + h, the fifth reads chunk 8 / zeros.  Raw chunks
	// of the NEXT row tile are requested before the current one is swept (their latency is of the order of a whole sweep).
	uint4 araw[2][5];
	auto loadA = [&](int rowT) {
#pragma unroll
		for (int t = 0; t < 2; t++) {
			const int row = rowT + 32 * t + r;
			if (row < B.row1) {
				const uint4* src = A.Hs + (long long)(P.srcOff + row) * ROW_CHUNKS;
#pragma unroll
				for (int s = 0; s < 4; s++) araw[t][s] = src[2 * s + h];
				araw[t][4] = h == 0 ? src[8] : make_uint4(0, 0, 0, 0);
			} else {
#pragma unroll
				for (int s = 0; s < 4; s++) araw[t][s] = make_uint4(0, 0, 0, 0);
				araw[t][4] = h == 0 ? extChunk(BIG16, 0.0f, 1.0f, 1.0f) : make_uint4(0, 0, 0, 0);
			}
		}
	};
	if (B.row0 + 64 * wave < B.row1) loadA(B.row0 + 64 * wave);
	for (int rowT = B.row0 + 64 * wave; rowT < B.row1; rowT += 256) {
		h16x8 a[2][5];
#pragma unroll
		for (int t = 0; t < 2; t++) {
#pragma unroll
			for (int s = 0; s < 4; s++) a[t][s] = asHalf8(araw[t][s]) * (_Float16)(-2.0f);
			a[t][4] = asHalf8(araw[t][4]);
		}
		if (rowT + 256 < B.row1 && !BHIP_ABLATE(A, 4)) loadA(rowT + 256);
		// per accumulator register: C layout row = (reg&3) + 8*(reg>>2) + 4h of the tile, col = lane&31
		unsigned int rowM[32];        // PASS 1: running row minimum of accumulator register (t, g) = [16 t + g] (bit pattern of a positive float)
#pragma unroll
		for (int k = 0; k < 32; k++) rowM[k] = 0xFFFFFFFFu;
		if (PASS == 2) {
			waveSyncLds();   // the previous tile's reads of rowThrLds are over
			float thr = -INFINITY;
			if (rowT + lane < B.row1) {
				const float band = 2.0f * (C16 * (A.nrmS[P.srcOff + rowT + lane] + maxN) + ABS16);
				thr = __uint_as_float(A.rowKey[P.rowBase + rowT + lane]) + band;
			}
			rowThrLds[wave][lane] = thr;
			waveSyncLds();
		}
		// one step = column tiles ct and ct + 1.  BHIP_ASSOC_PEEL: the steps with both tiles first (`two` is a constant in the unrolled
		// round: no branch between their MFMAs, every accumulator starts from the zero operand), then the single last tile of an odd count
#pragma unroll
		for (int round = 0; round <= BHIP_ASSOC_PEEL; round++)
		for (int ct = round == 0 ? 0 : (ntile & ~1); ct < (BHIP_ASSOC_PEEL && round == 0 ? (ntile & ~1) : ntile); ct += 2) {
			const bool two = BHIP_ASSOC_PEEL ? round == 0 : ct + 1 < ntile;   // wave-uniform: an odd tile count leaves the last step with one column tile
			const int cA_ = 32 * ct + r, cB_ = cA_ + 32;
			f32x16 acc[2][2];
#pragma unroll
			for (int t = 0; t < 2; t++)
#pragma unroll
				for (int c = 0; c < 2; c++)
#pragma unroll
					for (int g = 0; g < 16; g++) acc[t][c][g] = (c == 0 || two) ? 0.0f : INFINITY;   // a missing second tile never wins a minimum / passes a threshold
#pragma unroll
			for (int s = 0; s < 5 && !BHIP_ABLATE(A, 1); s++) {
				const int ch = s < 4 ? 2 * s + h : 8 + h;
				const h16x8 b0 = asHalf8(tileB[ct][ch * 33 + r]);
				acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0][s], b0, acc[0][0], 0, 0, 0);
				acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1][s], b0, acc[1][0], 0, 0, 0);
				if (two) {
					const h16x8 b1 = asHalf8(tileB[ct + 1][ch * 33 + r]);
					acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0][s], b1, acc[0][1], 0, 0, 0);
					acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1][s], b1, acc[1][1], 0, 0, 0);
				}
			}
			if (BHIP_ABLATE(A, 2)) continue;
			if (PASS == 1) {
				unsigned int cA = 0xFFFFFFFFu, cB = 0xFFFFFFFFu;
#pragma unroll
				for (int t = 0; t < 2; t++)
#pragma unroll
					for (int g = 0; g < 16; g++) {
						const unsigned int uA = __float_as_uint(acc[t][0][g]), uB = __float_as_uint(acc[t][1][g]);   // positive floats (+inf for a missing tile): bit order == value order
						rowM[16 * t + g] = min(rowM[16 * t + g], min(uA, uB));
						cA = min(cA, uA);
						cB = min(cB, uB);
					}
				cA = min(cA, (unsigned int)__shfl_xor((int)cA, 32, 64));
				cB = min(cB, (unsigned int)__shfl_xor((int)cB, 32, 64));
				if (h == 0) {
					atomicMin(&colLds[cA_], cA);
					if (two) atomicMin(&colLds[cB_], cB);
				}
			} else {
				const float tA = __uint_as_float(colLds[cA_]);
				const float tB = two ? __uint_as_float(colLds[cB_]) : -INFINITY;
				const int colA = B.col0 + cA_, colB = B.col0 + cB_;
#pragma unroll
				for (int t = 0; t < 2; t++)
#pragma unroll
					for (int j = 0; j < 4; j++) {
						// rows 8 j + 4 h + 0..3 of tile t = accumulator registers 4 j .. 4 j + 3: one 16-byte LDS read (same address across a half-wave)
						const float4 rv = *(const float4*)&rowThrLds[wave][32 * t + 8 * j + 4 * h];
						const float rthr[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
						for (int q = 0; q < 4; q++) {
							const int g = 4 * j + q;
							const float dA = acc[t][0][g], dB = acc[t][1][g];
							const bool rA = dA <= rthr[q], rB = dB <= rthr[q], qA = dA <= tA, qB = dB <= tB;
							if (__ballot(rA || rB || qA || qB) != 0ull) {   // wave-uniform, a few times per step
								const int rr = rowT + 32 * t + (g & 3) + 8 * (g >> 2) + 4 * h;
								candAdd(A, candBuf, candN, rA || qA, B.p, rr, colA);
								candAdd(A, candBuf, candN, rB || qB, B.p, rr, colB);
							}
						}
					}
			}
		}
		if (PASS == 1) {
#pragma unroll
			for (int k = 0; k < 32; k++) {
				// minimum over the 32 lanes of the half-wave: four DPP exchanges inside a row of 16 lanes (quad swaps, half-row and row mirror:
				// plain VALU operands, no LDS round trip) and one cross-row exchange
				unsigned int v = rowM[k];
				if (!BHIP_ABLATE(A, 64)) {
					v = min(v, (unsigned int)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
					v = min(v, (unsigned int)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
					v = min(v, (unsigned int)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
					v = min(v, (unsigned int)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
					v = min(v, (unsigned int)__shfl_xor((int)v, 16, 64));
				}
				const int rr = rowT + 32 * (k >> 4) + (k & 3) + 8 * ((k & 15) >> 2) + 4 * h;
				if (r == 0 && rr < B.row1 && !BHIP_ABLATE(A, 16)) atomicMin(&A.rowKey[P.rowBase + rr], v);
			}
		} else {
			waveSyncLds();
			if (*candN > CAND_LDS / 2) { candFlush(A, candBuf, candN, B.p, lane); waveSyncLds(); if (lane == 0) *candN = 0; waveSyncLds(); }
		}
	}
	if (PASS == 2) candFlush(A, candBuf, candN, B.p, lane);
	if (PASS == 1) {
		__syncthreads();   // every wave's LDS minima are in
		for (int c = tid; c < ncol && !BHIP_ABLATE(A, 32); c += 256) atomicMin(&A.colKey[P.colBase + B.col0 + c], colLds[c]);
	}
}

// exact sequential fp64 score of every listed pair + exact minima per row / column (scores are >= 0: bit order == value order)
__global__ __launch_bounds__(256) void k_assoc_exact(const double* __restrict__ src, const double* __restrict__ dst, const AssocProblem* __restrict__ probs,
													   AssocCand* __restrict__ cand, const int* __restrict__ counter, int cap,
													   unsigned long long* __restrict__ rowBest, unsigned long long* __restrict__ colBest) {
	const int n = min(*counter, cap);
	for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
		AssocCand* c = &cand[t];
		const AssocProblem P = probs[c->p];
		const double* a = src + (long long)(P.srcOff + c->i) * 64;
		const double* b = dst + (long long)(P.dstOff + c->j) * 64;
		double total = 0;
#pragma unroll 8
		for (int k = 0; k < 64; k++) {
			const double d = a[k] - b[k];
			total += d * d;
		}
		c->score = total;
		const unsigned long long bits = (unsigned long long)__double_as_longlong(total);
		atomicMin(&rowBest[P.rowBase + c->i], bits);
		atomicMin(&colBest[P.colBase + c->j], bits);
	}
}

// among the pairs that attain the exact minimum: largest destination index per row; count + any source index per column
__global__ __launch_bounds__(256) void k_assoc_argsel(const AssocProblem* __restrict__ probs, const AssocCand* __restrict__ cand,
														const int* __restrict__ counter, int cap, const unsigned long long* __restrict__ rowBest,
														const unsigned long long* __restrict__ colBest, int* __restrict__ rowArg, int* __restrict__ colArg,
														int* __restrict__ colCnt) {
	const int n = min(*counter, cap);
	for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
		const AssocCand c = cand[t];
		const AssocProblem P = probs[c.p];
		const unsigned long long bits = (unsigned long long)__double_as_longlong(c.score);
		if (bits == rowBest[P.rowBase + c.i]) atomicMax(&rowArg[P.rowBase + c.i], c.j);
		if (bits == colBest[P.colBase + c.j]) {
			atomicAdd(&colCnt[P.colBase + c.j], 1);
			atomicMax(&colArg[P.colBase + c.j], c.i);
		}
	}
}

__global__ __launch_bounds__(256) void k_assoc_resolve(const AssocProblem* __restrict__ probs, double maxErr, int backwards,
														 const unsigned long long* __restrict__ rowBest, const int* __restrict__ rowArg,
														 const int* __restrict__ colArg, const int* __restrict__ colCnt, const int* __restrict__ flags, int cap,
														 int* __restrict__ pairs, double* __restrict__ fit) {
	// launched before the host has seen the flags: a run the host will not use (it decides from the same words) writes nothing
	if (assocDegenerate(flags, cap)) return;
	const AssocProblem P = probs[blockIdx.y];
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P.ns; i += gridDim.x * blockDim.x) {
		const int m = rowArg[P.rowBase + i];
		const double best = __longlong_as_double((long long)rowBest[P.rowBase + i]);
		int outPair = -1;
		double outFit = maxErr;
		if (m >= 0 && best <= maxErr) {
			outPair = m;
			outFit = best;
			if (backwards) {
				if (!(colArg[P.colBase + m] == i && colCnt[P.colBase + m] == 1)) { outPair = -1; outFit = DBL_MAX; }
			}
		}
		pairs[P.srcOff + i] = outPair;
		fit[P.srcOff + i] = outFit;
	}
}

// ---------------------------------------------------------------------------------------------------------------
// Returns BHIP_OK and sets *usedMfma = 1 when the MFMA path produced the result; *usedMfma = 0 means the caller must run the exact path.
int bhip_assoc_l2_mfma_batched(bhip_ctx* ctx, AssocMfmaWork& W, const double* dev_src, const double* dev_dst, int count, const long long* srcOff,
								 const int* ns, const long long* dstOff, const int* nd, double maxErr, int backwards, int* dev_pairs, double* dev_fit,
								 int* usedMfma) {
	*usedMfma = 0;
	if (count <= 0) { *usedMfma = 1; return BHIP_OK; }
	std::vector<AssocProblem> probs(count);
	std::vector<AssocBlock> blocks;
	long long maxSrcRow = 0, maxDstRow = 0, rowTotal = 0, colTotal = 0;
	double flopsPerPass = 0;
	for (int p = 0; p < count; p++) {
		if (ns[p] <= 0 || nd[p] <= 0) return BHIP_OK;  // empty problems go through the exact path (trivial there)
		if (srcOff[p] + ns[p] > 0x7fffffffLL || dstOff[p] + nd[p] > 0x7fffffffLL) return BHIP_OK;
		probs[p] = {(int)srcOff[p], ns[p], (int)dstOff[p], nd[p], (int)rowTotal, (int)colTotal};
		maxSrcRow = std::max(maxSrcRow, srcOff[p] + ns[p]);
		maxDstRow = std::max(maxDstRow, dstOff[p] + nd[p]);
		rowTotal += ns[p];
		colTotal += nd[p];
		flopsPerPass += 2.0 * ns[p] * (double)nd[p] * 64;
		if (rowTotal > 0x3fffffffLL || colTotal > 0x3fffffffLL) return BHIP_OK;
	}
	// block table: one block per (problem, column strip of <= STRIP_COLS columns, row chunk); the rows are split only when there are too few
	// strips to fill the chip (a block then accumulates column minima over its chunk and the chunks meet in the global atomics)
	auto buildBlocks = [&]() {
		long long strips = 0;
		for (int p = 0; p < count; p++) strips += (nd[p] + STRIP_COLS - 1) / STRIP_COLS;
		int rowSplit = (int)std::max<long long>(1, (1024 + strips - 1) / strips);
		{ const char* e = getenv("BHIP_ASSOC_ROWSPLIT"); if (e && atoi(e) > 0) rowSplit = atoi(e); }   // tests: force row chunks / whole-problem sweeps
		for (int p = 0; p < count; p++) {
			int chunk = (ns[p] + rowSplit - 1) / rowSplit;
			chunk = std::max(256, ((chunk + 255) / 256) * 256);   // whole turns of the four waves
			for (int c0 = 0; c0 < nd[p]; c0 += STRIP_COLS)
				for (int r0 = 0; r0 < ns[p]; r0 += chunk) blocks.push_back({p, r0, std::min(ns[p], r0 + chunk), c0, std::min(nd[p], c0 + STRIP_COLS)});
		}
		if (count >= 16) {
			// Workgroup ids go round-robin over the 8 XCDs: give all blocks of a problem the same id residue so that its destination rows are
			// fetched into ONE XCD's L2 instead of eight (problems are dealt to the residues in turn; short queues are padded with empty entries).
			std::vector<AssocBlock> q[8];
			for (const AssocBlock& b : blocks) q[b.p & 7].push_back(b);
			size_t longest = 0;
			for (int x = 0; x < 8; x++) longest = std::max(longest, q[x].size());
			blocks.assign(longest * 8, AssocBlock{0, 0, 0, 0, 0});
			for (int x = 0; x < 8; x++)
				for (size_t k = 0; k < q[x].size(); k++) blocks[k * 8 + x] = q[x][k];
		}
	};
	const bool shared = dev_src == dev_dst;
	const long long rowsS = shared ? std::max(maxSrcRow, maxDstRow) : maxSrcRow;
	const int cap = (int)std::min<long long>(0x3fffffffLL, 8 * (rowTotal + colTotal) + 4096);

	BHIP_TRY(W.Fs.reserve(ctx, (size_t)rowsS * ROW_CHUNKS * 16));
	BHIP_TRY(W.nrmS.reserve(ctx, (size_t)rowsS * 4));
	if (!shared) {
		BHIP_TRY(W.Fd.reserve(ctx, (size_t)maxDstRow * ROW_CHUNKS * 16));
		BHIP_TRY(W.nrmD.reserve(ctx, (size_t)maxDstRow * 4));
	}
	BHIP_TRY(W.keys.reserve(ctx, (size_t)(rowTotal + colTotal) * 4));
	BHIP_TRY(W.best.reserve(ctx, (size_t)(rowTotal + colTotal) * 8));
	BHIP_TRY(W.args.reserve(ctx, (size_t)(rowTotal + 2 * colTotal) * 4));
	BHIP_TRY(W.cand.reserve(ctx, (size_t)cap * sizeof(AssocCand)));
	BHIP_TRY(W.flags.reserve(ctx, 64));

	hipStream_t st = ctx->stream;
	int* flags = W.flags.as<int>();       // [0] non-finite, [1] max norm bits, [2] number of listed pairs, [3] scale exponent of the run
	int* counters = flags + 2;
	_Float16* Hs = W.Fs.as<_Float16>();
	float* nS = W.nrmS.as<float>();
	_Float16* Hd = shared ? Hs : W.Fd.as<_Float16>();
	float* nD = shared ? nS : W.nrmD.as<float>();
	unsigned int* rowKey = W.keys.as<unsigned int>();
	unsigned int* colKey = rowKey + rowTotal;
	unsigned long long* rowBest = W.best.as<unsigned long long>();
	unsigned long long* colBest = rowBest + rowTotal;
	int* rowArg = W.args.as<int>();
	int* colArg = rowArg + rowTotal;
	int* colCnt = colArg + colTotal;
	const long long nk = rowTotal + colTotal;
	int maxNs = 0;
	for (int p = 0; p < count; p++) maxNs = std::max(maxNs, ns[p]);
	// both tables live in one device buffer: [problems | blocks]
	const size_t blocksAt = (probs.size() * sizeof(AssocProblem) + 15) & ~(size_t)15;

	MfmaArgs A;
	A.Hs = (const uint4*)Hs; A.Hd = (const uint4*)Hd;
	A.rowKey = rowKey; A.colKey = colKey; A.nrmS = nS; A.nrmD = nD; A.flags = flags;
	A.cand = W.cand.as<AssocCand>(); A.counter = counters; A.cap = cap;
#ifdef BHIP_EXPERIMENTS
	{ const char* e = getenv("BHIP_ASSOC_ABLATE"); A.ablate = e ? atoi(e) : 0; }
#endif
	const unsigned gS = (unsigned)((rowsS + 16 * PREP_ROWS - 1) / (16 * PREP_ROWS)), gD = (unsigned)((maxDstRow + 16 * PREP_ROWS - 1) / (16 * PREP_ROWS));
	const double prepRows = (double)(rowsS + (shared ? 0 : maxDstRow));

	// The tables go into the page-locked staging block; k_assoc_init reads them from there.  The block is rewritten only after the launch
	// that reads it has run: every complete call waits for an event recorded behind that launch (the flags read-back); a call that left
	// early did not, and is waited for here.
	buildBlocks();
	const size_t tableBytes = (blocksAt + blocks.size() * sizeof(AssocBlock) + 15) & ~(size_t)15;
	BHIP_TRY(W.probs.reserve(ctx, tableBytes));
	if (W.tablesInFlight) { BHIP_HIP(ctx, hipStreamSynchronize(st)); W.tablesInFlight = false; }
	if (tableBytes > W.tables.cap) BHIP_TRY(W.tables.reserve(ctx, tableBytes * 2));
	memcpy(W.tables.p, probs.data(), probs.size() * sizeof(AssocProblem));
	memcpy((char*)W.tables.p + blocksAt, blocks.data(), blocks.size() * sizeof(AssocBlock));
	void* tablesDev = nullptr;   // the staging block as the device sees it
	BHIP_HIP(ctx, hipHostGetDevicePointer(&tablesDev, W.tables.p, 0));
	if (!W.flagsRead) BHIP_HIP(ctx, hipEventCreateWithFlags(&W.flagsRead.h, hipEventDisableTiming));
	A.probs = W.probs.as<AssocProblem>();
	A.blocks = (const AssocBlock*)((const char*)W.probs.p + blocksAt);
	const unsigned nblocks = (unsigned)blocks.size();

	// First run: the scale exponent of the previous call is assumed and the descriptors are read once.  Only when the norms read back at the
	// end do not fit it is the whole path repeated with the measured exponent (k_assoc_norms, then k_assoc_half): a change of the inputs'
	// magnitude by more than 4x between two calls on one context, which costs that call one extra run.
	for (int run = 0; run < 2; run++) {
		const bool hinted = run == 0;
		const long long tabWords = hinted ? (long long)(tableBytes / 16) : 0;
		W.tablesInFlight = true;
		hipLaunchKernelGGL(k_assoc_init, dim3((unsigned)((std::max(nk, tabWords) + 255) / 256)), dim3(256), 0, st, rowKey, rowBest, rowArg, nk, colTotal, flags,
						   hinted ? W.scaleHint : 0, (const uint4*)tablesDev, W.probs.as<uint4>(), tabWords);
		if (hinted) {
			ProfScope ps(ctx, "k_assoc_prep", prepRows * (64 * 8 + ROW_CHUNKS * 16));
			hipLaunchKernelGGL(k_assoc_prep_hinted, dim3(gS), dim3(256), 0, st, dev_src, rowsS, W.scaleHint, nS, flags, Hs);
			if (!shared) hipLaunchKernelGGL(k_assoc_prep_hinted, dim3(gD), dim3(256), 0, st, dev_dst, maxDstRow, W.scaleHint, nD, flags, Hd);
		} else {
			ProfScope ps(ctx, "k_assoc_prep", prepRows * (2 * 64 * 8 + ROW_CHUNKS * 16));
			hipLaunchKernelGGL(k_assoc_norms, dim3(gS), dim3(256), 0, st, dev_src, rowsS, nS, flags);
			if (!shared) hipLaunchKernelGGL(k_assoc_norms, dim3(gD), dim3(256), 0, st, dev_dst, maxDstRow, nD, flags);
			hipLaunchKernelGGL(k_assoc_half, dim3(gS), dim3(256), 0, st, dev_src, rowsS, nS, flags, Hs);   // sets flags[3]
			if (!shared) hipLaunchKernelGGL(k_assoc_half, dim3(gD), dim3(256), 0, st, dev_dst, maxDstRow, nD, flags, Hd);
		}
		{
			ProfScope ps(ctx, "k_assoc_mfma_pass1", 0, flopsPerPass);
			hipLaunchKernelGGL(k_assoc_mfma<1>, dim3(nblocks), dim3(256), 0, st, A);
		}
		{
			ProfScope ps(ctx, "k_assoc_mfma_pass2", 0, flopsPerPass);
			hipLaunchKernelGGL(k_assoc_mfma<2>, dim3(nblocks), dim3(256), 0, st, A);
		}
		{
			ProfScope ps(ctx, "k_assoc_exact");
			// about one listed pair per thread (the list length is only known on the device: 2.3 per row is typical, the grid-stride loop takes the rest)
			const unsigned exactBlocks = (unsigned)std::min<long long>(16384, std::max<long long>(256, (3 * (rowTotal + colTotal) / 2 + 255) / 256));
			hipLaunchKernelGGL(k_assoc_exact, dim3(exactBlocks), dim3(256), 0, st, dev_src, dev_dst, A.probs, A.cand, counters, cap, rowBest, colBest);
			hipLaunchKernelGGL(k_assoc_argsel, dim3(exactBlocks), dim3(256), 0, st, A.probs, A.cand, counters, cap, rowBest, colBest, rowArg, colArg, colCnt);
		}
		// The result kernel goes out before the flags have come back, so the GPU does not wait for the host's answer: it reads the same
		// flags and writes nothing for a run the host is about to reject (assocDegenerate on both sides).  The host waits for the
		// read-back alone (the event behind it); the result kernel runs while the flags travel, and the caller's next work queues behind it.
		BHIP_HIP(ctx, hipMemcpyAsync(ctx->hostScratch.p, flags, 16, hipMemcpyDeviceToHost, st));
		BHIP_HIP(ctx, hipEventRecord(W.flagsRead, st));
		hipLaunchKernelGGL(k_assoc_resolve, dim3((maxNs + 255) / 256, count), dim3(256), 0, st, A.probs, maxErr, backwards, rowBest, rowArg, colArg, colCnt,
						   flags, cap, dev_pairs, dev_fit);
		BHIP_HIP(ctx, hipEventSynchronize(W.flagsRead));
		W.tablesInFlight = false;
		BHIP_HIP(ctx, hipGetLastError());
		const int* hf = ctx->hostScratch.as<int>();
		if (hf[0] != 0) return BHIP_OK;  // non-finite values: *usedMfma stays 0, and the hint stays what it was
		float maxRaw;
		memcpy(&maxRaw, &hf[1], 4);
		if (maxRaw > 0.0f) W.scaleHint = scaleExp(maxRaw);   // all-zero descriptors say nothing about the next call's
		if (!scaleHolds(maxRaw, hf[3])) continue;            // the hint did not fit (the measured exponent always does)
		if (hf[2] > cap) return BHIP_OK;                     // candidate list overflow: exact path
		*usedMfma = 1;
		return BHIP_OK;
	}
	return BHIP_OK;
}
