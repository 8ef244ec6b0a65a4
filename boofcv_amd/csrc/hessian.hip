// K2: Fast-Hessian determinant-of-Hessian intensity from the integral image, bit-exact with the reference.
//
// Reference: IntegralImageFeatureIntensity.hessian  F:alg/feature/detect/intensity/IntegralImageFeatureIntensity.java:43-56
//   -> hessianBorder  F:alg/feature/detect/intensity/impl/ImplIntegralImageFeatureIntensity.java:72-113  (clamped box sums)
//   -> hessianInner   ...:132-213  (32 integral-image taps per pixel)
//   box kernels       I:alg/transform/ii/DerivativeIntegralImage.java:102-158
//   block_zero        I:alg/transform/ii/impl/ImplIntegralImageOps.java:195-214, convolveSparse :172-183
// Two plans, equally exact.  Gather (k_hessian): every pixel of every level of one octave is one thread that fetches its taps itself.
// Staged rows (k_hessian_rows, octaves with a power-of-two step >= 4): the inner pixels of a computed level take their taps from LDS, where
// a workgroup has put the ten image rows of one output row with coalesced loads; the border pixels and the shared levels' pixels that
// must be recomputed or copied go through the gather form in a compact launch (k_hessian_frame).  The staged levels of the default
// schedule (size 75 at step 4, 99 and 147 at step 8) take k_hessian_rows_fixed: compile-time geometry, a band of rows per workgroup, the
// levels of several octaves in one launch.  BHIP_DETECT_GATHER=1 forces the gather plan, BHIP_HESSIAN_ROWS_GENERIC=1 the run-time rows
// kernel.  fp32, no FMA contraction (-ffp-contract=off), expressions in the reference's order.
// Bound: HBM (+L2 gather).  Algorithmic bytes per octave: 4P (ii read) + levels * 4P/skip^2 (intensity write).
#include "hessian_dev.h"
#include <algorithm>

struct HessParams {
	ImgView ii;
	int skip, w, h, nlevels;
	int nrun, runLevel[BHIP_MAX_LEVELS];   // the levels this launch produces (outer levels may be left to k_nms_scalespace)
	float* out;             // [image][level][h][outStride]
	long long levelStride, imageStrideOut;
	int outStride;
	HessLevel lv[BHIP_MAX_LEVELS];
	HessLevelSource from[BHIP_MAX_LEVELS];
	int srcBorder[BHIP_MAX_LEVELS];   // shared levels: the producing octave's (step skip/2) inner-region border, width and height
	int srcW, srcH;
};

// one output pixel of one level, gather form: computed, copied from the octave below, or left as the producing octave wrote it
template <class T>
__device__ __forceinline__ void hessianPixel(const HessParams& P, int img, int level, int x, int y) {
	const HessLevel L = P.lv[level];
	if (P.from[level].src) {
		// Same kernel size one octave down.  A response depends on the pixel and the kernel size, and on which of the reference's two
		// forms evaluates it: hessianInner sums the Dyy boxes as ((br - bl) - tr) + tl, the border form (block_zero) as ((br - tr) - bl) + tl,
		// so the two can differ in the last bit.  The inner regions of the two octaves are not the same set of pixels (borderOrig depends
		// on the step), hence: copy where both octaves use the same form, compute in place on the few rows / columns where they do not.
		const bool inner = x >= L.border && x < P.w - L.border && y >= L.border && y < P.h - L.border;
		const int bp = P.srcBorder[level];
		const int px = 2 * x, py = 2 * y;
		const bool srcInner = px >= bp && px < P.srcW - bp && py >= bp && py < P.srcH - bp;
		if (srcInner == inner) {
			const HessLevelSource S = P.from[level];
			if (S.inPlace) return;   // the producing octave has written this pixel into this very plane
			P.out[(long long)img * P.imageStrideOut + (long long)level * P.levelStride + (long long)y * P.outStride + x] =
				S.src[(long long)img * S.imageStride + (long long)(y * S.step) * S.stride + x * S.step];
			return;
		}
	}
	const T* __restrict__ d = (const T*)P.ii.data + (long long)img * P.ii.imageStride;
	P.out[(long long)img * P.imageStrideOut + (long long)level * P.levelStride + (long long)y * P.outStride + x] =
		hessianCompute<T>(d, P.ii.stride, P.ii.width, P.ii.height, L, P.skip, P.w, P.h, x, y);
}

template <class T>
__global__ __launch_bounds__(256) void k_hessian(HessParams P) {
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	const int y = blockIdx.y;
	const int img = blockIdx.z / P.nrun;
	const int level = P.runLevel[blockIdx.z - img * P.nrun];
	if (x >= P.w) return;
	hessianPixel<T>(P, img, level, x, y);
}

// ---------------- staged-rows plan ----------------
#define BHIP_HESS_ROWS 10   // image rows the 32 taps of hessianInner lie in: 2 (Dxx) + 4 (Dyy) + 4 (Dxy)
// words staged per group of row r: the Dxx and Dxy rows carry four taps, the Dyy rows two
__host__ __device__ constexpr int hessRowWords(int r) { return r >= 2 && r < 6 ? 2 : 4; }

// The pixels of a run level the frame launch leaves out: the rectangle [x0, x1) x [y0, y1) (empty: none).  The others are numbered
// row by row: the rows above it, the rows below it, then the columns left and right of it.
struct HessFrame {
	int x0, x1, y0, y1;
	int count;
};
struct HessFrameParams {
	HessFrame fr[BHIP_MAX_LEVELS];   // by run index
};

template <class T>
__global__ __launch_bounds__(256) void k_hessian_frame(HessParams P, HessFrameParams F) {
	const int img = blockIdx.y / P.nrun;
	const int run = blockIdx.y - img * P.nrun;
	const HessFrame f = F.fr[run];
	int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= f.count) return;
	const int above = f.y0 * P.w, below = (P.h - f.y1) * P.w;
	int x, y;
	if (idx < above + below) {
		y = idx / P.w;
		x = idx - y * P.w;
		if (idx >= above) y += f.y1 - f.y0;
	} else {
		idx -= above + below;
		const int side = P.w - (f.x1 - f.x0);
		y = idx / side;
		x = idx - y * side;
		y += f.y0;
		if (x >= f.x0) x += f.x1 - f.x0;
	}
	hessianPixel<T>(P, img, P.runLevel[run], x, y);
}

// How one computed level is staged.  An x-tile of TX outputs of output row y reads image rows y * skip + dy[r]; of row r it needs, for
// output i, the columns c0 + skip * i + (tap offsets), c0 = the tile's first tap column.  The columns are grouped by `skip`: group q of row
// r starts at column c0 + dc[r] + skip * q and its first hessRowWords(r) columns are staged: the run the column phases of the row's taps
// span (at a step of 4 the runs of a four-tap row join up to the whole row segment), element e into plane e of the row:
// lds[base[r] + e * G + q].  So the loads of neighbouring lanes are neighbouring 16- or 8-byte runs, and tap j of output i is
// lds[tap[j] + i]: neighbouring lanes, neighbouring banks.
struct HessRowLevel {
	int level;
	int x0, nx, y0, ny;   // the inner region, in output pixels
	int TX, ntiles, G;
	float norm;
	int dy[BHIP_HESS_ROWS], dc[BHIP_HESS_ROWS], base[BHIP_HESS_ROWS];
	int tap[32];          // xx(r, k): 4 r + k; yy(k, s): 8 + 2 k + s; xy(r, c): 16 + 4 r + c
};
struct HessRowParams {
	ImgView ii;
	int skip, batch, nlv;
	int ymin, nrows;        // output rows any staged level has inner pixels in
	int tilesPerRow;        // sum of the levels' ntiles
	int blocksPerImage;     // nrows * tilesPerRow
	float* out;
	long long levelStride, imageStrideOut;
	int outStride;
	HessRowLevel lv[BHIP_MAX_LEVELS];
};

template <class T>
struct HessTapsLds {
	const T* lds;   // + the output's index in its tile
	const int* tap;
	__device__ __forceinline__ T xx(int r, int k) const { return lds[tap[4 * r + k]]; }
	__device__ __forceinline__ T yy(int k, int s) const { return lds[tap[8 + 2 * k + s]]; }
	__device__ __forceinline__ T xy(int r, int c) const { return lds[tap[16 + 4 * r + c]]; }
};

typedef unsigned int hess_u2 __attribute__((ext_vector_type(2), aligned(4)));
typedef unsigned int hess_u4 __attribute__((ext_vector_type(4), aligned(4)));

// One workgroup = one image, one staged level, one output row, one x-tile.  Block b runs on XCD b % 8 (blocks are dealt round-robin): it
// takes image (b / 8 / blocksPerImage) * 8 + b % 8, so an XCD works through whole images, and within an image the blocks go row by row, so
// the rows an XCD has in flight are a band of the image that fits its L2 and each tap row is fetched from memory once.
template <class T>
__global__ __launch_bounds__(256) void k_hessian_rows(HessRowParams P) {
	extern __shared__ __attribute__((aligned(16))) unsigned int hessLds[];
	const int slot = blockIdx.x >> 3;
	const int img = (slot / P.blocksPerImage) * 8 + (blockIdx.x & 7);
	if (img >= P.batch) return;
	const int within = slot % P.blocksPerImage;
	const int y = P.ymin + within / P.tilesPerRow;
	int tile = within % P.tilesPerRow, li = 0;
	while (li < P.nlv - 1 && tile >= P.lv[li].ntiles) { tile -= P.lv[li].ntiles; li++; }
	const HessRowLevel& L = P.lv[li];
	if (y < L.y0 || y >= L.y0 + L.ny) return;
	const int first = tile * L.TX;                 // first output of the tile, counted from the first inner column
	const int n = min(L.TX, L.nx - first);         // outputs of this tile
	const int W = P.ii.width;
	const unsigned int* __restrict__ d = (const unsigned int*)P.ii.data + (long long)img * P.ii.imageStride;

	// stage: wave k takes groups 64 k .. 64 k + 63 of every row (a row has at most 256 groups), all its loads in flight before the first
	// is written to LDS; a run is one load where it lies inside its image row, and goes word by word at the row's ends (nothing outside
	// [0, W) of the row is touched)
	const int q = threadIdx.x;
	if (q < n + L.G - L.TX) {   // the groups the tile's n outputs reach
		unsigned int v[BHIP_HESS_ROWS][4];
#pragma unroll
		for (int r = 0; r < BHIP_HESS_ROWS; r++) {
			const int rw = hessRowWords(r);
			const int Y = y * P.skip + L.dy[r];                       // inside the image for every inner pixel
			const int c = first * P.skip + L.dc[r] + P.skip * q;      // dc counts from the first inner output's first tap column
			const unsigned int* __restrict__ src = d + (long long)Y * P.ii.stride + c;
			if (c >= 0 && c + rw <= W) {
				if (rw == 4) { const hess_u4 t = *(const hess_u4*)src; v[r][0] = t.x; v[r][1] = t.y; v[r][2] = t.z; v[r][3] = t.w; }
				else { const hess_u2 t = *(const hess_u2*)src; v[r][0] = t.x; v[r][1] = t.y; }
			} else {
#pragma unroll
				for (int e = 0; e < rw; e++) v[r][e] = c + e >= 0 && c + e < W ? src[e] : 0;
			}
		}
#pragma unroll
		for (int r = 0; r < BHIP_HESS_ROWS; r++) {
			unsigned int* dst = hessLds + L.base[r] + q;
#pragma unroll
			for (int e = 0; e < hessRowWords(r); e++) dst[e * L.G] = v[r][e];
		}
	}
	__syncthreads();

	const int i = threadIdx.x;
	if (i >= n) return;
	float Dxx, Dyy, Dxy;
	hessianInnerExpr<T>(HessTapsLds<T>{(const T*)hessLds + i, L.tap}, Dxx, Dyy, Dxy);
	P.out[(long long)img * P.imageStrideOut + (long long)L.level * P.levelStride + (long long)y * P.outStride + L.x0 + first + i] =
		hessianDeterminant(Dxx, Dyy, Dxy, L.norm);
}

// ---------------- staged rows, compile-time geometry ----------------
// The computed levels of the coarse octaves of the reference's default schedule: size 75 at step 4, sizes 99 and 147 at step 8.  For these
// everything hessPlanRows derives from (step, size) is a constant of the instantiation: the ten row distances, the column distances, plane
// and group of every tap (each tap is a ds_read with an immediate offset).  The planes have a fixed pitch of 256 words whatever the tile
// width, so a workgroup always holds 32 KiB of LDS.
#define BHIP_HESS_PITCH 256
template <int SKIP, int SIZE>
struct HessFixedGeo {
	static constexpr int bS = SIZE / 3, bL = SIZE - bS - 1, rF = SIZE / 2, rS = bL / 2;
	static constexpr int borderOrig = rF + 1 + (SKIP - (rF + 1) % SKIP), border = borderOrig / SKIP, lost = borderOrig - rF - 1;
	static constexpr int xyOff(int i) { return i == 0 ? 0 : i == 1 ? bS : i == 2 ? bS + 1 : 2 * bS + 1; }
	// staged row r (0-1 Dxx, 2-5 Dyy, 6-9 Dxy): its distance from row y * SKIP, and the column of its tap k from the output's first tap column
	static constexpr int dy(int r) { return r < 2 ? -rS - 1 + r * bL : r < 6 ? -rF - 1 + (r - 2) * bS : -bS - 1 + xyOff(r - 6); }
	static constexpr int off(int r, int k) { return r < 2 ? k * bS : r < 6 ? rF - rS + k * bL : rF - bS + xyOff(k); }
	static constexpr int dc(int r) { return lost + off(r, 0); }
	static constexpr int plane(int r, int k) { return (off(r, k) - off(r, 0)) % SKIP; }
	static constexpr int group(int r, int k) { return (off(r, k) - off(r, 0)) / SKIP; }
	static constexpr int maxGroup = 3 * bS / SKIP;   // the last Dxx tap: 3 bS >= bL, 2 bS + 1
	static constexpr int txCap = BHIP_HESS_PITCH - (maxGroup + 1);
	static constexpr int base(int r) { return BHIP_HESS_PITCH * (r <= 2 ? 4 * r : r <= 6 ? 8 + 2 * (r - 2) : 16 + 4 * (r - 6)); }
	static constexpr int tap(int r, int k) { return base(r) + plane(r, k) * BHIP_HESS_PITCH + group(r, k); }
	static constexpr bool planesFit() {
		for (int r = 0; r < BHIP_HESS_ROWS; r++)
			for (int k = 0; k < hessRowWords(r); k++)
				if (plane(r, k) >= hessRowWords(r) || group(r, k) > maxGroup) return false;
		return true;
	}
};
#define BHIP_HESS_FIXED_LDS (32 * BHIP_HESS_PITCH * 4)

template <class T, class G>
struct HessTapsFixed {
	const T* lds;   // + the output's index in its tile
	__device__ __forceinline__ T xx(int r, int k) const { return lds[G::tap(r, k)]; }
	__device__ __forceinline__ T yy(int k, int s) const { return lds[G::tap(2 + k, s)]; }
	__device__ __forceinline__ T xy(int r, int c) const { return lds[G::tap(6 + r, c)]; }
};

// what is left of a level at run time: where its inner pixels are, how they are tiled, where they go
struct HessFixedLevel {
	float* out;             // the level's plane of image 0
	long long imageStrideOut;
	int outStride;
	int x0, nx, y0, ny;     // the inner region, in output pixels
	int TX, ntiles;
	float norm;
};
#define BHIP_HESS_FIXED_LEVELS 3   // (4, 75), (8, 99), (8, 147), in this order
struct HessFixedParams {
	ImgView ii;
	int batch, band;        // band: output rows per workgroup
	int end0, end1;         // blocks of an image below end0: level 0, below end1: level 1, the others: level 2
	int blocksPerImage;
	HessFixedLevel lv[BHIP_HESS_FIXED_LEVELS];
};

// One workgroup: one x-tile and `band` consecutive output rows (fewer at the lower end of the inner region) of one level of one image.
// Everything that does not depend on the row is set up once; a row is ten loads per thread, a barrier, 32 taps, a store.  The loads of a
// row wait in registers while the taps of the row before are read from LDS.
template <class T, int SKIP, int SIZE>
__device__ __forceinline__ void hessRowsBand(const ImgView& ii, const HessFixedLevel& L, int band, int img, int blk, unsigned int* lds) {
	typedef HessFixedGeo<SKIP, SIZE> G;
	static_assert((SKIP & (SKIP - 1)) == 0 && SKIP >= 4 && SIZE % 3 == 0 && G::planesFit() && G::txCap >= 64, "not a staged-rows geometry");
	const int tile = blk % L.ntiles, yFirst = L.y0 + (blk / L.ntiles) * band;
	const int yEnd = min(yFirst + band, L.y0 + L.ny);
	const int first = tile * L.TX;                 // first output of the tile, counted from the first inner column
	const int n = min(L.TX, L.nx - first);         // outputs of this tile
	const int W = ii.width;
	const int q = threadIdx.x;
	const bool stages = q < n + G::maxGroup + 1;   // the groups the tile's n outputs reach
	const int c0 = (first + q) * SKIP;
	// row r of output row y starts at src + dy(r) * stride + dc(r); nothing outside [0, W) of an image row is touched
	const unsigned int* __restrict__ src = (const unsigned int*)ii.data + (long long)img * ii.imageStride + (long long)(yFirst * SKIP) * ii.stride + c0;
	float* __restrict__ dst = L.out + (long long)img * L.imageStrideOut + (long long)yFirst * L.outStride + L.x0 + first + q;
	unsigned int v[BHIP_HESS_ROWS][4];
	auto loadRows = [&]() {
#pragma unroll
		for (int r = 0; r < BHIP_HESS_ROWS; r++) {
			const int rw = hessRowWords(r);
			const int c = c0 + G::dc(r);
			const unsigned int* __restrict__ s = src + (long long)G::dy(r) * ii.stride + G::dc(r);
			if (c >= 0 && c + rw <= W) {
				if (rw == 4) { const hess_u4 t = *(const hess_u4*)s; v[r][0] = t.x; v[r][1] = t.y; v[r][2] = t.z; v[r][3] = t.w; }
				else { const hess_u2 t = *(const hess_u2*)s; v[r][0] = t.x; v[r][1] = t.y; }
			} else {
#pragma unroll
				for (int e = 0; e < rw; e++) v[r][e] = c + e >= 0 && c + e < W ? s[e] : 0;
			}
		}
	};
	if (stages) loadRows();
	for (int y = yFirst; y < yEnd; y++) {
		if (y > yFirst) __syncthreads();   // the row before has been read
		if (stages) {
#pragma unroll
			for (int r = 0; r < BHIP_HESS_ROWS; r++)
#pragma unroll
				for (int e = 0; e < hessRowWords(r); e++) lds[G::base(r) + e * BHIP_HESS_PITCH + q] = v[r][e];
		}
		__syncthreads();
		src += (long long)SKIP * ii.stride;
		if (stages && y + 1 < yEnd) loadRows();   // the next row's loads are in flight while this row's taps are read
		if (q < n) {
			float Dxx, Dyy, Dxy;
			hessianInnerExpr<T>(HessTapsFixed<T, G>{(const T*)lds + q}, Dxx, Dyy, Dxy);
			*dst = hessianDeterminant(Dxx, Dyy, Dxy, L.norm);
		}
		dst += L.outStride;
	}
}

// Block b runs on XCD b % 8 and takes image (b / 8 / blocksPerImage) * 8 + b % 8, as in k_hessian_rows: an XCD works through whole images,
// and within an image level by level, the bands of a level in row order.
template <class T>
__global__ __launch_bounds__(256) void k_hessian_rows_fixed(HessFixedParams P) {
	extern __shared__ __attribute__((aligned(16))) unsigned int hessLds[];
	const int slot = blockIdx.x >> 3;
	const int img = (slot / P.blocksPerImage) * 8 + (blockIdx.x & 7);
	if (img >= P.batch) return;
	const int within = slot % P.blocksPerImage;
	if (within < P.end0) hessRowsBand<T, 4, 75>(P.ii, P.lv[0], P.band, img, within, hessLds);
	else if (within < P.end1) hessRowsBand<T, 8, 99>(P.ii, P.lv[1], P.band, img, within - P.end0, hessLds);
	else hessRowsBand<T, 8, 147>(P.ii, P.lv[2], P.band, img, within - P.end1, hessLds);
}
static int hessFixedIndex(int skip, int size) { return skip == 4 && size == 75 ? 0 : skip == 8 && size == 99 ? 1 : skip == 8 && size == 147 ? 2 : -1; }
#define BHIP_HESS_BAND 2   // output rows per workgroup of k_hessian_rows_fixed: 1, 2, 3, 4, 6, 8, 16 measured ("Open performance items", item 3)

// Plans the staged-rows form of a launch: which levels are staged and how (R), and which pixels are left to the gather form (F).  False:
// the launch stays with the gather plan (a step that is not a power of two or below 4, taps whose column phases span more than the
// 16- or 8-byte run of their row, a kernel so wide that a tile would hold fewer than 64 outputs, no computed level with inner pixels).
static bool hessPlanRows(const HessParams& P, int batch, HessRowParams& R, HessFrameParams& F, int* ldsBytes) {
	const int skip = P.skip;
	if (skip < 4 || (skip & (skip - 1)) != 0) return false;
	R.ii = P.ii; R.skip = skip; R.batch = batch; R.nlv = 0;
	R.out = P.out; R.levelStride = P.levelStride; R.imageStrideOut = P.imageStrideOut; R.outStride = P.outStride;
	R.tilesPerRow = 0;
	int ymin = P.h, ymax = 0, ldsWords = 0;
	for (int run = 0; run < P.nrun; run++) {
		const int level = P.runLevel[run];
		const HessLevel& L = P.lv[level];
		HessFrame& f = F.fr[run];
		f = HessFrame{0, 0, 0, 0, P.w * P.h};
		// the inner region; for a level the octave below wrote in place, the part of it that octave evaluated with the inner form too
		int x0 = L.border, x1 = P.w - L.border, y0 = L.border, y1 = P.h - L.border;
		const HessLevelSource& S = P.from[level];
		if (S.src) {
			if (!S.inPlace) continue;   // every pixel is copied or computed
			const int bp = P.srcBorder[level];
			x0 = std::max(x0, (bp + 1) / 2); x1 = std::min(x1, (P.srcW - bp + 1) / 2);
			y0 = std::max(y0, (bp + 1) / 2); y1 = std::min(y1, (P.srcH - bp + 1) / 2);
		}
		if (x1 <= x0 || y1 <= y0) continue;
		if (S.src) {   // nothing to do inside
			f = HessFrame{x0, x1, y0, y1, P.w * P.h - (x1 - x0) * (y1 - y0)};
			continue;
		}
		HessRowLevel& V = R.lv[R.nlv];
		V.level = level; V.x0 = x0; V.nx = x1 - x0; V.y0 = y0; V.ny = y1 - y0; V.norm = L.norm;
		// tap columns relative to the output's first tap column, row by row
		int off[BHIP_HESS_ROWS][4], nt[BHIP_HESS_ROWS];
		for (int r = 0; r < 2; r++) {
			V.dy[r] = -L.rS - 1 + r * L.bL; nt[r] = 4;
			for (int k = 0; k < 4; k++) off[r][k] = k * L.bS;
		}
		for (int k = 0; k < 4; k++) {
			V.dy[2 + k] = -L.rF - 1 + k * L.bS; nt[2 + k] = 2;
			for (int s = 0; s < 2; s++) off[2 + k][s] = L.rF - L.rS + s * L.bL;
		}
		for (int r = 0; r < 4; r++) {
			V.dy[6 + r] = -L.bS - 1 + hessXyOffset(r, L.bS); nt[6 + r] = 4;
			for (int c = 0; c < 4; c++) off[6 + r][c] = L.rF - L.bS + hessXyOffset(c, L.bS);
		}
		int plane[BHIP_HESS_ROWS][4], grp[BHIP_HESS_ROWS][4], maxGroup = 0;
		bool ok = true;
		for (int r = 0; r < BHIP_HESS_ROWS; r++) {
			// a group starts at the row's first tap, so a tap's plane is its distance from that tap modulo the step (the offsets ascend).  A
			// pattern whose planes do not fit the row's run (the default sizes give 0..3 and 0..1) is not rotated: the launch stays with the gather
			V.dc[r] = L.lost + off[r][0];
			for (int k = 0; k < nt[r]; k++) {
				const int rel = off[r][k] - off[r][0];
				plane[r][k] = rel % skip;
				grp[r][k] = rel / skip;
				maxGroup = std::max(maxGroup, grp[r][k]);
				if (plane[r][k] >= hessRowWords(r)) ok = false;
			}
		}
		// tile width: the groups of a row (outputs + the groups the farthest tap reaches over) fill whole waves of 64 loads
		const int txCap = 256 - (maxGroup + 1);
		if (!ok || txCap < 64) return false;
		V.ntiles = (V.nx + txCap - 1) / txCap;
		V.TX = (V.nx + V.ntiles - 1) / V.ntiles;
		V.G = V.TX + maxGroup + 1;
		int words = 0;
		for (int r = 0; r < BHIP_HESS_ROWS; r++) { V.base[r] = words; words += hessRowWords(r) * V.G; }
		for (int j = 0; j < 32; j++) {
			const int r = j < 8 ? j / 4 : j < 16 ? 2 + (j - 8) / 2 : 6 + (j - 16) / 4;
			const int k = j < 8 ? j % 4 : j < 16 ? (j - 8) % 2 : (j - 16) % 4;
			V.tap[j] = V.base[r] + plane[r][k] * V.G + grp[r][k];
		}
		ldsWords = std::max(ldsWords, words);
		f = HessFrame{x0, x1, y0, y1, P.w * P.h - (x1 - x0) * (y1 - y0)};
		ymin = std::min(ymin, y0); ymax = std::max(ymax, y1);
		R.tilesPerRow += V.ntiles;
		R.nlv++;
	}
	if (R.nlv == 0) return false;
	R.ymin = ymin; R.nrows = ymax - ymin;
	R.blocksPerImage = R.nrows * R.tilesPerRow;
	*ldsBytes = ldsWords * 4;   // at most 32 KiB: 32 planes of G <= 256 words, so five workgroups fit a CU's LDS
	return true;
}

// the rows of an octave on the staged-rows plan that have not been launched yet
struct HessPendingRows {
	HessRowParams R;
	int size[BHIP_MAX_LEVELS];   // kernel size of R.lv[i]
	int ldsBytes;
	double bytes;                // algorithmic bytes of the octave
};

template <class T>
static int hessLaunchPending(bhip_ctx* ctx, std::vector<HessPendingRows>& pending, const ImgView& iiView, int batch, bool generic) {
	if (pending.empty()) return BHIP_OK;
	// the compile-time-geometry kernel takes the launch when every staged level is one of its three, each at most once
	const HessRowLevel* fixedLevel[BHIP_HESS_FIXED_LEVELS] = {nullptr, nullptr, nullptr};
	const HessRowParams* fixedOctave[BHIP_HESS_FIXED_LEVELS] = {nullptr, nullptr, nullptr};
	bool fixed = !generic;
	double bytes = 0;
	for (const HessPendingRows& p : pending) {
		bytes += p.bytes - (&p == &pending[0] ? 0.0 : 4.0 * iiView.width * iiView.height * batch);   // the integral image counts once
		for (int i = 0; i < p.R.nlv && fixed; i++) {
			const int k = hessFixedIndex(p.R.skip, p.size[i]);
			if (k < 0 || fixedLevel[k]) fixed = false;
			else { fixedLevel[k] = &p.R.lv[i]; fixedOctave[k] = &p.R; }
		}
	}
	if (fixed) {
		HessFixedParams X;
		memset(&X, 0, sizeof X);
		X.ii = iiView; X.batch = batch; X.band = BHIP_HESS_BAND;
#ifdef BHIP_EXPERIMENTS
		if (const char* e = getenv("BHIP_HESSIAN_ROWS_BAND")) X.band = std::min(std::max(atoi(e), 1), 64);
#endif
		int blocks[BHIP_HESS_FIXED_LEVELS];
		for (int k = 0; k < BHIP_HESS_FIXED_LEVELS; k++) {
			blocks[k] = 0;
			if (!fixedLevel[k]) continue;
			const HessRowLevel& V = *fixedLevel[k];
			const HessRowParams& R = *fixedOctave[k];
			X.lv[k] = HessFixedLevel{R.out + (long long)V.level * R.levelStride, R.imageStrideOut, R.outStride, V.x0, V.nx, V.y0, V.ny, V.TX, V.ntiles, V.norm};
			blocks[k] = V.ntiles * ((V.ny + X.band - 1) / X.band);
		}
		X.end0 = blocks[0]; X.end1 = blocks[0] + blocks[1]; X.blocksPerImage = X.end1 + blocks[2];
		ProfScope ps(ctx, "k_hessian_rows", bytes);
		hipLaunchKernelGGL(k_hessian_rows_fixed<T>, dim3(8 * ((batch + 7) / 8) * X.blocksPerImage), dim3(256), BHIP_HESS_FIXED_LDS, ctx->stream, X);
	} else {
		for (const HessPendingRows& p : pending) {
			ProfScope ps(ctx, "k_hessian_rows", p.bytes);
			hipLaunchKernelGGL(k_hessian_rows<T>, dim3(8 * ((batch + 7) / 8) * p.R.blocksPerImage), dim3(256), p.ldsBytes, ctx->stream, p.R);
		}
	}
	pending.clear();
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// One octave of bhip_launch_hessian_octaves: the gather plan is one launch; the staged-rows plan launches its frame pixels and queues its rows.
template <class T>
static int hessLaunchOctave(bhip_ctx* ctx, DevImg<const T> ii, const HessOctave& oct, bool gather, bool generic, std::vector<HessPendingRows>& pending) {
	const int skip = oct.skip, nlevels = oct.nlevels;
	const int* sizes = oct.sizes;
	const DevImg<float> level0 = oct.level0;
	const long long levelStride = oct.levelStride;
	const HessLevelSource* from = oct.from;
	const unsigned int skipMask = oct.skipMask;
	if (nlevels > BHIP_MAX_LEVELS) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "too many scales per octave");
	const int batch = ii.batch;
	HessParams P;
	P.ii = bhip_kernel_view(ii);
	P.skip = skip;
	P.w = ii.width / skip;
	P.h = ii.height / skip;
	P.nlevels = nlevels;
	P.out = level0.data; P.levelStride = levelStride; P.imageStrideOut = level0.imageStride; P.outStride = level0.stride;
	for (int i = 0; i < nlevels; i++) {
		P.lv[i] = bhipMakeHessLevel(sizes[i], skip);
		P.from[i] = from ? from[i] : HessLevelSource{nullptr, 0, 0, 1, 0};
		P.srcBorder[i] = 0;
		if (P.from[i].src) {
			if (skip % 2 != 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "a shared level needs an octave at half the step");
			P.srcBorder[i] = bhipMakeHessLevel(sizes[i], skip / 2).border;
		}
	}
	P.srcW = skip >= 2 ? ii.width / (skip / 2) : 0;
	P.srcH = skip >= 2 ? ii.height / (skip / 2) : 0;
	P.nrun = 0;
	for (int i = 0; i < nlevels; i++)
		if (!(skipMask & (1u << i))) P.runLevel[P.nrun++] = i;
	if (P.w <= 0 || P.h <= 0 || P.nrun == 0) return BHIP_OK;
	// algorithmic bytes: the integral image once + every level's intensity written once
	const double bytes = 4.0 * ii.width * ii.height * batch + 4.0 * P.nrun * (double)P.w * P.h * batch;
	// a level copied from a plane whose rows are still queued: those rows go first
	for (int i = 0; i < nlevels; i++) {
		const HessLevelSource& S = P.from[i];
		if (!S.src || S.inPlace) continue;
		bool waits = false;
		for (const HessPendingRows& p : pending)
			for (int k = 0; k < p.R.nlv; k++)
				if (S.src == p.R.out + (long long)p.R.lv[k].level * p.R.levelStride) waits = true;
		if (waits) { BHIP_TRY(hessLaunchPending<T>(ctx, pending, P.ii, batch, generic)); break; }
	}
	HessPendingRows Q;
	HessFrameParams F;
	if (gather || !hessPlanRows(P, batch, Q.R, F, &Q.ldsBytes)) {
		dim3 grid((P.w + 255) / 256, P.h, batch * P.nrun);
		ProfScope ps(ctx, skip == 1 ? "k_hessian_skip1" : "k_hessian_skipN", bytes);
		hipLaunchKernelGGL(k_hessian<T>, grid, dim3(256), 0, ctx->stream, P);
	} else {
		int maxCount = 0;
		for (int i = 0; i < P.nrun; i++) maxCount = std::max(maxCount, F.fr[i].count);
		if (maxCount > 0) {
			ProfScope ps(ctx, "k_hessian_frame");
			hipLaunchKernelGGL(k_hessian_frame<T>, dim3((maxCount + 255) / 256, batch * P.nrun), dim3(256), 0, ctx->stream, P, F);
		}
		for (int k = 0; k < Q.R.nlv; k++) Q.size[k] = sizes[Q.R.lv[k].level];
		Q.bytes = bytes;
		pending.push_back(Q);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// The octaves in order.  The rows of the octaves on the staged-rows plan depend on the integral image alone and write pixels no frame
// launch touches, so they wait for one launch behind the last octave.  Only where a later octave copies from a plane whose rows are
// still waiting are these launched first.
template <class T>
int bhip_launch_hessian_octaves(bhip_ctx* ctx, DevImg<const T> ii, int noct, const HessOctave* octs) {
	const bool gather = bhip_env_flag("BHIP_DETECT_GATHER");              // parity cross-check of the two plans
	const bool generic = bhip_env_flag("BHIP_HESSIAN_ROWS_GENERIC");      // parity cross-check of the two staged-rows kernels
	std::vector<HessPendingRows> pending;
	for (int o = 0; o < noct; o++) BHIP_TRY(hessLaunchOctave<T>(ctx, ii, octs[o], gather, generic, pending));
	return hessLaunchPending<T>(ctx, pending, bhip_kernel_view(ii), ii.batch, generic);
}
template int bhip_launch_hessian_octaves(bhip_ctx*, DevImg<const int32_t>, int, const HessOctave*);
template int bhip_launch_hessian_octaves(bhip_ctx*, DevImg<const float>, int, const HessOctave*);

template <class T>
int bhip_launch_hessian(bhip_ctx* ctx, DevImg<const T> ii, int skip, int nlevels, const int* sizes, DevImg<float> level0, long long levelStride,
						const HessLevelSource* from, unsigned int skipMask) {
	const HessOctave o{skip, nlevels, sizes, level0, levelStride, from, skipMask};
	return bhip_launch_hessian_octaves<T>(ctx, ii, 1, &o);
}
template int bhip_launch_hessian(bhip_ctx*, DevImg<const int32_t>, int, int, const int*, DevImg<float>, long long, const HessLevelSource*, unsigned int);
template int bhip_launch_hessian(bhip_ctx*, DevImg<const float>, int, int, const int*, DevImg<float>, long long, const HessLevelSource*, unsigned int);
