// Pyramid KLT point tracker: PyramidKltTracker / KltTracker / BilinearRectangle_F32 / _U8 / _S16 and the list logic of PointTrackerKltPyramid.
//   F:alg/tracker/klt/KltTracker.java:147-495, PyramidKltTracker.java:58-151
//   I:alg/interpolate/impl/BilinearRectangle_F32.java:64-172, BilinearRectangle_U8.java:65-173, BilinearRectangle_S16.java:66-168
//   G:abst/feature/tracker/PointTrackerKltPyramid.java:139-348   (G: = main/boofcv-geo/src/main/java/boofcv/)
//
// Shape: one wave per track.  The iteration count, the inside / border choice and every fault test are then uniform over the wave; the 64
// lanes share the (2r+1)^2 template elements: each lane interpolates its elements and forms their products, the results go through LDS,
// and the sums the reference forms in one fp32 chain (Gxx, Gyy, Gxy, Ex, Ey, the error) are added in template order by one lane per sum --
// the up to five sums of an iteration are independent chains on five lanes.  No sum is re-associated and nothing is contracted
// (-ffp-contract=off), so every value equals the single-threaded Java arithmetic bit for bit.
//
// The one deliberate deviation: where computeSubImageBounds / region throw IllegalArgumentException for a float round-off position at the
// border (the exception leaves process() in Java), the track gets the fault BHIP_KLT_REFERENCE_THROWS and is dropped; no kernel reads
// outside the image.
//
// Pixel types: the kernels are templates over the image and derivative types, <float, float> and <uint8_t, int16_t>.  BilinearRectangle_U8 /
// _S16 are the F32 expression on the four taps converted to float (& 0xFF, sign-extended), every such integer is exact in fp32, so the
// integer instantiation performs the fp32 operations of the float one on float copies of the same arrays.
#include "common.h"
#include "klt_dev.h"
#include <cfloat>
#include <cmath>

#define KLT_LEN BHIP_KLT_MAX_LEN

struct KltShared {
	float D[KLT_LEN], X[KLT_LEN], Y[KLT_LEN];        // template of the current layer
	float cur[KLT_LEN];                               // currDesc
	float pEx[KLT_LEN], pEy[KLT_LEN];                 // d * derivX, d * derivY (also |d| for computeError)
	float pXX[KLT_LEN], pYY[KLT_LEN], pXY[KLT_LEN];   // derivX^2, derivY^2, derivX * derivY
	unsigned char ok[KLT_LEN + 3];                    // element takes part in the sums
	float sum[5];
	int cnt;
};

// one lane per sum adds `arr` over the elements whose ok flag is set, in template order; lane 0 also counts them
__device__ __forceinline__ void kltChains(KltShared& S, int lane, int nsum, int len, const float* a0, const float* a1, const float* a2, const float* a3,
										  const float* a4) {
	if (lane < nsum) {
		const float* arr = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : lane == 3 ? a3 : a4;
		float s = 0;
		int c = 0;
		// a skipped element adds +0 instead of branching: s starts at +0 and a sum that has +0 in it is never -0, so s + 0 == s bit for bit,
		// and the loads of the chain do not wait for a branch
#pragma unroll 5
		for (int i = 0; i < len; i++) {
			const bool ok = S.ok[i] != 0;
			s += ok ? arr[i] : 0.0f;
			c += ok;
		}
		S.sum[lane] = s;
		if (lane == 0) S.cnt = c;
	}
}

// KltTracker.setDescription :147-240 for one layer by one wave.  Writes the templates to tD / tX / tY (global) and leaves them in S.
// Returns 1 / 0 (the reference's boolean) or -1 where the reference throws.
template <class TI, class TD>
__device__ int kltDescribeLayer(const TI* img, const TD* dxI, const TD* dyI, int stride, int W, int H, int r, const bhip_klt_cfg& cfg, float x,
								float y, float* tD, float* tX, float* tY, float& Gxx, float& Gxy, float& Gyy, KltShared& S, int lane) {
	const int wF = 2 * r + 1, len = wF * wF;
	const KltBounds Bd(r, W, H);
	const bool inside = Bd.inside(x, y);
	if (!inside && Bd.outside(x, y)) return 0;
	KltSub B;
	KltRegion R;
	if (inside) {
		B.dx0 = 0; B.dy0 = 0; B.dx1 = wF; B.dy1 = wF; B.bad = false;
		R = kltRegion(x - r, y - r, wF, wF, W, H);
	} else {
		B = kltSubBounds(x, y, r, wF, W, H);
		if (B.bad) return -1;
		R = kltRegion(B.sx0, B.sy0, B.dx1 - B.dx0, B.dy1 - B.dy0, W, H);
	}
	if (R.bad) return -1;
	__syncthreads();   // the previous user of S is done
	for (int e = lane; e < len; e += 64) {
		const int j = e % wF, i = e / wF;
		const bool in = j >= B.dx0 && j < B.dx1 && i >= B.dy0 && i < B.dy1;
		// outside the visible part desc is NaN (ImageMiscOps.fill); the reference leaves derivX / derivY stale there and never reads them: 0 here
		float d = NAN, gx = 0, gy = 0;
		if (in) {
			d = kltRegionAt(R, img, stride, j - B.dx0, i - B.dy0);
			gx = kltRegionAt(R, dxI, stride, j - B.dx0, i - B.dy0);
			gy = kltRegionAt(R, dyI, stride, j - B.dx0, i - B.dy0);
		}
		S.D[e] = d; S.X[e] = gx; S.Y[e] = gy;
		tD[e] = d; tX[e] = gx; tY[e] = gy;
		S.pXX[e] = gx * gx; S.pYY[e] = gy * gy; S.pXY[e] = gx * gy;
		S.ok[e] = inside ? 1 : !(d != d);   // internalSetDescription sums every element, the border form skips NaN
	}
	__syncthreads();
	kltChains(S, lane, 3, len, S.pXX, S.pYY, S.pXY, nullptr, nullptr);
	__syncthreads();
	Gxx = S.sum[0]; Gyy = S.sum[1]; Gxy = S.sum[2];
	const int total = S.cnt;
	const float det = Gxx * Gyy - Gxy * Gxy;
	return det >= cfg.minDeterminant * total ? 1 : 0;
}

// PyramidKltTracker.setDescription :58-71 at (fx, fy) for the track of table entry g
template <class TI, class TD>
__device__ int kltDescribeTrack(const KltPyrT<TI, TD>& P, const KltTab& T, const bhip_klt_cfg& cfg, int b, int g, float fx, float fy, KltShared& S, int lane) {
	const long long n = (long long)T.batch * T.cap;
	for (int l = 0; l < P.numLayers; l++) {
		const float scale = P.scale[l];
		const float x = fx / scale, y = fy / scale;
		const long long o = (long long)b * P.frameStride + P.off[l];
		float* t = T.tmpl + ((long long)g * T.L + l) * 3 * T.len;
		float Gxx = 0, Gxy = 0, Gyy = 0;
		const int ok = kltDescribeLayer(P.img + o, P.dx + o, P.dy + o, P.stride[l], P.w[l], P.h[l], T.r, cfg, x, y, t, t + T.len, t + 2 * T.len, Gxx, Gxy, Gyy,
										S, lane);
		if (lane == 0) {
			T.lx[l * n + g] = x; T.ly[l * n + g] = y;
			T.gxx[l * n + g] = Gxx; T.gxy[l * n + g] = Gxy; T.gyy[l * n + g] = Gyy;
		}
		if (ok != 1) return ok;
	}
	return 1;
}

// KltTracker.track :251-325 on one layer; the template is in S (D, X, Y, pXX, pYY, pXY).  x, y move even when a fault is returned.
template <class TI>
__device__ int kltTrackLayer(const TI* img, int stride, int W, int H, int r, const bhip_klt_cfg& cfg, float& x, float& y, float sGxx, float sGxy,
							 float sGyy, float& error, int& iters, KltShared& S, int lane) {
	const int wF = 2 * r + 1, len = wF * wF;
	const KltBounds Bd(r, W, H);
	if (Bd.outside(x, y)) return BHIP_KLT_OUT_OF_BOUNDS;
	bool hole = false;
	for (int e = lane; e < len; e += 64) hole |= S.D[e] != S.D[e];
	const bool complete = __ballot(hole) == 0;   // isDescriptionComplete
	const float origX = x, origY = y;
	float Gxx = sGxx, Gyy = sGyy, Gxy = sGxy, det = 0;
	if (complete) {
		det = Gxx * Gyy - Gxy * Gxy;
		if (det < cfg.minDeterminant * len) return BHIP_KLT_FAILED;
	}
	for (int iter = 0; iter < cfg.maxIterations; iter++) {
		float Ex, Ey;
		iters++;
		if (complete && Bd.inside(x, y)) {   // computeE
			const KltRegion R = kltRegion(x - r, y - r, wF, wF, W, H);
			if (R.bad) return BHIP_KLT_REFERENCE_THROWS;
			__syncthreads();
			for (int e = lane; e < len; e += 64) {
				const float c = kltRegionAt(R, img, stride, e % wF, e / wF);
				const float d = S.D[e] - c;
				S.cur[e] = c;
				S.pEx[e] = d * S.X[e];
				S.pEy[e] = d * S.Y[e];
				S.ok[e] = 1;
			}
			__syncthreads();
			kltChains(S, lane, 2, len, S.pEx, S.pEy, nullptr, nullptr, nullptr);
			__syncthreads();
			Ex = S.sum[0]; Ey = S.sum[1];
		} else {                             // computeGandE_border
			iters += 1 << 16;
			const KltSub B = kltSubBounds(x, y, r, wF, W, H);
			if (B.bad) return BHIP_KLT_REFERENCE_THROWS;
			const KltRegion R = kltRegion(B.sx0, B.sy0, B.dx1 - B.dx0, B.dy1 - B.dy0, W, H);
			if (R.bad) return BHIP_KLT_REFERENCE_THROWS;
			__syncthreads();
			for (int e = lane; e < len; e += 64) {
				const int j = e % wF, i = e / wF;
				const bool in = j >= B.dx0 && j < B.dx1 && i >= B.dy0 && i < B.dy1;
				const float c = in ? kltRegionAt(R, img, stride, j - B.dx0, i - B.dy0) : NAN;
				const float t = S.D[e];
				const float d = t - c;
				S.cur[e] = c;
				S.pEx[e] = d * S.X[e];
				S.pEy[e] = d * S.Y[e];
				S.ok[e] = !(t != t || c != c);
			}
			__syncthreads();
			kltChains(S, lane, 5, len, S.pEx, S.pEy, S.pXX, S.pYY, S.pXY);
			__syncthreads();
			Ex = S.sum[0]; Ey = S.sum[1]; Gxx = S.sum[2]; Gyy = S.sum[3]; Gxy = S.sum[4];
			const int total = S.cnt;
			det = Gxx * Gyy - Gxy * Gxy;
			if (det <= cfg.minDeterminant * total) return BHIP_KLT_FAILED;
		}
		const float dx = (Gyy * Ex - Gxy * Ey) / det;
		const float dy = (Gxx * Ey - Gxy * Ex) / det;
		x += dx;
		y += dy;
		if (Bd.outside(x, y)) return BHIP_KLT_OUT_OF_BOUNDS;
		if (fabsf(x - origX) > wF || fabsf(y - origY) > wF) return BHIP_KLT_DRIFTED;
		if (fabsf(dx) < cfg.minPositionDelta && fabsf(dy) < cfg.minPositionDelta) break;
	}
	// computeError :346-359 against currDesc of the last iteration
	__syncthreads();
	for (int e = lane; e < len; e += 64) {
		const float t = S.D[e], c = S.cur[e];
		S.pEx[e] = fabsf(t - c);
		S.ok[e] = !(t != t || c != c);
	}
	__syncthreads();
	kltChains(S, lane, 1, len, S.pEx, nullptr, nullptr, nullptr, nullptr);
	__syncthreads();
	error = S.sum[0] / S.cnt;
	return error > cfg.maxPerPixelError ? BHIP_KLT_LARGE_ERROR : BHIP_KLT_SUCCESS;
}

// PyramidKltTracker.track :113-151 for every active track: fault, error and the new position (tx, ty; feature.x,y stay as they were)
template <class TI, class TD>
__global__ __launch_bounds__(64) void k_klt_track(KltPyrT<TI, TD> P, KltTab T, bhip_klt_cfg cfg) {
	__shared__ KltShared S;
	const int b = blockIdx.y, lane = threadIdx.x;
	if ((int)blockIdx.x >= T.nAct[b]) return;
	const int g = b * T.cap + T.act[b * T.cap + blockIdx.x];
	const long long n = (long long)T.batch * T.cap;
	float x = T.x[g], y = T.y[g], error = T.err[g];
	int fault = BHIP_KLT_SUCCESS, iters = 0;   // iters: Lucas-Kanade iterations of this track() | those that took the border form << 16
	for (int l = P.numLayers - 1; l >= 0; l--) {
		const float scale = P.scale[l];
		x /= scale;
		y /= scale;
		const float* t = T.tmpl + ((long long)g * T.L + l) * 3 * T.len;
		__syncthreads();
		for (int e = lane; e < T.len; e += 64) {
			const float d = t[e], gx = t[T.len + e], gy = t[2 * T.len + e];
			S.D[e] = d; S.X[e] = gx; S.Y[e] = gy;
			S.pXX[e] = gx * gx; S.pYY[e] = gy * gy; S.pXY[e] = gx * gy;
		}
		__syncthreads();
		float fx = x, fy = y;
		fault = kltTrackLayer(P.img + (long long)b * P.frameStride + P.off[l], P.stride[l], P.w[l], P.h[l], T.r, cfg, fx, fy, T.gxx[l * n + g],
							  T.gxy[l * n + g], T.gyy[l * n + g], error, iters, S, lane);
		if (lane == 0) { T.lx[l * n + g] = fx; T.ly[l * n + g] = fy; }
		if (fault != BHIP_KLT_SUCCESS) break;
		x = fx * scale;
		y = fy * scale;
	}
	if (lane == 0) {
		T.fault[g] = fault;
		T.err[g] = error;
		T.iters[g] = iters;
		if (fault == BHIP_KLT_SUCCESS) { T.tx[g] = x; T.ty[g] = y; }
	}
}

template <class TI, class TD>
__global__ __launch_bounds__(64) void k_klt_describe(KltPyrT<TI, TD> P, KltTab T, bhip_klt_cfg cfg, int mode, const int* count) {
	__shared__ KltShared S;
	const int lane = threadIdx.x;
	int b = blockIdx.y, g;
	float fx, fy;
	if (mode == 0 || mode == 2) {
		if ((int)blockIdx.x >= T.nAct[b]) return;
		g = b * T.cap + T.act[b * T.cap + blockIdx.x];
	} else if (mode == 1) {
		if ((int)blockIdx.x >= count[b]) return;
		g = b * T.cap + T.freeL[b * T.cap + T.nFree[b] - count[b] + blockIdx.x];
	} else {
		g = count[blockIdx.x];
		if (g < 0) return;
		b = g / T.cap;
	}
	if (mode == 0) {
		if (T.fault[g] != BHIP_KLT_SUCCESS) {
			if (lane == 0) T.keep[g] = 0;
			return;
		}
		fx = T.tx[g]; fy = T.ty[g];
		const int ix = (int)fx, iy = (int)fy;   // image.isInBounds((int)t.x, (int)t.y)
		if (!(ix >= 0 && ix < P.frameW && iy >= 0 && iy < P.frameH)) {
			if (lane == 0) T.keep[g] = 0;
			return;
		}
	} else {
		fx = T.x[g]; fy = T.y[g];
	}
	const int ok = kltDescribeTrack(P, T, cfg, b, g, fx, fy, S, lane);
	if (lane == 0) {
		// spawnTracks / addTrack do not look at setDescription's result (checkValidSpawn is always true): only a position where the
		// reference throws keeps a candidate from becoming a track
		T.keep[g] = mode == 1 ? ok >= 0 : ok == 1;
		if (ok < 0) T.fault[g] = BHIP_KLT_REFERENCE_THROWS;
		if (mode == 0 && ok == 1) { T.x[g] = fx; T.y[g] = fy; }
	}
}

// ---- list logic: one block per sequence, lists keep the reference's order ----
__global__ void k_klt_init(KltTab T, int firstSlot) {
	const int b = blockIdx.x;
	const int base = firstSlot == 0 ? 0 : T.nFree[b];
	__syncthreads();
	for (int s = firstSlot + threadIdx.x; s < T.cap; s += blockDim.x) T.freeL[b * T.cap + base + (s - firstSlot)] = s;
	if (threadIdx.x == 0) {
		T.nFree[b] = base + T.cap - firstSlot;
		if (firstSlot == 0) { T.nAct[b] = 0; T.nDrp[b] = 0; T.nSpw[b] = 0; T.total[b] = 0; }
	}
}

__global__ void k_klt_begin(KltTab T) {
	const int b = blockIdx.x;
	const int nd = T.nDrp[b], nf = T.nFree[b];
	__syncthreads();
	for (int i = threadIdx.x; i < nd; i += blockDim.x) T.freeL[b * T.cap + nf + i] = T.drp[b * T.cap + i];
	if (threadIdx.x == 0) { T.nFree[b] = nf + nd; T.nDrp[b] = 0; T.nSpw[b] = 0; }
}

// exclusive rank of `flag` among the 256 threads of the block and the block's total
__device__ __forceinline__ int kltRank256(bool flag, int* sh /*4*/, int& total) {
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const unsigned long long m = __ballot(flag);
	__syncthreads();
	if (lane == 0) sh[w] = __popcll(m);
	__syncthreads();
	int off = 0;
	total = 0;
	for (int k = 0; k < 4; k++) {
		if (k < w) off += sh[k];
		total += sh[k];
	}
	return off + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(256) void k_klt_compact(KltTab T, int toUnused) {
	__shared__ int sh[4];
	const int b = blockIdx.x, n = T.nAct[b];
	int* act = T.act + b * T.cap;
	int* out = toUnused ? T.freeL + b * T.cap : T.drp + b * T.cap;
	int nk = 0, nd = toUnused ? T.nFree[b] : T.nDrp[b];
	for (int c0 = 0; c0 < n; c0 += 256) {
		const int i = c0 + threadIdx.x;
		const int s = i < n ? act[i] : 0;
		const bool k = i < n && T.keep[b * T.cap + s] != 0, d = i < n && !k;
		int tk, td;
		const int rk = kltRank256(k, sh, tk);   // the barriers inside order every read of this chunk before the writes below
		const int rd = kltRank256(d, sh, td);
		if (k) act[nk + rk] = s;
		if (d) out[nd + rd] = s;
		nk += tk;
		nd += td;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		T.nAct[b] = nk;
		if (toUnused) T.nFree[b] = nd; else T.nDrp[b] = nd;
	}
}

// spawnTracks: the exclusion list -- Float.MAX_VALUE at ((int)(x / scaleBottom), (int)(y / scaleBottom)) of every active track
__global__ void k_klt_mark_exclude(KltTab T, float scale0, float* intensity, long long imageStride, int stride, int w, int h) {
	const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= T.nAct[b]) return;
	const int g = b * T.cap + T.act[b * T.cap + i];
	const int x = (int)(T.x[g] / scale0), y = (int)(T.y[g] / scale0);
	if (x >= 0 && x < w && y >= 0 && y < h) intensity[b * imageStride + (long long)y * stride + x] = FLT_MAX;
}

// candidate i of sequence b takes the slot at freeL[nFree - count + i] and the position pt * scaleBottom
__global__ void k_klt_spawn_place(KltTab T, const int16_t* xy, int xyCap, const int* count, float scale0) {
	const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count[b]) return;
	const int g = b * T.cap + T.freeL[b * T.cap + T.nFree[b] - count[b] + i];
	T.x[g] = xy[((long long)b * xyCap + i) * 2] * scale0;
	T.y[g] = xy[((long long)b * xyCap + i) * 2 + 1] * scale0;
	T.fault[g] = BHIP_KLT_SUCCESS;
	T.err[g] = 0;
	T.iters[g] = 0;
}

// candidates (all but those at a position where the reference throws) join active and spawned in detector order with
// featureId = totalFeatures++; the others stay unused
__global__ __launch_bounds__(256) void k_klt_spawn_commit(KltTab T, const int* count) {
	__shared__ int sh[4];
	const int b = blockIdx.x, n = count[b];
	int* fl = T.freeL + b * T.cap + T.nFree[b] - n;
	int na = T.nAct[b], ns = 0, nf = 0;
	const long long id0 = T.total[b];
	for (int c0 = 0; c0 < n; c0 += 256) {
		const int i = c0 + threadIdx.x;
		const int s = i < n ? fl[i] : 0;
		const bool k = i < n && T.keep[b * T.cap + s] != 0, d = i < n && !k;
		int tk, td;
		const int rk = kltRank256(k, sh, tk);
		const int rd = kltRank256(d, sh, td);
		if (k) {
			T.act[b * T.cap + na + rk] = s;
			T.spw[b * T.cap + ns + rk] = s;
			T.id[b * T.cap + s] = id0 + ns + rk;
		}
		if (d) fl[nf + rd] = s;
		na += tk; ns += tk; nf += td;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		T.nAct[b] = na;
		T.nSpw[b] = ns;
		T.nFree[b] = T.nFree[b] - n + nf;
		T.total[b] = id0 + ns;
	}
}

// addTrack(x, y), in call order: inside the frame -> a slot, appended to active whatever setDescription says, no featureId (-1 here).
// list[i] = table entry of request i, or -1
__global__ void k_klt_add(KltTab T, const int* seq, const double* xy, int n, int frameW, int frameH, unsigned char* ok, int* list) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	for (int i = 0; i < n; i++) {
		const int b = seq[i];
		const double x = xy[2 * i], y = xy[2 * i + 1];
		const int ix = (int)x, iy = (int)y;
		const bool in = b >= 0 && b < T.batch && ix >= 0 && ix < frameW && iy >= 0 && iy < frameH && T.nFree[b] > 0;
		ok[i] = in;
		list[i] = -1;
		if (!in) continue;
		const int s = T.freeL[b * T.cap + --T.nFree[b]];
		const int g = b * T.cap + s;
		T.act[b * T.cap + T.nAct[b]++] = s;
		T.x[g] = (float)x; T.y[g] = (float)y;
		T.id[g] = -1; T.fault[g] = BHIP_KLT_SUCCESS; T.err[g] = 0; T.iters[g] = 0;
		list[i] = g;
	}
}

__global__ void k_klt_keep_all(KltTab T) {
	const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < T.nAct[b]) T.keep[b * T.cap + T.act[b * T.cap + i]] = 1;
}
// dropTrack: the first active track of the sequence with that featureId that an earlier request has not taken
__global__ void k_klt_match_drop(KltTab T, const int* seq, const long long* id, int n, unsigned char* ok) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	for (int i = 0; i < n; i++) {
		const int b = seq[i];
		ok[i] = 0;
		if (b < 0 || b >= T.batch) continue;
		for (int k = 0; k < T.nAct[b]; k++) {
			const int g = b * T.cap + T.act[b * T.cap + k];
			if (T.keep[g] && T.id[g] == id[i]) { T.keep[g] = 0; ok[i] = 1; break; }
		}
	}
}

__global__ void k_klt_drop_all(KltTab T, int resetTotal) {
	const int b = blockIdx.x;
	const int na = T.nAct[b], nd = T.nDrp[b], nf = T.nFree[b];
	__syncthreads();
	for (int i = threadIdx.x; i < na; i += blockDim.x) T.freeL[b * T.cap + nf + i] = T.act[b * T.cap + i];
	for (int i = threadIdx.x; i < nd; i += blockDim.x) T.freeL[b * T.cap + nf + na + i] = T.drp[b * T.cap + i];
	if (threadIdx.x == 0) {
		T.nFree[b] = nf + na + nd; T.nAct[b] = 0; T.nDrp[b] = 0;
		if (resetTotal) T.total[b] = 0;
	}
}

__global__ void k_klt_gather(KltTab T, int which, int b, int n, long long* id, float* xy, int* fault, float* err) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int* list = which == 0 ? T.act : which == 1 ? T.spw : T.drp;
	const int g = b * T.cap + list[b * T.cap + i];
	id[i] = T.id[g];
	xy[2 * i] = T.x[g]; xy[2 * i + 1] = T.y[g];
	fault[i] = T.fault[g];
	err[i] = T.err[g];
}

// templates and G of one layer of the tracks of one list, in list order: tmpl [n][3][len] (desc, derivX, derivY), G [n][3] (Gxx, Gyy, Gxy)
__global__ __launch_bounds__(64) void k_klt_gather_templates(KltTab T, int which, int b, int layer, int n, float* tmpl, float* G) {
	const int i = blockIdx.x;
	if (i >= n) return;
	const int* list = which == 0 ? T.act : which == 1 ? T.spw : T.drp;
	const int g = b * T.cap + list[b * T.cap + i];
	const long long N = (long long)T.batch * T.cap;
	const float* t = T.tmpl + ((long long)g * T.L + layer) * 3 * T.len;
	for (int e = threadIdx.x; e < 3 * T.len; e += 64) tmpl[(long long)i * 3 * T.len + e] = t[e];
	if (threadIdx.x == 0) { G[3 * i] = T.gxx[layer * N + g]; G[3 * i + 1] = T.gyy[layer * N + g]; G[3 * i + 2] = T.gxy[layer * N + g]; }
}

// tracks, iterations and border-form iterations of the last process() over all sequences (its tracks are now in active or dropped)
__global__ __launch_bounds__(256) void k_klt_stats(KltTab T, unsigned long long* out) {
	const int b = blockIdx.x, na = T.nAct[b], nd = T.nDrp[b];
	unsigned long long it = 0, bd = 0;
	for (int i = threadIdx.x; i < na + nd; i += blockDim.x) {
		const int s = i < na ? T.act[b * T.cap + i] : T.drp[b * T.cap + i - na];
		const int v = T.iters[b * T.cap + s];
		it += v & 0xffff;
		bd += (unsigned)v >> 16;
	}
	if (it || bd) { atomicAdd(out + 1, it); atomicAdd(out + 2, bd); }
	if (threadIdx.x == 0) atomicAdd(out, (unsigned long long)(na + nd));
}

// ---- dense optical flow, generic form: one wave per pixel (DenseOpticalFlowKlt.process :78-98, the part before checkNeighbors) ----
// feature.setPosition(px, py); setDescription on the source pyramid (every layer, PyramidKltTracker :58-71), then track on the destination
// pyramid (:113-151).  The templates of all layers stay in dynamic LDS ([L][3][len], then Gxx, Gxy, Gyy of every layer): nothing goes to a
// track table.  The record holds the fault, and error and flow = (feature.x - px, feature.y - py) where the track succeeded (0 elsewhere).
template <class TI, class TD>
__global__ __launch_bounds__(64) void k_klt_flow_track(KltPyrT<TI, TD> P, const TI* dst, int r, bhip_klt_cfg cfg, FlowRec* rec, unsigned long long* stats) {
	__shared__ KltShared S;
	extern __shared__ float flowStore[];
	const int lane = threadIdx.x, px = blockIdx.x, py = blockIdx.y, b = blockIdx.z;
	const int len = (2 * r + 1) * (2 * r + 1);
	float* G = flowStore + P.numLayers * 3 * len;
	const long long frame = (long long)b * P.frameStride;
	const float fx0 = px, fy0 = py;
	int fault = BHIP_KLT_SUCCESS, iters = 0;
	for (int l = 0; l < P.numLayers; l++) {
		const float scale = P.scale[l];
		const long long o = frame + P.off[l];
		float* t = flowStore + l * 3 * len;
		float Gxx = 0, Gxy = 0, Gyy = 0;
		const int ok = kltDescribeLayer(P.img + o, P.dx + o, P.dy + o, P.stride[l], P.w[l], P.h[l], r, cfg, fx0 / scale, fy0 / scale, t, t + len, t + 2 * len, Gxx, Gxy,
										Gyy, S, lane);
		if (ok != 1) { fault = ok < 0 ? BHIP_KLT_REFERENCE_THROWS : BHIP_FLOW_NO_DESCRIPTION; break; }
		if (lane == 0) { G[3 * l] = Gxx; G[3 * l + 1] = Gxy; G[3 * l + 2] = Gyy; }
	}
	float x = fx0, y = fy0, error = 0;
	if (fault == BHIP_KLT_SUCCESS) {
		for (int l = P.numLayers - 1; l >= 0; l--) {
			const float scale = P.scale[l];
			x /= scale;
			y /= scale;
			const float* t = flowStore + l * 3 * len;
			__syncthreads();
			for (int e = lane; e < len; e += 64) {
				const float d = t[e], gx = t[len + e], gy = t[2 * len + e];
				S.D[e] = d; S.X[e] = gx; S.Y[e] = gy;
				S.pXX[e] = gx * gx; S.pYY[e] = gy * gy; S.pXY[e] = gx * gy;
			}
			__syncthreads();
			float fx = x, fy = y;
			fault = kltTrackLayer(dst + frame + P.off[l], P.stride[l], P.w[l], P.h[l], r, cfg, fx, fy, G[3 * l], G[3 * l + 1], G[3 * l + 2], error, iters, S, lane);
			if (fault != BHIP_KLT_SUCCESS) break;
			x = fx * scale;
			y = fy * scale;
		}
	}
	if (lane == 0) {
		const bool ok = fault == BHIP_KLT_SUCCESS;
		FlowRec R;
		R.fault = fault; R.error = ok ? error : 0.0f; R.dx = ok ? x - fx0 : 0.0f; R.dy = ok ? y - fy0 : 0.0f;
		rec[((long long)b * P.frameH + py) * P.frameW + px] = R;
		if (iters & 0xffff) atomicAdd(stats, (unsigned long long)(iters & 0xffff));
	}
}

// ---- launchers ----
#define KLT_DONE(ctx) do { BHIP_HIP(ctx, hipGetLastError()); return BHIP_OK; } while (0)

int bhip_launch_klt_init(bhip_ctx* ctx, KltTab T, int firstSlot) {
	hipLaunchKernelGGL(k_klt_init, dim3(T.batch), dim3(256), 0, ctx->stream, T, firstSlot);
	KLT_DONE(ctx);
}
int bhip_launch_klt_begin(bhip_ctx* ctx, KltTab T) {
	hipLaunchKernelGGL(k_klt_begin, dim3(T.batch), dim3(256), 0, ctx->stream, T);
	KLT_DONE(ctx);
}
int bhip_launch_klt_track(bhip_ctx* ctx, KltPyr P, KltTab T, bhip_klt_cfg cfg, int maxActive) {
	if (maxActive <= 0) return BHIP_OK;
	ProfScope prof(ctx, "k_klt_track");
	hipLaunchKernelGGL((k_klt_track<float, float>), dim3(maxActive, T.batch), dim3(64), 0, ctx->stream, P, T, cfg);
	KLT_DONE(ctx);
}
int bhip_launch_klt_track(bhip_ctx* ctx, KltPyrU8 P, KltTab T, bhip_klt_cfg cfg, int maxActive) {
	if (maxActive <= 0) return BHIP_OK;
	ProfScope prof(ctx, "k_klt_track_u8");
	hipLaunchKernelGGL((k_klt_track<uint8_t, int16_t>), dim3(maxActive, T.batch), dim3(64), 0, ctx->stream, P, T, cfg);
	KLT_DONE(ctx);
}
int bhip_launch_klt_describe(bhip_ctx* ctx, KltPyr P, KltTab T, bhip_klt_cfg cfg, int mode, const int* count, int maxCount) {
	if (maxCount <= 0) return BHIP_OK;
	ProfScope prof(ctx, "k_klt_describe");
	hipLaunchKernelGGL((k_klt_describe<float, float>), dim3(maxCount, mode == 3 ? 1 : T.batch), dim3(64), 0, ctx->stream, P, T, cfg, mode, count);
	KLT_DONE(ctx);
}
int bhip_launch_klt_describe(bhip_ctx* ctx, KltPyrU8 P, KltTab T, bhip_klt_cfg cfg, int mode, const int* count, int maxCount) {
	if (maxCount <= 0) return BHIP_OK;
	ProfScope prof(ctx, "k_klt_describe_u8");
	hipLaunchKernelGGL((k_klt_describe<uint8_t, int16_t>), dim3(maxCount, mode == 3 ? 1 : T.batch), dim3(64), 0, ctx->stream, P, T, cfg, mode, count);
	KLT_DONE(ctx);
}
int bhip_launch_klt_compact(bhip_ctx* ctx, KltTab T, int toUnused) {
	ProfScope prof(ctx, "k_klt_compact");
	hipLaunchKernelGGL(k_klt_compact, dim3(T.batch), dim3(256), 0, ctx->stream, T, toUnused);
	KLT_DONE(ctx);
}
int bhip_launch_klt_mark_exclude(bhip_ctx* ctx, KltTab T, float scale0, DevImg<float> intensity, int maxActive) {
	if (maxActive <= 0) return BHIP_OK;
	hipLaunchKernelGGL(k_klt_mark_exclude, dim3((maxActive + 255) / 256, T.batch), dim3(256), 0, ctx->stream, T, scale0, intensity.data, intensity.imageStride,
					   intensity.stride, intensity.width, intensity.height);
	KLT_DONE(ctx);
}
int bhip_launch_klt_spawn_place(bhip_ctx* ctx, KltTab T, const int16_t* xy, int xyCap, const int* count, float scale0, int maxCount) {
	if (maxCount <= 0) return BHIP_OK;
	hipLaunchKernelGGL(k_klt_spawn_place, dim3((maxCount + 255) / 256, T.batch), dim3(256), 0, ctx->stream, T, xy, xyCap, count, scale0);
	KLT_DONE(ctx);
}
int bhip_launch_klt_spawn_commit(bhip_ctx* ctx, KltTab T, const int* count) {
	hipLaunchKernelGGL(k_klt_spawn_commit, dim3(T.batch), dim3(256), 0, ctx->stream, T, count);
	KLT_DONE(ctx);
}
int bhip_launch_klt_add(bhip_ctx* ctx, KltTab T, const int* seq, const double* xy, int n, int frameW, int frameH, unsigned char* ok, int* list) {
	hipLaunchKernelGGL(k_klt_add, dim3(1), dim3(64), 0, ctx->stream, T, seq, xy, n, frameW, frameH, ok, list);
	KLT_DONE(ctx);
}
int bhip_launch_klt_match_drop(bhip_ctx* ctx, KltTab T, const int* seq, const long long* id, int n, unsigned char* ok, int maxActive) {
	if (maxActive > 0) hipLaunchKernelGGL(k_klt_keep_all, dim3((maxActive + 255) / 256, T.batch), dim3(256), 0, ctx->stream, T);
	hipLaunchKernelGGL(k_klt_match_drop, dim3(1), dim3(64), 0, ctx->stream, T, seq, id, n, ok);
	KLT_DONE(ctx);
}
int bhip_launch_klt_drop_all(bhip_ctx* ctx, KltTab T, int resetTotal) {
	hipLaunchKernelGGL(k_klt_drop_all, dim3(T.batch), dim3(256), 0, ctx->stream, T, resetTotal);
	KLT_DONE(ctx);
}
int bhip_launch_klt_stats(bhip_ctx* ctx, KltTab T, unsigned long long* out) {
	hipLaunchKernelGGL(k_klt_stats, dim3(T.batch), dim3(256), 0, ctx->stream, T, out);
	KLT_DONE(ctx);
}
int bhip_launch_klt_gather_templates(bhip_ctx* ctx, KltTab T, int which, int seq, int layer, int n, float* tmpl, float* G) {
	if (n <= 0) return BHIP_OK;
	hipLaunchKernelGGL(k_klt_gather_templates, dim3(n), dim3(64), 0, ctx->stream, T, which, seq, layer, n, tmpl, G);
	KLT_DONE(ctx);
}
int bhip_launch_klt_gather(bhip_ctx* ctx, KltTab T, int which, int seq, int n, long long* id, float* xy, int* fault, float* err) {
	if (n <= 0) return BHIP_OK;
	hipLaunchKernelGGL(k_klt_gather, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, T, which, seq, n, id, xy, fault, err);
	KLT_DONE(ctx);
}
template <class TI, class TD>
static int flowTrackWave(bhip_ctx* ctx, const char* tag, KltPyrT<TI, TD> P, const TI* dst, int r, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats) {
	ProfScope prof(ctx, tag);
	const size_t lds = ((size_t)P.numLayers * 3 * (2 * r + 1) * (2 * r + 1) + 3 * P.numLayers) * sizeof(float);
	hipLaunchKernelGGL((k_klt_flow_track<TI, TD>), dim3(P.frameW, P.frameH, batch), dim3(64), lds, ctx->stream, P, dst, r, cfg, rec, stats);
	KLT_DONE(ctx);
}
int bhip_launch_flow_track_wave(bhip_ctx* ctx, KltPyr P, const float* dst, int r, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats) {
	return flowTrackWave(ctx, "k_flow_track_wave", P, dst, r, cfg, batch, rec, stats);
}
int bhip_launch_flow_track_wave(bhip_ctx* ctx, KltPyrU8 P, const uint8_t* dst, int r, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats) {
	return flowTrackWave(ctx, "k_flow_track_wave_u8", P, dst, r, cfg, batch, rec, stats);
}
