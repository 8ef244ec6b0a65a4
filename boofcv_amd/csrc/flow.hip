// Dense KLT optical flow: DenseOpticalFlowKlt behind FactoryDenseOpticalFlow.flowKlt.
//   F:alg/flow/DenseOpticalFlowKlt.java:62-131, F:abst/flow/FlowKlt_to_DenseOpticalFlow.java:76-86, F:factory/flow/FactoryDenseOpticalFlow.java:61-82
//   F:alg/tracker/klt/KltTracker.java:147-495, PyramidKltTracker.java:58-151 (the arithmetic, shared with klt.hip through klt_dev.h)
//
// Two stages.  The track stage runs the reference's per-pixel work -- feature.setPosition(x, y), setDescription on the source pyramid, track on
// the destination pyramid -- for every pixel independently and leaves one FlowRec per pixel.  The reduce stage is checkNeighbors without its
// raster-order loop (below).
//
// Track stage, lane-per-pixel form (radius 1..3): a wave owns 64 consecutive pixels of a row and each lane runs the reference's loops over the
// (2r+1)^2 template elements itself, so every sum the Java forms in one fp32 chain (Gxx, Gyy, Gxy, Ex, Ey, the error) is that chain in that
// order with no cross-lane step; nothing is contracted (-ffp-contract=off).  A lane's three templates of the current layer (desc, derivX,
// derivY) live in LDS laid out [array][element][lane]: the 64 lanes of a wave touch 64 consecutive dwords, one per bank, so no access
// conflicts; that is 3 (2r+1)^2 256 B per wave -- 6.75 KB, 18.75 KB, 36.75 KB at r = 1, 2, 3 -- and with one wave per block the 160 KB of a CU
// hold 23, 8 and 4 waves.  The LDS of a lane is private to it: the kernel has no barrier.  setDescription is evaluated for every layer first
// (it returns false before any tracking starts); the templates are then formed again layer by layer from the top down, just before the layer
// is tracked -- they depend only on the integer pixel and the source pyramid -- so no template goes to global memory.  Iteration counts differ
// between lanes; finished lanes idle under the exec mask.
// The generic form (one wave per pixel, any radius up to 7) is k_klt_flow_track in klt.hip.
//
// Reduce stage.  Call pixel q a success with (score_q, flow_q) when its own track succeeded.  In the reference, slot p is visited by the
// checkNeighbors of every success in its clipped window, in raster order, and by its own unconditional write (score_p * 0.7f, flow_p) at
// time p, which wipes what earlier pixels left.  So the value of slot p is a fold in raster order over: the own entry, when p succeeded,
// followed by the successes after p; or, when p failed, all successes of the window.  The fold is the reference's own test, on the stored
// fp32 values: replace when the held score is greater, or equal with a strictly greater motion x^2 + y^2.  One thread per slot runs that fold
// over a tile of records staged in LDS with its halo.  Where nothing was written the slot is (NaN, 0): markInvalid() of a new ImageFlow.
#include "common.h"
#include "klt_dev.h"
#include <cfloat>
#include <cmath>

extern __shared__ float flowLds[];   // [3][len][64]: desc, derivX, derivY of the lane's current layer

#define FLOW_D(e) flowLds[(e) * 64 + lane]
#define FLOW_X(e) flowLds[(LEN + (e)) * 64 + lane]
#define FLOW_Y(e) flowLds[(2 * LEN + (e)) * 64 + lane]

// KltTracker.setDescription :147-240 for one layer by one lane; the templates go to the lane's LDS column.  Returns 1 / 0 (the reference's
// boolean) or -1 where the reference throws.  hole: desc has a NaN (isDescriptionComplete is false).
template <int RAD, class TI, class TD>
__device__ __forceinline__ int flowDescribe(const TI* img, const TD* dxI, const TD* dyI, int stride, int W, int H, const bhip_klt_cfg& cfg, float x, float y, int lane,
											float& Gxx, float& Gxy, float& Gyy, bool& hole) {
	constexpr int WF = 2 * RAD + 1, LEN = WF * WF;
	const KltBounds Bd(RAD, W, H);
	const bool inside = Bd.inside(x, y);
	if (!inside && Bd.outside(x, y)) return 0;
	KltSub B;
	KltRegion R;
	if (inside) {
		B.dx0 = 0; B.dy0 = 0; B.dx1 = WF; B.dy1 = WF; B.bad = false;
		R = kltRegion(x - RAD, y - RAD, WF, WF, W, H);
	} else {
		B = kltSubBounds(x, y, RAD, WF, W, H);
		if (B.bad) return -1;
		R = kltRegion(B.sx0, B.sy0, B.dx1 - B.dx0, B.dy1 - B.dy0, W, H);
	}
	if (R.bad) return -1;
	float sxx = 0, syy = 0, sxy = 0;
	int total = 0;
	hole = false;
	for (int i = 0; i < WF; i++) {
		for (int j = 0; j < WF; j++) {
			const int e = i * WF + j;
			const bool in = j >= B.dx0 && j < B.dx1 && i >= B.dy0 && i < B.dy1;
			// outside the visible part desc is NaN; the reference leaves derivX / derivY stale there and never reads them: 0 here
			float d = NAN, gx = 0, gy = 0;
			if (in) {
				d = kltRegionAt(R, img, stride, j - B.dx0, i - B.dy0);
				gx = kltRegionAt(R, dxI, stride, j - B.dx0, i - B.dy0);
				gy = kltRegionAt(R, dyI, stride, j - B.dx0, i - B.dy0);
			}
			FLOW_D(e) = d; FLOW_X(e) = gx; FLOW_Y(e) = gy;
			hole |= d != d;
			// internalSetDescription sums every element, the border form skips NaN.  A skipped element adds +0: a sum that started at +0 is
			// never -0, so s + 0 == s bit for bit
			const bool ok = inside || !(d != d);
			sxx += ok ? gx * gx : 0.0f;
			syy += ok ? gy * gy : 0.0f;
			sxy += ok ? gx * gy : 0.0f;
			total += ok;
		}
	}
	Gxx = sxx; Gyy = syy; Gxy = sxy;
	const float det = Gxx * Gyy - Gxy * Gxy;
	return det >= cfg.minDeterminant * total ? 1 : 0;
}

// KltTracker.track :251-325 on one layer by one lane; the template is in the lane's LDS column.  computeError's sum runs along with every
// iteration (same elements, same order), so currDesc is not kept: the value of the last iteration is the one the reference computes.
template <int RAD, class TI>
__device__ __forceinline__ int flowTrackLayer(const TI* img, int stride, int W, int H, const bhip_klt_cfg& cfg, float& x, float& y, float sGxx, float sGxy, float sGyy,
											  bool hole, int lane, float& error, int& iters) {
	constexpr int WF = 2 * RAD + 1, LEN = WF * WF;
	const KltBounds Bd(RAD, W, H);
	if (Bd.outside(x, y)) return BHIP_KLT_OUT_OF_BOUNDS;
	const bool complete = !hole;
	const float origX = x, origY = y;
	float Gxx = sGxx, Gyy = sGyy, Gxy = sGxy, det = 0;
	if (complete) {
		det = Gxx * Gyy - Gxy * Gxy;
		if (det < cfg.minDeterminant * LEN) return BHIP_KLT_FAILED;
	}
	float errSum = 0;
	int errCnt = 0;
	for (int iter = 0; iter < cfg.maxIterations; iter++) {
		iters++;
		const bool border = !(complete && Bd.inside(x, y));   // computeGandE_border, else computeE
		KltSub B;
		KltRegion R;
		if (border) {
			B = kltSubBounds(x, y, RAD, WF, W, H);
			if (B.bad) return BHIP_KLT_REFERENCE_THROWS;
			R = kltRegion(B.sx0, B.sy0, B.dx1 - B.dx0, B.dy1 - B.dy0, W, H);
		} else {
			B.dx0 = 0; B.dy0 = 0; B.dx1 = WF; B.dy1 = WF;
			R = kltRegion(x - RAD, y - RAD, WF, WF, W, H);
		}
		if (R.bad) return BHIP_KLT_REFERENCE_THROWS;
		float Ex = 0, Ey = 0, bxx = 0, byy = 0, bxy = 0;
		int total = 0;
		errSum = 0;
		errCnt = 0;
		for (int i = 0; i < WF; i++) {
			for (int j = 0; j < WF; j++) {
				const int e = i * WF + j;
				const bool in = j >= B.dx0 && j < B.dx1 && i >= B.dy0 && i < B.dy1;
				const float c = in ? kltRegionAt(R, img, stride, j - B.dx0, i - B.dy0) : NAN;
				const float t = FLOW_D(e), gx = FLOW_X(e), gy = FLOW_Y(e);
				const float d = t - c;
				const bool valid = !(t != t || c != c);
				const bool ok = !border || valid;   // computeE sums every element
				Ex += ok ? d * gx : 0.0f;
				Ey += ok ? d * gy : 0.0f;
				bxx += valid ? gx * gx : 0.0f;
				byy += valid ? gy * gy : 0.0f;
				bxy += valid ? gx * gy : 0.0f;
				total += valid;
				errSum += valid ? fabsf(d) : 0.0f;   // computeError :346-359
				errCnt += valid;
			}
		}
		if (border) {
			Gxx = bxx; Gyy = byy; Gxy = bxy;
			det = Gxx * Gyy - Gxy * Gxy;
			if (det <= cfg.minDeterminant * total) return BHIP_KLT_FAILED;
		}
		const float dx = (Gyy * Ex - Gxy * Ey) / det;
		const float dy = (Gxx * Ey - Gxy * Ex) / det;
		x += dx;
		y += dy;
		if (Bd.outside(x, y)) return BHIP_KLT_OUT_OF_BOUNDS;
		if (fabsf(x - origX) > WF || fabsf(y - origY) > WF) return BHIP_KLT_DRIFTED;
		if (fabsf(dx) < cfg.minPositionDelta && fabsf(dy) < cfg.minPositionDelta) break;
	}
	error = errSum / errCnt;
	return error > cfg.maxPerPixelError ? BHIP_KLT_LARGE_ERROR : BHIP_KLT_SUCCESS;
}

template <int RAD, class TI, class TD>
__global__ __launch_bounds__(64) void k_flow_track_lane(KltPyrT<TI, TD> P, const TI* dst, bhip_klt_cfg cfg, FlowRec* rec, unsigned long long* stats) {
	const int lane = threadIdx.x, px = blockIdx.x * 64 + lane, py = blockIdx.y, b = blockIdx.z;
	const long long frame = (long long)b * P.frameStride;
	const int top = P.numLayers - 1;
	int iters = 0;
	if (px < P.frameW) {
		const float fx0 = px, fy0 = py;
		int fault = BHIP_KLT_SUCCESS;
		float Gxx = 0, Gxy = 0, Gyy = 0;
		bool hole = false;
		// PyramidKltTracker.setDescription :58-71: false as soon as one layer says false.  The last layer described is the first one tracked.
		for (int l = 0; l <= top; l++) {
			const float scale = P.scale[l];
			const long long o = frame + P.off[l];
			const int ok = flowDescribe<RAD>(P.img + o, P.dx + o, P.dy + o, P.stride[l], P.w[l], P.h[l], cfg, fx0 / scale, fy0 / scale, lane, Gxx, Gxy, Gyy, hole);
			if (ok != 1) { fault = ok < 0 ? BHIP_KLT_REFERENCE_THROWS : BHIP_FLOW_NO_DESCRIPTION; break; }
		}
		float x = fx0, y = fy0, error = 0;
		if (fault == BHIP_KLT_SUCCESS) {
			for (int l = top; l >= 0; l--) {   // PyramidKltTracker.track :113-151
				const float scale = P.scale[l];
				const long long o = frame + P.off[l];
				x /= scale;
				y /= scale;
				if (l != top) flowDescribe<RAD>(P.img + o, P.dx + o, P.dy + o, P.stride[l], P.w[l], P.h[l], cfg, fx0 / scale, fy0 / scale, lane, Gxx, Gxy, Gyy, hole);
				float fx = x, fy = y;
				fault = flowTrackLayer<RAD>(dst + o, P.stride[l], P.w[l], P.h[l], cfg, fx, fy, Gxx, Gxy, Gyy, hole, lane, error, iters);
				if (fault != BHIP_KLT_SUCCESS) break;
				x = fx * scale;
				y = fy * scale;
			}
		}
		const bool ok = fault == BHIP_KLT_SUCCESS;
		FlowRec R;
		R.fault = fault; R.error = ok ? error : 0.0f; R.dx = ok ? x - fx0 : 0.0f; R.dy = ok ? y - fy0 : 0.0f;
		rec[((long long)b * P.frameH + py) * P.frameW + px] = R;
	}
	for (int s = 32; s > 0; s >>= 1) iters += __shfl_xor(iters, s);
	if (lane == 0 && iters) atomicAdd(stats, (unsigned long long)iters);
}

// ---- reduce ----
#define FLOW_TX 32
#define FLOW_TY 8
#define FLOW_TILE_MAX ((FLOW_TX + 2 * BHIP_KLT_MAX_RADIUS) * (FLOW_TY + 2 * BHIP_KLT_MAX_RADIUS))

__global__ __launch_bounds__(FLOW_TX* FLOW_TY) void k_flow_reduce(const FlowRec* rec, int r, DevImg<float> flow) {
	__shared__ FlowRec tile[FLOW_TILE_MAX];
	const int W = flow.width, H = flow.height, b = blockIdx.z;
	const int tw = FLOW_TX + 2 * r, th = FLOW_TY + 2 * r;
	const int x0 = blockIdx.x * FLOW_TX - r, y0 = blockIdx.y * FLOW_TY - r;
	const int tid = threadIdx.y * FLOW_TX + threadIdx.x;
	rec += (long long)b * W * H;
	for (int i = tid; i < tw * th; i += FLOW_TX * FLOW_TY) {
		const int gx = x0 + i % tw, gy = y0 + i / tw;
		FlowRec v;
		v.fault = -1; v.error = 0; v.dx = 0; v.dy = 0;   // outside the image: no pixel
		if (gx >= 0 && gx < W && gy >= 0 && gy < H) v = rec[(long long)gy * W + gx];
		tile[i] = v;
	}
	__syncthreads();
	const int px = blockIdx.x * FLOW_TX + threadIdx.x, py = blockIdx.y * FLOW_TY + threadIdx.y;
	if (px >= W || py >= H) return;
	const bool ownOk = tile[(py - y0) * tw + (px - x0)].fault == BHIP_KLT_SUCCESS;
	float bs = FLT_MAX, bx = NAN, by = 0;   // scores[] = Float.MAX_VALUE, markInvalid() on a new ImageFlow.D
	const int wy0 = max(0, py - r), wy1 = min(H, py + r + 1), wx0 = max(0, px - r), wx1 = min(W, px + r + 1);
	for (int wy = wy0; wy < wy1; wy++) {
		for (int wx = wx0; wx < wx1; wx++) {
			const FlowRec q = tile[(wy - y0) * tw + (wx - x0)];
			if (q.fault != BHIP_KLT_SUCCESS) continue;
			if (wy == py && wx == px) {   // the own write :91-92; its own checkNeighbors visit changes nothing
				bs = q.error * 0.7f; bx = q.dx; by = q.dy;
				continue;
			}
			if (ownOk && (wy < py || (wy == py && wx < px))) continue;   // wiped by the own write
			const float score = q.error;
			bool take = bs > score;
			if (!take && bs == score) {   // "Pick solution with the least motion when ambiguous"
				const float m0 = bx * bx + by * by;
				const float m1 = q.dx * q.dx + q.dy * q.dy;
				take = m1 < m0;
			}
			if (take) { bs = score; bx = q.dx; by = q.dy; }
		}
	}
	float* o = flow.data + (long long)b * flow.imageStride + (long long)py * flow.stride + 2 * px;
	o[0] = bx;
	o[1] = by;
}

// ---- launchers ----
template <int RAD, class TI, class TD>
static void flowLaunchLane(bhip_ctx* ctx, KltPyrT<TI, TD> P, const TI* dst, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats) {
	constexpr size_t lds = (size_t)3 * (2 * RAD + 1) * (2 * RAD + 1) * 64 * sizeof(float);
	hipLaunchKernelGGL((k_flow_track_lane<RAD, TI, TD>), dim3((P.frameW + 63) / 64, P.frameH, batch), dim3(64), lds, ctx->stream, P, dst, cfg, rec, stats);
}
template <class TI, class TD>
static int flowTrackLane(bhip_ctx* ctx, const char* tag, KltPyrT<TI, TD> P, const TI* dst, int r, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats) {
	if (r < 1 || r > BHIP_FLOW_LANE_MAX_RADIUS) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "the lane-per-pixel flow kernel takes radius 1..3");
	ProfScope prof(ctx, tag);
	if (r == 1) flowLaunchLane<1>(ctx, P, dst, cfg, batch, rec, stats);
	else if (r == 2) flowLaunchLane<2>(ctx, P, dst, cfg, batch, rec, stats);
	else flowLaunchLane<3>(ctx, P, dst, cfg, batch, rec, stats);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
int bhip_launch_flow_track_lane(bhip_ctx* ctx, KltPyr P, const float* dst, int r, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats) {
	return flowTrackLane(ctx, "k_flow_track_lane", P, dst, r, cfg, batch, rec, stats);
}
int bhip_launch_flow_track_lane(bhip_ctx* ctx, KltPyrU8 P, const uint8_t* dst, int r, bhip_klt_cfg cfg, int batch, FlowRec* rec, unsigned long long* stats) {
	return flowTrackLane(ctx, "k_flow_track_lane_u8", P, dst, r, cfg, batch, rec, stats);
}
int bhip_launch_flow_reduce(bhip_ctx* ctx, const FlowRec* rec, int r, DevImg<float> flow) {
	ProfScope prof(ctx, "k_flow_reduce");
	hipLaunchKernelGGL(k_flow_reduce, dim3((flow.width + FLOW_TX - 1) / FLOW_TX, (flow.height + FLOW_TY - 1) / FLOW_TY, flow.batch), dim3(FLOW_TX, FLOW_TY), 0,
					   ctx->stream, rec, r, flow);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
