// K8: pyramid layer steps of boofcv-ip (down-sampling convolution on GrayF32 and GrayU8, the fused layer kernel, batched image copies).
// The float forms keep the reference's evaluation order with no FMA contraction; the integer forms are exact.
#include "ip_dev.h"

// ---------------- down-sampling convolution (pyramid layer step) ----------------
// ConvolveImageDownNormalized.horizontal/vertical   I:alg/filter/convolve/ConvolveImageDownNormalized.java:53-86
//   interior  I:alg/filter/convolve/down/ConvolveDownNoBorderUnrolled_F32_F32.java:140-154,351-366 (widths 3..11, first tap assigns)
//             I:alg/filter/convolve/down/ConvolveDownNoBorderStandard.java:43-110 (total = 0 first)
//   border    I:alg/filter/convolve/down/ConvolveDownNormalized_JustBorder.java:43-139
//   naive     I:alg/filter/convolve/down/ConvolveDownNormalizedNaive.java:40-94 (kernel.width >= image.width)
//   ranges    I:alg/filter/convolve/down/UtilDownConvolve.java:27-44
// The reference runs interior, then left border, then right border; a later loop overwrites an earlier one.  Per output index D
// along the filtered axis that order collapses to: right border if D*skip in [offsetEnd, sideTrunc); else left border if
// D*skip < offset; else interior centred on D*skip + offset%skip while that is <= maxSide; else the pixel is not written.
// (offset%skip != 0 only for skip >= 3 with radius > skip: the reference then samples off-grid and leaves one column untouched;
// reproduced as is.)
struct ConvDownParams {
	const float* in;
	float* out;
	long long inImageStride, outImageStride;
	int inStride, outStride, width, height;   // input size
	int skip, kw, radius;
	int unrolled, naive;
	int offset, offsetRem, maxSide, offsetEnd, sideTrunc;   // along the filtered axis
	int skipInterior;   // general kernel only: the interior outputs have been written by a streaming kernel
	float k[BHIP_MAX_TAPS];
};

template <bool VERTICAL>
__global__ __launch_bounds__(256) void k_conv_down(ConvDownParams P) {
	int ox = blockIdx.x * blockDim.x + threadIdx.x;
	int oy = blockIdx.y;
	const int outW = VERTICAL ? P.width : P.width / P.skip;
	if (P.skipInterior) {
		// border fix-up after a streaming kernel: the grid covers only the outputs whose centre lies left of `offset` or at / beyond
		// `offsetEnd` (horizontal: flat grid, consecutive threads take the border columns of one row, then the next row)
		const int outSide = (VERTICAL ? P.height : P.width) / P.skip;
		const int nl = min((P.offset + P.skip - 1) / P.skip, outSide), dR0 = max(nl, min((P.offsetEnd + P.skip - 1) / P.skip, outSide));
		const int nb = nl + (outSide - dR0);
		if (nb <= 0) return;
		int t;
		if (VERTICAL) { t = oy; }
		else { oy = ox / nb; t = ox - oy * nb; if (oy >= P.height) return; }
		if (t >= nb) return;
		const int D = t < nl ? t : dR0 + (t - nl);
		if (VERTICAL) oy = D; else ox = D;
	}
	if (ox >= outW) return;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	const int D = VERTICAL ? oy : ox;
	const int side = VERTICAL ? P.height : P.width;
	const long long step = VERTICAL ? P.inStride : 1;
	const int r = P.radius;
	int centre = D * P.skip;
	int k0, k1;   // tap range [k0,k1] relative to the centre
	bool normalise = true;
	if (P.naive) {
		k0 = max(-r, -centre);
		k1 = min(r, side - 1 - centre);
	} else if (centre >= P.offsetEnd && centre < P.sideTrunc) {
		k0 = -r;
		k1 = min(r, side - centre - 1);
	} else if (centre < P.offset) {
		k0 = -centre;
		k1 = r;
	} else {
		centre += P.offsetRem;
		if (centre > P.maxSide || P.skipInterior) return;
		k0 = -r; k1 = r;
		normalise = false;
	}
	const float* src = VERTICAL ? img + (long long)centre * P.inStride + ox : img + (long long)oy * P.inStride + centre;
	float result;
	if (normalise) {
		float total = 0, weight = 0;
		for (int k = k0; k <= k1; k++) {
			const float w = P.k[k + r];
			weight += w;
			total += src[k * step] * w;
		}
		result = total / weight;
	} else {
		const float* s0 = src - r * step;
		result = P.unrolled ? tapsUnrolled(s0, step, P.k, P.kw) : tapsStandard(s0, step, P.k, P.kw);
	}
	P.out[(long long)blockIdx.z * P.outImageStride + (long long)oy * P.outStride + ox] = result;
}

// ---- streaming forms for skip 2 and the unrolled widths 3 and 5 (the discrete pyramid's usual layer step) ----
// Only INTERIOR outputs (the closed form above) are written here; the general kernel adds the border outputs afterwards (skipInterior).
__device__ __forceinline__ bool downInterior(const ConvDownParams& P, int D) {
	const int centre = D * P.skip;
	if (centre >= P.offsetEnd && centre < P.sideTrunc) return false;   // right border
	if (centre < P.offset) return false;                               // left border
	return centre + P.offsetRem <= P.maxSide;
}
// Horizontal: lane l owns input columns 4l..4l+3 of a 256-column strip = outputs 2l, 2l+1 (centres 4l and 4l+2; the kernel reaches at most
// two columns into the neighbouring chunks, which arrive by lane shifts); rows as in k_conv_h_stream.
#define CD_ROWS 8
template <int KW>
__global__ __launch_bounds__(256) void k_conv_down_h_stream(ConvDownParams P) {
	constexpr int R = KW / 2, NB = 4;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x = blockIdx.x * 256 + 4 * lane;          // first input column of this lane
	const int y0 = (blockIdx.y * 4 + wave) * CD_ROWS;
	if (x >= P.width || y0 >= P.height) return;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	float* outImg = P.out + (long long)blockIdx.z * P.outImageStride;
	const int yEnd = min(y0 + CD_ROWS, P.height);
	const int outW = P.width / 2;
	const int D0 = x >> 1;                              // outputs D0, D0 + 1
	const bool w0 = D0 < outW && downInterior(P, D0), w1 = D0 + 1 < outW && downInterior(P, D0 + 1);
	const bool first = lane == 0, last = lane == 63;
	float4 own[NB], edge[NB];
	auto fetch = [&](float4& own, float4& edge, int y) {
		if (y < yEnd) {
			const float* row = img + (long long)y * P.inStride;
			own = loadRow4(row, x, P.width);
			if (first) edge = loadRow4(row, x - 4, P.width);
			if (last) edge = loadRow4(row, x + 4, P.width);
		}
	};
	auto emit = [&](const float4& own, const float4& edge, int y) {
		if (y >= yEnd) return;   // wave-uniform
		float4 lf, rt;
		lf.z = __shfl_up(own.z, 1, 64); lf.w = __shfl_up(own.w, 1, 64);
		rt.x = __shfl_down(own.x, 1, 64);
		if (first) { lf.z = edge.z; lf.w = edge.w; }
		if (last) rt.x = edge.x;
		// v[i] = input column x - 2 + i
		const float v[7] = {lf.z, lf.w, own.x, own.y, own.z, own.w, rt.x};
		float r[2];
#pragma unroll
		for (int j = 0; j < 2; j++) {
			// centre x + 2 j = v[2 + 2 j]; taps centre - R .. centre + R, first tap assigns (ConvolveDownNoBorderUnrolled_F32_F32)
			float total = v[2 + 2 * j - R] * P.k[0];
#pragma unroll
			for (int i = 1; i < KW; i++) total += v[2 + 2 * j - R + i] * P.k[i];
			r[j] = total;
		}
		float* dst = outImg + (long long)y * P.outStride + D0;
		if (w0 && w1) *reinterpret_cast<float2*>(dst) = make_float2(r[0], r[1]);
		else { if (w0) dst[0] = r[0]; if (w1) dst[1] = r[1]; }
	};
#pragma unroll
	for (int q = 0; q < NB; q++) fetch(own[q], edge[q], y0 + q);
	for (int y = y0; y < yEnd; y += NB) {
#pragma unroll
		for (int q = 0; q < NB; q++) {
			emit(own[q], edge[q], y + q);
			fetch(own[q], edge[q], y + q + NB);
		}
	}
}
// Vertical: lane l owns columns 4l..4l+3; a wave produces CD_ROWS_V output rows, walking the 2 CD_ROWS_V + KW - 2 input rows it needs once
// through a register window of KW rows (two new rows per output).
#define CD_ROWS_V 8
template <int KW>
__global__ __launch_bounds__(256) void k_conv_down_v_stream(ConvDownParams P) {
	constexpr int R = KW / 2;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x = blockIdx.x * 256 + 4 * lane;
	const int outH = P.height / 2;
	const int o0 = (blockIdx.y * 4 + wave) * CD_ROWS_V;
	if (x >= P.width || o0 >= outH) return;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	float* outImg = P.out + (long long)blockIdx.z * P.outImageStride + x;
	const int oEnd = min(o0 + CD_ROWS_V, outH);
	const bool full4 = x + 3 < P.width;
	auto loadRow = [&](int yy) -> float4 {
		if (yy < 0 || yy >= P.height) return make_float4(0, 0, 0, 0);   // only ever feeds outputs that are not interior
		return loadRow4(img + (long long)yy * P.inStride, x, P.width);
	};
	// win[i] = input row 2 o - R + i of the current output o
	float4 win[KW];
#pragma unroll
	for (int i = 0; i < KW; i++) win[i] = loadRow(2 * o0 - R + i);
	for (int o = o0; o < oEnd; o++) {
		float4 n0 = make_float4(0, 0, 0, 0), n1 = n0;
		if (o + 1 < oEnd) { n0 = loadRow(2 * o + R + 1); n1 = loadRow(2 * o + R + 2); }   // the two rows the next output adds
		if (downInterior(P, o)) {
			float r[4] = {win[0].x * P.k[0], win[0].y * P.k[0], win[0].z * P.k[0], win[0].w * P.k[0]};
#pragma unroll
			for (int i = 1; i < KW; i++) { r[0] += win[i].x * P.k[i]; r[1] += win[i].y * P.k[i]; r[2] += win[i].z * P.k[i]; r[3] += win[i].w * P.k[i]; }
			float* dst = outImg + (long long)o * P.outStride;
			if (full4) *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
			else
				for (int q = 0; q < 4 && x + q < P.width; q++) dst[q] = r[q];
		}
#pragma unroll
		for (int i = 0; i + 2 < KW; i++) win[i] = win[i + 2];
		win[KW - 2] = n0;
		win[KW - 1] = n1;
	}
}

static int downMaxSide(int sideLength, int skip, int radius) {
	int ret = sideLength - (sideLength % skip);
	if (ret + radius >= sideLength) {
		ret = sideLength - radius - 1;
		ret = ret - (ret % skip);
	} else {
		ret -= skip;
	}
	return ret;
}
static int downOffset(int skip, int radius) { return radius <= skip ? skip : radius + radius % skip; }

// What the two down-sampling launchers share: ConvolveImageDownNoBorder.checkParameters*, the view and the taps unpacked into the kernel's
// params struct (ConvDownParams / ConvDownU8Params), the position classes along the filtered axis, and the test that every loop of the
// reference stays inside the image.
template <class Params, class K, class T>
static int convDownSetup(bhip_ctx* ctx, bool vertical, const K* kernel, int kw, DevImg<const T> in, DevImg<T> out, int skip, Params& P) {
	const int width = in.width, height = in.height;
	if (kw <= 0 || kw > BHIP_MAX_TAPS) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "kernel width not supported");
	// ConvolveImageDownNoBorder.checkParameters* (I:alg/filter/convolve/ConvolveImageDownNoBorder.java:160-186)
	if (skip <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "Skip must be >= 1");
	if (out.width < width / skip) return bhip_fail(ctx, BHIP_ERR_INVALID, "Output width is too small");
	if (out.height < height / skip) return bhip_fail(ctx, BHIP_ERR_INVALID, "Output height is too small");
	// checkParametersH/V on the no-border path; on the naive path GrayF32.set would throw ImageAccessException for the same shapes
	if (vertical && out.width < width) return bhip_fail(ctx, BHIP_ERR_INVALID, "Output width is too small");
	if (!vertical && out.height < height) return bhip_fail(ctx, BHIP_ERR_INVALID, "Output height is too small");
	P.in = in.data; P.out = out.data; P.inImageStride = in.imageStride; P.outImageStride = out.imageStride; P.inStride = in.stride; P.outStride = out.stride;
	P.width = width; P.height = height; P.skip = skip; P.kw = kw; P.radius = kw / 2;
	for (int i = 0; i < kw; i++) P.k[i] = kernel[i];
	if constexpr (std::is_integral_v<K>) {   // the integer form divides by the kernel's sum
		long long sum = 0;
		for (int i = 0; i < kw; i++) sum += kernel[i];
		if (sum == 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "/ by zero (the kernel sums to 0)");
	}
	const int r = P.radius;
	const int side = vertical ? height : width;
	P.naive = kw >= width ? 1 : 0;   // sic: the vertical form tests the image WIDTH as well
	P.offset = downOffset(skip, r);
	P.offsetRem = P.offset % skip;
	P.maxSide = downMaxSide(side, skip, r);
	P.offsetEnd = P.maxSide + skip;
	P.sideTrunc = side - side % skip;
	if (!P.naive) {
		if (kw % 2 != 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "Non symmetric odd kernels not supported");
		// every loop of the reference must stay inside the image along the filtered axis (Java would throw
		// ArrayIndexOutOfBounds or silently read the neighbouring row)
		bool ok = true;
		if (P.offset <= P.maxSide) ok = ok && P.offset - r >= 0;
		int lastLeft = ((P.offset - 1) / skip) * skip;                        // largest multiple of skip below offset
		ok = ok && lastLeft + r < side;
		if (P.offsetEnd < P.sideTrunc) ok = ok && P.offsetEnd - r >= 0;
		if (!ok) return bhip_fail(ctx, BHIP_ERR_INVALID, "kernel does not fit the image along the filtered axis");
	}
	return BHIP_OK;
}

int bhip_launch_conv_down(bhip_ctx* ctx, bool vertical, const float* kernel, int kw, DevImg<const float> in, DevImg<float> out, int skip) {
	const int width = in.width, height = in.height, batch = in.batch;
	ConvDownParams P;
	BHIP_TRY(convDownSetup(ctx, vertical, kernel, kw, in, out, skip, P));
	P.unrolled = (kw % 2 == 1 && (kw == 3 || kw == 5 || kw == 7 || kw == 9 || kw == 11)) ? 1 : 0;
	const int gw = vertical ? width : width / skip;
	const int gh = vertical ? height / skip : height;
	if (gw <= 0 || gh <= 0 || batch <= 0) return BHIP_OK;
	ProfScope prof(ctx, vertical ? "k_conv_down_v" : "k_conv_down_h", 4.0 * batch * ((double)width * height + (double)gw * gh));
	dim3 grid((gw + 255) / 256, gh, batch);
	P.skipInterior = 0;
	// skip 2, unrolled widths 3 / 5, 16-byte aligned rows: the interior goes through the streaming kernels, the general kernel adds the borders
	const bool stream = !P.naive && skip == 2 && P.unrolled && (kw == 3 || kw == 5) && P.offsetRem == 0 && vec4(in) && vec4(out);
	if (stream) {
		if (vertical) {
			dim3 g((width + 255) / 256, (gh + 4 * CD_ROWS_V - 1) / (4 * CD_ROWS_V), batch);
			if (kw == 3) hipLaunchKernelGGL(k_conv_down_v_stream<3>, g, dim3(256), 0, ctx->stream, P);
			else hipLaunchKernelGGL(k_conv_down_v_stream<5>, g, dim3(256), 0, ctx->stream, P);
		} else {
			dim3 g((width + 255) / 256, (height + 4 * CD_ROWS - 1) / (4 * CD_ROWS), batch);
			if (kw == 3) hipLaunchKernelGGL(k_conv_down_h_stream<3>, g, dim3(256), 0, ctx->stream, P);
			else hipLaunchKernelGGL(k_conv_down_h_stream<5>, g, dim3(256), 0, ctx->stream, P);
		}
		P.skipInterior = 1;
	}
	if (stream) {
		// the few border outputs of the filtered axis (see k_conv_down, skipInterior)
		const int outSide = (vertical ? height : width) / skip;
		const int nl = std::min((P.offset + skip - 1) / skip, outSide), dR0 = std::max(nl, std::min((P.offsetEnd + skip - 1) / skip, outSide));
		const int nb = nl + (outSide - dR0);
		if (nb > 0) {
			if (vertical) hipLaunchKernelGGL(k_conv_down<true>, dim3((gw + 255) / 256, nb, batch), dim3(256), 0, ctx->stream, P);
			else hipLaunchKernelGGL(k_conv_down<false>, dim3((unsigned)(((long long)height * nb + 255) / 256), 1, batch), dim3(256), 0, ctx->stream, P);
		}
	} else if (vertical) hipLaunchKernelGGL(k_conv_down<true>, grid, dim3(256), 0, ctx->stream, P);
	else hipLaunchKernelGGL(k_conv_down<false>, grid, dim3(256), 0, ctx->stream, P);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---- one pyramid layer in ONE pass: PyramidDiscreteSampleBlur.process's horizontal.process(prev, temp); vertical.process(temp, layer)
// (I:alg/transform/pyramid/PyramidDiscreteSampleBlur.java:88-118) for the usual step -- skip 2, widths 3 / 5.  Same scheme as
// k_blur_fused: a wave owns 256 input columns (128 outputs) x PL_ROWS output rows, walks the input rows once, forms the horizontally
// down-convolved row in registers (the value the reference leaves in `temp`: lane = input columns 4l..4l+3 = outputs 2l, 2l+1) and
// feeds a register ring from which every second input row yields one output row.  `temp` never exists: 4 P_in read + P_in written
// (+ 2R re-read rows per strip) instead of 4(P + P/2) + 4(P/2 + P/4).  Position classes per axis as in k_conv_down (skip 2: left border
// = output 0, right border = outputs centred in [offsetEnd, sideTrunc), interior between; every output of the layer is written).
#define PL_ROWS 16
struct PyrLayerParams {
	const float* in; float* out;
	long long inImageStride, outImageStride;
	int inStride, outStride, width, height;   // input size; outputs: width/2 x height/2
	int offsetX, maxSideX, offsetEndX, sideTruncX;
	int offsetY, maxSideY, offsetEndY, sideTruncY;
	float k[16];
};
// 0 = interior, 1 = border (normalised over the taps inside the image), -1 = not an output of this layer
__device__ __forceinline__ int pyrClass(int D, int outSide, int offset, int maxSide, int offsetEnd, int sideTrunc) {
	if (D >= outSide) return -1;
	const int centre = 2 * D;
	if (centre >= offsetEnd && centre < sideTrunc) return 1;
	if (centre < offset) return 1;
	return centre <= maxSide ? 0 : -1;
}
template <int KW>
__global__ __launch_bounds__(256) void k_pyr_layer_fused(PyrLayerParams P) {
	constexpr int R = KW / 2;   // <= 2: the kernel reaches at most two columns into the neighbouring chunks
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x = blockIdx.x * 256 + 4 * lane;          // first input column of this lane
	const int W = P.width, H = P.height, outW = W / 2, outH = H / 2;
	const int o0 = (blockIdx.y * 4 + wave) * PL_ROWS;
	if (x >= W || o0 >= outH) return;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	float* outImg = P.out + (long long)blockIdx.z * P.outImageStride;
	const int oEnd = min(o0 + PL_ROWS, outH);
	const int D0 = x >> 1;
	const int c0 = pyrClass(D0, outW, P.offsetX, P.maxSideX, P.offsetEndX, P.sideTruncX), c1 = pyrClass(D0 + 1, outW, P.offsetX, P.maxSideX, P.offsetEndX, P.sideTruncX);
	const int yFirst = 2 * o0 - R, yLast = min(2 * (oEnd - 1) + R, H - 1);   // input rows of the strip (clipped below when read)
	auto fetch = [&](float4 (&buf)[3], int yy) {
		if (yy >= 0 && yy <= yLast) {
			const float* row = img + (long long)yy * P.inStride;
#pragma unroll
			for (int c = 0; c < 3; c++) buf[c] = loadRow4(row, x - 4 + 4 * c, W);
		}
	};
	// the two outputs of this lane in one input row: what ConvolveImageDownNormalized.horizontal leaves in `temp`
	auto hdown = [&](const float4 (&buf)[3]) -> float2 {
		const float v[12] = {buf[0].x, buf[0].y, buf[0].z, buf[0].w, buf[1].x, buf[1].y, buf[1].z, buf[1].w, buf[2].x, buf[2].y, buf[2].z, buf[2].w};
		float r[2];
#pragma unroll
		for (int j = 0; j < 2; j++) {
			float t[KW];
#pragma unroll
			for (int i = 0; i < KW; i++) t[i] = v[4 + 2 * j - R + i];   // centre = input column x + 2 j = v[4 + 2 j]
			const int cls = j == 0 ? c0 : c1;
			r[j] = cls == 0 ? blurTapsInterior<KW>(t, P.k) : blurTapsBorder<KW>(t, P.k, x + 2 * j - R, W);
		}
		return make_float2(r[0], r[1]);
	};
	float2 ring[KW];   // ring[i] = `temp` row (yy - 2R + i) once input row yy has been pushed
#pragma unroll
	for (int i = 0; i < KW; i++) ring[i] = make_float2(0, 0);
	float4 cur[3], nxt[3];
#pragma unroll
	for (int c = 0; c < 3; c++) { cur[c] = make_float4(0, 0, 0, 0); nxt[c] = make_float4(0, 0, 0, 0); }
	fetch(cur, yFirst);
	fetch(nxt, yFirst + 1);
#pragma unroll 1
	for (int yy = yFirst; yy <= 2 * (oEnd - 1) + R; yy++) {
		float2 hrow = make_float2(0, 0);
		if (yy >= 0 && yy < H) hrow = hdown(cur);
#pragma unroll
		for (int c = 0; c < 3; c++) cur[c] = nxt[c];
		fetch(nxt, yy + 2);
#pragma unroll
		for (int i = 0; i + 1 < KW; i++) ring[i] = ring[i + 1];
		ring[KW - 1] = hrow;
		const int cy = yy - R;                   // centre row of the window now in the ring
		if (cy >= 2 * o0 && (cy & 1) == 0) {
			const int o = cy >> 1;
			const int cls = pyrClass(o, outH, P.offsetY, P.maxSideY, P.offsetEndY, P.sideTruncY);   // wave-uniform
			if (cls >= 0) {
				float r[2];
#pragma unroll
				for (int q = 0; q < 2; q++) {
					float tv[KW];
#pragma unroll
					for (int i = 0; i < KW; i++) tv[i] = q == 0 ? ring[i].x : ring[i].y;
					r[q] = cls == 0 ? blurTapsInterior<KW>(tv, P.k) : blurTapsBorder<KW>(tv, P.k, cy - R, H);
				}
				float* dst = outImg + (long long)o * P.outStride + D0;
				if (c0 >= 0 && c1 >= 0) *reinterpret_cast<float2*>(dst) = make_float2(r[0], r[1]);
				else { if (c0 >= 0) dst[0] = r[0]; if (c1 >= 0) dst[1] = r[1]; }
			}
		}
	}
}

// ---------------- batched image copy (pyramid layer 0 at scale 1: ImagePyramidBase keeps a copy of the input) ----------------
__global__ __launch_bounds__(256) void k_copy_images(const float* __restrict__ in, long long inImageStride, int inStride, float* __restrict__ out,
													   long long outImageStride, int outStride, int width, int height, int vec) {
	const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
	if (x >= width) return;
	const float* src = in + (long long)blockIdx.z * inImageStride + x;
	float* dst = out + (long long)blockIdx.z * outImageStride + x;
	for (int y = blockIdx.y; y < height; y += gridDim.y) {
		const float* s = src + (long long)y * inStride;
		float* d = dst + (long long)y * outStride;
		if (vec && x + 3 < width) *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(s);
		else
			for (int q = 0; q < 4 && x + q < width; q++) d[q] = s[q];
	}
}
// *done = false: the shape / kernel is outside what the fused layer kernel covers (the caller runs the two passes through `temp`)
int bhip_launch_pyr_layer_fused(bhip_ctx* ctx, const float* kernel, int kw, DevImg<const float> in, DevImg<float> out, int skip, bool* done) {
	const int width = in.width, height = in.height, batch = in.batch;
	*done = false;
	if (skip != 2 || !(kw == 3 || kw == 5) || batch <= 0) return BHIP_OK;
	const int r = kw / 2;
	if (kw >= width / 2 || kw >= height) return BHIP_OK;        // naive forms (the reference's vertical pass tests the width of `temp`, width / 2)
	if (width / 2 <= 0 || height / 2 <= 0) return BHIP_OK;
	if (!(vec4(in) && (reinterpret_cast<uintptr_t>(out.data) & 7) == 0 && out.stride % 2 == 0 && out.imageStride % 2 == 0)) return BHIP_OK;
	if (bhip_env_flag("BHIP_PYRAMID_TWO_PASS")) return BHIP_OK;  // parity cross-check of the two forms
	PyrLayerParams P;
	P.in = in.data; P.out = out.data; P.inImageStride = in.imageStride; P.outImageStride = out.imageStride; P.inStride = in.stride; P.outStride = out.stride;
	P.width = width; P.height = height;
	for (int i = 0; i < kw; i++) P.k[i] = kernel[i];
	for (int axis = 0; axis < 2; axis++) {
		const int side = axis == 0 ? width : height;
		const int offset = downOffset(2, r), maxSide = downMaxSide(side, 2, r), offsetEnd = maxSide + 2, sideTrunc = side - side % 2;
		if (offset % 2 != 0) return BHIP_OK;
		// the same fit checks bhip_launch_conv_down makes (a shape it rejects must be rejected there, with its message)
		bool ok = true;
		if (offset <= maxSide) ok = ok && offset - r >= 0;
		const int lastLeft = ((offset - 1) / 2) * 2;
		ok = ok && lastLeft + r < side;
		if (offsetEnd < sideTrunc) ok = ok && offsetEnd - r >= 0;
		if (!ok) return BHIP_OK;
		if (axis == 0) { P.offsetX = offset; P.maxSideX = maxSide; P.offsetEndX = offsetEnd; P.sideTruncX = sideTrunc; }
		else { P.offsetY = offset; P.maxSideY = maxSide; P.offsetEndY = offsetEnd; P.sideTruncY = sideTrunc; }
	}
	// algorithmic bytes: the two passes of SURVEY 8d, 4 (P_in + P_out) each
	const double Pin = (double)width * height, Ptmp = (double)(width / 2) * height, Pout = (double)(width / 2) * (height / 2);
	ProfScope prof(ctx, "k_pyr_layer_fused", 4.0 * batch * ((Pin + Ptmp) + (Ptmp + Pout)));
	dim3 grid((width + 255) / 256, (height / 2 + 4 * PL_ROWS - 1) / (4 * PL_ROWS), batch);
	if (kw == 3) hipLaunchKernelGGL(k_pyr_layer_fused<3>, grid, dim3(256), 0, ctx->stream, P);
	else hipLaunchKernelGGL(k_pyr_layer_fused<5>, grid, dim3(256), 0, ctx->stream, P);
	BHIP_HIP(ctx, hipGetLastError());
	*done = true;
	return BHIP_OK;
}

int bhip_launch_copy_images(bhip_ctx* ctx, DevImg<const float> in, DevImg<float> out) {
	if (in.width <= 0 || in.height <= 0 || in.batch <= 0) return BHIP_OK;
	const int vec = vec4(in) && vec4(out);
	dim3 grid((in.width + 1023) / 1024, std::min(in.height, 256), in.batch);
	hipLaunchKernelGGL(k_copy_images, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width,
					   in.height, vec);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// ---------------- GrayU8 down-sampling convolution (integer pyramid layer step) ----------------
// ConvolveImageDownNormalized.horizontal/vertical(Kernel1D_S32, GrayU8, GrayI8, skip)   I:alg/filter/convolve/ConvolveImageDownNormalized.java:109-137
//   interior  I:alg/filter/convolve/down/ConvolveDownNoBorderStandard.java:329-394 == ConvolveDownNoBorderUnrolled_U8_I8_Div:
//             (byte)((total + divisor/2) / divisor), divisor = kernel.computeSum()
//   border    I:alg/filter/convolve/down/ConvolveDownNormalized_JustBorder.java:262-358: (byte)((total + weight/2) / weight) over the taps inside
//   naive     I:alg/filter/convolve/down/ConvolveDownNormalizedNaive.java:133-187 (kernel.width >= image.width, in the vertical call too)
// The position classes along the filtered axis are those of k_conv_down (same UtilDownConvolve ranges).  All three forms are one integer
// expression: the interior's divisor is the weight of the full tap range.  Plain int division (Java's, truncating) for any S32 kernel.
struct ConvDownU8Params {
	const uint8_t* in;
	uint8_t* out;
	long long inImageStride, outImageStride;
	int inStride, outStride, width, height;   // input size
	int skip, kw, radius, naive;
	int offset, offsetRem, maxSide, offsetEnd, sideTrunc;   // along the filtered axis
	int k[BHIP_MAX_TAPS];
};
// taps [k0, k1] around `centre` of output D along an axis of `side` pixels; false: the reference does not write this output
__device__ __forceinline__ bool downU8Range(const ConvDownU8Params& P, int D, int side, int& centre, int& k0, int& k1) {
	const int r = P.radius;
	centre = D * P.skip;
	if (P.naive) {
		k0 = max(-r, -centre);
		k1 = min(r, side - 1 - centre);
	} else if (centre >= P.offsetEnd && centre < P.sideTrunc) {
		k0 = -r;
		k1 = min(r, side - centre - 1);
	} else if (centre < P.offset) {
		k0 = -centre;
		k1 = r;
	} else {
		centre += P.offsetRem;
		if (centre > P.maxSide) return false;
		k0 = -r; k1 = r;
	}
	return true;
}
__device__ __forceinline__ unsigned downU8Round(int total, int weight) { return weight != 0 ? (unsigned)((total + weight / 2) / weight) & 255u : 0u; }
__device__ __forceinline__ void downU8Store(uint8_t* dst, const unsigned (&v)[4], const bool (&wr)[4]) {
	if (wr[0] && wr[1] && wr[2] && wr[3] && (reinterpret_cast<uintptr_t>(dst) & 3) == 0)
		*reinterpret_cast<unsigned*>(dst) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
	else {
#pragma unroll
		for (int j = 0; j < 4; j++)
			if (wr[j]) dst[j] = (uint8_t)v[j];
	}
}
// a thread owns four neighbouring outputs of one row, stored as one dword where the row end and the alignment allow
__global__ __launch_bounds__(256) void k_conv_down_h_u8(ConvDownU8Params P) {
	const int outW = P.width / P.skip;
	const int ox = (blockIdx.x * 256 + threadIdx.x) * 4;
	if (ox >= outW) return;
	const uint8_t* row = P.in + (long long)blockIdx.z * P.inImageStride + (long long)blockIdx.y * P.inStride;
	unsigned v[4];
	bool wr[4];
	// the usual layer step (skip 2, radius <= 2) away from the row ends: the four outputs are centred on input columns 2 ox + {0, 2, 4, 6}
	// and read columns 2 ox - 2 .. 2 ox + 8, which are four dwords from 2 ox - 4 when the row is dword aligned
	const int c0 = 2 * ox;
	if (P.skip == 2 && P.radius <= 2 && !P.naive && ox + 3 < outW && c0 - 4 >= 0 && c0 + 12 <= P.width && c0 >= P.offset && c0 + 6 <= P.maxSide &&
		(reinterpret_cast<uintptr_t>(row + c0) & 3) == 0) {
		const uint4 q = make_uint4(*reinterpret_cast<const unsigned*>(row + c0 - 4), *reinterpret_cast<const unsigned*>(row + c0),
								   *reinterpret_cast<const unsigned*>(row + c0 + 4), *reinterpret_cast<const unsigned*>(row + c0 + 8));
		const unsigned w[4] = {q.x, q.y, q.z, q.w};
		int b[16];   // b[i] = input column c0 - 4 + i
#pragma unroll
		for (int i = 0; i < 16; i++) b[i] = (w[i >> 2] >> (8 * (i & 3))) & 255;
		int kk[5], weight = 0;   // the kernel centred in five taps (zeros around a narrower one): every register index below is a constant
#pragma unroll
		for (int i = 0; i < 5; i++) {
			const int t = i - 2 + P.radius;
			kk[i] = t >= 0 && t < P.kw ? P.k[t] : 0;
			weight += kk[i];
		}
#pragma unroll
		for (int j = 0; j < 4; j++) {
			int total = 0;
#pragma unroll
			for (int i = 0; i < 5; i++) total += b[2 + 2 * j + i] * kk[i];
			v[j] = downU8Round(total, weight);
			wr[j] = true;
		}
		downU8Store(P.out + (long long)blockIdx.z * P.outImageStride + (long long)blockIdx.y * P.outStride + ox, v, wr);
		return;
	}
#pragma unroll
	for (int j = 0; j < 4; j++) {
		int centre, k0, k1;
		v[j] = 0;
		wr[j] = ox + j < outW && downU8Range(P, ox + j, P.width, centre, k0, k1);
		if (!wr[j]) continue;
		int total = 0, weight = 0;
		for (int k = k0; k <= k1; k++) {
			const int w = P.k[k + P.radius];
			weight += w;
			total += row[centre + k] * w;
		}
		v[j] = downU8Round(total, weight);
	}
	downU8Store(P.out + (long long)blockIdx.z * P.outImageStride + (long long)blockIdx.y * P.outStride + ox, v, wr);
}
// a thread owns four neighbouring columns of one output row: every tap row is one dword load where aligned
__global__ __launch_bounds__(256) void k_conv_down_v_u8(ConvDownU8Params P) {
	const int x = (blockIdx.x * 256 + threadIdx.x) * 4, oy = blockIdx.y;
	if (x >= P.width) return;
	int centre, k0, k1;
	if (!downU8Range(P, oy, P.height, centre, k0, k1)) return;   // uniform over the grid row
	const uint8_t* src = P.in + (long long)blockIdx.z * P.inImageStride + (long long)centre * P.inStride + x;
	const bool full4 = x + 3 < P.width;
	int total[4] = {0, 0, 0, 0}, weight = 0;
	for (int k = k0; k <= k1; k++) {
		const int w = P.k[k + P.radius];
		const uint8_t* s = src + (long long)k * P.inStride;
		weight += w;
		if (full4 && (reinterpret_cast<uintptr_t>(s) & 3) == 0) {
			const unsigned q = *reinterpret_cast<const unsigned*>(s);
			total[0] += (int)(q & 255) * w; total[1] += (int)((q >> 8) & 255) * w; total[2] += (int)((q >> 16) & 255) * w; total[3] += (int)(q >> 24) * w;
		} else {
#pragma unroll
			for (int j = 0; j < 4; j++)
				if (x + j < P.width) total[j] += s[j] * w;
		}
	}
	unsigned v[4];
	bool wr[4];
#pragma unroll
	for (int j = 0; j < 4; j++) { v[j] = downU8Round(total[j], weight); wr[j] = x + j < P.width; }
	downU8Store(P.out + (long long)blockIdx.z * P.outImageStride + (long long)oy * P.outStride + x, v, wr);
}

// ---- batched GrayU8 image copy (layer 0 of the integer pyramid at scale 1).  A thread moves 16 bytes; the views a caller hands over start
// anywhere, so both sides are accessed without an alignment assumption (memcpy of a uint4: gfx950 global memory takes unaligned vector
// accesses).
__global__ __launch_bounds__(256) void k_copy_images_u8(const uint8_t* __restrict__ in, long long inImageStride, int inStride, uint8_t* __restrict__ out,
														  long long outImageStride, int outStride, int width, int height) {
	const int x = (blockIdx.x * 256 + threadIdx.x) * 16;
	if (x >= width) return;
	const uint8_t* src = in + (long long)blockIdx.z * inImageStride + x;
	uint8_t* dst = out + (long long)blockIdx.z * outImageStride + x;
	for (int y = blockIdx.y; y < height; y += gridDim.y) {
		const uint8_t* s = src + (long long)y * inStride;
		uint8_t* d = dst + (long long)y * outStride;
		if (x + 15 < width) {
			uint4 v;
			__builtin_memcpy(&v, s, 16);
			__builtin_memcpy(d, &v, 16);
		} else
			for (int q = 0; q < 16 && x + q < width; q++) d[q] = s[q];
	}
}
int bhip_launch_copy_images(bhip_ctx* ctx, DevImg<const uint8_t> in, DevImg<uint8_t> out) {
	if (in.width <= 0 || in.height <= 0 || in.batch <= 0) return BHIP_OK;
	dim3 grid((in.width + 4095) / 4096, std::min(in.height, 512), in.batch);
	hipLaunchKernelGGL(k_copy_images_u8, grid, dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride, out.stride, in.width,
					   in.height);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

int bhip_launch_conv_down(bhip_ctx* ctx, bool vertical, const int32_t* kernel, int kw, DevImg<const uint8_t> in, DevImg<uint8_t> out, int skip) {
	const int width = in.width, height = in.height, batch = in.batch;
	ConvDownU8Params P;
	BHIP_TRY(convDownSetup(ctx, vertical, kernel, kw, in, out, skip, P));
	const int gw = vertical ? width : width / skip;
	const int gh = vertical ? height / skip : height;
	if (gw <= 0 || gh <= 0 || batch <= 0) return BHIP_OK;
	ProfScope prof(ctx, vertical ? "k_conv_down_v_u8" : "k_conv_down_h_u8", 1.0 * batch * ((double)width * height + (double)gw * gh));
	const dim3 grid((gw + 1023) / 1024, gh, batch);
	if (vertical) hipLaunchKernelGGL(k_conv_down_v_u8, grid, dim3(256), 0, ctx->stream, P);
	else hipLaunchKernelGGL(k_conv_down_h_u8, grid, dim3(256), 0, ctx->stream, P);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
