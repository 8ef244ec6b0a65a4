// K8: boofcv-ip convolutions behind the BOverride* hooks (separable convolution, Gaussian blur, 2-D convolution, mean and median blur).
// All fp32 with the reference's evaluation order and no FMA contraction.
//
// Reference:
//   ConvolveImageNoBorder.horizontal/vertical     I:alg/filter/convolve/ConvolveImageNoBorder.java:53-77
//     unrolled widths 3,5,7,9,11 (first tap assigns)  I:alg/filter/convolve/noborder/ConvolveImageUnrolled_SB_F32_F32.java:50-150,152-180,347-382
//     standard (total = 0 first)                      I:alg/filter/convolve/noborder/ConvolveImageStandard_SB.java:44-104
//   ConvolveImageNormalized.horizontal/vertical   I:alg/filter/convolve/ConvolveImageNormalized.java:48-93
//     border re-normalisation                         I:alg/filter/convolve/normalized/ConvolveNormalized_JustBorder_SB.java:42-145
//     kernel wider than the image                     I:alg/filter/convolve/normalized/ConvolveNormalizedNaive_SB.java:37-84
// Bound: HBM (8P bytes per separable pass); taps are re-read through L1/L2.
#include "ip_dev.h"

// General form: one output pixel per thread, taps through L1 / L2.  Any base address, stride and width (sub-images with odd strides,
// kernels wider than the image); the tiled kernels below take over whenever rows are 16-byte aligned.
template <bool VERTICAL>
__global__ __launch_bounds__(256) void k_conv(ConvParams P) {
	int x = blockIdx.x * blockDim.x + threadIdx.x;
	int y = blockIdx.y;
	const int extent = VERTICAL ? P.height : P.width;
	const int offL = P.koff, offR = P.kw - P.koff - 1;
	if (P.borderOnly) {
		// border fix-up after a streaming kernel: index t of the filtered axis runs over the offL leading and offR trailing positions
		// (horizontal: the grid is flat, consecutive threads take the border columns of one row, then the next row)
		const int nb = offL + offR;
		if (!VERTICAL) {
			if (nb <= 0) return;
			y = x / nb;
			x -= y * nb;
			if (y >= P.height) return;
		}
		int& t = VERTICAL ? y : x;
		if (t >= nb) return;
		t = t < offL ? t : extent - offR + (t - offL);
	}
	if (x >= P.width) return;
	const int pos = VERTICAL ? y : x;
	const long long step = VERTICAL ? P.inStride : 1;
	const float* src = P.in + (long long)blockIdx.z * P.inImageStride + (long long)y * P.inStride + x;
	const bool interior = pos >= offL && pos < extent - offR;
	float result;
	if (interior && P.mode == 3) return;
	if (interior && P.mode != 2) {
		const float* s = src - offL * step;
		result = P.unrolled ? tapsUnrolled(s, step, P.k, P.kw) : tapsStandard(s, step, P.k, P.kw);
	} else {
		if (P.mode == 0) return;
		const int k0 = max(0, offL - pos);
		const int k1 = min(P.kw, extent - pos + offL);
		float total = 0, weight = 0;
		for (int k = k0; k < k1; k++) {
			const float w = P.k[k];
			weight += w;
			total += src[(long long)(k - offL) * step] * w;
		}
		result = total / weight;
	}
	P.out[(long long)blockIdx.z * P.outImageStride + (long long)y * P.outStride + x] = result;
}

// ---- tiled forms: rows staged once in LDS with 16-byte loads, every tap served from LDS ----
// Horizontal pass.  A block takes CT_ROWS rows x 256 columns; wave w stages and filters rows w, w+4, ...: the row segment plus the
// kernel's reach (rounded to 16-byte chunks) goes to LDS once, then lane l produces columns l, l+64, l+128, l+192 of the segment, so
// every LDS read and every global store of a wave touches 64 consecutive floats.
// (Measured alternative that lost: a wave walking a strip of 16 rows through two LDS row buffers of its own, the next row's loads under the
// tap loop, no block barrier, a quarter of the workgroups: 1.16 ms against 0.85 ms for 41 taps on 64 x 1080p.)
#define CT_W 256
#define CT_ROWS 8
template <int KW>
__global__ __launch_bounds__(256) void k_conv_h_tile(ConvParams P, int padL, int ldsRow) {
	extern __shared__ float lds[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int xt0 = blockIdx.x * CT_W;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	float* outImg = P.out + (long long)blockIdx.z * P.outImageStride;
	const int nChunks = ldsRow >> 2;
	const int y0 = blockIdx.y * CT_ROWS;
#pragma unroll
	for (int q = 0; q < CT_ROWS / 4; q++) {
		const int y = y0 + wave + 4 * q;
		if (y >= P.height) break;
		const float* src = img + (long long)y * P.inStride;
		float* row = lds + (wave + 4 * q) * ldsRow;
		for (int c = lane; c < nChunks; c += 64) *reinterpret_cast<float4*>(row + 4 * c) = loadRow4(src, xt0 - padL + 4 * c, P.width);
	}
	// the kernel's coefficients behind the rows: one broadcast LDS read per tap serves the lane's four outputs
	float* kl = lds + CT_ROWS * ldsRow;
	if ((int)threadIdx.x < P.kw) kl[threadIdx.x] = P.k[threadIdx.x];
	__syncthreads();
	const int kw = KW > 0 ? KW : P.kw;
	// Run-time widths: the reference's interior expression -- total = (0 +) s0*k0; total += s_i*k_i in tap order -- is formed for the four
	// outputs of a lane together (every tap of every output lies inside the staged row, whose cells outside the image hold 0 and are only
	// ever combined into values that are not stored); interior outputs are stored, the few border outputs of the frame tiles take convOne.
	const bool fast = KW == 0 && P.mode != 2 && P.mode != 3;
	const int offRh = kw - P.koff - 1;
#pragma unroll
	for (int q = 0; q < CT_ROWS / 4; q++) {
		const int y = y0 + wave + 4 * q;
		if (y >= P.height) break;
		const float* row = lds + (wave + 4 * q) * ldsRow + padL - P.koff;
		float* dst = outImg + (long long)y * P.outStride;
		if (fast) {
			// (the two taps of a pair are 64 words apart: one ds_read2st64_b32 fills a register pair for the packed multiply-add)
			typedef float f32x2 __attribute__((ext_vector_type(2)));
			const float* s0 = row + lane;
			const float k0 = kl[0];
			f32x2 a = f32x2{s0[0], s0[64]} * k0, b = f32x2{s0[128], s0[192]} * k0;
			if (!P.unrolled) { a = f32x2{0.0f, 0.0f} + a; b = f32x2{0.0f, 0.0f} + b; }
			// Four taps per step, the eight pair reads written out: left to itself the compiler pairs ADJACENT taps of one column (ds_read2_b32)
			// and then spends two moves per tap on re-pairing them for the packed arithmetic (910 vector instructions per wave instead of ~500).
			int i = 1;
			unsigned int ad = (unsigned int)(uintptr_t)(s0 + 1);   // LDS byte address of tap 1 of the lane's first output
			for (; i + 4 <= kw; i += 4, ad += 16u) {
				f32x2 p0, p1, p2, p3, q0, q1, q2, q3;
				const unsigned int a1 = ad + 4u, a2 = ad + 8u, a3 = ad + 12u;
				const float ka = kl[i], kb = kl[i + 1], kc = kl[i + 2], kd = kl[i + 3];   // issued first: the wait below covers them as well
				asm volatile("ds_read2st64_b32 %0, %8 offset0:0 offset1:1\n\t"
							 "ds_read2st64_b32 %4, %8 offset0:2 offset1:3\n\t"
							 "ds_read2st64_b32 %1, %9 offset0:0 offset1:1\n\t"
							 "ds_read2st64_b32 %5, %9 offset0:2 offset1:3\n\t"
							 "ds_read2st64_b32 %2, %10 offset0:0 offset1:1\n\t"
							 "ds_read2st64_b32 %6, %10 offset0:2 offset1:3\n\t"
							 "ds_read2st64_b32 %3, %11 offset0:0 offset1:1\n\t"
							 "ds_read2st64_b32 %7, %11 offset0:2 offset1:3\n\t"
							 "s_waitcnt lgkmcnt(0)"
							 : "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3), "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3)
							 : "v"(ad), "v"(a1), "v"(a2), "v"(a3)
							 : "memory");
				a += p0 * ka; b += q0 * ka;
				a += p1 * kb; b += q1 * kb;
				a += p2 * kc; b += q2 * kc;
				a += p3 * kd; b += q3 * kd;
			}
			for (; i < kw; i++) {
				const float k = kl[i];
				a += f32x2{s0[i], s0[64 + i]} * k;
				b += f32x2{s0[128 + i], s0[192 + i]} * k;
			}
			const float t[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int xl = lane + 64 * j, x = xt0 + xl;
				if (x >= P.width) continue;
				if (x >= P.koff && x < P.width - offRh) dst[x] = t[j];
				else {
					float r;
					if (convOne<KW>(P, row + xl, 1, x, P.width, r, kl)) dst[x] = r;
				}
			}
			continue;
		}
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int xl = lane + 64 * j, x = xt0 + xl;
			float r;
			if (x < P.width && convOne<KW>(P, row + xl, 1, x, P.width, r, kl)) dst[x] = r;
		}
	}
}

// Vertical pass.  A block takes CV_ROWS output rows x 256 columns: the CV_ROWS + kw - 1 input rows are staged in LDS (one row per wave
// instruction, 16 bytes per lane), then wave w filters rows w, w+4, ...; lane l owns columns 4l .. 4l+3, so taps are ds_read_b128
// and results leave as 16-byte stores.
#define CV_ROWS 32
// NW = waves per block.  The run-time widths (wide kernels) run 16 waves per block: a block's LDS is (CV_ROWS + kw - 1) KB -- 72 KB for 41 taps, two
// blocks per CU -- so four waves per block left two waves per SIMD to hide the LDS latency of a tap loop (41 taps: 0.81 -> 0.53 ms per 64 x 1080p).
template <int KW, int NW = 4>
__global__ __launch_bounds__(64 * NW) void k_conv_v_tile(ConvParams P) {
	extern __shared__ float lds[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x = blockIdx.x * CT_W + 4 * lane;
	const int y0 = blockIdx.y * CV_ROWS;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	float* outImg = P.out + (long long)blockIdx.z * P.outImageStride;
	const int kw = KW > 0 ? KW : P.kw;
	const int nStage = min(CV_ROWS, P.height - y0) + kw - 1;
	const int yTop = y0 - P.koff;
	if (x < P.width) {
		for (int i = wave; i < nStage; i += NW) {
			const int yy = yTop + i;
			if (yy >= 0 && yy < P.height) *reinterpret_cast<float4*>(lds + i * CT_W + 4 * lane) = loadRow4(img + (long long)yy * P.inStride, x, P.width);
		}
	}
	float* kl = lds + (CV_ROWS + kw - 1) * CT_W;   // the kernel's coefficients behind the rows (one broadcast read per tap)
	if ((int)threadIdx.x < kw) kl[threadIdx.x] = P.k[threadIdx.x];
	__syncthreads();
	if (x >= P.width) return;
	const int offR = kw - P.koff - 1;
	for (int q = wave; q < CV_ROWS; q += NW) {
		const int y = y0 + q;
		if (y >= P.height) break;
		const float* s = lds + q * CT_W + 4 * lane;
		if (KW == 0 && P.mode != 2 && P.mode != 3 && y >= P.koff && y < P.height - offR && x + 3 < P.width) {
			// interior row (wave-uniform): the lane's four columns together, taps as 16-byte LDS reads, packed fp32 -- per column the
			// reference's expression, total = (0 +) s0*k0; total += s_i*k_i in tap order
			typedef float f32x2 __attribute__((ext_vector_type(2)));
			const float4 v0 = *reinterpret_cast<const float4*>(s);
			const float k0 = kl[0];
			f32x2 lo = f32x2{v0.x, v0.y} * k0, hi = f32x2{v0.z, v0.w} * k0;
			if (!P.unrolled) { lo = f32x2{0.0f, 0.0f} + lo; hi = f32x2{0.0f, 0.0f} + hi; }
#pragma unroll 4
			for (int i = 1; i < kw; i++) {
				const float4 v = *reinterpret_cast<const float4*>(s + i * CT_W);
				const float k = kl[i];
				lo += f32x2{v.x, v.y} * k;
				hi += f32x2{v.z, v.w} * k;
			}
			*reinterpret_cast<float4*>(outImg + (long long)y * P.outStride + x) = make_float4(lo.x, lo.y, hi.x, hi.y);
			continue;
		}
		float r[4];
		bool wr = true;
#pragma unroll
		for (int j = 0; j < 4; j++) wr = convOne<KW>(P, s + j, CT_W, y, P.height, r[j], kl);   // same position class for the four columns
		if (!wr) continue;
		float* dst = outImg + (long long)y * P.outStride + x;
		if (x + 3 < P.width) *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
		else
			for (int j = 0; j < 4 && x + j < P.width; j++) dst[j] = r[j];
	}
}

// ---- streaming forms for the reference's unrolled widths (3..11, centred): no LDS, every input row loaded once per strip ----
// Horizontal: lane l owns columns 4l..4l+3 of a 256-column strip and walks CS_ROWS rows; a row's taps are NL aligned 16-byte loads
// (own chunk + the chunks the kernel reaches into; neighbouring lanes' chunks are L1 hits), results leave as one 16-byte store.
#define CS_ROWS 8
template <int KW>
__global__ __launch_bounds__(256) void k_conv_h_stream(ConvParams P) {
	constexpr int R = KW / 2, NC = (R + 3) / 4, NL = 1 + 2 * NC, PL = 4 * NC;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x = blockIdx.x * 256 + 4 * lane;
	const int y0 = (blockIdx.y * 4 + wave) * CS_ROWS;
	if (x >= P.width || y0 >= P.height) return;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	float* outImg = P.out + (long long)blockIdx.z * P.outImageStride;
	const int yEnd = min(y0 + CS_ROWS, P.height);
	// interior pixels only: the border columns (normalised forms) are written afterwards by the general kernel (borderOnly launch)
	const bool allInterior = x >= R && x + 3 < P.width - R;
	// NB row buffers take turns: while row y is filtered and stored, the chunks of the next NB - 1 rows are in flight (a wave has to keep
	// several KB on the way to cover the HBM latency at 8 waves per SIMD)
	constexpr int NB = KW <= 5 ? 4 : (KW <= 7 ? 3 : 2);
	if constexpr (NC == 1) {
		// kernels that reach at most one chunk to either side: every lane loads its own chunk only and receives the neighbours' chunks by
		// lane shifts; the strip's first / last lane fetch the chunk beyond the strip themselves (one extra 16-byte request per row and side)
		float4 own[NB], edge[NB];
		const bool first = lane == 0, last = lane == 63;
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
			lf.x = __shfl_up(own.x, 1, 64); lf.y = __shfl_up(own.y, 1, 64); lf.z = __shfl_up(own.z, 1, 64); lf.w = __shfl_up(own.w, 1, 64);
			rt.x = __shfl_down(own.x, 1, 64); rt.y = __shfl_down(own.y, 1, 64); rt.z = __shfl_down(own.z, 1, 64); rt.w = __shfl_down(own.w, 1, 64);
			if (first) lf = edge;
			if (last) rt = edge;
			const float v[12] = {lf.x, lf.y, lf.z, lf.w, own.x, own.y, own.z, own.w, rt.x, rt.y, rt.z, rt.w};
			float r[4];
#pragma unroll
			for (int j = 0; j < 4; j++) {
				float total = v[PL - R + j] * P.k[0];
#pragma unroll
				for (int i = 1; i < KW; i++) total += v[PL - R + j + i] * P.k[i];
				r[j] = total;
			}
			float* dst = outImg + (long long)y * P.outStride + x;
			if (allInterior) *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
			else {
#pragma unroll
				for (int j = 0; j < 4; j++)
					if (x + j >= R && x + j < P.width - R) dst[j] = r[j];
			}
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
		return;
	}
	float4 buf[NB][NL];
	auto fetch = [&](float4 (&buf)[NL], int y) {
		if (y < yEnd) {
			const float* row = img + (long long)y * P.inStride;
#pragma unroll
			for (int c = 0; c < NL; c++) buf[c] = loadRow4(row, x - PL + 4 * c, P.width);
		}
	};
	auto emit = [&](const float4 (&buf)[NL], int y) {
		if (y >= yEnd) return;
		float v[4 * NL];
#pragma unroll
		for (int c = 0; c < NL; c++) { v[4 * c] = buf[c].x; v[4 * c + 1] = buf[c].y; v[4 * c + 2] = buf[c].z; v[4 * c + 3] = buf[c].w; }
		float r[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			float total = v[PL - R + j] * P.k[0];
#pragma unroll
			for (int i = 1; i < KW; i++) total += v[PL - R + j + i] * P.k[i];
			r[j] = total;
		}
		float* dst = outImg + (long long)y * P.outStride + x;
		if (allInterior) *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
		else {
#pragma unroll
			for (int j = 0; j < 4; j++)
				if (x + j >= R && x + j < P.width - R) dst[j] = r[j];
		}
	};
#pragma unroll
	for (int q = 0; q < NB; q++) fetch(buf[q], y0 + q);
	for (int y = y0; y < yEnd; y += NB) {
#pragma unroll
		for (int q = 0; q < NB; q++) {
			emit(buf[q], y + q);
			fetch(buf[q], y + q + NB);
		}
	}
}

// Vertical: lane l owns columns 4l..4l+3 and walks a strip of CS_ROWS_V output rows with the KW input rows of the current output in a
// register ring of KW+PF slots (the extra slots receive the rows of the next PF outputs while the current one is computed).  Strips that touch the top or
// bottom border evaluate the border rules per row from the same ring.
#define CS_ROWS_V 16
template <int KW>
__global__ __launch_bounds__(256) void k_conv_v_stream(ConvParams P) {
	constexpr int PF = KW <= 5 ? 3 : 2;        // rows requested ahead of the output being computed
	constexpr int R = KW / 2, RING = KW + PF;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x = blockIdx.x * 256 + 4 * lane;
	const int y0 = (blockIdx.y * 4 + wave) * CS_ROWS_V;
	if (x >= P.width || y0 >= P.height) return;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride + x;
	float* outImg = P.out + (long long)blockIdx.z * P.outImageStride + x;
	const int yEnd = min(y0 + CS_ROWS_V, P.height);
	const bool full4 = x + 3 < P.width;
	auto loadRow = [&](int yy) -> float4 {
		if (yy < 0 || yy >= P.height) return make_float4(0, 0, 0, 0);
		return loadRow4(img + (long long)yy * P.inStride - x, x, P.width);
	};
	float4 ring[RING];
	// ring[(t + i) % RING] = input row y0 - R + t + i, the tap i of output row y0 + t
#pragma unroll
	for (int i = 0; i < KW + PF - 1; i++) ring[i] = loadRow(y0 - R + i);
	for (int tb = 0; y0 + tb < yEnd; tb += RING) {
#pragma unroll
		for (int j = 0; j < RING; j++) {
			const int y = y0 + tb + j;
			if (y < yEnd) {
				if (y + PF < yEnd) ring[(j + KW + PF - 1) % RING] = loadRow(y + PF + R);   // a spare slot receives the last tap of the output PF rows on
				float r[4];
				const float4 t0 = ring[j % RING];
				r[0] = t0.x * P.k[0]; r[1] = t0.y * P.k[0]; r[2] = t0.z * P.k[0]; r[3] = t0.w * P.k[0];
#pragma unroll
				for (int i = 1; i < KW; i++) {
					const float4 t = ring[(j + i) % RING];
					r[0] += t.x * P.k[i]; r[1] += t.y * P.k[i]; r[2] += t.z * P.k[i]; r[3] += t.w * P.k[i];
				}
				if (y >= R && y < P.height - R) {   // interior rows only: the border rows are written by the general kernel (borderOnly launch)
					float* dst = outImg + (long long)y * P.outStride;
					if (full4) *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
					else
						for (int q = 0; q < 4 && x + q < P.width; q++) dst[q] = r[q];
				}
			}
		}
	}
}

// ---- Gaussian blur in ONE pass over the image (BlurImageOps.gaussian = ConvolveImageNormalized.horizontal into `storage`, then
// ConvolveImageNormalized.vertical into the output: I:alg/filter/blur/BlurImageOps.java:406-425) for the reference's unrolled widths.
// A wave owns a strip of 256 columns x BF_ROWS output rows and walks down the input rows once: a row is loaded (16 bytes per lane),
// filtered horizontally in registers -- the value the reference would have stored in `storage`, border columns included -- and pushed
// into a register ring of the last KW filtered rows, from which the vertical filter produces one output row per input row.  The
// intermediate image never exists: 4P read + 4P written (+ 2R re-read rows per strip) instead of 16P for the two passes.  Every value is
// formed by the reference's expression for its position class, in its tap order:
//   interior  total = s0*k0; total += s_i*k_i                                   (ConvolveImageUnrolled_SB_F32_F32.java:152-180,384-425)
//   border    weight += k; total += s*k over the taps inside the image; total / weight   (ConvolveNormalized_JustBorder_SB.java:60-88,108-140)
#define BF_ROWS 32   // output rows per wave strip
// Measured alternatives that lost (A/B in one run, 64 x 1080p, r = 2 / r = 5: this form 0.27 / 0.64 ms): chunk-bounds tests hoisted out of
// the row loop with plain 16-byte loads 0.31 / 0.87 ms; one row of look-ahead instead of two for widths 9, 11 (107 instead of 126
// registers) 0.76 ms; 64-row strips for widths 9, 11 0.65 ms at 1080p but 0.31 instead of 0.25 ms on 8 x 4K.
// (the tap expressions of a filtered value, blurTapsInterior / blurTapsBorder, are in ip_dev.h: k_pyr_layer_fused forms its values with them too)
template <int KW, int WPB = 4>
__global__ __launch_bounds__(64 * WPB) void k_blur_fused(ConvParams P) {
	constexpr int R = KW / 2, NC = (R + 3) / 4, NL = 1 + 2 * NC, PL = 4 * NC;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x = blockIdx.x * 256 + 4 * lane;
	constexpr int ROWS = BF_ROWS;
	const int y0 = (blockIdx.y * WPB + wave) * ROWS;
	if (x >= P.width || y0 >= P.height) return;
	const int W = P.width, H = P.height;
	const float* img = P.in + (long long)blockIdx.z * P.inImageStride;
	float* outImg = P.out + (long long)blockIdx.z * P.outImageStride + x;
	const int yEnd = min(y0 + ROWS, H);
	const bool colsInterior = x >= R && x + 3 < W - R;     // all four columns are interior columns of the horizontal pass
	const bool full4 = x + 3 < W;
	const int yLast = min(yEnd + R, H);                    // input rows of the strip: [max(y0 - R, 0), yLast)
	// the lane's chunk of a row and the chunks the kernel reaches into (neighbouring lanes' chunks: L1 hits)
	auto fetch = [&](float4 (&buf)[NL], int yy) {
		if (yy >= 0 && yy < yLast) {
			const float* row = img + (long long)yy * P.inStride;
#pragma unroll
			for (int c = 0; c < NL; c++) buf[c] = loadRow4(row, x - PL + 4 * c, W);
		}
	};
	// horizontal pass of one row for the lane's four columns: the value ConvolveImageNormalized.horizontal leaves in `storage`
	auto hfilter = [&](const float4 (&buf)[NL]) -> float4 {
		float v[4 * NL];
#pragma unroll
		for (int c = 0; c < NL; c++) { v[4 * c] = buf[c].x; v[4 * c + 1] = buf[c].y; v[4 * c + 2] = buf[c].z; v[4 * c + 3] = buf[c].w; }
		if (colsInterior) {
			// the four columns as two packed pairs: column j's tap i is v[PL - R + j + i], so the pairs are neighbouring array elements;
			// component-wise the reference's expression (total = s0*k0; total += s_i*k_i), half the additions of four scalar chains
			typedef float f32x2 __attribute__((ext_vector_type(2)));
			f32x2 lo = f32x2{v[PL - R], v[PL - R + 1]} * P.k[0], hi = f32x2{v[PL - R + 2], v[PL - R + 3]} * P.k[0];
#pragma unroll
			for (int i = 1; i < KW; i++) {
				lo += f32x2{v[PL - R + i], v[PL - R + 1 + i]} * P.k[i];
				hi += f32x2{v[PL - R + 2 + i], v[PL - R + 3 + i]} * P.k[i];
			}
			return make_float4(lo.x, lo.y, hi.x, hi.y);
		}
		float r[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			float t[KW];
#pragma unroll
			for (int i = 0; i < KW; i++) t[i] = v[PL - R + j + i];
			r[j] = (x + j >= R && x + j < W - R) ? blurTapsInterior<KW>(t, P.k) : blurTapsBorder<KW>(t, P.k, x + j - R, W);
		}
		return make_float4(r[0], r[1], r[2], r[3]);
	};
	// ring[i] = horizontally filtered row (yy - 2R + i) once input row yy has been pushed: the KW taps of output row yy - R, in tap order.
	// The ring is shifted by register moves (KW x 4 per row, against 16 KW multiply-adds), which keeps the row loop one small body.
	float4 ring[KW];
#pragma unroll
	for (int i = 0; i < KW; i++) ring[i] = make_float4(0, 0, 0, 0);
	float4 cur[NL], nxt[NL];   // two rows in flight ahead of the one being filtered
#pragma unroll
	for (int c = 0; c < NL; c++) { cur[c] = make_float4(0, 0, 0, 0); nxt[c] = make_float4(0, 0, 0, 0); }
	fetch(cur, y0 - R);
	fetch(nxt, y0 - R + 1);
#pragma unroll 1
	for (int yy = y0 - R; yy < yEnd + R; yy++) {
		float4 hrow = make_float4(0, 0, 0, 0);
		if (yy >= 0 && yy < H) hrow = hfilter(cur);   // rows outside the image are never used as taps (wave-uniform branch)
#pragma unroll
		for (int c = 0; c < NL; c++) cur[c] = nxt[c];
		fetch(nxt, yy + 2);
#pragma unroll
		for (int i = 0; i + 1 < KW; i++) ring[i] = ring[i + 1];
		ring[KW - 1] = hrow;
		const int y = yy - R;   // the output row whose last tap just arrived
		if (y >= y0) {
			const bool rowInterior = y >= R && y < H - R;   // wave-uniform
			float r[4];
			if (rowInterior) {
				// the four columns as two packed pairs (v_pk_mul_f32 / v_pk_add_f32): component-wise the reference's expression, half the instructions
				typedef float f32x2 __attribute__((ext_vector_type(2)));
				f32x2 lo = f32x2{ring[0].x, ring[0].y} * P.k[0], hi = f32x2{ring[0].z, ring[0].w} * P.k[0];
#pragma unroll
				for (int i = 1; i < KW; i++) {
					lo += f32x2{ring[i].x, ring[i].y} * P.k[i];
					hi += f32x2{ring[i].z, ring[i].w} * P.k[i];
				}
				r[0] = lo.x; r[1] = lo.y; r[2] = hi.x; r[3] = hi.y;
			} else {
#pragma unroll
				for (int q = 0; q < 4; q++) {
					float tv[KW];
#pragma unroll
					for (int i = 0; i < KW; i++) tv[i] = q == 0 ? ring[i].x : q == 1 ? ring[i].y : q == 2 ? ring[i].z : ring[i].w;
					r[q] = blurTapsBorder<KW>(tv, P.k, y - R, H);
				}
			}
			float* dst = outImg + (long long)y * P.outStride;
			if (full4) *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
			else
				for (int q = 0; q < 4 && x + q < W; q++) dst[q] = r[q];
		}
	}
}

int bhip_launch_conv(bhip_ctx* ctx, bool vertical, bool normalized, const float* kernel, int kw, int koff, DevImg<const float> in, DevImg<float> out) {
	const int width = in.width, height = in.height, batch = in.batch;
	if (kw <= 0 || kw > BHIP_MAX_TAPS || koff < 0 || koff >= kw) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "kernel width not supported");
	if (width <= 0 || height <= 0 || batch <= 0) return BHIP_OK;
	ConvParams P;
	P.in = in.data; P.out = out.data; P.inStride = in.stride; P.outStride = out.stride; P.width = width; P.height = height; P.kw = kw; P.koff = koff;
	P.inImageStride = in.imageStride; P.outImageStride = out.imageStride;
	for (int i = 0; i < kw; i++) P.k[i] = kernel[i];
	P.unrolled = (koff == kw / 2 && kw % 2 == 1 && (kw == 3 || kw == 5 || kw == 7 || kw == 9 || kw == 11)) ? 1 : 0;
	P.mode = 0;
	P.borderOnly = 0;
	if (normalized) setNormalizedMode(P, vertical ? height : width);
	ProfScope prof(ctx, vertical ? "k_conv_v" : "k_conv_h", 8.0 * width * height * batch);
	// tiled forms need 16-byte aligned rows on both sides; the naive form (kernel wider than the image) stays on the general kernel
	const bool tiled = P.mode != 2 && vec4(in) && vec4(out) && kw <= 97;
	if (!tiled) {
		dim3 grid((width + 255) / 256, height, batch);
		if (vertical) hipLaunchKernelGGL(k_conv<true>, grid, dim3(256), 0, ctx->stream, P);
		else hipLaunchKernelGGL(k_conv<false>, grid, dim3(256), 0, ctx->stream, P);
	} else if (P.unrolled) {
		// the reference's unrolled widths: register-streaming kernels
		const int rows = vertical ? CS_ROWS_V : CS_ROWS;
		dim3 grid((width + 255) / 256, (height + 4 * rows - 1) / (4 * rows), batch);
#define LAUNCH_S(KWT)                                                                                      \
	do {                                                                                                   \
		if (vertical) hipLaunchKernelGGL(k_conv_v_stream<KWT>, grid, dim3(256), 0, ctx->stream, P);        \
		else hipLaunchKernelGGL(k_conv_h_stream<KWT>, grid, dim3(256), 0, ctx->stream, P);                 \
	} while (0)
		switch (kw) {
		case 3: LAUNCH_S(3); break;
		case 5: LAUNCH_S(5); break;
		case 7: LAUNCH_S(7); break;
		case 9: LAUNCH_S(9); break;
		default: LAUNCH_S(11); break;
		}
#undef LAUNCH_S
		if (P.mode == 1) {
			// the kw - 1 border columns (rows) with the re-normalised formula: a thin launch of the general kernel
			P.borderOnly = 1;
			if (vertical) hipLaunchKernelGGL(k_conv<true>, dim3((width + 255) / 256, kw - 1, batch), dim3(256), 0, ctx->stream, P);
			else hipLaunchKernelGGL(k_conv<false>, dim3((unsigned)(((long long)height * (kw - 1) + 255) / 256), 1, batch), dim3(256), 0, ctx->stream, P);
		}
	} else if (vertical) {
		dim3 grid((width + CT_W - 1) / CT_W, (height + CV_ROWS - 1) / CV_ROWS, batch);
		const size_t ldsBytes = (size_t)(CV_ROWS + kw - 1) * CT_W * 4 + (size_t)kw * 4;   // rows + the kernel
		if (ldsBytes > 65536) BHIP_HIP(ctx, hipFuncSetAttribute((const void*)k_conv_v_tile<0, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes));
		hipLaunchKernelGGL((k_conv_v_tile<0, 16>), grid, dim3(1024), ldsBytes, ctx->stream, P);
	} else {
		const int offR = kw - koff - 1;
		const int padL = (koff + 3) & ~3, padR = (offR + 3) & ~3;
		const int ldsRow = CT_W + padL + padR;
		dim3 grid((width + CT_W - 1) / CT_W, (height + CT_ROWS - 1) / CT_ROWS, batch);
		const size_t ldsBytes = (size_t)CT_ROWS * ldsRow * 4 + (size_t)kw * 4;   // rows + the kernel
#define LAUNCH_H(KWT) hipLaunchKernelGGL(k_conv_h_tile<KWT>, grid, dim3(256), ldsBytes, ctx->stream, P, padL, ldsRow)
		LAUNCH_H(0);
#undef LAUNCH_H
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// BlurImageOps.gaussian in one pass; returns *done = false when the shape / kernel is outside what the fused kernel covers (the caller
// then runs the two separable passes)
int bhip_launch_blur_fused(bhip_ctx* ctx, const float* kernel, int kw, DevImg<const float> in, DevImg<float> out, bool* done) {
	const int width = in.width, height = in.height, batch = in.batch;
	*done = false;
	if (width <= 0 || height <= 0 || batch <= 0) { *done = true; return BHIP_OK; }
	const bool unrolled = kw == 3 || kw == 5 || kw == 7 || kw == 9 || kw == 11;
	if (!unrolled || kw >= width || kw >= height) return BHIP_OK;   // standard-form widths and the naive form (kernel wider than the image)
	if (!(vec4(in) && vec4(out))) return BHIP_OK;
	if (bhip_env_flag("BHIP_BLUR_TWO_PASS")) return BHIP_OK;        // parity cross-check of the two forms
	ConvParams P;
	P.in = in.data; P.out = out.data; P.inStride = in.stride; P.outStride = out.stride; P.width = width; P.height = height; P.kw = kw; P.koff = kw / 2;
	P.inImageStride = in.imageStride; P.outImageStride = out.imageStride;
	for (int i = 0; i < kw; i++) P.k[i] = kernel[i];
	P.unrolled = 1; P.mode = 1; P.borderOnly = 0;
	{
		// ConvolveImageNormalized: re-normalise when |sum - 1| > 1e-4 (both passes see the same kernel)
		float sum = 0;
		for (int i = 0; i < kw; i++) sum += P.k[i];
		float diff = sum - 1.0f;
		if (diff < 0) diff = -diff;
		if (diff > 1e-4f) {
			float total = 0;
			for (int i = 0; i < kw; i++) total += P.k[i];
			for (int i = 0; i < kw; i++) P.k[i] /= total;
		}
	}
	// algorithmic bytes: the two separable passes of SURVEY 8d (8P each)
	ProfScope prof(ctx, "k_blur_fused", 16.0 * width * height * batch);
	const int rowsPerWave = BF_ROWS;
	dim3 grid((width + 255) / 256, (height + 4 * rowsPerWave - 1) / (4 * rowsPerWave), batch);
	switch (kw) {
	case 3: hipLaunchKernelGGL(k_blur_fused<3>, grid, dim3(256), 0, ctx->stream, P); break;
	case 5: hipLaunchKernelGGL(k_blur_fused<5>, grid, dim3(256), 0, ctx->stream, P); break;
	case 7: hipLaunchKernelGGL(k_blur_fused<7>, grid, dim3(256), 0, ctx->stream, P); break;
	// the wide kernels run one wave per workgroup: at 125 registers a CU holds 16 waves either way, but a wave slot is then free again as soon
	// as ITS strip is done instead of when the slowest of four is (r = 5 on 64 x 1080p: 0.64 -> 0.62 ms)
	case 9: hipLaunchKernelGGL((k_blur_fused<9, 1>), dim3(grid.x, (height + rowsPerWave - 1) / rowsPerWave, batch), dim3(64), 0, ctx->stream, P); break;
	default: hipLaunchKernelGGL((k_blur_fused<11, 1>), dim3(grid.x, (height + rowsPerWave - 1) / rowsPerWave, batch), dim3(64), 0, ctx->stream, P); break;
	}
	BHIP_HIP(ctx, hipGetLastError());
	*done = true;
	return BHIP_OK;
}

// ---------------- remaining BOverride hooks: 2-D convolution, mean blur, median blur ----------------
// ConvolveImageNoBorder.convolve(Kernel2D_F32)   I:alg/filter/convolve/ConvolveImageNoBorder.java:79-90
//   unrolled widths 3..11: row sums from 0, added in order   I:.../noborder/ConvolveImageUnrolled_SB_F32_F32.java:592-644
//   standard: one running total, row-major                   I:.../noborder/ConvolveImageStandard_SB.java:106-134
#define BHIP_MAX_TAPS2D 441   // 21 x 21
struct Conv2DParams {
	const float* in; float* out;
	int inStride, outStride, width, height, kw, koff, unrolled;
	float k[BHIP_MAX_TAPS2D];
};
__global__ __launch_bounds__(256) void k_conv2d(Conv2DParams P) {
	const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
	const int oL = P.koff, oR = P.kw - P.koff - 1;
	if (x < oL || x >= P.width - oR || y < oL || y >= P.height - oR) return;
	const float* s = P.in + (long long)(y - oL) * P.inStride + (x - oL);
	float total = 0;
	if (P.unrolled) {
		for (int i = 0; i < P.kw; i++) {
			float rowTotal = 0;
			for (int j = 0; j < P.kw; j++) rowTotal += s[(long long)i * P.inStride + j] * P.k[i * P.kw + j];
			total = i == 0 ? rowTotal : total + rowTotal;
		}
	} else {
		int ik = 0;
		for (int i = 0; i < P.kw; i++)
			for (int j = 0; j < P.kw; j++) total += s[(long long)i * P.inStride + j] * P.k[ik++];
	}
	P.out[(long long)y * P.outStride + x] = total;
}
int bhip_launch_conv2d(bhip_ctx* ctx, const float* kernel, int kw, int koff, DevImg<const float> in, DevImg<float> out) {
	const int width = in.width, height = in.height;
	if (kw <= 0 || kw * kw > BHIP_MAX_TAPS2D || koff < 0 || koff >= kw) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "kernel width not supported");
	Conv2DParams P;
	P.in = in.data; P.out = out.data; P.inStride = in.stride; P.outStride = out.stride; P.width = width; P.height = height; P.kw = kw; P.koff = koff;
	P.unrolled = (koff == kw / 2 && kw % 2 == 1 && (kw == 3 || kw == 5 || kw == 7 || kw == 9 || kw == 11)) ? 1 : 0;
	for (int i = 0; i < kw * kw; i++) P.k[i] = kernel[i];
	ProfScope prof(ctx, "k_conv2d", 8.0 * width * height);
	hipLaunchKernelGGL(k_conv2d, dim3((width + 255) / 256, height), dim3(256), 0, ctx->stream, P);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// BlurImageOps.mean -> ConvolveImageMean.horizontal / vertical  I:alg/filter/convolve/ConvolveImageMean.java:55-101
//   interior: float running sums, total / divisor   I:alg/filter/convolve/noborder/ImplConvolveMean.java:281-357 (single-threaded order)
//   border: ConvolveNormalized_JustBorder_SB with the table kernel (k_conv mode 3)
// As in the corner intensity, a row (then a column) is one sequential chain; one thread each.
__global__ __launch_bounds__(64) void k_mean_rows(const float* __restrict__ in, long long inImageStride, int inStride, float* __restrict__ out,
												  long long outImageStride, int outStride, int width, int height, int radius) {
	const int y = blockIdx.x * blockDim.x + threadIdx.x;
	if (y >= height) return;
	const int kw = 2 * radius + 1;
	const float divisor = (float)kw;
	const float* r = in + (long long)blockIdx.z * inImageStride + (long long)y * inStride;
	float* o = out + (long long)blockIdx.z * outImageStride + (long long)y * outStride;
	float total = 0;
	for (int i = 0; i < kw; i++) total += r[i];
	o[radius] = total / divisor;
	int i = kw;
	for (; i + 16 <= width; i += 16) {
		float a[16], b[16], q[16];
#pragma unroll
		for (int k = 0; k < 16; k++) { a[k] = r[i - kw + k]; b[k] = r[i + k]; }
#pragma unroll
		for (int k = 0; k < 16; k++) { total -= a[k]; total += b[k]; q[k] = total / divisor; }
#pragma unroll
		for (int k = 0; k < 16; k++) o[i - radius + k] = q[k];
	}
	for (; i < width; i++) {
		total -= r[i - kw];
		total += r[i];
		o[i - radius] = total / divisor;
	}
}
__global__ __launch_bounds__(256) void k_mean_cols(const float* __restrict__ in, long long inImageStride, int inStride, float* __restrict__ out,
												   long long outImageStride, int outStride, int width, int height, int radius) {
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= width) return;
	in += (long long)blockIdx.z * inImageStride;
	out += (long long)blockIdx.z * outImageStride;
	const int kw = 2 * radius + 1;
	const float divisor = (float)kw;
	float total = 0;
	for (int k = 0; k < kw; k++) total += in[(long long)k * inStride + x];
	out[(long long)radius * outStride + x] = total / divisor;
	int y = radius + 1;
	for (; y + 8 <= height - radius; y += 8) {
		float a[8], b[8];
#pragma unroll
		for (int k = 0; k < 8; k++) { a[k] = in[(long long)(y + k + radius - kw) * inStride + x]; b[k] = in[(long long)(y + k + radius) * inStride + x]; }
#pragma unroll
		for (int k = 0; k < 8; k++) {
			total = total - a[k];
			total += b[k];
			out[(long long)(y + k) * outStride + x] = total / divisor;
		}
	}
	for (; y < height - radius; y++) {
		total = total - in[(long long)(y + radius - kw) * inStride + x];
		total += in[(long long)(y + radius) * inStride + x];
		out[(long long)y * outStride + x] = total / divisor;
	}
}
// one direction of the mean blur: in / out of the same shape, every image of the batch
int bhip_launch_mean(bhip_ctx* ctx, bool vertical, DevImg<const float> in, DevImg<float> out, int radius) {
	const int width = in.width, height = in.height;
	const int kw = 2 * radius + 1;
	if (kw > BHIP_MAX_TAPS) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "mean radius not supported");
	float ker[BHIP_MAX_TAPS];
	const float val = 1.0f / (float)kw;   // FactoryKernel.table1D_F32(radius, true)
	for (int i = 0; i < kw; i++) ker[i] = val;
	const int extent = vertical ? height : width;
	if (kw > extent) return bhip_launch_conv(ctx, vertical, true, ker, kw, radius, in, out);   // ConvolveImageNormalized
	// border first (k_conv mode 3), then the interior chains
	{
		ConvParams P;
		P.in = in.data; P.out = out.data; P.inStride = in.stride; P.outStride = out.stride; P.width = width; P.height = height; P.kw = kw; P.koff = radius;
		P.inImageStride = in.imageStride; P.outImageStride = out.imageStride; P.borderOnly = 0;
		for (int i = 0; i < kw; i++) P.k[i] = ker[i];
		P.unrolled = 0; P.mode = 3;
		dim3 grid((width + 255) / 256, height, in.batch);
		if (vertical) hipLaunchKernelGGL(k_conv<true>, grid, dim3(256), 0, ctx->stream, P);
		else hipLaunchKernelGGL(k_conv<false>, grid, dim3(256), 0, ctx->stream, P);
	}
	ProfScope prof(ctx, vertical ? "k_mean_cols" : "k_mean_rows", 8.0 * width * height * in.batch);
	if (vertical)
		hipLaunchKernelGGL(k_mean_cols, dim3((width + 255) / 256, 1, in.batch), dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride,
						   out.stride, width, height, radius);
	else
		hipLaunchKernelGGL(k_mean_rows, dim3((height + 63) / 64, 1, in.batch), dim3(64), 0, ctx->stream, in.data, in.imageStride, in.stride, out.data, out.imageStride,
						   out.stride, width, height, radius);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

// BlurImageOps.median(GrayF32) -> ImplMedianSortNaive.process  I:alg/filter/blur/impl/ImplMedianSortNaive.java:97-135: the (count/2)-th order
// statistic of the window clipped to the image.  16x16 pixel tiles staged in LDS with their halo; each thread finds the window
// element v with #(w < v) <= k < #(w <= v) -- comparisons only, so the result is the reference's value exactly.
#define MED_T 16
__global__ __launch_bounds__(MED_T * MED_T) void k_median(const float* __restrict__ in, int inStride, float* __restrict__ out, int outStride, int width, int height,
															int radius) {
	extern __shared__ float tile[];
	const int TW = MED_T + 2 * radius;
	const int x0 = blockIdx.x * MED_T - radius, y0 = blockIdx.y * MED_T - radius;
	for (int i = threadIdx.y * MED_T + threadIdx.x; i < TW * TW; i += MED_T * MED_T) {
		const int ty = i / TW, tx = i - ty * TW;
		const int gx = x0 + tx, gy = y0 + ty;
		tile[i] = (gx >= 0 && gx < width && gy >= 0 && gy < height) ? in[(long long)gy * inStride + gx] : 0.0f;
	}
	__syncthreads();
	const int x = blockIdx.x * MED_T + threadIdx.x, y = blockIdx.y * MED_T + threadIdx.y;
	if (x >= width || y >= height) return;
	const int minI = max(0, y - radius) - y0, maxI = min(height, y + radius + 1) - y0;   // tile coordinates
	const int minJ = max(0, x - radius) - x0, maxJ = min(width, x + radius + 1) - x0;
	const int count = (maxI - minI) * (maxJ - minJ), k = count / 2;
	float result = 0;
	for (int i = minI; i < maxI; i++)
		for (int j = minJ; j < maxJ; j++) {
			const float v = tile[i * TW + j];
			int less = 0, leq = 0;
			for (int a = minI; a < maxI; a++)
				for (int b = minJ; b < maxJ; b++) {
					const float w = tile[a * TW + b];
					less += w < v ? 1 : 0;
					leq += w <= v ? 1 : 0;
				}
			if (less <= k && k < leq) result = v;
		}
	out[(long long)y * outStride + x] = result;
}
int bhip_launch_median(bhip_ctx* ctx, DevImg<const float> in, DevImg<float> out, int radius) {
	const int width = in.width, height = in.height;
	if (radius > 8) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "median radius > 8 is not supported on the GPU");
	const int TW = MED_T + 2 * radius;
	ProfScope prof(ctx, "k_median", 8.0 * width * height);
	hipLaunchKernelGGL(k_median, dim3((width + MED_T - 1) / MED_T, (height + MED_T - 1) / MED_T), dim3(MED_T, MED_T), (size_t)TW * TW * 4, ctx->stream, in.data, in.stride,
					   out.data, out.stride, width, height, radius);
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
