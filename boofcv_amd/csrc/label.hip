// ---------------------------------------------------------------------------------------------------------------
// The labelled GrayS32 image and the blob count of BinaryImageOps.contour(input, rule, output) (I:alg/filter/binary/BinaryImageOps.java:457-469,
// LinearContourLabelChang2004.process :96-152 with ContourTracer), ConnectRule.FOUR and EIGHT.  A pixel equal to 1 is foreground, anything
// else background (label 0).  The reference numbers a blob when its raster scan first meets one of its pixels, so its labelled image is
// "connected components, numbered from 1 in the raster order of each component's first pixel" and the contour count is the number of
// components (tests/test_binaryops_reference.py checks the restated reference against exactly that).  The ordered contour point lists are a
// serial walk and are not produced.
//
// parent[] holds, per image, one int per pixel: -1 for background, else the linear index y*width + x of another pixel of the same component.
// INVARIANT: parent[p] <= p, and a link is only ever lowered (atomicMin).  Every find() loop therefore walks strictly decreasing indices
// and ends; a cycle is impossible.  The root of a component is its smallest linear index = its first pixel in raster order.
//
// No workgroup waits for another: each phase that needs another phase's results is its own launch.
//   1. k_label_tile     union-find over a 32 x 32 tile in LDS, roots written to parent[] as image indices
//   2. k_label_merge    pixels in the first row / column of a tile are united with their neighbours across the tile edge (for EIGHT the
//                       diagonal ones too, which covers tile corners).  Other workgroups change parent[] meanwhile and L1 / the per-XCD L2s
//                       are not coherent within a launch, so EVERY access to parent[] here is an agent-scope atomic (relaxed load, atomicMin).
//   3. k_label_flatten  parent[p] = root(p) (only ever an ancestor is stored, so concurrent finds stay correct); roots counted per row
//   4. k_label_scan     exclusive scan of the row counts per image; the total is numBlobs
//   5. k_label_rank     per row, ballot + popcount ranks the roots in raster order: out[root] = rank + 1, background 0.  Ranks go to the
//                       output image, never into parent[], which the next phase still reads roots from
//   6. k_label_write    out[p] = out[root(p)] for the other foreground pixels (reads root positions, writes the others: disjoint)
// ---------------------------------------------------------------------------------------------------------------
#include "common.h"
#include <algorithm>

#define LT 32   // tile side

// ---- LDS union-find (one workgroup) ----
__device__ __forceinline__ int ldsLoad(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int findL(const int* L, int i) {
	int p;
	while ((p = ldsLoad(L + i)) != i) i = p;   // strictly decreasing
	return i;
}
__device__ __forceinline__ void uniteL(int* L, int a, int b) {
	for (;;) {
		a = findL(L, a);
		b = findL(L, b);
		if (a == b) return;
		if (a < b) { const int t = a; a = b; b = t; }
		const int old = atomicMin(L + a, b);   // the larger root now points at the smaller one, unless somebody lowered it first
		if (old == a) return;
		a = old;                               // old < a: still strictly decreasing
	}
}
// ---- the same on parent[] in global memory, every access an agent-scope atomic ----
__device__ __forceinline__ int parentLoad(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int findG(const int* P, int i) {
	int p;
	while ((p = parentLoad(P + i)) != i) i = p;
	return i;
}
__device__ __forceinline__ void uniteG(int* P, int a, int b) {
	for (;;) {
		a = findG(P, a);
		b = findG(P, b);
		if (a == b) return;
		if (a < b) { const int t = a; a = b; b = t; }
		const int old = atomicMin(P + a, b);
		if (old == a) return;
		a = old;
	}
}

__global__ __launch_bounds__(256) void k_label_tile(const uint8_t* __restrict__ in, long long inImageStride, int inStride, int width, int height, int eight,
													int* __restrict__ parent) {
	__shared__ int L[LT * LT];
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * LT, y0 = blockIdx.y * LT;
	const uint8_t* src = in + (long long)blockIdx.z * inImageStride;
	int* P = parent + (long long)blockIdx.z * width * height;
#pragma unroll
	for (int k = 0; k < 4; k++) {
		const int i = tid + 256 * k, lx = i & (LT - 1), ly = i >> 5;
		const int gx = x0 + lx, gy = y0 + ly;
		const bool fg = gx < width && gy < height && src[(long long)gy * inStride + gx] == 1;
		L[i] = fg ? i : -1;
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < 4; k++) {
		const int i = tid + 256 * k, lx = i & (LT - 1), ly = i >> 5;
		if (ldsLoad(L + i) < 0) continue;   // background stays -1 for good
		if (lx > 0 && ldsLoad(L + i - 1) >= 0) uniteL(L, i, i - 1);
		if (ly > 0) {
			if (ldsLoad(L + i - LT) >= 0) uniteL(L, i, i - LT);
			if (eight) {
				if (lx > 0 && ldsLoad(L + i - LT - 1) >= 0) uniteL(L, i, i - LT - 1);
				if (lx < LT - 1 && ldsLoad(L + i - LT + 1) >= 0) uniteL(L, i, i - LT + 1);
			}
		}
	}
	__syncthreads();
	// tile raster order and image raster order agree inside a tile, so the smallest tile index is the smallest image index
#pragma unroll
	for (int k = 0; k < 4; k++) {
		const int i = tid + 256 * k, lx = i & (LT - 1), ly = i >> 5;
		const int gx = x0 + lx, gy = y0 + ly;
		if (gx >= width || gy >= height) continue;
		int v = -1;
		if (L[i] >= 0) {
			const int r = findL(L, i);
			v = (y0 + (r >> 5)) * width + x0 + (r & (LT - 1));
		}
		P[gy * width + gx] = v;
	}
}

// boundary < nby: the row y = (boundary + 1) * LT, one lane per x; otherwise the column x = (boundary - nby + 1) * LT, one lane per y
__global__ __launch_bounds__(256) void k_label_merge(int width, int height, int eight, int nby, int nbx, int* parent) {
	int* P = parent + (long long)blockIdx.z * width * height;
	const int t = blockIdx.x * 256 + threadIdx.x;
	for (int bnd = blockIdx.y; bnd < nby + nbx; bnd += gridDim.y) {
		if (bnd < nby) {
			const int y = (bnd + 1) * LT, x = t;
			if (x >= width) continue;
			const int p = y * width + x;
			if (parentLoad(P + p) < 0) continue;
			const int q = p - width;
			if (parentLoad(P + q) >= 0) uniteG(P, p, q);
			if (eight) {
				if (x > 0 && parentLoad(P + q - 1) >= 0) uniteG(P, p, q - 1);
				if (x < width - 1 && parentLoad(P + q + 1) >= 0) uniteG(P, p, q + 1);
			}
		} else {
			const int x = (bnd - nby + 1) * LT, y = t;
			if (y >= height) continue;
			const int p = y * width + x;
			if (parentLoad(P + p) < 0) continue;
			if (parentLoad(P + p - 1) >= 0) uniteG(P, p, p - 1);
			if (eight) {
				if (y > 0 && parentLoad(P + p - 1 - width) >= 0) uniteG(P, p, p - 1 - width);
				if (y < height - 1 && parentLoad(P + p - 1 + width) >= 0) uniteG(P, p, p - 1 + width);
			}
		}
	}
}

// one wave per row
__global__ __launch_bounds__(256) void k_label_flatten(int width, int height, int* parent, int* __restrict__ rowCount) {
	const int y = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (y >= height) return;
	int* P = parent + (long long)blockIdx.z * width * height + (long long)y * width;
	const int* P0 = parent + (long long)blockIdx.z * width * height;
	int count = 0;
	for (int x = lane; x < width; x += 64) {
		const int v = parentLoad(P + x);
		if (v < 0) continue;
		const int r = findG(P0, v);
		if (r != v) __hip_atomic_store(P + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (r == y * width + x) count++;
	}
	for (int d = 32; d > 0; d >>= 1) count += __shfl_xor(count, d);
	if (lane == 0) rowCount[(long long)blockIdx.z * height + y] = count;
}

// rowCount -> exclusive prefix in place, numBlobs[image] = total; one workgroup per image walks the rows in chunks of 256
__global__ __launch_bounds__(256) void k_label_scan(int height, int* __restrict__ rowCount, int* __restrict__ numBlobs) {
	__shared__ int s[256];
	__shared__ int carry;
	int* c = rowCount + (long long)blockIdx.x * height;
	const int tid = threadIdx.x;
	if (tid == 0) carry = 0;
	__syncthreads();
	for (int y0 = 0; y0 < height; y0 += 256) {
		const int y = y0 + tid;
		const int v = y < height ? c[y] : 0;
		s[tid] = v;
		__syncthreads();
		for (int d = 1; d < 256; d <<= 1) {
			const int a = tid >= d ? s[tid - d] : 0;
			__syncthreads();
			s[tid] += a;
			__syncthreads();
		}
		const int base = carry;
		if (y < height) c[y] = base + s[tid] - v;
		__syncthreads();
		if (tid == 255) carry = base + s[255];
		__syncthreads();
	}
	if (tid == 0) numBlobs[blockIdx.x] = carry;
}

// one wave per row: roots get rank + 1 in raster order, background gets 0
__global__ __launch_bounds__(256) void k_label_rank(int width, int height, const int* __restrict__ parent, const int* __restrict__ rowStart, int32_t* __restrict__ out,
													long long outImageStride, int outStride) {
	const int y = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (y >= height) return;
	const int* P = parent + (long long)blockIdx.z * width * height + (long long)y * width;
	int32_t* o = out + (long long)blockIdx.z * outImageStride + (long long)y * outStride;
	int base = rowStart[(long long)blockIdx.z * height + y];
	for (int xb = 0; xb < width; xb += 64) {
		const int x = xb + lane;
		const int v = x < width ? P[x] : -1;
		const bool root = v >= 0 && v == y * width + x;
		const unsigned long long m = __ballot(root);
		if (root) o[x] = base + __popcll(m & ((1ull << lane) - 1ull)) + 1;
		else if (x < width && v < 0) o[x] = 0;
		base += __popcll(m);
	}
}
__global__ __launch_bounds__(256) void k_label_write(int width, int height, const int* __restrict__ parent, int32_t* out, long long outImageStride, int outStride) {
	const int x = blockIdx.x * 256 + threadIdx.x;
	if (x >= width) return;
	const int* P = parent + (long long)blockIdx.z * width * height;
	int32_t* o = out + (long long)blockIdx.z * outImageStride;
	for (int y = blockIdx.y; y < height; y += gridDim.y) {
		const int p = y * width + x;
		const int v = P[p];
		if (v < 0 || v == p) continue;
		const int ry = v / width, rx = v - ry * width;
		o[(long long)y * outStride + x] = o[(long long)ry * outStride + rx];
	}
}

size_t bhip_label_scratch(int width, int height, int images) { return ((size_t)width * height + height) * images * 4; }
// scratch: bhip_label_scratch(width, height, in.batch) bytes; width * height fits an int (checked by the caller)
int bhip_launch_label_blobs(bhip_ctx* ctx, bool eight, DevImg<const uint8_t> in, DevImg<int32_t> out, int* devNumBlobs, void* scratch) {
	const int W = in.width, H = in.height, B = in.batch;
	int* parent = (int*)scratch;
	int* rows = parent + (size_t)W * H * B;
	const int tx = (W + LT - 1) / LT, ty = (H + LT - 1) / LT;
	const int e = eight ? 1 : 0;
	{
		ProfScope prof(ctx, "k_label_tile", 5.0 * W * H * B);
		hipLaunchKernelGGL(k_label_tile, dim3(tx, ty, B), dim3(256), 0, ctx->stream, in.data, in.imageStride, in.stride, W, H, e, parent);
	}
	if (tx + ty > 2) {
		ProfScope prof(ctx, "k_label_merge");
		hipLaunchKernelGGL(k_label_merge, dim3((std::max(W, H) + 255) / 256, std::min((ty - 1) + (tx - 1), 65535), B), dim3(256), 0, ctx->stream, W, H, e, ty - 1, tx - 1,
						   parent);
	}
	{
		ProfScope prof(ctx, "k_label_flatten", 8.0 * W * H * B);
		hipLaunchKernelGGL(k_label_flatten, dim3((H + 3) / 4, 1, B), dim3(256), 0, ctx->stream, W, H, parent, rows);
	}
	hipLaunchKernelGGL(k_label_scan, dim3(B), dim3(256), 0, ctx->stream, H, rows, devNumBlobs);
	{
		ProfScope prof(ctx, "k_label_rank", 8.0 * W * H * B);
		hipLaunchKernelGGL(k_label_rank, dim3((H + 3) / 4, 1, B), dim3(256), 0, ctx->stream, W, H, parent, rows, out.data, out.imageStride, out.stride);
	}
	{
		ProfScope prof(ctx, "k_label_write", 8.0 * W * H * B);
		hipLaunchKernelGGL(k_label_write, dim3((W + 255) / 256, std::min(H, 1024), B), dim3(256), 0, ctx->stream, W, H, parent, out.data, out.imageStride, out.stride);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
