// ---------------------------------------------------------------------------------------------------------------
// Edge features of a gradient on batches of device frames (F:alg/feature/detect/edge/*.java), any row / image stride:
//   intensityAbs on GrayS16 derivatives      impl/ImplGradientToEdgeFeatures.java:151-169: |dx| + |dy| in int, stored as float
//                                            (the GrayF32 form is k_grad_intensity of gradient.hip)
//   nonMaxSuppressionCrude4                  GradientToEdgeFeatures.java:143-157, 248-262 -> impl/ImplEdgeNonMaxSuppressionCrude.java
//                                            inner4 :50-115, border4 :155-242 (GrayF32 derivatives) and the GrayI form after it
// Crude suppression: the step (dx, dy) is the sign of the two derivatives (+1 where the derivative is > 0, else -1: zero and NaN step
// backwards), the pixel keeps its intensity unless the intensity at (x-dx, y-dy) or at (x+dx, y+dy) is greater, and the border loops read
// the intensity through ImageBorderValue(0).  That makes one rule for every pixel: a neighbour outside the image is 0.  (Width or height
// 1 and 2 have no inner pixels; the border loops then write the same value more than once.)
// ---------------------------------------------------------------------------------------------------------------
#include "common.h"

__global__ __launch_bounds__(256) void k_grad_intensity_abs_s16(const int16_t* __restrict__ dx, const int16_t* __restrict__ dy, long long dImageStride, int dStride,
																 float* __restrict__ out, long long oImageStride, int oStride, int width) {
	const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
	if (x >= width) return;
	const long long i = (long long)blockIdx.z * dImageStride + (long long)y * dStride + x;
	out[(long long)blockIdx.z * oImageStride + (long long)y * oStride + x] = (float)(abs((int)dx[i]) + abs((int)dy[i]));
}
int bhip_launch_grad_intensity_abs_s16(bhip_ctx* ctx, DevImg<const int16_t> dx, DevImg<const int16_t> dy, DevImg<float> out) {
	if (dx.stride != dy.stride || dx.imageStride != dy.imageStride) return bhip_fail(ctx, BHIP_ERR_INVALID, "dx and dy must share one layout");
	{
		ProfScope prof(ctx, "k_grad_intensity_abs_s16", 8.0 * dx.width * dx.height * dx.batch);
		hipLaunchKernelGGL(k_grad_intensity_abs_s16, dim3((dx.width + 255) / 256, dx.height, dx.batch), dim3(256), 0, ctx->stream, dx.data, dy.data, dx.imageStride,
						   dx.stride, out.data, out.imageStride, out.stride, dx.width);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}

template <class T>
__global__ __launch_bounds__(256) void k_edge_nonmax_crude4(const float* __restrict__ intensity, long long iImageStride, int iStride, const T* __restrict__ derivX,
															 const T* __restrict__ derivY, long long dImageStride, int dStride, float* __restrict__ out,
															 long long oImageStride, int oStride, int width, int height) {
	const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
	if (x >= width) return;
	const float* I = intensity + (long long)blockIdx.z * iImageStride;
	const long long d = (long long)blockIdx.z * dImageStride + (long long)y * dStride + x;
	const int dx = derivX[d] > 0 ? 1 : -1, dy = derivY[d] > 0 ? 1 : -1;
	const float middle = I[(long long)y * iStride + x];
	const int lx = x - dx, ly = y - dy, rx = x + dx, ry = y + dy;
	const float left = (lx >= 0 && lx < width && ly >= 0 && ly < height) ? I[(long long)ly * iStride + lx] : 0.0f;
	const float right = (rx >= 0 && rx < width && ry >= 0 && ry < height) ? I[(long long)ry * iStride + rx] : 0.0f;
	out[(long long)blockIdx.z * oImageStride + (long long)y * oStride + x] = (left > middle || right > middle) ? 0.0f : middle;
}
// intensity and out must not overlap (a pixel reads its neighbours' intensities)
template <class T>
int bhip_launch_edge_nonmax_crude4(bhip_ctx* ctx, DevImg<const float> intensity, DevImg<const T> dx, DevImg<const T> dy, DevImg<float> out) {
	if (dx.stride != dy.stride || dx.imageStride != dy.imageStride) return bhip_fail(ctx, BHIP_ERR_INVALID, "dx and dy must share one layout");
	const int W = intensity.width, H = intensity.height, B = intensity.batch;
	{
		ProfScope prof(ctx, "k_edge_nonmax_crude4", (8.0 + 2.0 * sizeof(T)) * W * H * B);
		hipLaunchKernelGGL(k_edge_nonmax_crude4<T>, dim3((W + 255) / 256, H, B), dim3(256), 0, ctx->stream, intensity.data, intensity.imageStride, intensity.stride, dx.data,
						   dy.data, dx.imageStride, dx.stride, out.data, out.imageStride, out.stride, W, H);
	}
	BHIP_HIP(ctx, hipGetLastError());
	return BHIP_OK;
}
template int bhip_launch_edge_nonmax_crude4<float>(bhip_ctx*, DevImg<const float>, DevImg<const float>, DevImg<const float>, DevImg<float>);
template int bhip_launch_edge_nonmax_crude4<int16_t>(bhip_ctx*, DevImg<const float>, DevImg<const int16_t>, DevImg<const int16_t>, DevImg<float>);
