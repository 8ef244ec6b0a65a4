// Host-side synthesis of the small Gaussian weight tables the orientation / SURF kernels read.
// Restates I:factory/filter/kernel/FactoryKernelGaussian.java (gaussian :120-135, gaussian1D_F32 :218-238,
// gaussian2D_F64 :297-306, sigmaForRadius :388, radiusForSigma :404, gaussianWidth :418-448) and
// I:alg/filter/kernel/KernelMath.java (convolve2D :365-383, normalizeSumToOne :417-452, convert :556-620).
// UtilGaussian.computePDF is a ddogleg function (not in the reference tree): exp(-d^2/(2 s^2)) / (s sqrt(2 pi)).
#include "common.h"
#include <cmath>
#include <limits>

static double pdf(double sigma, double sample) {
	return std::exp(-sample * sample / (2.0 * sigma * sigma)) / (sigma * std::sqrt(2.0 * M_PI));
}
static double sigmaForRadius(double radius) { return (radius * 2.0 + 1.0) / 5.0; }
static int radiusForSigma(double sigma) { return (int)std::ceil((5.0 * sigma - 1) / 2); }

static std::vector<double> outerNormalized(const std::vector<double>& k1) {
	const size_t w = k1.size();
	std::vector<double> out(w * w);
	size_t idx = 0;
	for (size_t i = 0; i < w; i++)
		for (size_t j = 0; j < w; j++) out[idx++] = k1[i] * k1[j];
	double total = 0;
	for (double v : out) total += v;
	for (double& v : out) v /= total;
	return out;
}

std::vector<double> bhip_gaussian2d_f64(double sigma, int radius) {
	if (radius <= 0) radius = radiusForSigma(sigma);
	else if (sigma <= 0) sigma = sigmaForRadius(radius);
	std::vector<double> k1;
	for (int i = radius; i >= -radius; i--) k1.push_back(pdf(sigma, i));
	return outerNormalized(k1);
}

std::vector<double> bhip_gaussian_width(double sigma, int width) {
	if (sigma <= 0) sigma = sigmaForRadius(width / 2);
	if (width % 2 == 1) {
		int radius = width / 2;
		std::vector<double> k1;
		for (int i = radius; i >= -radius; i--) k1.push_back(pdf(sigma, i));
		return outerNormalized(k1);
	}
	const int r = width / 2 - 1;
	std::vector<double> out((size_t)width * width);
	double sum = 0;
	for (int y = 0; y < width; y++) {
		double dy = (y <= r ? std::abs(y - r) : std::abs(y - r - 1)) + 0.5;
		for (int x = 0; x < width; x++) {
			double dx = (x <= r ? std::abs(x - r) : std::abs(x - r - 1)) + 0.5;
			double val = pdf(sigma, std::sqrt(dx * dx + dy * dy));
			out[(size_t)y * width + x] = val;
			sum += val;
		}
	}
	for (double& v : out) v /= sum;
	return out;
}

std::vector<float> bhip_gaussian1d_f32(double sigma, int radius) {
	if (radius <= 0) radius = radiusForSigma(sigma);
	else if (sigma <= 0) sigma = sigmaForRadius(radius);
	std::vector<float> k;
	for (int i = radius; i >= -radius; i--) k.push_back((float)pdf(sigma, i));
	float total = 0;
	for (float v : k) total += v;
	for (float& v : k) v /= total;
	return k;
}

// FactoryKernelGaussian.gaussian(Kernel1D_S32.class, -1, radius) = gaussian(1, false, 32, -1, radius) (FactoryKernelGaussian.java:120-160):
// the un-normalised float PDF (gaussian1D_F32(sigma, radius, true, false), :218-238) through KernelMath.convert(k, MIN_FRAC = 1/100f)
// (KernelMath.java:556-620): min = the smallest |v| >= max|v| * minFrac, out[i] = (int)(v[i] / min).  radius must be > 0.
std::vector<int32_t> bhip_gaussian1d_s32(int radius) {
	const double sigma = sigmaForRadius(radius);
	std::vector<float> k;
	for (int i = radius; i >= -radius; i--) k.push_back((float)pdf(sigma, i));
	float max = 0;
	for (float v : k) if (std::fabs(v) > max) max = std::fabs(v);
	const float minValue = max * (1.0f / 100.0f);
	float min = std::numeric_limits<float>::max();
	for (float v : k) {
		const float a = std::fabs(v);
		if (a < min && a >= minValue) min = a;
	}
	std::vector<int32_t> out;
	for (float v : k) out.push_back((int32_t)(v / min));
	return out;
}

// DescribeDenseHogAlg.computeWeightBlockPixels (F:alg/feature/dense/DescribeDenseHogAlg.java:121-161): computePDF(0, radius, d) per axis with
// sigma = half the side, an offset of 0.5 on even sides, the products divided by the largest.  A side of one pixel has sigma 0: the reference's
// arithmetic then gives NaN, and so does this
std::vector<double> bhip_dense_hog_weight_table(int rows, int cols) {
	std::vector<double> weights((size_t)rows * cols);
	const double offsetRow = rows % 2 == 0 ? 0.5 : 0, offsetCol = cols % 2 == 0 ? 0.5 : 0;
	const int radiusRow = rows / 2, radiusCol = cols / 2;
	size_t index = 0;
	for (int row = 0; row < rows; row++) {
		const double drow = row - radiusRow + offsetRow;
		const double pdfRow = pdf(radiusRow, drow);
		for (int col = 0; col < cols; col++) {
			const double dcol = col - radiusCol + offsetCol;
			const double pdfCol = pdf(radiusCol, dcol);
			weights[index++] = pdfCol * pdfRow;
		}
	}
	double max = 0;
	for (double v : weights)
		if (v > max) max = v;
	for (double& v : weights) v /= max;
	return weights;
}

// OrientationHistogramSift's constructor (F:alg/feature/orientation/OrientationHistogramSift.java:108-114): (int)(4*4/0.1) samples of
// exp(-0.5 * (i * 0.1)), the host's exp (unpinned against Java's Math.exp)
std::vector<double> bhip_sift_exp_table() {
	const double approximateStep = 0.1;
	std::vector<double> samples((size_t)(int)(4 * 4 / approximateStep));
	for (size_t i = 0; i < samples.size(); i++) {
		const double dx2 = (double)(int)i * approximateStep;
		samples[i] = std::exp(-0.5 * dx2);
	}
	return samples;
}

// DescribeSiftCommon.createGaussianWeightKernel (F:alg/feature/describe/DescribeSiftCommon.java:103-108): gaussian1D_F32(sigma, radius, odd = false,
// normalize = false) (:226-231: the float PDF at i - 0.5, i = radius .. -radius + 1), KernelMath.convolve2D (float products), divided by
// KernelMath.maxAbs over all 4 * radius^2 elements
std::vector<float> bhip_sift_gaussian_weight(double sigma, int radius) {
	std::vector<float> k1;
	for (int i = radius; i > -radius; i--) k1.push_back((float)pdf(sigma, i - 0.5));
	const size_t w = k1.size();
	std::vector<float> out(w * w);
	size_t idx = 0;
	for (size_t i = 0; i < w; i++)
		for (size_t j = 0; j < w; j++) out[idx++] = k1[i] * k1[j];
	float max = 0;
	for (float v : out) if (std::fabs(v) > max) max = std::fabs(v);
	for (float& v : out) v /= max;
	return out;
}
