package boofcv.hip;

import boofcv.alg.InputSanityCheck;
import boofcv.struct.QueueCorner;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayS16;
import boofcv.struct.image.GrayU8;
import georegression.misc.CachedSineCosine_F32;

/** The image stages of the Hough line detectors (main/boofcv-feature/.../alg/feature/detect/line/HoughTransformBinary.java with
 *  HoughParametersPolar, and the gradient FactoryDerivative.prewitt gives HoughGradient_to_DetectLine) over the host-buffer exports
 *  bhip_prewitt_*, bhip_hough_polar_bins, bhip_hough_binary_polar_u8 and bhip_nonmax_block_relaxed_f32.  The reference has no BOverride hook
 *  for these classes, so this is a provider class: a HoughTransformBinary subclass overrides computeParameters / extractLines with
 *  houghBinaryPolar and nonmaxRelaxed and keeps transformToLine, isTransformValid and the merge in Java.  Results are bit for bit those of
 *  the single-threaded Java classes.
 *  Differences: a vote whose linear index falls outside the transform is dropped where the reference throws
 *  ArrayIndexOutOfBoundsException; images of more than 2^24 pixels are refused (a float count stops there).
 *  The gradient foot-of-norm transform, the crude edge suppression and the mean-shift refinement have device-resident exports only
 *  (bhip_hough_gradient_foot_dev_*, bhip_edge_nonmax_crude4_dev_*, bhip_mean_shift_peak_dev_f32): they are reached through device buffers.
 *  Not provided: houghLinePolar(ConfigHoughGradient, ...), houghLineFootSub, lineRansac, GrayS32 derivatives.
 *  UNCOMPILED SOURCE. */
public final class HoughLinesHip {
	private HoughLinesHip() {}

	// border of bhip_prewitt_*: 0 = null, 1 = ImageBorderValue(0), 2 = BorderType.EXTENDED
	public static final int BORDER_NONE = 0, BORDER_ZERO = 1, BORDER_EXTENDED = 2;

	/** GradientPrewitt.process(GrayF32, GrayF32, GrayF32, border) */
	public static void prewitt(GrayF32 orig, GrayF32 derivX, GrayF32 derivY, int border) {
		InputSanityCheck.reshapeOneIn(orig, derivX, derivY);
		if (derivX.startIndex != derivY.startIndex || derivX.stride != derivY.stride) throw new IllegalArgumentException("derivX and derivY must share their layout");
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.prewittF32(ctx, orig.data, orig.startIndex, orig.stride, orig.width, orig.height, derivX.data, derivY.data, derivX.startIndex,
				derivX.stride, border));
	}

	/** GradientPrewitt.process(GrayU8, GrayS16, GrayS16, border) */
	public static void prewitt(GrayU8 orig, GrayS16 derivX, GrayS16 derivY, int border) {
		InputSanityCheck.reshapeOneIn(orig, derivX, derivY);
		if (derivX.startIndex != derivY.startIndex || derivX.stride != derivY.stride) throw new IllegalArgumentException("derivX and derivY must share their layout");
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.prewittU8S16(ctx, orig.data, orig.startIndex, orig.stride, orig.width, orig.height, derivX.data, derivY.data, derivX.startIndex,
				derivX.stride, border));
	}

	/** HoughParametersPolar.initialize followed by HoughTransformBinary.computeParameters on a cleared transform: reshapes `transform` to
	 *  numBinsRange x numBinsAngle and fills it with the counts.  tableTrig: the parameters' CachedSineCosine_F32(0, (float)Math.PI, numBinsAngle). */
	public static void houghBinaryPolar(GrayU8 binary, double rangeResolution, int numBinsAngle, CachedSineCosine_F32 tableTrig, GrayF32 transform) {
		int[] numBinsRange = new int[1];
		float[] rMax = new float[1];
		if (BoofHip.houghPolarBins(binary.width, binary.height, rangeResolution, numBinsRange, rMax) != 0) throw new IllegalArgumentException("bad image size");
		if (numBinsRange[0] <= 0) throw new IllegalArgumentException("the transform has no range bins");
		transform.reshape(numBinsRange[0], numBinsAngle);
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.houghBinaryPolarU8(ctx, binary.data, binary.startIndex, binary.stride, binary.width, binary.height, rangeResolution, numBinsAngle,
				tableTrig.c, tableTrig.s, transform.data, transform.startIndex, transform.stride, transform.width, transform.height));
	}

	/** NonMaxBlock.process with NonMaxBlockSearchRelaxed.Max, the extractor of FactoryFeatureExtractor.nonmax(ConfigExtract(radius, threshold,
	 *  border, false)): foundMax is reset and filled in the reference's order */
	public static void nonmaxRelaxed(GrayF32 intensity, int radius, float threshold, int border, QueueCorner foundMax) {
		final long ctx = BoofHipContext.get();
		int cap = Math.max(1, intensity.width * intensity.height);
		short[] xy = new short[2 * cap];
		int[] n = new int[1];
		BoofHip.check(ctx, BoofHip.nonmaxBlockRelaxedF32(ctx, intensity.data, intensity.startIndex, intensity.stride, intensity.width, intensity.height, radius, threshold,
				border, xy, cap, n));
		foundMax.reset();
		for (int i = 0; i < Math.min(n[0], cap); i++) foundMax.add(xy[2 * i], xy[2 * i + 1]);
	}
}
