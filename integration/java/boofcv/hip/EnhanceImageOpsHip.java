package boofcv.hip;

import boofcv.alg.InputSanityCheck;
import boofcv.concurrency.IWorkArrays;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;

/** EnhanceImageOps (main/boofcv-ip/.../alg/enhance/EnhanceImageOps.java) on GrayU8 (sharpen also on GrayF32) and ImageStatistics.histogram(GrayU8, ..),
 *  over the bhip_histogram_* / bhip_apply_transform_* / bhip_equalize_local_* / bhip_sharpen_* exports.  The reference has no BOverride hook for
 *  EnhanceImageOps, so this is a provider class with the same static signatures: call EnhanceImageOpsHip.equalizeLocal(...) where the code called
 *  EnhanceImageOps.equalizeLocal(...).  Results are bit for bit those of the single-threaded Java methods.
 *  Differences: equalizeLocal and sharpen refuse an output that overlaps the input, a radius beyond 255 and a histogramLength outside 1 .. 256
 *  (IllegalArgumentException); equalizeLocal ranks a pixel >= histogramLength like any other, histogram drops a pixel outside
 *  minValue .. minValue + histogram.length - 1 and applyTransform writes 0 for a pixel beyond the table, where the reference throws
 *  ArrayIndexOutOfBoundsException; workArrays is not used.  equalize is the reference's own host loop.
 *  Not provided: the GrayU16 / GrayS8 / GrayS16 / GrayS32 forms.
 *  UNCOMPILED SOURCE. */
public final class EnhanceImageOpsHip {
	private EnhanceImageOpsHip() {}

	// BHIP_EQLOCAL_AUTO of include/boofhip.h
	private static final int PATH_AUTO = 0;

	public static void histogram(GrayU8 input, int minValue, int[] histogram) {
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.histogramU8(ctx, input.data, input.startIndex, input.stride, input.width, input.height, minValue, histogram.length, histogram));
	}

	public static void equalize(int[] histogram, int[] transform) {
		// host logic (int arithmetic, as bhip_equalize_table_dev does on the device): prefix sums scaled by (length - 1) / total
		final int n = histogram.length;
		int total = 0;
		for (int h : histogram) total += h;
		int running = 0;
		for (int i = 0; i < n; i++) {
			running += histogram[i];
			transform[i] = running * (n - 1) / total;
		}
	}

	public static void applyTransform(GrayU8 input, int[] transform, GrayU8 output) {
		output.reshape(input.width, input.height);
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.applyTransformU8(ctx, input.data, input.startIndex, input.stride, input.width, input.height, transform, transform.length,
				output.data, output.startIndex, output.stride));
	}

	public static void equalizeLocal(GrayU8 input, int radius, GrayU8 output, int histogramLength, IWorkArrays workArrays) {
		if (output.data == input.data) throw new IllegalArgumentException("input and output must not share their array");
		output.reshape(input.width, input.height);
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.equalizeLocalU8(ctx, input.data, input.startIndex, input.stride, input.width, input.height, radius, histogramLength, PATH_AUTO,
				output.data, output.startIndex, output.stride));
	}

	private static void sharpen(int rule, GrayU8 input, GrayU8 output) {
		InputSanityCheck.checkSameShape(input, output);
		if (output.data == input.data) throw new IllegalArgumentException("input and output must not share their array");
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.sharpenU8(ctx, rule, input.data, input.startIndex, input.stride, input.width, input.height, output.data, output.startIndex,
				output.stride));
	}

	private static void sharpen(int rule, GrayF32 input, GrayF32 output) {
		InputSanityCheck.checkSameShape(input, output);
		if (output.data == input.data) throw new IllegalArgumentException("input and output must not share their array");
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.sharpenF32(ctx, rule, input.data, input.startIndex, input.stride, input.width, input.height, output.data, output.startIndex,
				output.stride));
	}

	public static void sharpen4(GrayU8 input, GrayU8 output) { sharpen(4, input, output); }

	public static void sharpen4(GrayF32 input, GrayF32 output) { sharpen(4, input, output); }

	public static void sharpen8(GrayU8 input, GrayU8 output) { sharpen(8, input, output); }

	public static void sharpen8(GrayF32 input, GrayF32 output) { sharpen(8, input, output); }
}
