package boofcv.hip;

import boofcv.alg.feature.detect.intensity.FastCornerDetector;
import boofcv.struct.QueueCorner;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;

/** FastCornerDetector (main/boofcv-feature/.../alg/feature/detect/intensity/FastCornerDetector.java:67-200) whose process() calls run on the
 *  device: bhip_fast_u8 / bhip_fast_f32 classify every interior pixel with the rule the ImplFastCorner{9..12} decision trees search, score it as
 *  ImplFastHelper_U8 / _F32 do and return the dark / bright corner lists in raster order, with the per-row early stop of maxFeaturesFraction.
 *  It is a FastCornerDetector, so WrapperFastCornerIntensity, WrapFastToPointDetector and FactoryDetectPoint.createGeneral take it as they take
 *  the Java one:
 *      new GeneralFeatureDetector<>(new WrapperFastCornerIntensity<>(new FastCornerHip<>(20, 9, GrayU8.class)), extractor)
 *  Deviations (include/boofhip.h): a negative pixelTol is refused; the intensity image is written as a whole -- 0 in the 3-pixel border and in the
 *  rows after an early stop, where the Java detector leaves what an earlier frame put there.  UNCOMPILED SOURCE. */
public class FastCornerHip<T extends ImageGray<T>> extends FastCornerDetector<T> {
	private final float pixelTol;
	private final int minContinuous;
	private final Class<T> imageType;
	private short[] low = new short[0], high = new short[0];
	private final int[] nLow = new int[1], nHigh = new int[1];

	public FastCornerHip(float pixelTol, int minContinuous, Class<T> imageType) {
		super(null);   // the helper is never consulted: both process() forms are overridden
		if (imageType != GrayU8.class && imageType != GrayF32.class) throw new IllegalArgumentException("Unknown image type");
		if (minContinuous < 9 || minContinuous > 12) throw new IllegalArgumentException("Specified minCont is not supported");
		this.pixelTol = pixelTol;
		this.minContinuous = minContinuous;
		this.imageType = imageType;
	}

	@Override public void process(T image, GrayF32 intensity) { run(image, intensity); }

	@Override public void process(T image) { run(image, null); }

	private void run(T image, GrayF32 intensity) {
		final long ctx = BoofHipContext.get();
		final int w = image.width, h = image.height;
		// the detector stops after the row that reaches the limit, so a list is never longer than the limit plus that row
		final int cap = Math.max(1, Math.min(Math.max(w - 6, 0)*Math.max(h - 6, 0), (int)(maxFeaturesFraction*w*h) + w));
		if (low.length < 2*cap) { low = new short[2*cap]; high = new short[2*cap]; }
		final float[] inten = intensity != null ? intensity.data : null;
		final int iStart = intensity != null ? intensity.startIndex : 0, iStride = intensity != null ? intensity.stride : 0;
		if (imageType == GrayU8.class) {
			GrayU8 in = (GrayU8)image;
			BoofHip.check(ctx, BoofHip.fastU8(ctx, in.data, in.startIndex, in.stride, w, h, (int)pixelTol, minContinuous, maxFeaturesFraction, inten, iStart, iStride,
					low, nLow, high, nHigh, cap));
		} else {
			GrayF32 in = (GrayF32)image;
			BoofHip.check(ctx, BoofHip.fastF32(ctx, in.data, in.startIndex, in.stride, w, h, pixelTol, minContinuous, maxFeaturesFraction, inten, iStart, iStride,
					low, nLow, high, nHigh, cap));
		}
		fill(getCornersLow(), low, nLow[0]);
		fill(getCornersHigh(), high, nHigh[0]);
	}

	private static void fill(QueueCorner list, short[] xy, int n) {
		list.reset();
		for (int i = 0; i < n; i++) list.add(xy[2*i], xy[2*i + 1]);
	}
}
