package boofcv.hip;

import boofcv.abst.feature.detect.extract.ConfigExtract;
import boofcv.abst.feature.detect.interest.ConfigSiftDetector;
import boofcv.abst.feature.detect.interest.InterestPointDetector;
import boofcv.abst.feature.describe.ConfigSiftScaleSpace;
import boofcv.struct.feature.ScalePoint;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;
import boofcv.struct.image.ImageType;
import georegression.struct.point.Point2D_F64;
import org.ddogleg.struct.FastQueue;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

/** InterestPointDetector&lt;GrayF32 | GrayU8&gt; as FactoryInterestPoint.sift(configSS, configDet, imageType) builds it
 *  (main/boofcv-feature/.../factory/feature/detect/interest/FactoryInterestPoint.java:133-148: WrapSiftDetector over SiftDetector, SiftScaleSpace and
 *  NonMaxLimiter), with detect() on the device: bhip_sift_detect_f32 / bhip_sift_detect_u8 -- the scale space, the strict min / max block
 *  non-maximum suppression of every DoG image, the 3x3x3 test, the edge test and the sub-pixel fit.  Built by FactoryInterestPointHip.sift.
 *  Detections are bit for bit those of the single-threaded Java classes, in their order; where[4*i ..] records the octave, the DoG index and the
 *  pixel of detection i.  Math.pow is the C library's pow there; with maxFeaturesPerScale &gt; 0 the order QuickSelect leaves is the restated
 *  routine's.  The constructor throws what SiftScaleSpace's and SiftDetector's throw; limits (include/boofhip.h: octave images up to 32767 a
 *  side, blur kernels up to 255 taps, the strict extractor) make check() throw RuntimeException and the caller uses the Java path.
 *  Orientation and description stay Java.  UNCOMPILED SOURCE. */
public class SiftDetectorHip<T extends ImageGray<T>> implements InterestPointDetector<T> {
	private final Class<T> inputType;
	private final ByteBuffer cfg;
	private final FastQueue<ScalePoint> detections = new FastQueue<>(ScalePoint.class, true);
	private double[] x = new double[4096], y = new double[4096], scale = new double[4096];
	private byte[] white = new byte[4096];
	private short[] where = new short[4*4096];
	private final int[] count = new int[1];

	/** bhip_sift_cfg: int firstOctave @0, lastOctave @4, numScales @8, double sigma0 @16, int extractRadius @24, float extractThreshold @28,
	 *  int extractIgnoreBorder @32, extractUseStrictRule @36, extractDetectMin @40, extractDetectMax @44, maxFeaturesPerScale @48, double edgeR @56;
	 *  64 bytes */
	SiftDetectorHip(ConfigSiftScaleSpace ss, ConfigSiftDetector det, Class<T> inputType) {
		if (ss.lastOctave <= ss.firstOctave) throw new IllegalArgumentException("Last octave must be more than the first octave");
		if (ss.numScales < 1) throw new IllegalArgumentException("Number of scales must be >= 1");
		ConfigExtract e = det.extract;
		e.checkValidity();
		if (!e.detectMaximums || !e.detectMinimums) throw new IllegalArgumentException("The extractor must be able to detect maximums and minimums");
		if (det.edgeR < 1) throw new IllegalArgumentException("R must be >= 1");
		if (e.ignoreBorder != 1) throw new RuntimeException("Non-max should have an ignore border of 1");
		this.inputType = inputType;
		cfg = ByteBuffer.allocateDirect(64).order(ByteOrder.nativeOrder());
		cfg.putInt(0, ss.firstOctave).putInt(4, ss.lastOctave).putInt(8, ss.numScales).putDouble(16, ss.sigma0);
		cfg.putInt(24, e.radius).putFloat(28, e.threshold).putInt(32, e.ignoreBorder).putInt(36, e.useStrictRule ? 1 : 0);
		cfg.putInt(40, e.detectMinimums ? 1 : 0).putInt(44, e.detectMaximums ? 1 : 0).putInt(48, Math.max(det.maxFeaturesPerScale, 0)).putDouble(56, det.edgeR);
	}

	@Override public void detect(T image) {
		final long ctx = BoofHipContext.get();
		for (;;) {
			final int cap = x.length;
			if (inputType == GrayF32.class) {
				GrayF32 in = (GrayF32)image;
				BoofHip.check(ctx, BoofHip.siftDetectF32(ctx, cfg, in.data, in.startIndex, in.stride, in.width, in.height, x, y, scale, white, where, count, cap));
			} else {
				GrayU8 in = (GrayU8)image;
				BoofHip.check(ctx, BoofHip.siftDetectU8(ctx, cfg, in.data, in.startIndex, in.stride, in.width, in.height, x, y, scale, white, where, count, cap));
			}
			if (count[0] <= cap) break;
			// the list did not fit: once more with room for all of it
			x = new double[count[0]]; y = new double[count[0]]; scale = new double[count[0]]; white = new byte[count[0]]; where = new short[4*count[0]];
		}
		detections.reset();
		for (int i = 0; i < count[0]; i++) {
			ScalePoint p = detections.grow();
			p.x = x[i]; p.y = y[i]; p.scale = scale[i]; p.white = white[i] != 0;
		}
	}

	public FastQueue<ScalePoint> getDetections() { return detections; }
	/** octave, DoG index, pixel x, pixel y of detection i at where[4*i .. 4*i+3] */
	public short[] getWhere() { return where; }

	@Override public int getNumberOfFeatures() { return detections.size(); }
	@Override public Point2D_F64 getLocation(int featureIndex) { return detections.get(featureIndex); }
	@Override public double getRadius(int featureIndex) { return detections.get(featureIndex).scale; }
	@Override public double getOrientation(int featureIndex) { return 0; }
	@Override public boolean hasScale() { return true; }
	@Override public boolean hasOrientation() { return false; }
	public ImageType<T> getInputType() { return ImageType.single(inputType); }
}
