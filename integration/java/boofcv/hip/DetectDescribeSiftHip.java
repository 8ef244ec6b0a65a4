package boofcv.hip;

import boofcv.abst.feature.describe.ConfigSiftDescribe;
import boofcv.abst.feature.describe.ConfigSiftScaleSpace;
import boofcv.abst.feature.detdesc.ConfigCompleteSift;
import boofcv.abst.feature.detdesc.DetectDescribePoint;
import boofcv.abst.feature.detect.extract.ConfigExtract;
import boofcv.abst.feature.detect.interest.ConfigSiftDetector;
import boofcv.abst.feature.orientation.ConfigSiftOrientation;
import boofcv.struct.feature.BrightFeature;
import boofcv.struct.feature.ScalePoint;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;
import georegression.struct.point.Point2D_F64;
import org.ddogleg.struct.FastQueue;
import org.ddogleg.struct.GrowQueue_F64;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

/** DetectDescribePoint&lt;GrayF32 | GrayU8, BrightFeature&gt; as FactoryDetectDescribe.sift(config) builds it
 *  (main/boofcv-feature/.../factory/feature/detdesc/FactoryDetectDescribe.java:72-96: DetectDescribe_CompleteSift over CompleteSift,
 *  OrientationHistogramSift and DescribePointSift), with detect() on the device: bhip_csift_f32 / bhip_csift_u8.  Built by
 *  FactoryDetectDescribeHip.sift.  The number of angles of every detection -- hence the count and the order of features -- and every
 *  ScalePoint and white flag are those of the single-threaded Java classes; angles and descriptor elements differ from theirs by the last ulp
 *  of atan2 / sin / cos alone (include/boofhip.h, bhip_csift_cfg).  Limits there (histogramSize up to 256, sample grids up to 48 wide,
 *  descriptors up to 2048 elements, and the detector's) make check() throw RuntimeException and the caller uses the Java path.
 *  UNCOMPILED SOURCE. */
public class DetectDescribeSiftHip<T extends ImageGray<T>> implements DetectDescribePoint<T, BrightFeature> {
	private final Class<T> inputType;
	private final ByteBuffer cfg, desc;
	private final int dof;
	private final FastQueue<ScalePoint> locations = new FastQueue<>(ScalePoint.class, true);
	private final FastQueue<BrightFeature> features;
	private final GrowQueue_F64 orientations = new GrowQueue_F64();
	private double[] x = new double[4096], y = new double[4096], scale = new double[4096], orientation = new double[4096], descriptors;
	private byte[] white = new byte[4096];
	private final int[] count = new int[1];

	/** bhip_sift_cfg as in SiftDetectorHip; bhip_csift_cfg: int histogramSize @0, double sigmaEnlarge @8, int widthSubregion @16, widthGrid @20,
	 *  numHistogramBins @24, double sigmaToPixels @32, weightingSigmaFraction @40, maxDescriptorElementValue @48; 56 bytes */
	DetectDescribeSiftHip(ConfigCompleteSift config, Class<T> inputType) {
		ConfigSiftScaleSpace ss = config.scaleSpace;
		ConfigSiftDetector det = config.detector;
		ConfigSiftOrientation ori = config.orientation;
		ConfigSiftDescribe de = config.describe;
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
		desc = ByteBuffer.allocateDirect(56).order(ByteOrder.nativeOrder());
		desc.putInt(0, ori.histogramSize).putDouble(8, ori.sigmaEnlarge);
		desc.putInt(16, de.widthSubregion).putInt(20, de.widthGrid).putInt(24, de.numHistogramBins);
		desc.putDouble(32, de.sigmaToPixels).putDouble(40, de.weightingSigmaFraction).putDouble(48, de.maxDescriptorElementValue);
		final int n = BoofHip.csiftDof(desc);
		if (n < 0) throw new RuntimeException("this SIFT orientation / describe config does not run on the GPU (status " + n + ")");
		dof = n;
		descriptors = new double[4096*dof];
		features = new FastQueue<BrightFeature>(BrightFeature.class, true) {
			@Override protected BrightFeature createInstance() { return new BrightFeature(dof); }
		};
	}

	@Override public void detect(T image) {
		final long ctx = BoofHipContext.get();
		for (;;) {
			final int cap = x.length;
			if (inputType == GrayF32.class) {
				GrayF32 in = (GrayF32)image;
				BoofHip.check(ctx, BoofHip.csiftF32(ctx, cfg, desc, in.data, in.startIndex, in.stride, in.width, in.height, x, y, scale, orientation, white, descriptors, count, cap));
			} else {
				GrayU8 in = (GrayU8)image;
				BoofHip.check(ctx, BoofHip.csiftU8(ctx, cfg, desc, in.data, in.startIndex, in.stride, in.width, in.height, x, y, scale, orientation, white, descriptors, count, cap));
			}
			if (count[0] <= cap) break;
			// the list did not fit: once more with room for all of it
			final int n = count[0];
			x = new double[n]; y = new double[n]; scale = new double[n]; orientation = new double[n]; white = new byte[n]; descriptors = new double[n*dof];
		}
		locations.reset();
		features.reset();
		orientations.reset();
		for (int i = 0; i < count[0]; i++) {
			ScalePoint p = locations.grow();
			p.x = x[i]; p.y = y[i]; p.scale = scale[i]; p.white = white[i] != 0;
			BrightFeature f = features.grow();
			f.white = p.white;
			System.arraycopy(descriptors, i*dof, f.value, 0, dof);
			orientations.add(orientation[i]);
		}
	}

	public FastQueue<ScalePoint> getLocations() { return locations; }
	public FastQueue<BrightFeature> getDescriptions() { return features; }
	public GrowQueue_F64 getOrientations() { return orientations; }
	public int getDescriptorLength() { return dof; }

	@Override public BrightFeature createDescription() { return new BrightFeature(dof); }
	@Override public BrightFeature getDescription(int index) { return features.get(index); }
	@Override public Class<BrightFeature> getDescriptionType() { return BrightFeature.class; }
	@Override public int getNumberOfFeatures() { return features.size(); }
	@Override public Point2D_F64 getLocation(int featureIndex) { return locations.get(featureIndex); }
	@Override public double getRadius(int featureIndex) { return locations.get(featureIndex).scale; }
	@Override public double getOrientation(int featureIndex) { return orientations.get(featureIndex); }
	@Override public boolean hasScale() { return true; }
	@Override public boolean hasOrientation() { return true; }
}
