package boofcv.hip;

import boofcv.abst.feature.describe.ConfigSiftDescribe;
import boofcv.abst.feature.dense.DescribeImageDense;
import boofcv.factory.feature.dense.ConfigDenseHoG;
import boofcv.factory.feature.dense.ConfigDenseSift;
import boofcv.struct.feature.TupleDesc_F64;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;
import boofcv.struct.image.ImageType;
import georegression.struct.point.Point2D_I32;
import org.ddogleg.struct.FastQueue;

import java.util.List;

/** DescribeImageDense&lt;GrayF32 | GrayU8, TupleDesc_F64&gt; as FactoryDescribeImageDense.hog(config, imageType) and .sift(config, imageType) build it
 *  (main/boofcv-feature/.../factory/feature/dense/FactoryDescribeImageDense.java:108-165: DescribeImageDenseHoG over DescribeDenseHogFastAlg /
 *  DescribeDenseHogAlg, behind DescribeImageDense_Convert for GrayU8; DescribeImageDenseSift over DescribeDenseSiftAlg), with process() on the
 *  device: bhip_dense_hog_f32 / _u8 and bhip_dense_sift_f32 / _u8.  Built by FactoryDescribeImageDenseHip.  Counts, locations and their order are
 *  those of the single-threaded Java classes; HOG descriptors equal theirs wherever Math.atan narrows to the same float, dense SIFT descriptors
 *  to the last ulp of Math.atan2 (include/boofhip.h, the bhip_dense_* section).  getLocations() are the centres of the regions, as the
 *  interface asks: the library reports a HOG block's top-left pixel and half the region is added here, as DescribeImageDenseHoG.process does.
 *  Limits there (descriptors up to 2048 elements, up to 64 bins, cells up to 32 pixels, SIFT windows up to 48 samples) make check() throw
 *  RuntimeException and the caller uses the Java path.
 *  UNCOMPILED SOURCE. */
public class DescribeImageDenseHip<T extends ImageGray<T>> implements DescribeImageDense<T, TupleDesc_F64> {
	private final Class<T> inputType;
	private final boolean sift;
	// HOG: orientationBins, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, stepBlock, fastVariant; SIFT: widthSubregion, widthGrid, numHistogramBins
	private final int[] a;
	private final double weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY;
	private final int dof, offX, offY;
	private final FastQueue<Point2D_I32> locations = new FastQueue<>(Point2D_I32.class, true);
	private final FastQueue<TupleDesc_F64> descriptions;
	private double[] descriptors = new double[0];
	private int[] xy = new int[0];
	private final int[] count = new int[1], out = new int[1];

	DescribeImageDenseHip(ConfigDenseHoG c, Class<T> inputType) {
		if (c.stepBlock <= 0) throw new IllegalArgumentException("stepBlock must be >= 1");
		this.inputType = inputType;
		sift = false;
		a = new int[]{c.orientationBins, c.pixelsPerCell, c.cellsPerBlockX, c.cellsPerBlockY, c.stepBlock, c.fastVariant ? 1 : 0};
		weightingSigmaFraction = maxDescriptorElementValue = periodX = periodY = 0;
		final int s = BoofHip.denseHogLayout(a[0], a[1], a[2], a[3], a[4], a[5], 1, 1, null, null, out, null, 0);
		if (s < 0) throw new RuntimeException("this dense HOG config does not run on the GPU (status " + s + ")");
		dof = out[0];
		offX = c.pixelsPerCell*c.cellsPerBlockX/2;
		offY = c.pixelsPerCell*c.cellsPerBlockY/2;
		descriptions = queue();
	}

	DescribeImageDenseHip(ConfigDenseSift c, Class<T> inputType) {
		c.checkValidity();
		this.inputType = inputType;
		sift = true;
		ConfigSiftDescribe d = c.sift;
		a = new int[]{d.widthSubregion, d.widthGrid, d.numHistogramBins};
		weightingSigmaFraction = d.weightingSigmaFraction;
		maxDescriptorElementValue = d.maxDescriptorElementValue;
		periodX = c.sampling.periodX;
		periodY = c.sampling.periodY;
		// the config's own checks, on a frame and periods that pass theirs
		final int s = BoofHip.denseSiftLayout(a[0], a[1], a[2], 1.0, 1.0, 1024, 1024, null, null, out, null, 0);
		if (s < 0) throw new RuntimeException("this dense SIFT config does not run on the GPU (status " + s + ")");
		dof = out[0];
		offX = offY = 0;
		descriptions = queue();
	}

	private FastQueue<TupleDesc_F64> queue() {
		return new FastQueue<TupleDesc_F64>(TupleDesc_F64.class, true) {
			@Override protected TupleDesc_F64 createInstance() { return new TupleDesc_F64(dof); }
		};
	}

	@Override public void process(T input) {
		final long ctx = BoofHipContext.get();
		// the grid of a frame depends on its size alone: the host function sizes the arrays
		final int n = sift ? BoofHip.denseSiftLayout(a[0], a[1], a[2], periodX, periodY, input.width, input.height, null, null, null, null, 0)
				: BoofHip.denseHogLayout(a[0], a[1], a[2], a[3], a[4], a[5], input.width, input.height, null, null, null, null, 0);
		if (n == -1) throw new IllegalArgumentException("no dense descriptors for this frame size (the reference throws too)");   // BHIP_ERR_INVALID
		if (n < 0) throw new RuntimeException("this frame size does not run on the GPU (status " + n + ")");
		if (descriptors.length < n*dof) { descriptors = new double[n*dof]; xy = new int[2*n]; }
		if (inputType == GrayF32.class) {
			GrayF32 in = (GrayF32)(ImageGray)input;
			BoofHip.check(ctx, sift ? BoofHip.denseSiftF32(ctx, a[0], a[1], a[2], weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY, in.data, in.startIndex,
					in.stride, in.width, in.height, descriptors, xy, count, n)
					: BoofHip.denseHogF32(ctx, a[0], a[1], a[2], a[3], a[4], a[5], in.data, in.startIndex, in.stride, in.width, in.height, descriptors, xy, count, n, null));
		} else {
			GrayU8 in = (GrayU8)(ImageGray)input;
			BoofHip.check(ctx, sift ? BoofHip.denseSiftU8(ctx, a[0], a[1], a[2], weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY, in.data, in.startIndex,
					in.stride, in.width, in.height, descriptors, xy, count, n)
					: BoofHip.denseHogU8(ctx, a[0], a[1], a[2], a[3], a[4], a[5], in.data, in.startIndex, in.stride, in.width, in.height, descriptors, xy, count, n, null));
		}
		locations.reset();
		descriptions.reset();
		for (int i = 0; i < n; i++) {
			locations.grow().set(xy[2*i] + offX, xy[2*i + 1] + offY);
			System.arraycopy(descriptors, i*dof, descriptions.grow().value, 0, dof);
		}
	}

	@Override public List<TupleDesc_F64> getDescriptions() { return descriptions.toList(); }
	@Override public List<Point2D_I32> getLocations() { return locations.toList(); }
	@Override public ImageType<T> getImageType() { return ImageType.single(inputType); }
	@Override public TupleDesc_F64 createDescription() { return new TupleDesc_F64(dof); }
	@Override public Class<TupleDesc_F64> getDescriptionType() { return TupleDesc_F64.class; }
}
