package boofcv.hip;

import javax.annotation.Nullable;

import boofcv.abst.feature.dense.DescribeImageDense;
import boofcv.factory.feature.dense.ConfigDenseHoG;
import boofcv.factory.feature.dense.ConfigDenseSift;
import boofcv.struct.feature.TupleDesc_F64;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;
import boofcv.struct.image.ImageType;

/** Same signatures as FactoryDescribeImageDense (main/boofcv-feature/.../factory/feature/dense/FactoryDescribeImageDense.java) for what the
 *  library implements, returning the same interface type, backed by libboofhip.so: hog (:136-165, both variants) and sift (:108-123) on
 *  single-band GrayF32 and GrayU8.  Not here, and the caller keeps the Java path: surfFast / surfStable (GenericDenseDescribeImageDense describes
 *  every grid point through DescribeRegionPoint at a fixed orientation and scale, an entry the SURF kernels do not have) and Planar / interleaved
 *  HOG (the MAX_F reduction of the bands' gradients).
 *  UNCOMPILED SOURCE (no JDK in the build image). */
public class FactoryDescribeImageDenseHip {
	private static void checkGray(Class<?> imageType) {
		if (imageType != GrayF32.class && imageType != GrayU8.class)
			throw new IllegalArgumentException("Image type not supported");
	}

	public static <T extends ImageGray<T>> DescribeImageDense<T, TupleDesc_F64>
	sift(@Nullable ConfigDenseSift config, Class<T> imageType) {
		checkGray(imageType);
		if (config == null) config = new ConfigDenseSift();
		return new DescribeImageDenseHip<>(config, imageType);
	}

	/** hog(config, imageType) (:136-165) for ImageType.single(GrayF32.class | GrayU8.class) */
	public static <T extends ImageGray<T>> DescribeImageDense<T, TupleDesc_F64>
	hog(@Nullable ConfigDenseHoG config, ImageType<T> imageType) {
		if (imageType.getFamily() != ImageType.Family.GRAY) throw new IllegalArgumentException("Image type not supported");
		checkGray(imageType.getImageClass());
		if (config == null) config = new ConfigDenseHoG();
		config.checkValidity();
		return new DescribeImageDenseHip<>(config, imageType.getImageClass());
	}
}
