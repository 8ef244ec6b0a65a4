package boofcv.hip;

import boofcv.abst.flow.DenseOpticalFlow;
import boofcv.alg.tracker.klt.PkltConfig;
import boofcv.factory.flow.ConfigHornSchunck;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayS16;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;

/** FactoryDenseOpticalFlow.flowKlt (main/boofcv-feature/.../factory/flow/FactoryDenseOpticalFlow.java:61-82) with the whole algorithm on the device.
 *  The reference has no hook for this factory, so the class is used where FactoryDenseOpticalFlow would be called:
 *      DenseOpticalFlow&lt;GrayF32&gt; alg = FactoryDenseOpticalFlowHip.flowKlt(null, 3, GrayF32.class, null);
 *  configKlt == null is new PkltConfig(), derivType == null the default derivative type; radius is the template radius and the neighbourhood
 *  radius (configKlt.templateRadius is not read, as in the reference).  GrayF32 with GrayF32 derivatives and GrayU8 with GrayS16 derivatives run
 *  on the device; every other pair throws RuntimeException: use the Java path.
 *  FactoryDenseOpticalFlow.hornSchunck (:122-138) likewise: config == null is new ConfigHornSchunck(); GrayF32 and GrayU8 run on the device.
 *  region (a serial best-match search with order-dependent ties), hornSchunckPyramid and broxWarping (in-place successive over-relaxation,
 *  whose results depend on raster order) have no device form: use the Java path.  UNCOMPILED SOURCE. */
public class FactoryDenseOpticalFlowHip {
	public static <I extends ImageGray<I>, D extends ImageGray<D>>
	DenseOpticalFlow<I> flowKlt(PkltConfig configKlt, int radius, Class<I> inputType, Class<D> derivType) {
		if (configKlt == null) configKlt = new PkltConfig();
		boolean f32 = inputType == GrayF32.class && (derivType == null || derivType == GrayF32.class);
		boolean u8 = inputType == GrayU8.class && (derivType == null || derivType == GrayS16.class);
		if (!f32 && !u8) throw new RuntimeException("only GrayF32 / GrayF32 and GrayU8 / GrayS16 run on the device (use the Java path)");
		return new DenseOpticalFlowKltHip<>(configKlt, radius, inputType);
	}

	public static <T extends ImageGray<T>>
	DenseOpticalFlow<T> hornSchunck(ConfigHornSchunck config, Class<T> imageType) {
		if (config == null) config = new ConfigHornSchunck();
		if (imageType != GrayF32.class && imageType != GrayU8.class) throw new RuntimeException("only GrayF32 and GrayU8 run on the device (use the Java path)");
		return new DenseOpticalFlowHornSchunckHip<>(config, imageType);
	}
}
