package boofcv.hip;

import boofcv.abst.filter.FilterImageInterface;
import boofcv.alg.transform.census.CensusTransform;
import boofcv.factory.transform.census.CensusVariants;
import boofcv.struct.image.GrayS32;
import boofcv.struct.image.GrayS64;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageBase;

/** FactoryCensusTransform.variant / blockDense (main/boofcv-ip/.../factory/transform/census/FactoryCensusTransform.java:48-93) for GrayU8 inputs,
 *  returning filters that run on the device (FilterCensusTransformHip).  The reference has no hook for this factory, so the class is called
 *  where FactoryCensusTransform would be:
 *      FilterImageInterface&lt;GrayU8, GrayS32&gt; census = FactoryCensusTransformHip.variant(CensusVariants.BLOCK_5_5);
 *  The sample lists are the reference's own (CensusTransform.createBlockSamples / createCircleSamples); the same exceptions are thrown.
 *  GrayU16 inputs stay on the Java path.
 *  UNCOMPILED SOURCE. */
public class FactoryCensusTransformHip {
	public static <Out extends ImageBase<Out>> FilterImageInterface<GrayU8, Out> variant(CensusVariants type) {
		switch (type) {
			case BLOCK_3_3: return blockDense(1);
			case BLOCK_5_5: return blockDense(2);
			case BLOCK_7_7: return blockDense(3);
			case BLOCK_9_7: return blockDense(4, 3);
			case BLOCK_13_5: return blockDense(5, 2);
			case CIRCLE_9: return new FilterCensusTransformHip(GrayS64.class, CensusTransform.createCircleSamples());
			default: throw new IllegalArgumentException("Unknown type " + type);
		}
	}

	public static <Out extends ImageBase<Out>> FilterImageInterface<GrayU8, Out> blockDense(int radius) {
		switch (radius) {
			case 1: return new FilterCensusTransformHip(GrayU8.class, null);
			case 2: return new FilterCensusTransformHip(GrayS32.class, null);
			case 3: return new FilterCensusTransformHip(GrayS64.class, CensusTransform.createBlockSamples(3));
			default: throw new IllegalArgumentException("Currently only radius 1 to 3 is supported");
		}
	}

	public static <Out extends ImageBase<Out>> FilterImageInterface<GrayU8, Out> blockDense(int radiusX, int radiusY) {
		return new FilterCensusTransformHip(GrayS64.class, CensusTransform.createBlockSamples(radiusX, radiusY));
	}
}
