package boofcv.hip;

import boofcv.abst.filter.FilterImageInterface;
import boofcv.struct.image.GrayS32;
import boofcv.struct.image.GrayS64;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageBase;
import boofcv.struct.image.ImageType;
import georegression.struct.point.Point2D_I32;
import org.ddogleg.struct.FastQueue;

/** FilterCensusTransformD33U8 / D55S32 / SampleS64 (main/boofcv-ip/.../abst/transform/census/) on GrayU8 inputs with the factory's border,
 *  CENSUS_BORDER = REFLECT, with process() on the device: bhip_census_u8_u8 (GrayU8 words), bhip_census_u8_s32 (GrayS32) and
 *  bhip_census_sample_u8_s64 (GrayS64, any list of at most 64 samples with offsets within -7 .. 7).  Built by FactoryCensusTransformHip.
 *  Results are bit for bit those of the Java classes, the `int bit` of sample_S64 included (a GrayS64 word is the sign extension of its low
 *  32 bits; include/boofhip.h).  Deviations: an image smaller than radius + 1 in either direction is refused (IllegalArgumentException), where
 *  the Java code throws or writes outside the image; offsets beyond 7 make check() throw RuntimeException and the caller uses the Java path.
 *  UNCOMPILED SOURCE. */
public class FilterCensusTransformHip<Out extends ImageBase<Out>> implements FilterImageInterface<GrayU8, Out> {
	private final Class<Out> outType;
	private final int[] samplesXY;   // GrayS64 only: (x, y) pairs

	FilterCensusTransformHip(Class<Out> outType, FastQueue<Point2D_I32> samples) {
		if (samples != null && samples.size > 64) throw new IllegalArgumentException("At most 64 sample points for now. size = " + samples.size);
		this.outType = outType;
		if (samples == null) {
			samplesXY = null;
		} else {
			samplesXY = new int[2*samples.size];
			for (int i = 0; i < samples.size; i++) {
				samplesXY[2*i] = samples.get(i).x;
				samplesXY[2*i + 1] = samples.get(i).y;
			}
		}
	}

	@Override public void process(GrayU8 in, Out out) {
		out.reshape(in.width, in.height);
		final long ctx = BoofHipContext.get();
		if (outType == (Class)GrayU8.class) {
			GrayU8 o = (GrayU8)(ImageBase)out;
			BoofHip.check(ctx, BoofHip.censusU8U8(ctx, in.data, in.startIndex, in.stride, in.width, in.height, o.data, o.startIndex, o.stride));
		} else if (outType == (Class)GrayS32.class) {
			GrayS32 o = (GrayS32)(ImageBase)out;
			BoofHip.check(ctx, BoofHip.censusU8S32(ctx, in.data, in.startIndex, in.stride, in.width, in.height, o.data, o.startIndex, o.stride));
		} else {
			GrayS64 o = (GrayS64)(ImageBase)out;
			BoofHip.check(ctx, BoofHip.censusSampleU8S64(ctx, samplesXY, samplesXY.length/2, in.data, in.startIndex, in.stride, in.width, in.height,
					o.data, o.startIndex, o.stride));
		}
	}

	@Override public int getHorizontalBorder() { return 0; }
	@Override public int getVerticalBorder() { return 0; }
	@Override public ImageType<GrayU8> getInputType() { return ImageType.single(GrayU8.class); }
	@Override public ImageType<Out> getOutputType() { return ImageType.single((Class)outType); }
}
