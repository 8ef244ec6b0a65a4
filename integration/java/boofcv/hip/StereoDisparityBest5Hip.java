package boofcv.hip;

import boofcv.abst.feature.disparity.StereoDisparity;
import boofcv.factory.feature.disparity.ConfigDisparityBMBest5;
import boofcv.factory.feature.disparity.DisparityError;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;
import boofcv.struct.image.ImageType;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

/** StereoDisparity&lt;GrayU8, GrayU8 | GrayF32&gt; as FactoryStereoDisparity.blockMatchBest5(ConfigDisparityBMBest5, GrayU8.class, dispType) builds it
 *  for errorType = SAD and errorType = CENSUS (main/boofcv-feature/.../factory/feature/disparity/FactoryStereoDisparity.java:146-201;
 *  DisparityScoreBMBestFive_S32 under WrapDisparityBlockMatchRowFormat / WrapDisparityBlockMatchCensus), with process() on the device:
 *  bhip_disparity_bm5_u8_u8 / _u8_f32 (SAD) and bhip_disparity_bm5_census_u8_u8 / _u8_f32 (CENSUS, config.configCensus.variant).  The reference
 *  has no hook for this factory, so the class is constructed where FactoryStereoDisparity.blockMatchBest5 would be called:
 *      StereoDisparity&lt;GrayU8, GrayF32&gt; alg = StereoDisparityBest5Hip.blockMatchBest5(config, GrayF32.class);
 *  Results are bit for bit those of the single-threaded Java classes (BoofConcurrency.USE_CONCURRENT = false) on a freshly constructed object:
 *  the disparity image is written as a whole by every process(), rangeDisparity where the Java code writes nothing -- the border of
 *  2 * regionRadius, and row 0 when regionRadiusY is 0, which DisparityScoreBMBestFive_S32 never selects.  An image lower than a sub-block is
 *  refused.  Limits: regionRadiusX / Y &lt;= 7, rangeDisparity &lt;= 256; beyond them, and for a census image smaller than the transform's
 *  radius + 1, check() throws RuntimeException and the caller uses the Java path, as for NCC and the other input types, which blockMatchBest5()
 *  here refuses.  The census images of getCLeft / getCRight are not kept: use FilterCensusTransformHip on the input.
 *  UNCOMPILED SOURCE. */
public class StereoDisparityBest5Hip<DI extends ImageGray<DI>> implements StereoDisparity<GrayU8, DI> {
	private final ConfigDisparityBMBest5 config;
	private final Class<DI> dispType;
	private final int variant;      // CensusVariants ordinal = bhip_census_variant; -1: errorType = SAD
	private final ByteBuffer cfg;   // bhip_disparity_bm_cfg: int[4], double, int, (pad), double
	private DI disparity;

	/** the checks of FactoryStereoDisparity.blockMatchBest5 and of the DisparityBlockMatchRowFormat constructor */
	public static <DI extends ImageGray<DI>> StereoDisparityBest5Hip<DI> blockMatchBest5(ConfigDisparityBMBest5 config, Class<DI> dispType) {
		if (config == null) config = new ConfigDisparityBMBest5();
		if (config.subpixel) {
			if (dispType != GrayF32.class) throw new IllegalArgumentException("With subpixel on, disparity image must be GrayF32");
		} else {
			if (dispType != GrayU8.class) throw new IllegalArgumentException("With subpixel on, disparity image must be GrayU8");
		}
		int variant = -1;
		if (config.errorType == DisparityError.CENSUS) variant = config.configCensus.variant.ordinal();
		else if (config.errorType != DisparityError.SAD) throw new RuntimeException("only errorType = SAD and CENSUS run on the device");
		int maxDisparity = config.minDisparity + config.rangeDisparity;
		if (maxDisparity <= 0) throw new IllegalArgumentException("Max disparity must be greater than zero. max=" + maxDisparity);
		if (config.minDisparity < 0 || config.minDisparity >= maxDisparity)
			throw new IllegalArgumentException("Min disparity must be >= 0 and < maxDisparity. min=" + config.minDisparity + " max=" + maxDisparity);
		return new StereoDisparityBest5Hip<>(config, dispType, variant);
	}

	private StereoDisparityBest5Hip(ConfigDisparityBMBest5 config, Class<DI> dispType, int variant) {
		this.config = config;
		this.dispType = dispType;
		this.variant = variant;
		cfg = ByteBuffer.allocateDirect(48).order(ByteOrder.nativeOrder());
		cfg.putInt(0, config.minDisparity).putInt(4, config.rangeDisparity).putInt(8, config.regionRadiusX).putInt(12, config.regionRadiusY);
		cfg.putDouble(16, config.maxPerPixelError).putInt(24, config.validateRtoL).putDouble(32, config.texture);
	}

	@SuppressWarnings("unchecked")
	@Override public void process(GrayU8 left, GrayU8 right) {
		if (left.width != right.width || left.height != right.height) throw new IllegalArgumentException("Image shapes do not match");
		final int w = left.width, h = left.height;
		if (config.minDisparity + config.rangeDisparity > w - 2*config.regionRadiusX)   // DisparityBlockMatchRowFormat.process: radiusX, not 2*radiusX
			throw new RuntimeException("The maximum disparity is too large for this image size: max size " + (w - 2*config.regionRadiusX));
		if (disparity == null || disparity.width != w || disparity.height != h)
			disparity = dispType == GrayF32.class ? (DI)new GrayF32(w, h) : (DI)new GrayU8(w, h);
		final long ctx = BoofHipContext.get();
		final int status;
		if (dispType == GrayF32.class) {
			GrayF32 d = (GrayF32)disparity;
			status = variant < 0
					? BoofHip.disparityBm5U8F32(ctx, cfg, left.data, left.startIndex, left.stride, right.data, right.startIndex, right.stride, w, h,
							d.data, d.startIndex, d.stride)
					: BoofHip.disparityBm5CensusU8F32(ctx, cfg, variant, left.data, left.startIndex, left.stride, right.data, right.startIndex, right.stride, w, h,
							d.data, d.startIndex, d.stride);
		} else {
			GrayU8 d = (GrayU8)disparity;
			status = variant < 0
					? BoofHip.disparityBm5U8U8(ctx, cfg, left.data, left.startIndex, left.stride, right.data, right.startIndex, right.stride, w, h,
							d.data, d.startIndex, d.stride)
					: BoofHip.disparityBm5CensusU8U8(ctx, cfg, variant, left.data, left.startIndex, left.stride, right.data, right.startIndex, right.stride, w, h,
							d.data, d.startIndex, d.stride);
		}
		BoofHip.check(ctx, status);   // throws for what the device refuses: the caller uses the Java path
	}

	@Override public DI getDisparity() { return disparity; }
	@Override public int getMinDisparity() { return config.minDisparity; }
	@Override public int getRangeDisparity() { return config.rangeDisparity; }
	@Override public int getInvalidValue() { return config.rangeDisparity; }
	@Override public int getBorderX() { return 2*config.regionRadiusX; }   // DisparityBlockMatchBestFive.getBorderX
	@Override public int getBorderY() { return 2*config.regionRadiusY; }
	@Override public ImageType<GrayU8> getInputType() { return ImageType.single(GrayU8.class); }
	@Override public Class<DI> getDisparityType() { return dispType; }
}
