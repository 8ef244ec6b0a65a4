package boofcv.hip;

import boofcv.abst.feature.disparity.StereoDisparity;
import boofcv.factory.feature.disparity.ConfigDisparityBM;
import boofcv.factory.feature.disparity.DisparityError;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;
import boofcv.struct.image.ImageType;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

/** StereoDisparity&lt;GrayU8, GrayU8 | GrayF32&gt; as FactoryStereoDisparity.blockMatch(ConfigDisparityBM, GrayU8.class, dispType) builds it for
 *  errorType = SAD (main/boofcv-feature/.../factory/feature/disparity/FactoryStereoDisparity.java:62-144; WrapDisparityBlockMatchRowFormat over
 *  DisparityScoreBM_S32 with BlockRowScoreSad.U8 and SelectErrorWithChecks_S32.DispU8 / SelectErrorSubpixel.S32_F32), with process() on the device:
 *  bhip_disparity_bm_u8_u8 (subpixel = false) / bhip_disparity_bm_u8_f32 (subpixel = true).  The reference has no hook for this factory, so the
 *  class is constructed where FactoryStereoDisparity.blockMatch would be called:
 *      StereoDisparity&lt;GrayU8, GrayF32&gt; alg = StereoDisparityHip.blockMatch(config, GrayF32.class);
 *  Results are bit for bit those of the Java classes.  Deviations (include/boofhip.h): the disparity image is written as a whole by every
 *  process() -- rangeDisparity in the rows and columns the Java code never writes, where it keeps what an earlier pair left there (the result of
 *  a freshly constructed Java object); an image lower than the region is refused.  Limits: regionRadiusX / Y &lt;= 7, rangeDisparity &lt;= 256;
 *  beyond them check() throws RuntimeException and the caller uses the Java path, as for NCC and the other input types.
 *  errorType = CENSUS: StereoDisparityCensusHip.  blockMatchBest5: StereoDisparityBest5Hip.
 *  UNCOMPILED SOURCE. */
public class StereoDisparityHip<DI extends ImageGray<DI>> implements StereoDisparity<GrayU8, DI> {
	private final ConfigDisparityBM config;
	private final Class<DI> dispType;
	private final ByteBuffer cfg;   // bhip_disparity_bm_cfg: int[4], double, int, (pad), double
	private DI disparity;

	/** the checks of FactoryStereoDisparity.blockMatch and of the DisparityBlockMatchRowFormat constructor */
	public static <DI extends ImageGray<DI>> StereoDisparityHip<DI> blockMatch(ConfigDisparityBM config, Class<DI> dispType) {
		if (config == null) config = new ConfigDisparityBM();
		if (config.subpixel) {
			if (dispType != GrayF32.class) throw new IllegalArgumentException("With subpixel on, disparity image must be GrayF32");
		} else {
			if (dispType != GrayU8.class) throw new IllegalArgumentException("With subpixel on, disparity image must be GrayU8");
		}
		if (config.errorType != DisparityError.SAD) throw new RuntimeException("only errorType = SAD runs on the device");
		int maxDisparity = config.minDisparity + config.rangeDisparity;
		if (maxDisparity <= 0) throw new IllegalArgumentException("Max disparity must be greater than zero. max=" + maxDisparity);
		if (config.minDisparity < 0 || config.minDisparity >= maxDisparity)
			throw new IllegalArgumentException("Min disparity must be >= 0 and < maxDisparity. min=" + config.minDisparity + " max=" + maxDisparity);
		return new StereoDisparityHip<>(config, dispType);
	}

	private StereoDisparityHip(ConfigDisparityBM config, Class<DI> dispType) {
		this.config = config;
		this.dispType = dispType;
		cfg = ByteBuffer.allocateDirect(48).order(ByteOrder.nativeOrder());
		cfg.putInt(0, config.minDisparity).putInt(4, config.rangeDisparity).putInt(8, config.regionRadiusX).putInt(12, config.regionRadiusY);
		cfg.putDouble(16, config.maxPerPixelError).putInt(24, config.validateRtoL).putDouble(32, config.texture);
	}

	@SuppressWarnings("unchecked")
	@Override public void process(GrayU8 left, GrayU8 right) {
		if (left.width != right.width || left.height != right.height) throw new IllegalArgumentException("Image shapes do not match");
		final int w = left.width, h = left.height;
		if (config.minDisparity + config.rangeDisparity > w - 2*config.regionRadiusX)   // DisparityBlockMatchRowFormat.process
			throw new RuntimeException("The maximum disparity is too large for this image size: max size " + (w - 2*config.regionRadiusX));
		if (disparity == null || disparity.width != w || disparity.height != h)
			disparity = dispType == GrayF32.class ? (DI)new GrayF32(w, h) : (DI)new GrayU8(w, h);
		final long ctx = BoofHipContext.get();
		if (dispType == GrayF32.class) {
			GrayF32 d = (GrayF32)disparity;
			BoofHip.check(ctx, BoofHip.disparityBmU8F32(ctx, cfg, left.data, left.startIndex, left.stride, right.data, right.startIndex, right.stride, w, h,
					d.data, d.startIndex, d.stride));
		} else {
			GrayU8 d = (GrayU8)disparity;
			BoofHip.check(ctx, BoofHip.disparityBmU8U8(ctx, cfg, left.data, left.startIndex, left.stride, right.data, right.startIndex, right.stride, w, h,
					d.data, d.startIndex, d.stride));
		}
	}

	@Override public DI getDisparity() { return disparity; }
	@Override public int getMinDisparity() { return config.minDisparity; }
	@Override public int getRangeDisparity() { return config.rangeDisparity; }
	@Override public int getInvalidValue() { return config.rangeDisparity; }
	@Override public int getBorderX() { return config.regionRadiusX; }
	@Override public int getBorderY() { return config.regionRadiusY; }
	@Override public ImageType<GrayU8> getInputType() { return ImageType.single(GrayU8.class); }
	@Override public Class<DI> getDisparityType() { return dispType; }
}
