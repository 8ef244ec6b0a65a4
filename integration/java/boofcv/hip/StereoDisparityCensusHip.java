package boofcv.hip;

import boofcv.abst.feature.disparity.StereoDisparity;
import boofcv.abst.filter.FilterImageInterface;
import boofcv.factory.feature.disparity.ConfigDisparityBM;
import boofcv.factory.feature.disparity.DisparityError;
import boofcv.factory.transform.census.CensusVariants;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageBase;
import boofcv.struct.image.ImageGray;
import boofcv.struct.image.ImageType;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

/** StereoDisparity&lt;GrayU8, GrayU8 | GrayF32&gt; as FactoryStereoDisparity.blockMatch(ConfigDisparityBM, GrayU8.class, dispType) builds it for
 *  errorType = CENSUS (main/boofcv-feature/.../factory/feature/disparity/FactoryStereoDisparity.java:85-102; WrapDisparityBlockMatchCensus over
 *  DisparityScoreBM_S32 with BlockRowScoreCensus.U8 / S32 / S64 on the census images of FactoryCensusTransform.variant(config.configCensus.variant)),
 *  with process() on the device: bhip_disparity_bm_census_u8_u8 (subpixel = false) / bhip_disparity_bm_census_u8_f32 (subpixel = true).  The
 *  reference has no hook for this factory, so the class is constructed where FactoryStereoDisparity.blockMatch would be called:
 *      StereoDisparity&lt;GrayU8, GrayF32&gt; alg = StereoDisparityCensusHip.blockMatch(config, GrayF32.class);
 *  Results are bit for bit those of the Java classes.  The census images of a pair stay on the device; getCLeft / getCRight compute them on
 *  demand with the filter (FilterCensusTransformHip) from the images the last process() was given.  Deviations and limits: those of
 *  StereoDisparityHip, and an image smaller than the census region's radius + 1 is refused (include/boofhip.h).
 *  UNCOMPILED SOURCE. */
public class StereoDisparityCensusHip<C extends ImageBase<C>, DI extends ImageGray<DI>> implements StereoDisparity<GrayU8, DI> {
	private final ConfigDisparityBM config;
	private final Class<DI> dispType;
	private final int variant;      // CensusVariants ordinal = bhip_census_variant
	private final FilterImageInterface<GrayU8, C> censusTran;
	private final ByteBuffer cfg;   // bhip_disparity_bm_cfg: int[4], double, int, (pad), double
	private DI disparity;
	private GrayU8 left, right;
	private C cleft, cright;

	/** the checks of FactoryStereoDisparity.blockMatch and of the DisparityBlockMatchRowFormat constructor */
	public static <C extends ImageBase<C>, DI extends ImageGray<DI>> StereoDisparityCensusHip<C, DI> blockMatch(ConfigDisparityBM config, Class<DI> dispType) {
		if (config == null) config = new ConfigDisparityBM();
		if (config.subpixel) {
			if (dispType != GrayF32.class) throw new IllegalArgumentException("With subpixel on, disparity image must be GrayF32");
		} else {
			if (dispType != GrayU8.class) throw new IllegalArgumentException("With subpixel on, disparity image must be GrayU8");
		}
		if (config.errorType != DisparityError.CENSUS) throw new IllegalArgumentException("Unsupported error type " + config.errorType + ": this class is the CENSUS form");
		CensusVariants v = config.configCensus.variant;
		FilterImageInterface<GrayU8, C> censusTran = FactoryCensusTransformHip.variant(v);
		int maxDisparity = config.minDisparity + config.rangeDisparity;
		if (maxDisparity <= 0) throw new IllegalArgumentException("Max disparity must be greater than zero. max=" + maxDisparity);
		if (config.minDisparity < 0 || config.minDisparity >= maxDisparity)
			throw new IllegalArgumentException("Min disparity must be >= 0 and < maxDisparity. min=" + config.minDisparity + " max=" + maxDisparity);
		return new StereoDisparityCensusHip<>(config, dispType, v.ordinal(), censusTran);
	}

	private StereoDisparityCensusHip(ConfigDisparityBM config, Class<DI> dispType, int variant, FilterImageInterface<GrayU8, C> censusTran) {
		this.config = config;
		this.dispType = dispType;
		this.variant = variant;
		this.censusTran = censusTran;
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
			BoofHip.check(ctx, BoofHip.disparityBmCensusU8F32(ctx, cfg, variant, left.data, left.startIndex, left.stride, right.data, right.startIndex, right.stride,
					w, h, d.data, d.startIndex, d.stride));
		} else {
			GrayU8 d = (GrayU8)disparity;
			BoofHip.check(ctx, BoofHip.disparityBmCensusU8U8(ctx, cfg, variant, left.data, left.startIndex, left.stride, right.data, right.startIndex, right.stride,
					w, h, d.data, d.startIndex, d.stride));
		}
		this.left = left;
		this.right = right;
		cleft = cright = null;
	}

	/** WrapDisparityBlockMatchCensus.getCLeft / getCRight: a 1 x 1 image before the first pair, as the constructor's createImage(1,1) */
	public C getCLeft() {
		if (cleft == null) {
			cleft = censusTran.getOutputType().createImage(1, 1);
			if (left != null) censusTran.process(left, cleft);
		}
		return cleft;
	}

	public C getCRight() {
		if (cright == null) {
			cright = censusTran.getOutputType().createImage(1, 1);
			if (right != null) censusTran.process(right, cright);
		}
		return cright;
	}

	public FilterImageInterface<GrayU8, C> getCensusTran() { return censusTran; }

	@Override public DI getDisparity() { return disparity; }
	@Override public int getMinDisparity() { return config.minDisparity; }
	@Override public int getRangeDisparity() { return config.rangeDisparity; }
	@Override public int getInvalidValue() { return config.rangeDisparity; }
	@Override public int getBorderX() { return config.regionRadiusX; }
	@Override public int getBorderY() { return config.regionRadiusY; }
	@Override public ImageType<GrayU8> getInputType() { return censusTran.getInputType(); }
	@Override public Class<DI> getDisparityType() { return dispType; }
}
