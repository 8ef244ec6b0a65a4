package boofcv.hip;

import boofcv.abst.filter.binary.GlobalBinaryFilter;
import boofcv.abst.filter.binary.GlobalFixedBinaryFilter;
import boofcv.abst.filter.binary.InputToBinary;
import boofcv.abst.filter.binary.InputToBinarySwitch;
import boofcv.abst.filter.binary.LocalGaussianBinaryFilter;
import boofcv.abst.filter.binary.LocalMeanBinaryFilter;
import boofcv.alg.filter.binary.ThresholdBlock;
import boofcv.alg.filter.binary.ThresholdBlockOtsu;
import boofcv.alg.filter.binary.impl.ThresholdBlockMean_F32;
import boofcv.alg.filter.binary.impl.ThresholdBlockMinMax_F32;
import boofcv.factory.filter.binary.ConfigThreshold;
import boofcv.factory.filter.binary.ConfigThresholdBlockMinMax;
import boofcv.factory.filter.binary.ConfigThresholdLocalOtsu;
import boofcv.factory.filter.binary.ThresholdType;
import boofcv.struct.ConfigLength;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;
import boofcv.struct.image.ImageType;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

/** InputToBinary&lt;GrayU8 | GrayF32&gt; objects over bhip_threshold_u8 / bhip_threshold_f32, as FactoryThresholdBinary.threshold(ConfigThreshold, type)
 *  builds them (main/boofcv-ip/.../factory/filter/binary/FactoryThresholdBinary.java:318-372), and what the BOverrideFactoryThresholdBinary hooks
 *  of BoofHipOverrides.install() return.  Results are bit for bit those of the single-threaded Java classes.
 *  On the device: FIXED, LOCAL_MEAN, LOCAL_GAUSSIAN, BLOCK_MIN_MAX, BLOCK_MEAN on GrayU8 and GrayF32; GLOBAL_OTSU (pixel range 0..255) and BLOCK_OTSU
 *  on GrayU8.  A hook of the reference's factory has no "not handled" answer, so for any other image type the hooks below build the Java object the
 *  factory would have built.  The factory's globalOtsu hook does not receive `scale` (FactoryThresholdBinary.java:277-281), so it stays unset:
 *  construct the device form with globalOtsu(minValue, maxValue, scale, down, type) below or with threshold(config, type).
 *  UNCOMPILED SOURCE. */
public final class FactoryThresholdBinaryHip {
	private FactoryThresholdBinaryHip() {}

	/** bhip_threshold_cfg: int type @0, double fixedThreshold @8, scale @16, int down @24, double widthLength @32, widthFraction @40,
	 *  int minPixelValue @48, maxPixelValue @52, thresholdFromLocalBlocks @56, double minimumSpread @64, int useOtsu2 @72, double tuning @80; 88 bytes */
	static ByteBuffer cfg(ThresholdType type, double fixedThreshold, double scale, boolean down, ConfigLength width, int minPixelValue, int maxPixelValue,
						  boolean thresholdFromLocalBlocks, double minimumSpread, boolean useOtsu2, double tuning) {
		ByteBuffer c = ByteBuffer.allocateDirect(88).order(ByteOrder.nativeOrder());
		c.putInt(0, type.ordinal()).putDouble(8, fixedThreshold).putDouble(16, scale).putInt(24, down ? 1 : 0);
		c.putDouble(32, width.length).putDouble(40, width.fraction).putInt(48, minPixelValue).putInt(52, maxPixelValue);
		c.putInt(56, thresholdFromLocalBlocks ? 1 : 0).putDouble(64, minimumSpread).putInt(72, useOtsu2 ? 1 : 0).putDouble(80, tuning);
		return c;
	}

	static boolean onDevice(ThresholdType type, Class<?> inputType) {
		switch (type) {
			case FIXED: case LOCAL_MEAN: case LOCAL_GAUSSIAN: case BLOCK_MIN_MAX: case BLOCK_MEAN:
				return inputType == GrayU8.class || inputType == GrayF32.class;
			case GLOBAL_OTSU: case BLOCK_OTSU:
				return inputType == GrayU8.class;
			default:
				return false;
		}
	}

	/** process() on the device; block types reshape the output as ThresholdBlock.process does, the others require the input's shape */
	static final class ThresholdHip<T extends ImageGray<T>> implements InputToBinary<T> {
		private final ByteBuffer cfg;
		private final Class<T> inputType;
		private final boolean block;

		ThresholdHip(ByteBuffer cfg, ThresholdType type, Class<T> inputType) {
			this.cfg = cfg;
			this.inputType = inputType;
			this.block = type == ThresholdType.BLOCK_MIN_MAX || type == ThresholdType.BLOCK_MEAN || type == ThresholdType.BLOCK_OTSU;
		}

		@Override public void process(T input, GrayU8 output) {
			if (block) output.reshape(input.width, input.height);
			else if (output.width != input.width || output.height != input.height) throw new IllegalArgumentException("Image shapes do not match");
			final long ctx = BoofHipContext.get();
			if (inputType == GrayU8.class) {
				GrayU8 in = (GrayU8)(ImageGray)input;
				BoofHip.check(ctx, BoofHip.thresholdU8(ctx, cfg, in.data, in.startIndex, in.stride, in.width, in.height, output.data, output.startIndex, output.stride));
			} else {
				GrayF32 in = (GrayF32)(ImageGray)input;
				BoofHip.check(ctx, BoofHip.thresholdF32(ctx, cfg, in.data, in.startIndex, in.stride, in.width, in.height, output.data, output.startIndex, output.stride));
			}
		}

		@Override public ImageType<T> getInputType() { return ImageType.single(inputType); }
	}

	private static <T extends ImageGray<T>> InputToBinary<T> device(ThresholdType type, double fixedThreshold, double scale, boolean down, ConfigLength width,
																  boolean local, double minimumSpread, boolean otsu2, double tuning, Class<T> inputType) {
		return new ThresholdHip<>(cfg(type, fixedThreshold, scale, down, width, 0, 255, local, minimumSpread, otsu2, tuning), type, inputType);
	}

	public static <T extends ImageGray<T>> InputToBinary<T> globalFixed(double threshold, boolean down, Class<T> inputType) {
		if (!onDevice(ThresholdType.FIXED, inputType)) return new GlobalFixedBinaryFilter<>(threshold, down, ImageType.single(inputType));
		return device(ThresholdType.FIXED, threshold, 1.0, down, ConfigLength.fixed(11), true, 10, true, 0, inputType);
	}

	public static <T extends ImageGray<T>> InputToBinary<T> globalOtsu(double minValue, double maxValue, double scale, boolean down, Class<T> inputType) {
		if (!onDevice(ThresholdType.GLOBAL_OTSU, inputType) || minValue != 0 || maxValue != 255)
			return new GlobalBinaryFilter.Otsu<>(minValue, maxValue, scale, down, ImageType.single(inputType));
		return device(ThresholdType.GLOBAL_OTSU, 0, scale, down, ConfigLength.fixed(11), true, 10, true, 0, inputType);
	}

	public static <T extends ImageGray<T>> InputToBinary<T> localMean(ConfigLength width, double scale, boolean down, Class<T> inputType) {
		if (!onDevice(ThresholdType.LOCAL_MEAN, inputType)) return new LocalMeanBinaryFilter<>(width, scale, down, ImageType.single(inputType));
		return device(ThresholdType.LOCAL_MEAN, 0, scale, down, width, true, 10, true, 0, inputType);
	}

	public static <T extends ImageGray<T>> InputToBinary<T> localGaussian(ConfigLength width, double scale, boolean down, Class<T> inputType) {
		if (!onDevice(ThresholdType.LOCAL_GAUSSIAN, inputType)) return new LocalGaussianBinaryFilter<>(width, scale, down, ImageType.single(inputType));
		return device(ThresholdType.LOCAL_GAUSSIAN, 0, scale, down, width, true, 10, true, 0, inputType);
	}

	@SuppressWarnings({"unchecked", "rawtypes"})
	public static <T extends ImageGray<T>> InputToBinary<T> blockMinMax(ConfigLength width, double scale, boolean down, double minimumSpread,
																		  boolean thresholdFromLocalBlocks, Class<T> inputType) {
		if (!onDevice(ThresholdType.BLOCK_MIN_MAX, inputType))   // the factory's own choice for every type but GrayU8
			return new ThresholdBlock(new ThresholdBlockMinMax_F32((float)minimumSpread, (float)scale, down), width, thresholdFromLocalBlocks, inputType);
		return device(ThresholdType.BLOCK_MIN_MAX, 0, scale, down, width, thresholdFromLocalBlocks, minimumSpread, true, 0, inputType);
	}

	@SuppressWarnings({"unchecked", "rawtypes"})
	public static <T extends ImageGray<T>> InputToBinary<T> blockMean(ConfigLength width, double scale, boolean down, boolean thresholdFromLocalBlocks,
																		Class<T> inputType) {
		if (!onDevice(ThresholdType.BLOCK_MEAN, inputType))
			return new ThresholdBlock(new ThresholdBlockMean_F32((float)scale, down), width, thresholdFromLocalBlocks, inputType);
		return device(ThresholdType.BLOCK_MEAN, 0, scale, down, width, thresholdFromLocalBlocks, 10, true, 0, inputType);
	}

	public static <T extends ImageGray<T>> InputToBinary<T> blockOtsu(boolean otsu2, ConfigLength width, double tuning, double scale, boolean down,
																		boolean thresholdFromLocalBlocks, Class<T> inputType) {
		if (!onDevice(ThresholdType.BLOCK_OTSU, inputType))   // InputToBinarySwitch converts the input to GrayU8 first
			return new InputToBinarySwitch<>(new ThresholdBlock<>(new ThresholdBlockOtsu(otsu2, tuning, scale, down), width, thresholdFromLocalBlocks, GrayU8.class), inputType);
		return device(ThresholdType.BLOCK_OTSU, 0, scale, down, width, thresholdFromLocalBlocks, 10, otsu2, tuning, inputType);
	}

	/** FactoryThresholdBinary.threshold(config, inputType) for the types above; IllegalArgumentException for the others (use the Java factory) */
	public static <T extends ImageGray<T>> InputToBinary<T> threshold(ConfigThreshold config, Class<T> inputType) {
		switch (config.type) {
			case FIXED: return globalFixed(config.fixedThreshold, config.down, inputType);
			case GLOBAL_OTSU: return globalOtsu(config.minPixelValue, config.maxPixelValue, config.scale, config.down, inputType);
			case LOCAL_MEAN: return localMean(config.width, config.scale, config.down, inputType);
			case LOCAL_GAUSSIAN: return localGaussian(config.width, config.scale, config.down, inputType);
			case BLOCK_MIN_MAX:
				return blockMinMax(config.width, config.scale, config.down, ((ConfigThresholdBlockMinMax)config).minimumSpread, config.thresholdFromLocalBlocks, inputType);
			case BLOCK_MEAN: return blockMean(config.width, config.scale, config.down, config.thresholdFromLocalBlocks, inputType);
			case BLOCK_OTSU: {
				ConfigThresholdLocalOtsu c = (ConfigThresholdLocalOtsu)config;
				return blockOtsu(c.useOtsu2, c.width, c.tuning, c.scale, c.down, c.thresholdFromLocalBlocks, inputType);
			}
			default:
				throw new IllegalArgumentException(config.type + " is not implemented on the device");
		}
	}
}
