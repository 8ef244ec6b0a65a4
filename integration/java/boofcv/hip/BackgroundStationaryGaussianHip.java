package boofcv.hip;

import boofcv.alg.background.stationary.BackgroundStationaryGaussian;
import boofcv.alg.misc.ImageMiscOps;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageBase;
import boofcv.struct.image.ImageType;

import java.nio.ByteBuffer;

/** BackgroundStationaryGaussian_SB / _PL (main/boofcv-feature/.../alg/background/stationary/BackgroundStationaryGaussian_SB.java:58-142,
 *  BackgroundStationaryGaussian_PL.java:72-180) with the mean / variance planes on the device: bhip_bg_create_gaussian, bhip_bg_update_*,
 *  bhip_bg_segment_*.  Bit for bit the Java result, the denormal default variance and the 0/0 and x/0 of segment() included.  "Not initialised"
 *  is `background.width == 1`, kept here as modelWidth; the library reproduces the never-initialised model of width 1.  UNCOMPILED SOURCE. */
public class BackgroundStationaryGaussianHip<T extends ImageBase<T>> extends BackgroundStationaryGaussian<T> {
	private final FactoryBackgroundModelHip.Native nat;
	private int modelWidth = 1, modelHeight = 1;

	public BackgroundStationaryGaussianHip(float learnRate, float threshold, ImageType<T> imageType) {
		super(learnRate, threshold, imageType);
		nat = new FactoryBackgroundModelHip.Native(FactoryBackgroundModelHip.Native.GAUSSIAN, imageType);
	}

	private void open(int w, int h) {
		ByteBuffer cfg = FactoryBackgroundModelHip.Native.struct(20);   // bhip_bg_gaussian_cfg: learnRate, threshold, initialVariance, minimumDifference, unknownValue
		cfg.putFloat(0, 0.05f).putFloat(4, 1f).putFloat(8, Float.MIN_VALUE).putFloat(12, 0f).putInt(16, 0);
		nat.open(cfg, w, h);
		long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.bgSetLearnRate(nat.handle, learnRate));
		BoofHip.check(ctx, BoofHip.bgSetThreshold(nat.handle, threshold));
		BoofHip.check(ctx, BoofHip.bgSetInitialVariance(nat.handle, initialVariance));
		BoofHip.check(ctx, BoofHip.bgSetMinimumDifference(nat.handle, minimumDifference));
		BoofHip.check(ctx, BoofHip.bgSetUnknownValue(nat.handle, getUnknownValue()));
	}

	@Override public void reset() {
		modelWidth = modelHeight = 1;
		if (nat.handle != 0) BoofHip.check(BoofHipContext.get(), BoofHip.bgReset(nat.handle, -1));
	}

	@Override public void updateBackground(T frame) {
		if (modelWidth == 1) {
			open(frame.width, frame.height);
			BoofHip.check(BoofHipContext.get(), BoofHip.bgReset(nat.handle, -1));
			modelWidth = frame.width;
			modelHeight = frame.height;
		} else if (modelWidth != frame.width || modelHeight != frame.height) {
			throw new IllegalArgumentException("Image shapes do not match");
		} else {
			open(frame.width, frame.height);
		}
		nat.call(false, frame, null);
	}

	@Override public void segment(T frame, GrayU8 segmented) {
		if (modelWidth == 1) {
			ImageMiscOps.fill(segmented, unknownValue);
			return;
		}
		if (modelWidth != frame.width || modelHeight != frame.height || segmented.width != frame.width || segmented.height != frame.height)
			throw new IllegalArgumentException("Image shapes do not match");
		open(frame.width, frame.height);
		nat.call(true, frame, segmented);
	}
}
