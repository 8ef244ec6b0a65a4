package boofcv.hip;

import boofcv.alg.background.stationary.BackgroundStationaryGmm;
import boofcv.alg.misc.ImageMiscOps;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageBase;
import boofcv.struct.image.ImageType;

import java.nio.ByteBuffer;

/** BackgroundStationaryGmm_SB / _MB (main/boofcv-feature/.../alg/background/stationary/BackgroundStationaryGmm.java:48-78,
 *  BackgroundStationaryGmm_SB.java:50-100, BackgroundStationaryGmm_MB.java:54-105; BackgroundGmmCommon.java:78-375) with the mixtures on the
 *  device: bhip_bg_create_gmm, bhip_bg_update_*, bhip_bg_segment_*.  Bit for bit the Java result.  The superclass is constructed as usual, so
 *  its `common` carries the parameters (its model array stays empty); common.unknownValue, which the reference refreshes only inside segment(),
 *  is handed to a new handle with bhip_bg_set_common_unknown_value.  More than 8 Gaussians: RuntimeException, use the Java class.
 *  The class sits in this package but reads the package-private `common` through the setters and getters only; decayCoef and maxGaussians are
 *  kept from the constructor.  UNCOMPILED SOURCE. */
public class BackgroundStationaryGmmHip<T extends ImageBase<T>> extends BackgroundStationaryGmm<T> {
	private final FactoryBackgroundModelHip.Native nat;
	private final float decayCoef;
	private final int maxGaussians;
	private float significantWeight;
	private int modelWidth, modelHeight, commonUnknown;

	public BackgroundStationaryGmmHip(float learningPeriod, float decayCoef, int maxGaussians, ImageType<T> imageType) {
		super(learningPeriod, decayCoef, maxGaussians, imageType);
		if (maxGaussians > 8) throw new RuntimeException("more than 8 Gaussians per pixel do not run on the device");
		this.decayCoef = decayCoef;
		this.maxGaussians = maxGaussians;
		this.significantWeight = Math.min(0.2f, 100*(1.0f/learningPeriod));
		nat = new FactoryBackgroundModelHip.Native(FactoryBackgroundModelHip.Native.GMM, imageType);
	}

	@Override public void setSignificantWeight(float value) {
		super.setSignificantWeight(value);
		significantWeight = value;
	}

	private void open(int w, int h) {
		// bhip_bg_gmm_cfg: learningPeriod, initialVariance, decayCoefient, maxDistance, numberOfGaussian, significantWeight, unknownValue
		ByteBuffer cfg = FactoryBackgroundModelHip.Native.struct(28);
		cfg.putFloat(0, 1000f).putFloat(4, 400f).putFloat(8, decayCoef).putFloat(12, 3f).putInt(16, maxGaussians).putFloat(20, 0.01f).putInt(24, 0);
		boolean created = nat.open(cfg, w, h);
		long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.bgSetLearningPeriod(nat.handle, getLearningPeriod()));
		BoofHip.check(ctx, BoofHip.bgSetInitialVariance(nat.handle, getInitialVariance()));
		BoofHip.check(ctx, BoofHip.bgSetMaxDistance(nat.handle, getMaxDistance()));
		BoofHip.check(ctx, BoofHip.bgSetSignificantWeight(nat.handle, significantWeight));
		BoofHip.check(ctx, BoofHip.bgSetUnknownValue(nat.handle, getUnknownValue()));
		if (created) BoofHip.check(ctx, BoofHip.bgSetCommonUnknownValue(nat.handle, commonUnknown));
	}

	@Override public void reset() {
		modelWidth = modelHeight = 0;
		if (nat.handle != 0) BoofHip.check(BoofHipContext.get(), BoofHip.bgReset(nat.handle, -1));
	}

	@Override public void updateBackground(T frame, GrayU8 mask) {
		open(frame.width, frame.height);
		if (modelWidth != frame.width || modelHeight != frame.height) {
			BoofHip.check(BoofHipContext.get(), BoofHip.bgReset(nat.handle, -1));
			modelWidth = frame.width;
			modelHeight = frame.height;
		}
		if (mask != null) mask.reshape(frame.width, frame.height);
		nat.call(false, frame, mask);
	}

	@Override public void segment(T frame, GrayU8 segmented) {
		if (modelWidth != frame.width || modelHeight != frame.height) {
			segmented.reshape(frame.width, frame.height);
			ImageMiscOps.fill(segmented, unknownValue);
			return;
		}
		commonUnknown = getUnknownValue();
		open(frame.width, frame.height);
		nat.call(true, frame, segmented);
	}
}
