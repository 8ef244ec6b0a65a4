package boofcv.hip;

import boofcv.alg.background.stationary.BackgroundStationaryBasic;
import boofcv.alg.misc.ImageMiscOps;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageBase;
import boofcv.struct.image.ImageType;

import java.nio.ByteBuffer;

/** BackgroundStationaryBasic_SB / _PL (main/boofcv-feature/.../alg/background/stationary/BackgroundStationaryBasic_SB.java:58-123,
 *  BackgroundStationaryBasic_PL.java:66-142) with the background image on the device: bhip_bg_create_basic, bhip_bg_update_u8 / _f32,
 *  bhip_bg_segment_u8 / _f32.  Bit for bit the Java result.  "Not initialised" is `background.width != frame.width`, kept here as modelWidth.
 *  getBackground() is not offered: fetch the model with BoofHip.bgFetchModel.  UNCOMPILED SOURCE. */
public class BackgroundStationaryBasicHip<T extends ImageBase<T>> extends BackgroundStationaryBasic<T> {
	private final FactoryBackgroundModelHip.Native nat;
	private int modelWidth, modelHeight;

	public BackgroundStationaryBasicHip(float learnRate, float threshold, ImageType<T> imageType) {
		super(learnRate, threshold, imageType);
		nat = new FactoryBackgroundModelHip.Native(FactoryBackgroundModelHip.Native.BASIC, imageType);
	}

	private void open(int w, int h) {
		ByteBuffer cfg = FactoryBackgroundModelHip.Native.struct(12);   // bhip_bg_basic_cfg: learnRate, threshold, unknownValue
		cfg.putFloat(0, 0.05f).putFloat(4, 1f).putInt(8, 0);
		nat.open(cfg, w, h);
		long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.bgSetLearnRate(nat.handle, learnRate));   // the setters validate nothing, like the Java fields
		BoofHip.check(ctx, BoofHip.bgSetThreshold(nat.handle, threshold));
		BoofHip.check(ctx, BoofHip.bgSetUnknownValue(nat.handle, getUnknownValue()));
	}

	@Override public void reset() {
		modelWidth = modelHeight = 0;
		if (nat.handle != 0) BoofHip.check(BoofHipContext.get(), BoofHip.bgReset(nat.handle, -1));
	}

	@Override public void updateBackground(T frame) {
		if (modelWidth != frame.width) {
			open(frame.width, frame.height);
			BoofHip.check(BoofHipContext.get(), BoofHip.bgReset(nat.handle, -1));
			modelWidth = frame.width;
			modelHeight = frame.height;
		} else if (modelHeight != frame.height) {
			throw new IllegalArgumentException("Image shapes do not match");
		} else {
			open(frame.width, frame.height);
		}
		nat.call(false, frame, null);
	}

	@Override public void segment(T frame, GrayU8 segmented) {
		if (modelWidth != frame.width) {
			ImageMiscOps.fill(segmented, unknownValue);
			return;
		}
		if (modelHeight != frame.height || segmented.width != frame.width || segmented.height != frame.height)
			throw new IllegalArgumentException("Image shapes do not match");
		open(frame.width, frame.height);
		nat.call(true, frame, segmented);
	}
}
