package boofcv.hip;

import boofcv.abst.feature.describe.ConfigSiftScaleSpace;
import boofcv.abst.feature.detect.interest.ConfigSiftDetector;
import boofcv.abst.feature.detect.interest.InterestPointDetector;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;

/** FactoryInterestPoint.sift on the device (main/boofcv-feature/.../factory/feature/detect/interest/FactoryInterestPoint.java:133-148); the
 *  reference has no hook for it, so callers name this factory.  UNCOMPILED SOURCE. */
public class FactoryInterestPointHip {
	/** sift(configSS, configDet, imageType): null = new ConfigSiftScaleSpace() / new ConfigSiftDetector().  GrayF32 and GrayU8; any other image
	 *  type throws RuntimeException: use FactoryInterestPoint.sift */
	public static <T extends ImageGray<T>> InterestPointDetector<T> sift(ConfigSiftScaleSpace configSS, ConfigSiftDetector configDet, Class<T> imageType) {
		if (configSS == null) configSS = new ConfigSiftScaleSpace();
		if (configDet == null) configDet = new ConfigSiftDetector();
		if (imageType != GrayF32.class && imageType != GrayU8.class)
			throw new RuntimeException("the SIFT detector runs on the device for GrayF32 and GrayU8 images only (use FactoryInterestPoint.sift)");
		return new SiftDetectorHip<>(configSS, configDet, imageType);
	}
}
