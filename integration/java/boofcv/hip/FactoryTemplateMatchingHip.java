package boofcv.hip;

import boofcv.alg.feature.detect.template.TemplateMatching;
import boofcv.alg.feature.detect.template.TemplateMatchingIntensity;
import boofcv.factory.feature.detect.template.TemplateScoreType;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;

/** FactoryTemplateMatching (main/boofcv-feature/.../factory/feature/detect/template/FactoryTemplateMatching.java:47-113) with the intensity on the
 *  device.  The reference has no hook for this factory, so the class is used where FactoryTemplateMatching would be called:
 *      TemplateMatching&lt;GrayU8&gt; matcher = FactoryTemplateMatchingHip.createMatcher(TemplateScoreType.NCC, GrayU8.class);
 *  createMatcher hands the device intensity to the Java TemplateMatching, whose extractor comes from FactoryFeatureExtractor.nonmax and so runs on the
 *  device too once BoofHipOverrides.install() has set BOverrideFactoryFeatureExtractor.nonmax; the selection of the N best stays the Java
 *  QuickSelect (bhip_template_select_f32 is the same step for callers that stay on the native side).  IllegalArgumentException where the Java
 *  factory throws it; CORRELATION (TemplateCorrelationFFT) throws RuntimeException: use the Java path.  UNCOMPILED SOURCE. */
public class FactoryTemplateMatchingHip {
	public static <T extends ImageGray<T>> TemplateMatchingIntensity<T> createIntensity(TemplateScoreType type, Class<T> imageType) {
		if (type == TemplateScoreType.CORRELATION) {
			if (imageType == GrayF32.class) throw new RuntimeException("TemplateCorrelationFFT does not run on the device (use the Java path)");
			throw new IllegalArgumentException("Image type not supported. " + imageType.getSimpleName());
		}
		switch (type) {
			case SUM_ABSOLUTE_DIFFERENCE:
			case SUM_SQUARE_ERROR:
			case NCC:
				if (imageType != GrayU8.class && imageType != GrayF32.class)
					throw new IllegalArgumentException("Image type not supported. " + imageType.getSimpleName());
				return new TemplateMatchingIntensityHip<>(type, imageType);
			default:
				throw new IllegalArgumentException("Unknown");
		}
	}

	public static <T extends ImageGray<T>> TemplateMatching<T> createMatcher(TemplateScoreType type, Class<T> imageType) {
		return new TemplateMatching<>(createIntensity(type, imageType));
	}
}
