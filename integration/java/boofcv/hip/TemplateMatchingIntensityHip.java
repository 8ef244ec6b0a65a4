package boofcv.hip;

import boofcv.alg.feature.detect.template.TemplateMatchingIntensity;
import boofcv.factory.feature.detect.template.TemplateScoreType;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;

/** TemplateMatchingIntensity&lt;GrayU8 | GrayF32&gt; as FactoryTemplateMatching.createIntensity(SUM_ABSOLUTE_DIFFERENCE | SUM_SQUARE_ERROR | NCC,
 *  imageType) builds it (main/boofcv-feature/.../factory/feature/detect/template/FactoryTemplateMatching.java:47-99; TemplateIntensityImage over
 *  TemplateSumAbsoluteDifference / TemplateSumSquaredError / TemplateNCC), with process() on the device: bhip_template_intensity_u8 /
 *  bhip_template_intensity_f32.  Built by FactoryTemplateMatchingHip.  Results are bit for bit those of the single-threaded Java classes; NCC
 *  uses EPS = (float)2^-21 for UtilEjml.F_EPS.  Deviation (include/boofhip.h): the intensity image is written as a whole by every process(), 0 in
 *  the border, also by process(template, mask), where the Java code keeps what an earlier call left in the border (the result of a freshly
 *  constructed Java object).  Limit: template width &lt;= 160; beyond it check() throws RuntimeException and the caller uses the Java path.
 *  UNCOMPILED SOURCE. */
public class TemplateMatchingIntensityHip<T extends ImageGray<T>> implements TemplateMatchingIntensity<T> {
	private final int score;          // TemplateScoreType ordinal = bhip_template_score
	private final boolean maximize;
	private final Class<T> imageType;
	private final GrayF32 intensity = new GrayF32(1, 1);
	private T image;
	private int borderX0, borderY0, borderX1, borderY1;

	TemplateMatchingIntensityHip(TemplateScoreType type, Class<T> imageType) {
		this.score = type.ordinal();
		this.maximize = type == TemplateScoreType.NCC;
		this.imageType = imageType;
	}

	@Override public void setInputImage(T image) { this.image = image; }

	@Override public void process(T template) { process(template, null); }

	@Override public void process(T template, T mask) {
		intensity.reshape(image.width, image.height);
		borderX0 = template.width/2;
		borderY0 = template.height/2;
		borderX1 = template.width - borderX0;
		borderY1 = template.height - borderY0;
		final long ctx = BoofHipContext.get();
		if (imageType == GrayU8.class) {
			GrayU8 i = (GrayU8)image, t = (GrayU8)template, m = (GrayU8)mask;
			BoofHip.check(ctx, BoofHip.templateIntensityU8(ctx, score, i.data, i.startIndex, i.stride, i.width, i.height, t.data, t.startIndex, t.stride, t.width,
					t.height, m == null ? null : m.data, m == null ? 0 : m.startIndex, m == null ? 0 : m.stride, m == null ? 0 : m.width, m == null ? 0 : m.height,
					intensity.data, intensity.startIndex, intensity.stride));
		} else {
			GrayF32 i = (GrayF32)image, t = (GrayF32)template, m = (GrayF32)mask;
			BoofHip.check(ctx, BoofHip.templateIntensityF32(ctx, score, i.data, i.startIndex, i.stride, i.width, i.height, t.data, t.startIndex, t.stride, t.width,
					t.height, m == null ? null : m.data, m == null ? 0 : m.startIndex, m == null ? 0 : m.stride, m == null ? 0 : m.width, m == null ? 0 : m.height,
					intensity.data, intensity.startIndex, intensity.stride));
		}
	}

	@Override public GrayF32 getIntensity() { return intensity; }
	@Override public boolean isBorderProcessed() { return false; }
	@Override public int getBorderX0() { return borderX0; }
	@Override public int getBorderX1() { return borderX1; }
	@Override public int getBorderY0() { return borderY0; }
	@Override public int getBorderY1() { return borderY1; }
	@Override public boolean isMaximize() { return maximize; }
}
