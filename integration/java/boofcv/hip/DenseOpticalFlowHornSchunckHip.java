package boofcv.hip;

import boofcv.abst.flow.DenseOpticalFlow;
import boofcv.factory.flow.ConfigHornSchunck;
import boofcv.struct.flow.ImageFlow;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;
import boofcv.struct.image.ImageType;

/** DenseOpticalFlow&lt;GrayF32 | GrayU8&gt; as FactoryDenseOpticalFlow.hornSchunck(ConfigHornSchunck, imageType) builds it
 *  (main/boofcv-feature/.../factory/flow/FactoryDenseOpticalFlow.java:122-138: HornSchunck_to_DenseOpticalFlow over HornSchunck_F32 / HornSchunck_U8),
 *  with process() on the device: bhip_flow_hs_f32 / bhip_flow_hs_u8 -- the three derivatives and numIterations Jacobi iterations from the zero flow
 *  (resetOutput is true and has no setter).  Built by FactoryDenseOpticalFlowHip.hornSchunck.  Results are bit for bit those of the Java classes.
 *  Deviations (include/boofhip.h): derivY(width-1, height-1), which the reference never writes, is 0, the value of a freshly constructed
 *  instance; HornSchunck_F32.computeDerivT's fourth tap reads image1's pixel (x+1, y+1) whatever the two strides are; a flow whose size differs
 *  from the images is refused (the Java indexes past it).  Limits: width * height &lt;= 2^28; beyond them check() throws RuntimeException and
 *  the caller uses the Java path.  UNCOMPILED SOURCE. */
public class DenseOpticalFlowHornSchunckHip<T extends ImageGray<T>> implements DenseOpticalFlow<T> {
	private final Class<T> inputType;
	private final float alpha;
	private int numIterations;
	private float[] xy = new float[0];

	DenseOpticalFlowHornSchunckHip(ConfigHornSchunck config, Class<T> inputType) {
		this.inputType = inputType;
		this.alpha = config.alpha;
		this.numIterations = config.numIterations;
	}

	public void setNumIterations(int numIterations) { this.numIterations = numIterations; }

	@Override public void process(T source, T destination, ImageFlow flow) {
		if (source.width != destination.width || source.height != destination.height) throw new IllegalArgumentException("Image shapes do not match");
		final int w = source.width, h = source.height;
		if (flow.width != w || flow.height != h) throw new IllegalArgumentException("the flow and the images differ in size");
		if (xy.length < 2*w*h) xy = new float[2*w*h];
		final long ctx = BoofHipContext.get();
		if (inputType == GrayF32.class) {
			GrayF32 s = (GrayF32)source, d = (GrayF32)destination;
			BoofHip.check(ctx, BoofHip.flowHsF32(ctx, alpha, numIterations, s.data, s.startIndex, s.stride, d.data, d.startIndex, d.stride, w, h, xy, 0, 2*w));
		} else {
			GrayU8 s = (GrayU8)source, d = (GrayU8)destination;
			BoofHip.check(ctx, BoofHip.flowHsU8(ctx, alpha, numIterations, s.data, s.startIndex, s.stride, d.data, d.startIndex, d.stride, w, h, xy, 0, 2*w));
		}
		for (int i = 0; i < w*h; i++) {
			ImageFlow.D f = flow.data[i];
			f.x = xy[2*i];
			f.y = xy[2*i + 1];
		}
	}

	@Override public ImageType<T> getInputType() { return ImageType.single(inputType); }
}
