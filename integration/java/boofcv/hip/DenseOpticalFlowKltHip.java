package boofcv.hip;

import boofcv.abst.flow.DenseOpticalFlow;
import boofcv.alg.tracker.klt.PkltConfig;
import boofcv.struct.flow.ImageFlow;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;
import boofcv.struct.image.ImageType;

import java.nio.ByteBuffer;

/** DenseOpticalFlow&lt;GrayF32 | GrayU8&gt; as FactoryDenseOpticalFlow.flowKlt(PkltConfig, radius, inputType, derivType) builds it
 *  (main/boofcv-feature/.../factory/flow/FactoryDenseOpticalFlow.java:61-82: FlowKlt_to_DenseOpticalFlow over DenseOpticalFlowKlt), with process()
 *  on the device: bhip_flow_klt_f32 / bhip_flow_klt_u8 -- both pyramids, the Sobel gradient of the source layers, a pyramid KLT track at every
 *  pixel and the checkNeighbors pass.  Built by FactoryDenseOpticalFlowHip.flowKlt.  Results are bit for bit those of the Java classes.
 *  Deviations (include/boofhip.h): a pixel whose track reaches a position where KltTracker throws counts as a failed track (in Java the exception
 *  leaves process()); a flow whose size differs from the images is refused (the Java indexes with the flow's width).  The library writes y = 0 for
 *  an invalid pixel; process() puts back the y the caller's ImageFlow held there, as markInvalid() leaves it.  Limits: radius &lt;= 7, at most 8
 *  pyramid layers; beyond them check() throws RuntimeException and the caller uses the Java path.  UNCOMPILED SOURCE. */
public class DenseOpticalFlowKltHip<T extends ImageGray<T>> implements DenseOpticalFlow<T> {
	private final Class<T> inputType;
	private final int radius;
	private final int[] scales;
	private final ByteBuffer cfg;   // bhip_klt_cfg
	private float[] xy = new float[0];

	DenseOpticalFlowKltHip(PkltConfig config, int radius, Class<T> inputType) {
		this.inputType = inputType;
		this.radius = radius;
		this.scales = config.pyramidScaling.clone();
		this.cfg = PointTrackerKltPyramidHip.pack(config.config);
	}

	@Override public void process(T source, T destination, ImageFlow flow) {
		if (source.width != destination.width || source.height != destination.height) throw new IllegalArgumentException("Image shapes do not match");
		final int w = source.width, h = source.height;
		if (flow.width != w || flow.height != h) throw new IllegalArgumentException("the flow and the images differ in size");
		if (xy.length < 2*w*h) xy = new float[2*w*h];
		final long ctx = BoofHipContext.get();
		if (inputType == GrayF32.class) {
			GrayF32 s = (GrayF32)source, d = (GrayF32)destination;
			BoofHip.check(ctx, BoofHip.flowKltF32(ctx, cfg, radius, scales, scales.length, s.data, s.startIndex, s.stride, d.data, d.startIndex, d.stride, w, h, xy, 0, 2*w));
		} else {
			GrayU8 s = (GrayU8)source, d = (GrayU8)destination;
			BoofHip.check(ctx, BoofHip.flowKltU8(ctx, cfg, radius, scales, scales.length, s.data, s.startIndex, s.stride, d.data, d.startIndex, d.stride, w, h, xy, 0, 2*w));
		}
		for (int i = 0; i < w*h; i++) {
			ImageFlow.D f = flow.data[i];
			f.x = xy[2*i];
			if (!Float.isNaN(f.x)) f.y = xy[2*i + 1];   // markInvalid() sets x only
		}
	}

	@Override public ImageType<T> getInputType() { return ImageType.single(inputType); }
}
