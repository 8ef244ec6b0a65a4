package boofcv.hip;

import boofcv.abst.feature.detect.interest.ConfigGeneralDetector;
import boofcv.abst.feature.tracker.PointTrack;
import boofcv.abst.feature.tracker.PointTracker;
import boofcv.alg.tracker.klt.KltConfig;
import boofcv.alg.tracker.klt.PkltConfig;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.util.ArrayList;
import java.util.HashMap;
import java.util.List;
import java.util.Map;

/** PointTracker<GrayF32> with the behaviour of FactoryPointTracker.klt(PkltConfig, ConfigGeneralDetector, GrayF32.class, GrayF32.class), or
 *  PointTracker<GrayU8> with that of klt(PkltConfig, ConfigGeneralDetector, GrayU8.class, GrayS16.class) (derivType null = GrayS16:
 *  GImageDerivativeOps.getDerivativeType): bhip_klt_create / bhip_klt_process_f32, or bhip_klt_create_u8 / bhip_klt_process_u8 -- the GrayU8 frame
 *  is uploaded as bytes, a quarter of the float upload, and pyramid and Sobel run on bytes / shorts
 *  (main/boofcv-geo/.../factory/feature/tracker/FactoryPointTracker.java:120-145 -> .../abst/feature/tracker/PointTrackerKltPyramid.java:139-348)
 *  over one bhip_klt with batch = 1: the pyramid, the EXTENDED-border Sobel layers, the Lucas-Kanade iterations, the template re-description,
 *  the Shi-Tomasi corners of spawnTracks() and the track lists stay on the device; a frame goes in, the lists come back.  PointTrack objects keep
 *  their identity (cookie, description) across frames by featureId.  Differences from the Java object (include/boofhip.h): addTrack is not offered
 *  (it assigns no featureId to look a track up by), ConfigGeneralDetector.maxFeatures > 0 is declined (RuntimeException: keep the Java tracker), and a
 *  track at one of the float round-off positions where KltTracker throws is dropped instead.  UNCOMPILED SOURCE. */
public class PointTrackerKltPyramidHip<T extends ImageGray<T>> implements PointTracker<T>, AutoCloseable {
	private final long ctx = BoofHipContext.create();
	private final PkltConfig config;
	private final ConfigGeneralDetector configExtract;
	private final boolean u8;
	private long klt;
	private int width, height;
	private boolean closed;
	private final Map<Long, PointTrack> tracks = new HashMap<>();

	/** the GrayF32 tracker, as before */
	public static PointTrackerKltPyramidHip<GrayF32> f32(PkltConfig config, ConfigGeneralDetector configExtract) {
		return new PointTrackerKltPyramidHip<>(config, configExtract, GrayF32.class);
	}

	/** imageType GrayF32.class (GrayF32 derivatives) or GrayU8.class (GrayS16 derivatives); any other type is declined: keep the Java tracker */
	public PointTrackerKltPyramidHip(PkltConfig config, ConfigGeneralDetector configExtract, Class<T> imageType) {
		if (imageType != (Class<?>)GrayF32.class && imageType != (Class<?>)GrayU8.class)
			throw new RuntimeException("only GrayF32 and GrayU8 sequences are tracked on the GPU");
		this.u8 = imageType == (Class<?>)GrayU8.class;
		this.config = config != null ? config : new PkltConfig();
		this.configExtract = configExtract != null ? configExtract : new ConfigGeneralDetector();
		if (this.configExtract.maxFeatures > 0 || !this.configExtract.useStrictRule || this.configExtract.detectMinimums || !this.configExtract.detectMaximums)
			throw new RuntimeException("only the strict maxima extractor without a feature limit is tracked on the GPU");
	}

	/** bhip_klt_cfg {int forbiddenBorder; float maxPerPixelError; int maxIterations; float minDeterminant, minPositionDelta;} -- KltConfig.java:32-49 */
	static ByteBuffer pack(KltConfig c) {
		ByteBuffer b = ByteBuffer.allocateDirect(20).order(ByteOrder.nativeOrder());
		b.putInt(c.forbiddenBorder).putFloat(c.maxPerPixelError).putInt(c.maxIterations).putFloat(c.minDeterminant).putFloat(c.minPositionDelta);
		return b;
	}

	private void create(int w, int h) {
		if (klt != 0) BoofHip.kltDestroy(klt);
		tracks.clear();
		long[] out = new long[1];
		// FactoryDetectPoint.createGeneral: ignoreBorder += radius; GeneralFeatureDetector: at least the intensity's border (Shi-Tomasi radius 1)
		int border = Math.max(configExtract.ignoreBorder + configExtract.radius, 1);
		BoofHip.check(ctx, u8
				? BoofHip.kltCreateU8(ctx, pack(config.config), config.templateRadius, config.pyramidScaling, config.pyramidScaling.length,
						configExtract.radius, configExtract.threshold, border, w, h, 1, out)
				: BoofHip.kltCreate(ctx, pack(config.config), config.templateRadius, config.pyramidScaling, config.pyramidScaling.length,
						configExtract.radius, configExtract.threshold, border, w, h, 1, out));
		klt = out[0];
		width = w;
		height = h;
	}

	@Override public void process(T image) {
		if (klt == 0 || image.width != width || image.height != height) create(image.width, image.height);
		if (u8) {
			GrayU8 g = (GrayU8)(Object)image;
			BoofHip.check(ctx, BoofHip.kltProcessU8(klt, new byte[][]{g.data}, new int[]{g.startIndex}, new int[]{g.stride}));
		} else {
			GrayF32 g = (GrayF32)(Object)image;
			BoofHip.check(ctx, BoofHip.kltProcessF32(klt, new float[][]{g.data}, new int[]{g.startIndex}, new int[]{g.stride}));
		}
	}

	@Override public void spawnTracks() {
		if (klt == 0) throw new IllegalArgumentException("process() has not been called");
		BoofHip.check(ctx, BoofHip.kltSpawn(klt, -1));
	}

	private List<PointTrack> fetch(int which, List<PointTrack> list) {
		if (list == null) list = new ArrayList<>();
		if (klt == 0) return list;
		int[][] n = new int[3][1];
		BoofHip.check(ctx, BoofHip.kltCounts(klt, n[0], n[1], n[2]));
		int count = n[which][0];
		if (count == 0) return list;
		long[] id = new long[count];
		float[] xy = new float[2 * count];
		BoofHip.check(ctx, BoofHip.kltFetch(klt, which, 0, id, xy, null, null));
		for (int i = 0; i < count; i++) {
			PointTrack p = tracks.get(id[i]);
			if (p == null) { p = new PointTrack(); p.featureId = id[i]; tracks.put(id[i], p); }
			p.set(xy[2 * i], xy[2 * i + 1]);
			list.add(p);
			if (which == 2) tracks.remove(id[i]);
		}
		return list;
	}

	@Override public List<PointTrack> getActiveTracks(List<PointTrack> list) { return fetch(0, list); }
	@Override public List<PointTrack> getNewTracks(List<PointTrack> list) { return fetch(1, list); }
	@Override public List<PointTrack> getDroppedTracks(List<PointTrack> list) { return fetch(2, list); }
	@Override public List<PointTrack> getAllTracks(List<PointTrack> list) { return getActiveTracks(list); }
	@Override public List<PointTrack> getInactiveTracks(List<PointTrack> list) { return list != null ? list : new ArrayList<PointTrack>(); }

	@Override public boolean dropTrack(PointTrack track) {
		if (klt == 0) return false;
		byte[] ok = new byte[1];
		BoofHip.check(ctx, BoofHip.kltDropTracks(klt, new int[]{0}, new long[]{track.featureId}, 1, ok));
		tracks.remove(track.featureId);
		return ok[0] != 0;
	}

	@Override public void dropAllTracks() {
		tracks.clear();
		if (klt != 0) BoofHip.check(ctx, BoofHip.kltDropAll(klt));
	}

	@Override public void reset() {
		tracks.clear();
		if (klt != 0) BoofHip.check(ctx, BoofHip.kltReset(klt));
	}

	@Override public void close() {
		if (closed) return;
		closed = true;
		if (klt != 0) BoofHip.kltDestroy(klt);
		BoofHip.ctxDestroy(ctx);
	}
}
