package boofcv.hip;

import boofcv.alg.background.stationary.BackgroundStationaryBasic;
import boofcv.alg.background.stationary.BackgroundStationaryGaussian;
import boofcv.alg.background.stationary.BackgroundStationaryGmm;
import boofcv.factory.background.ConfigBackgroundBasic;
import boofcv.factory.background.ConfigBackgroundGaussian;
import boofcv.factory.background.ConfigBackgroundGmm;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageBase;
import boofcv.struct.image.ImageGray;
import boofcv.struct.image.ImageType;
import boofcv.struct.image.Planar;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

/** FactoryBackgroundModel.stationaryBasic / stationaryGaussian / stationaryGmm (main/boofcv-feature/.../factory/background/
 *  FactoryBackgroundModel.java:47-64,112-141,193-225) returning the classes of this package, whose updateBackground / segment run on the device
 *  (bhip_bg_* of include/boofhip.h).  The reference has no hook for this factory, so it is called where FactoryBackgroundModel would be:
 *      BackgroundModelStationary&lt;GrayU8&gt; bg = FactoryBackgroundModelHip.stationaryGmm(null, ImageType.single(GrayU8.class));
 *  GrayU8 / GrayF32 and Planar of 1..4 such bands; interleaved images, other pixel types, more than 8 Gaussians and the moving* models throw
 *  RuntimeException: the caller uses FactoryBackgroundModel.  Same rules as there: stationaryBasic does not forward config.unknownValue.
 *  UNCOMPILED SOURCE. */
public class FactoryBackgroundModelHip {
	public static <T extends ImageBase<T>> BackgroundStationaryBasic<T> stationaryBasic(ConfigBackgroundBasic config, ImageType<T> imageType) {
		config.checkValidity();
		return new BackgroundStationaryBasicHip<>(config.learnRate, config.threshold, imageType);
	}

	public static <T extends ImageBase<T>> BackgroundStationaryGaussian<T> stationaryGaussian(ConfigBackgroundGaussian config, ImageType<T> imageType) {
		config.checkValidity();
		BackgroundStationaryGaussian<T> ret = new BackgroundStationaryGaussianHip<>(config.learnRate, config.threshold, imageType);
		ret.setInitialVariance(config.initialVariance);
		ret.setMinimumDifference(config.minimumDifference);
		ret.setUnknownValue(config.unknownValue);
		return ret;
	}

	public static <T extends ImageBase<T>> BackgroundStationaryGmm<T> stationaryGmm(ConfigBackgroundGmm config, ImageType<T> imageType) {
		if (config == null) config = new ConfigBackgroundGmm();
		else config.checkValidity();
		BackgroundStationaryGmm<T> ret = new BackgroundStationaryGmmHip<>(config.learningPeriod, config.decayCoefient, config.numberOfGaussian, imageType);
		ret.setInitialVariance(config.initialVariance);
		ret.setMaxDistance(config.maxDistance);
		ret.setSignificantWeight(config.significantWeight);
		ret.setUnknownValue(config.unknownValue);
		return ret;
	}

	/** One bhip_bg with one stream for frames of one size: what the three classes share.  The handle has a fixed frame size, so it is replaced
	 *  when the reference would re-initialise for another size. */
	static class Native {
		static final int BASIC = 0, GAUSSIAN = 1, GMM = 2;
		final int alg, family, pixel, bands;
		long handle;
		int width, height;

		Native(int alg, ImageType<?> type) {
			this.alg = alg;
			if (type.getFamily() == ImageType.Family.INTERLEAVED) throw new RuntimeException("interleaved images do not run on the device");
			Class<?> band = type.getImageClass();
			if (band != GrayU8.class && band != GrayF32.class) throw new RuntimeException("only GrayU8 and GrayF32 bands run on the device");
			family = type.getFamily() == ImageType.Family.GRAY ? 0 : 1;
			pixel = band == GrayU8.class ? 0 : 1;
			bands = family == 0 ? 0 : type.getNumBands();
			if (bands > 4) throw new RuntimeException("at most 4 bands run on the device");
		}

		/** the handle for width x height frames; cfg: the algorithm's config struct (bhip_bg_*_cfg).  true: a new handle was created */
		boolean open(ByteBuffer cfg, int w, int h) {
			if (handle != 0 && width == w && height == h) return false;
			close();
			long ctx = BoofHipContext.get();
			long[] out = new long[1];
			int st = alg == BASIC ? BoofHip.bgCreateBasic(ctx, cfg, family, pixel, bands, w, h, 1, out)
					: alg == GAUSSIAN ? BoofHip.bgCreateGaussian(ctx, cfg, family, pixel, bands, w, h, 1, out)
					: BoofHip.bgCreateGmm(ctx, cfg, family, pixel, bands, w, h, 1, out);
			BoofHip.check(ctx, st);
			handle = out[0];
			width = w;
			height = h;
			return true;
		}

		void close() {
			if (handle != 0) BoofHip.bgDestroy(handle);
			handle = 0;
		}

		static ByteBuffer struct(int bytes) { return ByteBuffer.allocateDirect(bytes).order(ByteOrder.nativeOrder()); }

		/** updateBackground(frame[, mask]) (segment == false) or segment(frame, mask) */
		@SuppressWarnings("rawtypes")
		void call(boolean segment, ImageBase frame, GrayU8 mask) {
			long ctx = BoofHipContext.get();
			byte[] m = mask == null ? null : mask.data;
			long ms = mask == null ? 0 : mask.startIndex;
			int mst = mask == null ? 0 : mask.stride;
			int st;
			if (frame instanceof Planar) {   // the bands are arrays of their own: one dense [band][y][x] copy
				Planar p = (Planar)frame;
				int n = width*height;
				if (pixel == 0) {
					byte[] all = new byte[n*bands];
					for (int b = 0; b < bands; b++) copyRows(((GrayU8)p.getBand(b)).data, (ImageGray)p.getBand(b), all, b*n);
					st = segment ? BoofHip.bgSegmentU8(handle, all, 0, 0, n, width, m, ms, 0, mst)
							: BoofHip.bgUpdateU8(handle, all, 0, 0, 0, n, width, 1, m, ms, 0, 0, mst);
				} else {
					float[] all = new float[n*bands];
					for (int b = 0; b < bands; b++) copyRows(((GrayF32)p.getBand(b)).data, (ImageGray)p.getBand(b), all, b*n);
					st = segment ? BoofHip.bgSegmentF32(handle, all, 0, 0, n, width, m, ms, 0, mst)
							: BoofHip.bgUpdateF32(handle, all, 0, 0, 0, n, width, 1, m, ms, 0, 0, mst);
				}
			} else if (pixel == 0) {
				GrayU8 g = (GrayU8)frame;
				st = segment ? BoofHip.bgSegmentU8(handle, g.data, g.startIndex, 0, 0, g.stride, m, ms, 0, mst)
						: BoofHip.bgUpdateU8(handle, g.data, g.startIndex, 0, 0, 0, g.stride, 1, m, ms, 0, 0, mst);
			} else {
				GrayF32 g = (GrayF32)frame;
				st = segment ? BoofHip.bgSegmentF32(handle, g.data, g.startIndex, 0, 0, g.stride, m, ms, 0, mst)
						: BoofHip.bgUpdateF32(handle, g.data, g.startIndex, 0, 0, 0, g.stride, 1, m, ms, 0, 0, mst);
			}
			BoofHip.check(ctx, st);
		}

		@SuppressWarnings("rawtypes")
		private void copyRows(Object src, ImageGray img, Object dst, int at) {
			for (int y = 0; y < height; y++) System.arraycopy(src, img.startIndex + y*img.stride, dst, at + y*width, width);
		}

		float[] fetch(int floats) {
			float[] out = new float[floats];
			BoofHip.check(BoofHipContext.get(), BoofHip.bgFetchModel(handle, 0, out));
			return out;
		}
	}
}
