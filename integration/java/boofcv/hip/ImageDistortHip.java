package boofcv.hip;

import boofcv.alg.distort.ImageDistort;
import boofcv.alg.distort.PixelTransformAffine_F32;
import boofcv.alg.distort.PixelTransformHomography_F32;
import boofcv.alg.distort.PointToPixelTransform_F32;
import boofcv.alg.distort.PointTransformHomography_F32;
import boofcv.alg.interpolate.InterpolationType;
import boofcv.struct.border.BorderType;
import boofcv.struct.distort.PixelTransform;
import boofcv.struct.distort.Point2Transform2_F32;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;
import georegression.struct.affine.Affine2D_F32;
import georegression.struct.homography.Homography2D_F32;
import georegression.struct.point.Point2D_F32;

/** ImageDistort&lt;T,T&gt; for T = GrayU8 or GrayF32 as FactoryDistort.distortSB(cached, interp, type) builds it
 *  (main/boofcv-ip/.../factory/distort/FactoryDistort.java:96-122) with interp = FactoryInterpolation.createPixelS(0, 255, NEAREST_NEIGHBOR |
 *  BILINEAR, ZERO | EXTENDED, type), with the three apply() forms on the device.  The reference has no hook for this factory, so the class is
 *  constructed where FactoryDistort.distortSB / DistortImageOps.distortSingle would be called:
 *      ImageDistort&lt;GrayU8,GrayU8&gt; d = new ImageDistortHip&lt;&gt;(GrayU8.class, InterpolationType.BILINEAR, BorderType.EXTENDED, false);
 *      d.setRenderAll(!skip); d.setModel(transform); d.apply(input, output);
 *  setModel: a PixelTransformAffine_F32, a PixelTransformHomography_F32, or a PointToPixelTransform_F32 over a PointTransformHomography_F32
 *  is evaluated in the kernel when cached is false (bhip_distort_model_u8 / _f32).  The formulas of that path are the library's own statement
 *  of georegression's AffinePointOps_F32 / HomographyPointOps_F32 (include/boofhip.h); a caller who needs bit equality with
 *  ImageDistortBasic_SB constructs with cached = true.  Every other transform, and cached = true, fills a map with dstToSrc.compute once per
 *  setModel / destination size, as ImageDistortCache_SB.init does (ImageDistortCache_SB.java:111-134), and runs bhip_distort_map_u8 / _f32:
 *  bit for bit the single-threaded Java result.  Deviations (include/boofhip.h): the map is indexed by y*width + x for every destination
 *  layout; source, destination and mask must not overlap.  What the device does not have (BICUBIC, POLYNOMIAL4, REFLECT, WRAP, NORMALIZED,
 *  other image types) makes the constructor or check() throw RuntimeException, and the caller uses the Java path.
 *  PointToPixelTransform_F32 keeps its point transform in a package-private field: the patch adds the one-line accessor
 *  `public Point2Transform2_F32 getTransform() { return alg; }` to it.
 *  UNCOMPILED SOURCE. */
public class ImageDistortHip<T extends ImageGray<T>> implements ImageDistort<T, T> {
	private static final int MODEL_AFFINE = 1, MODEL_HOMOGRAPHY = 2;   // BHIP_DISTORT_*

	private final Class<T> type;
	private final int interp, border;   // BHIP_INTERP_* / BHIP_BORDER_*: the enums' ordinals
	private final boolean cached;
	private PixelTransform<Point2D_F32> dstToSrc;
	private boolean renderAll = true;
	private int model;                  // 0: the map form
	private float[] coeff;
	private float[] map;
	private int mapWidth, mapHeight;
	private boolean dirty = true;

	public ImageDistortHip(Class<T> type, InterpolationType interpType, BorderType borderType, boolean cached) {
		if (type != GrayU8.class && type != GrayF32.class) throw new RuntimeException("only GrayU8 and GrayF32 are distorted on the device");
		if (interpType != InterpolationType.NEAREST_NEIGHBOR && interpType != InterpolationType.BILINEAR)
			throw new RuntimeException(interpType + " interpolation does not run on the device");
		if (borderType != BorderType.ZERO && borderType != BorderType.EXTENDED) throw new RuntimeException("border " + borderType + " does not run on the device");
		this.type = type;
		this.interp = interpType.ordinal();
		this.border = borderType.ordinal();
		this.cached = cached;
	}

	@Override public void setModel(PixelTransform<Point2D_F32> dstToSrc) {
		this.dstToSrc = dstToSrc;
		dirty = true;
		model = 0;
		coeff = null;
		if (cached) return;
		if (dstToSrc.getClass() == PixelTransformAffine_F32.class) {
			Affine2D_F32 a = ((PixelTransformAffine_F32)dstToSrc).getModel();
			model = MODEL_AFFINE;
			coeff = new float[]{a.a11, a.a12, a.a21, a.a22, a.tx, a.ty};
		} else if (dstToSrc.getClass() == PixelTransformHomography_F32.class) {
			setHomography(((PixelTransformHomography_F32)dstToSrc).getModel());
		} else if (dstToSrc.getClass() == PointToPixelTransform_F32.class) {
			Point2Transform2_F32 p = ((PointToPixelTransform_F32)dstToSrc).getTransform();
			if (p != null && p.getClass() == PointTransformHomography_F32.class) setHomography(((PointTransformHomography_F32)p).getModel());
		}
	}

	private void setHomography(Homography2D_F32 h) {
		model = MODEL_HOMOGRAPHY;
		coeff = new float[]{h.a11, h.a12, h.a13, h.a21, h.a22, h.a23, h.a31, h.a32, h.a33};
	}

	@Override public void apply(T srcImg, T dstImg) { run(srcImg, dstImg, null, 0, 0, dstImg.width, dstImg.height); }

	@Override public void apply(T srcImg, T dstImg, GrayU8 mask) { run(srcImg, dstImg, mask, 0, 0, dstImg.width, dstImg.height); }

	@Override public void apply(T srcImg, T dstImg, int dstX0, int dstY0, int dstX1, int dstY1) { run(srcImg, dstImg, null, dstX0, dstY0, dstX1, dstY1); }

	private void run(T src, T dst, GrayU8 mask, int x0, int y0, int x1, int y1) {
		if (mask != null && (mask.width != dst.width || mask.height != dst.height)) throw new IllegalArgumentException("the mask has the destination's size");
		final long ctx = BoofHipContext.get();
		final int ra = renderAll ? 1 : 0;
		final byte[] m = mask == null ? null : mask.data;
		final int ms = mask == null ? 0 : mask.startIndex, mt = mask == null ? 0 : mask.stride;
		if (model == 0) fillMap(dst.width, dst.height);
		if (type == GrayU8.class) {
			GrayU8 s = (GrayU8)(ImageGray)src, d = (GrayU8)(ImageGray)dst;
			BoofHip.check(ctx, model != 0
					? BoofHip.distortModelU8(ctx, s.data, s.startIndex, s.stride, s.width, s.height, model, coeff, d.width, d.height, x0, y0, x1, y1, interp, border, ra,
							d.data, d.startIndex, d.stride, m, ms, mt)
					: BoofHip.distortMapU8(ctx, s.data, s.startIndex, s.stride, s.width, s.height, map, d.width, d.height, x0, y0, x1, y1, interp, border, ra,
							d.data, d.startIndex, d.stride, m, ms, mt));
		} else {
			GrayF32 s = (GrayF32)(ImageGray)src, d = (GrayF32)(ImageGray)dst;
			BoofHip.check(ctx, model != 0
					? BoofHip.distortModelF32(ctx, s.data, s.startIndex, s.stride, s.width, s.height, model, coeff, d.width, d.height, x0, y0, x1, y1, interp, border, ra,
							d.data, d.startIndex, d.stride, m, ms, mt)
					: BoofHip.distortMapF32(ctx, s.data, s.startIndex, s.stride, s.width, s.height, map, d.width, d.height, x0, y0, x1, y1, interp, border, ra,
							d.data, d.startIndex, d.stride, m, ms, mt));
		}
	}

	/** ImageDistortCache_SB.init: the transform at every destination pixel, once per setModel / destination size */
	private void fillMap(int width, int height) {
		if (!dirty && map != null && mapWidth == width && mapHeight == height) return;
		if (map == null || map.length != 2*width*height) map = new float[2*width*height];
		Point2D_F32 p = new Point2D_F32();
		int i = 0;
		for (int y = 0; y < height; y++)
			for (int x = 0; x < width; x++) {
				dstToSrc.compute(x, y, p);
				map[i++] = p.x;
				map[i++] = p.y;
			}
		mapWidth = width;
		mapHeight = height;
		dirty = false;
	}

	@Override public void setRenderAll(boolean renderAll) { this.renderAll = renderAll; }
	@Override public boolean getRenderAll() { return renderAll; }
	@Override public PixelTransform<Point2D_F32> getModel() { return dstToSrc; }
}
