package boofcv.hip;

import boofcv.abst.feature.detect.extract.ConfigExtract;
import boofcv.abst.feature.detect.extract.NonMaxSuppression;
import boofcv.abst.filter.binary.InputToBinary;
import boofcv.alg.filter.blur.BOverrideBlurImageOps;
import boofcv.alg.filter.convolve.BOverrideConvolveImage;
import boofcv.alg.filter.convolve.BOverrideConvolveImageNormalized;
import boofcv.alg.filter.convolve.border.ConvolveJustBorder_General_SB;
import boofcv.core.image.border.ImageBorder_F32;
import boofcv.factory.feature.detect.extract.BOverrideFactoryFeatureExtractor;
import boofcv.factory.filter.binary.BOverrideFactoryThresholdBinary;
import boofcv.struct.ConfigLength;
import boofcv.struct.QueueCorner;
import boofcv.struct.convolve.Kernel1D_F32;
import boofcv.struct.convolve.Kernel2D_F32;
import boofcv.struct.image.GrayF32;
import boofcv.struct.image.GrayU8;
import boofcv.struct.image.ImageGray;

/**
 * Installs every BOverride hook the library implements (I:override/BOverrideManager.java:33-39 lists the hook classes).  A hook that throws
 * RuntimeException means "not handled, run the Java code" (BOverrideConvolveImage.java:53-62), which is what BoofHip.check does for any
 * non-zero status and what the type guards below do for images / kernels other than GrayF32 / Kernel*_F32 (the blurs also take GrayU8).
 * The hooks of BOverrideFactoryThresholdBinary have no such answer: they return an InputToBinary, the device's or the Java one
 * (FactoryThresholdBinaryHip).
 */
public final class BoofHipOverrides {
	private BoofHipOverrides() {}

	private static RuntimeException declined() { return new RuntimeException("boofhip: not handled"); }

	public static void install() {
		// ConvolveImage.horizontal/vertical/convolve(kernel, input, output, border) = no-border interior (GPU) + ConvolveJustBorder_General_SB (Java strip)
		BOverrideConvolveImage.horizontal = (kernel, input, output, border) -> {
			if (!(kernel instanceof Kernel1D_F32) || !(input instanceof GrayF32) || !(border instanceof ImageBorder_F32)) throw declined();
			Kernel1D_F32 k = (Kernel1D_F32)kernel; GrayF32 in = (GrayF32)input, out = (GrayF32)output;
			long ctx = BoofHipContext.get();
			BoofHip.check(ctx, BoofHip.convHF32(ctx, k.data, k.width, k.offset, in.data, in.startIndex, in.stride, in.width, in.height, out.data, out.startIndex, out.stride));
			((ImageBorder_F32)border).setImage(in);
			ConvolveJustBorder_General_SB.horizontal(k, (ImageBorder_F32)border, out);
		};
		BOverrideConvolveImage.vertical = (kernel, input, output, border) -> {
			if (!(kernel instanceof Kernel1D_F32) || !(input instanceof GrayF32) || !(border instanceof ImageBorder_F32)) throw declined();
			Kernel1D_F32 k = (Kernel1D_F32)kernel; GrayF32 in = (GrayF32)input, out = (GrayF32)output;
			long ctx = BoofHipContext.get();
			BoofHip.check(ctx, BoofHip.convVF32(ctx, k.data, k.width, k.offset, in.data, in.startIndex, in.stride, in.width, in.height, out.data, out.startIndex, out.stride));
			((ImageBorder_F32)border).setImage(in);
			ConvolveJustBorder_General_SB.vertical(k, (ImageBorder_F32)border, out);
		};
		BOverrideConvolveImage.convolve = (kernel, input, output, border) -> {
			if (!(kernel instanceof Kernel2D_F32) || !(input instanceof GrayF32) || !(border instanceof ImageBorder_F32)) throw declined();
			Kernel2D_F32 k = (Kernel2D_F32)kernel; GrayF32 in = (GrayF32)input, out = (GrayF32)output;
			long ctx = BoofHipContext.get();
			BoofHip.check(ctx, BoofHip.conv2dF32(ctx, k.data, k.width, k.offset, in.data, in.startIndex, in.stride, in.width, in.height, out.data, out.startIndex, out.stride));
			((ImageBorder_F32)border).setImage(in);
			ConvolveJustBorder_General_SB.convolve(k, (ImageBorder_F32)border, out);
		};
		// ConvolveImageNormalized.horizontal / vertical (the 2-D normalised form is not implemented on the GPU: left null = Java)
		BOverrideConvolveImageNormalized.horizontal = (kernel, input, output) -> {
			if (!(kernel instanceof Kernel1D_F32) || !(input instanceof GrayF32)) throw declined();
			Kernel1D_F32 k = (Kernel1D_F32)kernel; GrayF32 in = (GrayF32)input, out = (GrayF32)output;
			long ctx = BoofHipContext.get();
			BoofHip.check(ctx, BoofHip.convNormHF32(ctx, k.data, k.width, k.offset, in.data, in.startIndex, in.stride, in.width, in.height, out.data, out.startIndex, out.stride));
		};
		BOverrideConvolveImageNormalized.vertical = (kernel, input, output) -> {
			if (!(kernel instanceof Kernel1D_F32) || !(input instanceof GrayF32)) throw declined();
			Kernel1D_F32 k = (Kernel1D_F32)kernel; GrayF32 in = (GrayF32)input, out = (GrayF32)output;
			long ctx = BoofHipContext.get();
			BoofHip.check(ctx, BoofHip.convNormVF32(ctx, k.data, k.width, k.offset, in.data, in.startIndex, in.stride, in.width, in.height, out.data, out.startIndex, out.stride));
		};
		// BlurImageOps.mean / median / gaussian (BOverrideBlurImageOps.java:36-50)
		BOverrideBlurImageOps.mean = (input, output, radiusX, radiusY, storage) -> {
			if (input instanceof GrayU8) {   // BlurImageOps.mean(GrayU8): both passes round to bytes
				GrayU8 in = (GrayU8)input, out = (GrayU8)output;
				long ctx = BoofHipContext.get();
				BoofHip.check(ctx, BoofHip.meanU8(ctx, in.data, in.startIndex, in.stride, in.width, in.height, radiusX, radiusY, out.data, out.startIndex, out.stride));
				return;
			}
			if (!(input instanceof GrayF32)) throw declined();
			GrayF32 in = (GrayF32)input, out = (GrayF32)output;
			long ctx = BoofHipContext.get();
			BoofHip.check(ctx, BoofHip.meanF32(ctx, in.data, in.startIndex, in.stride, in.width, in.height, radiusX, radiusY, out.data, out.startIndex, out.stride));
		};
		BOverrideBlurImageOps.median = (input, output, radius) -> {
			if (!(input instanceof GrayF32)) throw declined();
			GrayF32 in = (GrayF32)input, out = (GrayF32)output;
			long ctx = BoofHipContext.get();
			BoofHip.check(ctx, BoofHip.medianF32(ctx, in.data, in.startIndex, in.stride, in.width, in.height, radius, out.data, out.startIndex, out.stride));
		};
		BOverrideBlurImageOps.gaussian = (input, output, sigmaX, radiusX, sigmaY, radiusY, storage) -> {
			if (input instanceof GrayU8) {   // the C ABI has the kernel FactoryKernelGaussian derives from the radius (sigma <= 0)
				if (sigmaX > 0 || sigmaY > 0 || radiusX != radiusY || radiusX <= 0) throw declined();
				GrayU8 in = (GrayU8)input, out = (GrayU8)output;
				long ctx = BoofHipContext.get();
				BoofHip.check(ctx, BoofHip.gaussianU8(ctx, in.data, in.startIndex, in.stride, in.width, in.height, radiusX, out.data, out.startIndex, out.stride));
				return;
			}
			if (!(input instanceof GrayF32) || sigmaX != sigmaY || radiusX != radiusY) throw declined();   // the C ABI has the isotropic form
			GrayF32 in = (GrayF32)input, out = (GrayF32)output;
			long ctx = BoofHipContext.get();
			BoofHip.check(ctx, BoofHip.gaussianF32(ctx, in.data, in.startIndex, in.stride, in.width, in.height, sigmaX, radiusX, out.data, out.startIndex, out.stride));
		};
		// FactoryFeatureExtractor.nonmax(ConfigExtract): the strict Max / Min / MinMax searches (relaxed rule / candidate lists stay on the Java path)
		BOverrideFactoryFeatureExtractor.nonmax = (ConfigExtract config) -> {
			config.checkValidity();
			if (!config.useStrictRule) throw declined();
			return new NonMaxHip(config);
		};
		// FactoryThresholdBinary: the types FactoryThresholdBinaryHip runs on the device.  Their handle methods are generic, hence classes, not lambdas.
		// globalOtsu stays unset: the factory does not pass `scale` to that hook (FactoryThresholdBinary.java:277-281).
		BOverrideFactoryThresholdBinary.globalFixed = new BOverrideFactoryThresholdBinary.GlobalFixed() {
			@Override public <T extends ImageGray<T>> InputToBinary<T> handle(double threshold, boolean down, Class<T> inputType) {
				return FactoryThresholdBinaryHip.globalFixed(threshold, down, inputType);
			}
		};
		BOverrideFactoryThresholdBinary.localMean = new BOverrideFactoryThresholdBinary.LocalMean() {
			@Override public <T extends ImageGray<T>> InputToBinary<T> handle(ConfigLength regionWidth, double scale, boolean down, Class<T> inputType) {
				return FactoryThresholdBinaryHip.localMean(regionWidth, scale, down, inputType);
			}
		};
		BOverrideFactoryThresholdBinary.localGaussian = new BOverrideFactoryThresholdBinary.LocalGaussian() {
			@Override public <T extends ImageGray<T>> InputToBinary<T> handle(ConfigLength regionWidth, double scale, boolean down, Class<T> inputType) {
				return FactoryThresholdBinaryHip.localGaussian(regionWidth, scale, down, inputType);
			}
		};
		BOverrideFactoryThresholdBinary.blockMinMax = new BOverrideFactoryThresholdBinary.LocalBlockMinMax() {
			@Override public <T extends ImageGray<T>> InputToBinary<T> handle(ConfigLength regionWidth, double scale, boolean down, double minimumSpread,
																			  boolean thresholdFromLocalBlocks, Class<T> inputType) {
				return FactoryThresholdBinaryHip.blockMinMax(regionWidth, scale, down, minimumSpread, thresholdFromLocalBlocks, inputType);
			}
		};
		BOverrideFactoryThresholdBinary.blockMean = new BOverrideFactoryThresholdBinary.LocalBlockMean() {
			@Override public <T extends ImageGray<T>> InputToBinary<T> handle(ConfigLength regionWidth, double scale, boolean down, boolean thresholdFromLocalBlocks,
																			  Class<T> inputType) {
				return FactoryThresholdBinaryHip.blockMean(regionWidth, scale, down, thresholdFromLocalBlocks, inputType);
			}
		};
		BOverrideFactoryThresholdBinary.blockOtsu = new BOverrideFactoryThresholdBinary.LocalBlockOtsu() {
			@Override public <T extends ImageGray<T>> InputToBinary<T> handle(boolean otsu2, ConfigLength regionWidth, double tuning, double scale, boolean down,
																			  boolean thresholdFromLocalBlocks, Class<T> inputType) {
				return FactoryThresholdBinaryHip.blockOtsu(otsu2, regionWidth, tuning, scale, down, thresholdFromLocalBlocks, inputType);
			}
		};
	}

	/** NonMaxSuppression over bhip_nonmax_block_f32 / bhip_nonmax_block_minmax_f32 (NonMaxBlock.process with the strict Max / Min / MinMax search,
	 *  block-raster order).  As in FactoryFeatureExtractor.nonmax, a config without maximums gets the Min search and thresholdMin starts at -threshold. */
	static final class NonMaxHip implements NonMaxSuppression {
		private int radius, border; private float thresholdMax, thresholdMin;
		private final boolean detectMin, detectMax;
		private short[] xyMin = new short[0], xyMax = new short[0];
		private final int[] nMin = new int[1], nMax = new int[1];
		NonMaxHip(ConfigExtract c) {
			radius = c.radius; border = c.ignoreBorder; thresholdMax = c.threshold; thresholdMin = -c.threshold;
			detectMax = c.detectMaximums; detectMin = c.detectMinimums || !c.detectMaximums;
		}

		@Override public void process(GrayF32 intensity, QueueCorner candidateMin, QueueCorner candidateMax, QueueCorner foundMin, QueueCorner foundMax) {
			long ctx = BoofHipContext.get();
			int step = radius + 1;
			int cap = Math.max(1, ((intensity.width - 2*border + step - 1)/step)*((intensity.height - 2*border + step - 1)/step));
			if (xyMax.length < 2*cap) xyMax = new short[2*cap];
			if (detectMin && xyMin.length < 2*cap) xyMin = new short[2*cap];
			nMin[0] = nMax[0] = 0;
			if (detectMin)
				BoofHip.check(ctx, BoofHip.nonmaxBlockMinmaxF32(ctx, intensity.data, intensity.startIndex, intensity.stride, intensity.width, intensity.height, radius,
						thresholdMin, thresholdMax, border, 1, detectMax ? 1 : 0, xyMin, nMin, xyMax, nMax, cap));
			else
				BoofHip.check(ctx, BoofHip.nonmaxBlockF32(ctx, intensity.data, intensity.startIndex, intensity.stride, intensity.width, intensity.height, radius,
						thresholdMax, border, xyMax, cap, nMax));
			if (foundMin != null) {   // NonMaxBlock.process resets the lists it is given
				foundMin.reset();
				for (int i = 0; i < nMin[0]; i++) foundMin.add(xyMin[2*i], xyMin[2*i + 1]);
			}
			if (foundMax != null) {
				foundMax.reset();
				for (int i = 0; i < nMax[0]; i++) foundMax.add(xyMax[2*i], xyMax[2*i + 1]);
			}
		}
		@Override public boolean getUsesCandidates() { return false; }
		@Override public float getThresholdMinimum() { return thresholdMin; }
		@Override public float getThresholdMaximum() { return thresholdMax; }
		@Override public void setThresholdMinimum(float t) { thresholdMin = t; }
		@Override public void setThresholdMaximum(float t) { thresholdMax = t; }
		@Override public void setIgnoreBorder(int b) { border = b; }
		@Override public int getIgnoreBorder() { return border; }
		@Override public void setSearchRadius(int r) { radius = r; }
		@Override public int getSearchRadius() { return radius; }
		@Override public boolean canDetectMaximums() { return detectMax; }
		@Override public boolean canDetectMinimums() { return detectMin; }
	}
}
