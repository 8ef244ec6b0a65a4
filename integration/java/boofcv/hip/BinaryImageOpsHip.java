package boofcv.hip;

import boofcv.alg.InputSanityCheck;
import boofcv.struct.ConnectRule;
import boofcv.struct.image.GrayS32;
import boofcv.struct.image.GrayU8;

/** The pixel operations of BinaryImageOps (main/boofcv-ip/.../alg/filter/binary/BinaryImageOps.java) and the labelled image of its contour(), over
 *  the bhip_binary_* / bhip_label_* / bhip_relabel_* exports.  The reference has no BOverride hook for BinaryImageOps, so this is a provider class
 *  with the same static signatures: call BinaryImageOpsHip.erode8(...) where the code called BinaryImageOps.erode8(...).  Results are bit for
 *  bit those of the single-threaded Java methods on images of 0 and 1.
 *  Differences: the neighbourhood operations refuse an output that overlaps the input (IllegalArgumentException); relabel leaves a pixel outside
 *  the table unchanged and labelToBinary turns one into 0, where the reference throws ArrayIndexOutOfBoundsException; contourLabels returns the
 *  number of blobs and fills the labelled image, the ordered contour point lists of contour() stay with the Java implementation.
 *  Not provided: thin, contour / contourExternal point lists, labelToClusters, clusterToBinary, other image types.
 *  UNCOMPILED SOURCE. */
public final class BinaryImageOpsHip {
	private BinaryImageOpsHip() {}

	// BHIP_LOGIC_*, BHIP_MORPH_*, BHIP_CONNECT_* of include/boofhip.h
	private static final int AND = 0, OR = 1, XOR = 2;
	private static final int ERODE4 = 0, DILATE4 = 1, ERODE8 = 2, DILATE8 = 3;

	private static int rule(ConnectRule rule) { return rule == ConnectRule.FOUR ? 4 : 8; }

	private static GrayU8 logic(int op, GrayU8 inputA, GrayU8 inputB, GrayU8 output) {
		InputSanityCheck.checkSameShape(inputA, inputB);
		output = InputSanityCheck.checkDeclare(inputA, output);
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.binaryLogicU8(ctx, op, inputA.data, inputA.startIndex, inputA.stride, inputB.data, inputB.startIndex, inputB.stride, inputA.width,
				inputA.height, output.data, output.startIndex, output.stride));
		return output;
	}

	public static GrayU8 logicAnd(GrayU8 inputA, GrayU8 inputB, GrayU8 output) { return logic(AND, inputA, inputB, output); }

	public static GrayU8 logicOr(GrayU8 inputA, GrayU8 inputB, GrayU8 output) { return logic(OR, inputA, inputB, output); }

	public static GrayU8 logicXor(GrayU8 inputA, GrayU8 inputB, GrayU8 output) { return logic(XOR, inputA, inputB, output); }

	public static GrayU8 invert(GrayU8 input, GrayU8 output) {
		output = InputSanityCheck.checkDeclare(input, output);
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.binaryInvertU8(ctx, input.data, input.startIndex, input.stride, input.width, input.height, output.data, output.startIndex, output.stride));
		return output;
	}

	private static GrayU8 morph(int op, GrayU8 input, int numTimes, GrayU8 output) {
		output = InputSanityCheck.checkDeclare(input, output);
		if (op == ERODE4 && numTimes <= 0) throw new IllegalArgumentException("numTimes must be >= 1");
		if (output.data == input.data) throw new IllegalArgumentException("input and output must not share their array");
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.binaryMorphU8(ctx, op, numTimes, input.data, input.startIndex, input.stride, input.width, input.height, output.data, output.startIndex,
				output.stride));
		return output;
	}

	public static GrayU8 erode4(GrayU8 input, int numTimes, GrayU8 output) { return morph(ERODE4, input, numTimes, output); }

	public static GrayU8 dilate4(GrayU8 input, int numTimes, GrayU8 output) { return morph(DILATE4, input, numTimes, output); }

	public static GrayU8 erode8(GrayU8 input, int numTimes, GrayU8 output) { return morph(ERODE8, input, numTimes, output); }

	public static GrayU8 dilate8(GrayU8 input, int numTimes, GrayU8 output) { return morph(DILATE8, input, numTimes, output); }

	private static GrayU8 edge(int rule, GrayU8 input, GrayU8 output, boolean outsideZero) {
		output = InputSanityCheck.checkDeclare(input, output);
		if (output.data == input.data) throw new IllegalArgumentException("input and output must not share their array");
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.binaryEdgeU8(ctx, rule, outsideZero ? 1 : 0, input.data, input.startIndex, input.stride, input.width, input.height, output.data,
				output.startIndex, output.stride));
		return output;
	}

	public static GrayU8 edge4(GrayU8 input, GrayU8 output, boolean outsideZero) { return edge(4, input, output, outsideZero); }

	public static GrayU8 edge8(GrayU8 input, GrayU8 output, boolean outsideZero) { return edge(8, input, output, outsideZero); }

	public static GrayU8 removePointNoise(GrayU8 input, GrayU8 output) {
		output = InputSanityCheck.checkDeclare(input, output);
		if (output.data == input.data) throw new IllegalArgumentException("input and output must not share their array");
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.binaryRemovePointNoiseU8(ctx, input.data, input.startIndex, input.stride, input.width, input.height, output.data, output.startIndex,
				output.stride));
		return output;
	}

	/** The labelled image and getContours().size of BinaryImageOps.contour(input, rule, output); the point lists are not produced.
	 *  @return the number of blobs; output holds 0 for background and 1..N in the raster order of each blob's first pixel */
	public static int contourLabels(GrayU8 input, ConnectRule rule, GrayS32 output) {
		if (output == null) throw new IllegalArgumentException("the labelled image is the result: pass one");
		InputSanityCheck.checkSameShape(input, output);
		final long ctx = BoofHipContext.get();
		int[] numBlobs = new int[1];
		BoofHip.check(ctx, BoofHip.labelBlobsU8S32(ctx, rule(rule), input.data, input.startIndex, input.stride, input.width, input.height, output.data, output.startIndex,
				output.stride, numBlobs));
		return numBlobs[0];
	}

	public static void relabel(GrayS32 input, int[] labels) {
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.relabelS32(ctx, input.data, input.startIndex, input.stride, input.width, input.height, labels, labels.length));
	}

	public static GrayU8 labelToBinary(GrayS32 labelImage, GrayU8 binaryImage) {
		binaryImage = InputSanityCheck.checkDeclare(labelImage, binaryImage, GrayU8.class);
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.labelToBinaryS32U8(ctx, labelImage.data, labelImage.startIndex, labelImage.stride, labelImage.width, labelImage.height,
				binaryImage.data, binaryImage.startIndex, binaryImage.stride, null, 0));
		return binaryImage;
	}

	public static GrayU8 labelToBinary(GrayS32 labelImage, GrayU8 binaryImage, boolean[] selectedBlobs) {
		binaryImage = InputSanityCheck.checkDeclare(labelImage, binaryImage, GrayU8.class);
		byte[] selected = new byte[selectedBlobs.length];
		for (int i = 0; i < selected.length; i++) selected[i] = (byte)(selectedBlobs[i] ? 1 : 0);
		final long ctx = BoofHipContext.get();
		BoofHip.check(ctx, BoofHip.labelToBinaryS32U8(ctx, labelImage.data, labelImage.startIndex, labelImage.stride, labelImage.width, labelImage.height,
				binaryImage.data, binaryImage.startIndex, binaryImage.stride, selected, selected.length));
		return binaryImage;
	}

	public static GrayU8 labelToBinary(GrayS32 labelImage, GrayU8 binaryImage, int numLabels, int... selected) {
		boolean[] selectedBlobs = new boolean[numLabels];
		for (int i = 0; i < selected.length; i++) selectedBlobs[selected[i]] = true;
		return labelToBinary(labelImage, binaryImage, selectedBlobs);
	}
}
