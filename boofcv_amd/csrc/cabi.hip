// C ABI of libboofhip.so (include/boofhip.h): context, the SURF detect+describe object, association, stage-level entry points.
// Host orchestration only -- all arithmetic lives in the kernels.  There is deliberately no CPU fallback.
// This file: the context and the handle registry, the Fast-Hessian detector and the SURF / BRIEF detect+describe object (bhip_surf).  The
// other families: cabi_detect.hip, cabi_assoc.hip, cabi_ip.hip, cabi_ops.hip, cabi_klt.hip, cabi_bg.hip; what the files share: cabi.h.
#include "cabi.h"

HandleRegistry& registry() {
	static HandleRegistry* r = [] {
		HandleRegistry* p = new HandleRegistry();
		atexit([] { registry().exiting = true; });   // registered after the HIP runtime loaded, so it runs before the runtime's teardown
		return p;
	}();
	return *r;
}

static int ctxCreate(int device, void* stream, bool useGiven, bhip_ctx** out) {
	if (!out) return BHIP_ERR_INVALID;
	*out = nullptr;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return BHIP_ERR_HIP;  // no GPU: fail loudly, never fall back
	if (device < 0 || device >= count) return BHIP_ERR_INVALID;
	if (hipSetDevice(device) != hipSuccess) return BHIP_ERR_HIP;
	std::unique_ptr<bhip_ctx_full> ctx(new (std::nothrow) bhip_ctx_full());
	if (!ctx) return BHIP_ERR_NOMEM;
	ctx->device = device;
	if (hipDeviceGetAttribute(&ctx->cuCount, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ctx->cuCount <= 0) return BHIP_ERR_HIP;
	if (useGiven) {
		ctx->stream = (hipStream_t)stream;
	} else {
		if (hipStreamCreateWithFlags(&ctx->ownedStream.h, hipStreamNonBlocking) != hipSuccess) return BHIP_ERR_HIP;
		ctx->stream = ctx->ownedStream;
	}
	if (ctx->hostScratch.reserve(ctx.get(), 1 << 20) != BHIP_OK) return BHIP_ERR_HIP;
	HandleRegistry& R = registry();
	std::lock_guard<std::mutex> lock(R.m);
	R.ctxs.insert(ctx.get());
	*out = ctx.release();
	return BHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Fast-Hessian detector: octave schedule + buffers (FastHessianFeatureDetector.detect :156-188, detectOctave :198-221)
// ---------------------------------------------------------------------------------------------------------------
struct FhLevelPlan {
	DetectLevelParams p;
	int level;  // index of the mid level inside its octave
};
struct FhOctavePlan {
	int skip, w, h, nlevels;
	int sizes[BHIP_MAX_LEVELS];
	std::vector<FhLevelPlan> mids;
	// execution plan (FhDetector::planExecution)
	bool fused = false, fixed = false;
	int shareFrom[BHIP_MAX_LEVELS];   // level of the previous octave with the same kernel size, or -1
	bool onDemand[BHIP_MAX_LEVELS];   // stand-alone octave: outer level left to k_nms_scalespace (evaluated around the NMS maxima only)
	int exportSlot[BHIP_MAX_LEVELS];  // fused producer: slot of this level in the export buffer, or -1
	int nexport = 0;
	size_t intenOff = 0, expOff = 0;  // floats, per-image strides below
	long long intenImageStride = 0, expImageStride = 0;
};

struct FhDetector {
	bhip_fh_cfg cfg;
	int W = 0, H = 0, batch = 0, cap = 0;
	bool plannedInt = false;   // the plan is for GrayS32 integral images (from GrayU8 frames; integer taps) instead of GrayF32 ones
	std::vector<FhOctavePlan> plan;
	int bitmapWords = 0;
	DevBuf inten, bitmap, prefix, cand, sorted, count, selKey, selIdx, selLevels;
	bool nBest() const { return cfg.maxFeaturesPerScale > 0; }   // SelectNBestFeatures between the NMS and the scale-space test
	std::vector<int> counts;   // per image, host
	long long total = 0;
	HipEvent countsRead;       // recorded behind the count read-back: the host waits for it alone, not for the ranking launched after it

	static bool unfusedOnly() { return bhip_env_flag("BHIP_DETECT_UNFUSED"); }   // parity cross-check of the two detector paths
	int makePlan(bhip_ctx* ctx, int width, int height) {
		plan.clear();
		if (cfg.numberScalesPerOctave > BHIP_MAX_LEVELS || cfg.numberScalesPerOctave < 1) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "numberScalesPerOctave out of range");
		if (cfg.extractRadius < 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "Search radius must be >= 1");
		if (cfg.initialSampleSize < 1 || cfg.initialSize < 3) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sample size / initial size");
		if (width >= 32768 || height >= 32768) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "image too large for Point2D_I16");
		int skip = cfg.initialSampleSize, sizeStep = cfg.scaleStepSize, octaveSize = cfg.initialSize;
		unsigned int bits = 0;
		const int step = cfg.extractRadius + 1;
		for (int octave = 0; octave < cfg.numberOfOctaves; octave++) {
			FhOctavePlan o;
			o.nlevels = cfg.numberScalesPerOctave;
			for (int i = 0; i < o.nlevels; i++) o.sizes[i] = octaveSize + i * sizeStep;
			const int maxSize = o.sizes[o.nlevels - 1];
			if (maxSize > width || maxSize > height) break;
			o.skip = skip;
			o.w = width / skip;
			o.h = height / skip;
			for (int i = 2; i < o.nlevels; i++) {
				FhLevelPlan m;
				m.level = i - 1;
				DetectLevelParams& p = m.p;
				p.skip = skip; p.w = o.w; p.h = o.h;
				p.sizeLower = o.sizes[m.level - 1]; p.sizeMid = o.sizes[m.level]; p.sizeUpper = o.sizes[m.level + 1];
				p.border = p.sizeMid / (2 * skip);
				const int rw = p.w - 2 * p.border, rh = p.h - 2 * p.border;
				p.nbx = rw > 0 ? (rw + step - 1) / step : 0;
				p.nby = rh > 0 ? (rh + step - 1) / step : 0;
				p.bitBase = bits;
				bits += (unsigned)p.nbx * (unsigned)p.nby;
				o.mids.push_back(m);
			}
			plan.push_back(o);
			skip += skip;
			octaveSize += sizeStep;
			sizeStep += sizeStep;
		}
		bitmapWords = (int)((bits + 31) / 32) + 1;
		return BHIP_OK;
	}

	static bool noShare() { return bhip_env_flag("BHIP_DETECT_NOSHARE"); }   // parity cross-check of the shared-level plan
	static bool denseOuter() { return bhip_env_flag("BHIP_DETECT_DENSE"); }  // parity cross-check: compute the outer levels of every octave densely
	// Which octaves run fused, and which levels are copied from the octave below instead of being recomputed.  A box-filter response
	// depends on (pixel, kernel size) only, and the default schedule repeats sizes: 15,27 | 27,51 | 51,99 are levels 1,3 of one octave and
	// levels 0,1 of the next, on a lattice twice as coarse.  Sharing is enabled where the unrolled inner form and the clamped border
	// form of the reference cover the same boxes (size = 3*blockSmall, odd), between a producer that keeps or exports its intensity and a
	// stand-alone consumer.  The two forms still round Dyy differently, and which pixels are "inner" depends on the step, so the
	// consumer (k_hessian) copies a pixel only when both octaves evaluate it with the same form and computes the rest itself.
	void planExecution() {
		for (auto& o : plan) {
			int ftx, fty, flds;
			// N-best selection needs every level's NMS list and intensity images in memory: stand-alone kernels
			o.fused = !unfusedOnly() && !nBest() && !o.mids.empty() && bhip_fused_plan(o.skip, o.nlevels, o.sizes, cfg.extractRadius, &ftx, &fty, &flds);
			o.fixed = o.fused && bhip_fused_is_fixed(o.skip, o.nlevels, o.sizes, cfg.extractRadius);
			if (plannedInt && !o.fixed) o.fused = false;   // integer taps: compile-time-geometry fused kernel or the stand-alone kernels
			o.nexport = 0;
			for (int i = 0; i < BHIP_MAX_LEVELS; i++) { o.shareFrom[i] = -1; o.exportSlot[i] = -1; o.onDemand[i] = false; }
		}
		// The first and last level of an octave are only read around the NMS maxima of their neighbour level: a stand-alone octave leaves
		// them to k_nms_scalespace unless they can be copied from the octave below.  (N-best selection reads whole levels: dense.)
		const bool sparseOuter = !denseOuter() && !nBest();
		for (size_t k = 0; k < plan.size(); k++) {
			FhOctavePlan& c = plan[k];
			if (k > 0 && !noShare()) shareLevels(c, plan[k - 1]);
			if (!c.fused && sparseOuter && c.nlevels >= 3)
				for (int i : {0, c.nlevels - 1})
					if (c.shareFrom[i] < 0) c.onDemand[i] = true;
		}
	}
	void shareLevels(FhOctavePlan& c, FhOctavePlan& p) {
		{
			if (c.fused || c.skip != 2 * p.skip) return;
			if (p.fused && !p.fixed) return;
			for (int i = 0; i < c.nlevels; i++) {
				const int size = c.sizes[i];
				if (size % 3 != 0 || size % 2 != 1) continue;
				for (int j = 0; j < p.nlevels; j++) {
					if (p.sizes[j] != size) continue;
					if (!p.fused && p.onDemand[j]) break;   // the producer does not hold this level
					if (p.fused) {
						if (p.exportSlot[j] < 0) {
							if (p.nexport >= 2) break;
							p.exportSlot[j] = p.nexport++;
						}
					}
					c.shareFrom[i] = j;
					break;
				}
			}
		}
	}

	// T: element type of the integral images that run() will be given (float or int32_t)
	template <class T>
	int prepare(bhip_ctx* ctx, int width, int height, int batch_) {
		constexpr bool isInt = std::is_same<T, int32_t>::value;
		if (width != W || height != H || plannedInt != isInt) { BHIP_TRY(makePlan(ctx, width, height)); plannedInt = isInt; planExecution(); }
		W = width; H = height; batch = batch_;
		if (cap == 0) cap = BHIP_SURF_INITIAL_CAPACITY;
		return allocate(ctx);
	}
	int allocate(bhip_ctx* ctx) {
		size_t intenFloats = 0;
		for (size_t k = 0; k < plan.size(); k++) {
			FhOctavePlan& o = plan[k];
			if (!o.fused) {
				o.intenImageStride = (long long)o.nlevels * o.w * o.h;
				o.intenOff = intenFloats;
				intenFloats += (size_t)o.intenImageStride * batch;
			}
		}
		BHIP_TRY(inten.reserve(ctx, intenFloats * 4 + 16));
		BHIP_TRY(bitmap.reserve(ctx, (size_t)bitmapWords * 4 * batch));
		BHIP_TRY(prefix.reserve(ctx, (size_t)bitmapWords * 4 * batch));
		BHIP_TRY(cand.reserve(ctx, (size_t)cap * sizeof(KeyPoint) * batch));
		BHIP_TRY(sorted.reserve(ctx, (size_t)cap * sizeof(KeyPoint) * batch));
		BHIP_TRY(count.reserve(ctx, (size_t)batch * 4 * 2));
		if (nBest()) {
			size_t nlv = 0;
			for (auto& o : plan) nlv += o.mids.size();
			BHIP_TRY(selKey.reserve(ctx, (size_t)cap * 4 * batch));
			BHIP_TRY(selIdx.reserve(ctx, (size_t)cap * 4 * batch));
			BHIP_TRY(selLevels.reserve(ctx, std::max<size_t>(nlv, 1) * 4 * 2 * batch));
		}
		return BHIP_OK;
	}

	// level l of the intensity planes of stand-alone octave o
	DevImg<float> level(const FhOctavePlan& o, int l) const { return {inten.as<float>() + o.intenOff + (size_t)l * o.w * o.h, o.intenImageStride, o.w, o.w, o.h, batch}; }
	// the stand-alone octaves plan[k0 .. k1): intensity levels, then NMS + scale-space test of their middle levels
	template <class T>
	int runStandAlone(bhip_ctx* ctx, DevImg<const T> ii, size_t k0, size_t k1) {
		std::vector<HessLevelSource> from((k1 - k0) * BHIP_MAX_LEVELS);
		std::vector<HessOctave> octs;
		std::vector<NmsLevelArgs> nms;
		for (size_t k = k0; k < k1; k++) {
			const FhOctavePlan& o = plan[k];
			HessLevelSource* f = &from[(k - k0) * BHIP_MAX_LEVELS];
			for (int i = 0; i < o.nlevels; i++) {
				f[i] = HessLevelSource{nullptr, 0, 0, 1, 0};
				const int j = o.shareFrom[i];
				if (j < 0 || k == 0) continue;
				const FhOctavePlan& p = plan[k - 1];
				if (p.fused) f[i] = HessLevelSource{level(o, i).data, o.intenImageStride, o.w, 1, 1};   // written in place by the fused octave
				else f[i] = HessLevelSource{level(p, j).data, p.intenImageStride, p.w, 2, 0};
			}
			unsigned int skipMask = 0;
			for (int i = 0; i < o.nlevels; i++)
				if (o.onDemand[i]) skipMask |= 1u << i;
			octs.push_back(HessOctave{o.skip, o.nlevels, o.sizes, level(o, 0), (long long)o.w * o.h, f, skipMask});
			auto held = [&](int l) { DevImg<const float> v = level(o, l); if (o.onDemand[l]) v.data = nullptr; return v; };   // nullptr: not in memory
			for (auto& m : o.mids) nms.push_back(NmsLevelArgs{held(m.level - 1), level(o, m.level), held(m.level + 1), m.p});
		}
		BHIP_TRY(bhip_launch_hessian_octaves(ctx, ii, (int)octs.size(), octs.data()));
		if (nBest()) {
			for (auto& a : nms)
				BHIP_TRY(bhip_launch_nms_scalespace(ctx, a.lower, a.mid, a.upper, a.p, cfg.extractRadius, cfg.detectThreshold, bitmap.as<unsigned int>(), bitmapWords,
													cand.as<KeyPoint>(), count.as<int>(), cap, true, ii));
			return BHIP_OK;
		}
		return bhip_launch_nms_scalespace_levels(ctx, (int)nms.size(), nms.data(), cfg.extractRadius, cfg.detectThreshold, bitmap.as<unsigned int>(), bitmapWords,
												 cand.as<KeyPoint>(), count.as<int>(), cap, ii);
	}
	// ii: the dense integral images prepare<T>() planned for.  Leaves the ordered key points in `sorted` ([image][cap]) and their counts in `counts`.
	template <class T>
	int run(bhip_ctx* ctx, DevImg<const T> ii) {
		for (int attempt = 0; attempt < 8; attempt++) {
			BHIP_HIP(ctx, hipMemsetAsync(bitmap.p, 0, (size_t)bitmapWords * 4 * batch, ctx->stream));
			BHIP_HIP(ctx, hipMemsetAsync(count.p, 0, (size_t)batch * 4 * 2, ctx->stream));
			for (size_t k = 0; k < plan.size(); k++) {
				FhOctavePlan& o = plan[k];
				if (o.fused) {
					// LDS-tiled fused octave: intensity never leaves the CU (except the levels the next octave shares)
					DetectLevelParams mp[BHIP_MAX_LEVELS];
					int ml[BHIP_MAX_LEVELS];
					for (size_t q = 0; q < o.mids.size(); q++) { mp[q] = o.mids[q].p; ml[q] = o.mids[q].level; }
					FusedExport ex{0, {0, 0}, nullptr, 0, 0, 0, {0, 0}};
					if (o.nexport > 0 && k + 1 < plan.size()) {
						// the shared levels go straight into the consuming octave's level planes: its k_hessian then only recomputes the
						// pixels the two octaves evaluate with different forms
						const FhOctavePlan& c = plan[k + 1];
						ex.n = o.nexport;
						for (int j = 0; j < o.nlevels; j++) if (o.exportSlot[j] >= 0) ex.level[o.exportSlot[j]] = j;
						ex.out = level(c, 0).data; ex.w = c.w; ex.h = c.h; ex.imageStride = c.intenImageStride;
						for (int i = 0; i < c.nlevels; i++) {
							const int j = c.shareFrom[i];
							if (j >= 0 && o.exportSlot[j] >= 0) ex.slotOffset[o.exportSlot[j]] = (long long)i * c.w * c.h;
						}
					}
					BHIP_TRY(bhip_launch_detect_fused(ctx, ii, o.skip, o.nlevels, o.sizes, (int)o.mids.size(), mp, ml, cfg.extractRadius,
													  cfg.detectThreshold, bitmap.as<unsigned int>(), bitmapWords, cand.as<KeyPoint>(), count.as<int>(), cap,
													  ex.n > 0 ? &ex : nullptr));
					continue;
				}
				// a run of stand-alone octaves: their Hessian launches, then the NMS of all their middle levels in one launch.  (N-best
				// selection lists every level's maxima by itself: octave by octave, level by level.)
				size_t end = k + 1;
				while (!nBest() && end < plan.size() && !plan[end].fused) end++;
				BHIP_TRY(runStandAlone(ctx, ii, k, end));
				k = end - 1;
			}
			BHIP_TRY(bhip_launch_word_prefix(ctx, bitmap.as<unsigned int>(), bitmapWords, batch, prefix.as<unsigned int>(), count.as<int>() + batch));
			counts.resize(batch);
			const bool viaScratch = (size_t)batch * 4 <= (1u << 20);
			BHIP_HIP(ctx, hipMemcpyAsync(viaScratch ? ctx->hostScratch.p : (void*)counts.data(), count.p, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
			if (!nBest()) {
				// The ranking needs device data only: it is launched before the host has the counts and runs while they travel, so the GPU
				// does not idle through the round trip.  The host waits for the copy alone (an event behind it), not for the ranking.  After
				// an overflow the kernel has ranked an incomplete list (it keeps inside `sorted`) and the loop runs again.
				// (N-best: the ranking and the selection both follow the read-back, as they always did.)
				if (!countsRead) BHIP_HIP(ctx, hipEventCreateWithFlags(&countsRead.h, hipEventDisableTiming));
				BHIP_HIP(ctx, hipEventRecord(countsRead, ctx->stream));
				BHIP_TRY(bhip_launch_rank_scatter(ctx, bitmap.as<unsigned int>(), bitmapWords, prefix.as<unsigned int>(), cand.as<KeyPoint>(), count.as<int>(),
												  cap, batch, sorted.as<KeyPoint>()));
				BHIP_HIP(ctx, hipEventSynchronize(countsRead));
			} else {
				BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
			}
			if (viaScratch) memcpy(counts.data(), ctx->hostScratch.p, (size_t)batch * 4);
			int maxCount = 0;
			total = 0;
			for (int c : counts) { maxCount = std::max(maxCount, c); total += c; }
			if (maxCount <= cap) {
				if (nBest()) {
					BHIP_TRY(bhip_launch_rank_scatter(ctx, bitmap.as<unsigned int>(), bitmapWords, prefix.as<unsigned int>(), cand.as<KeyPoint>(), count.as<int>(),
													  cap, batch, sorted.as<KeyPoint>()));
					BHIP_TRY(selectNBest(ctx));
				}
				return BHIP_OK;
			}
			// candidate list overflowed: grow and run the detector again
			cap = maxCount + maxCount / 4 + 64;
			BHIP_TRY(allocate(ctx));
		}
		return bhip_fail(ctx, BHIP_ERR_CAPACITY, "key point list kept overflowing");
	}
	// maxFeaturesPerScale > 0: `sorted` holds every level's NMS maxima (ranked, with intensities).  Per level: select, scale-space test,
	// sub-pixel fit (k_select_nbest, results into `cand`), then the levels are packed back into `sorted` and the counts re-read.
	int selectNBest(bhip_ctx* ctx) {
		int nlv = 0;
		for (auto& o : plan) nlv += (int)o.mids.size();
		int* levelStart = selLevels.as<int>();
		int* levelCount = levelStart + (size_t)std::max(nlv, 1) * batch;
		int li = 0;
		for (auto& o : plan)
			for (auto& m : o.mids) {
				BHIP_TRY(bhip_launch_select_nbest(ctx, level(o, m.level - 1), level(o, m.level), level(o, m.level + 1), m.p, cfg.extractRadius,
												  cfg.maxFeaturesPerScale, bitmap.as<unsigned int>(), prefix.as<unsigned int>(), bitmapWords, sorted.as<KeyPoint>(),
												  cap, selKey.as<float>(), selIdx.as<int>(), cand.as<KeyPoint>(), levelStart, levelCount, li, nlv));
				li++;
			}
		BHIP_TRY(bhip_launch_compact_levels(ctx, cand.as<KeyPoint>(), cap, levelStart, levelCount, nlv, batch, sorted.as<KeyPoint>(), count.as<int>()));
		BHIP_HIP(ctx, hipMemcpyAsync(counts.data(), count.p, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
		BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
		total = 0;
		for (int c : counts) total += c;
		return BHIP_OK;
	}
};

// ---------------------------------------------------------------------------------------------------------------
// SURF detect + describe object
// ---------------------------------------------------------------------------------------------------------------
// Everything a detect+describe object holds on its context's device (CtxChild); its owner synchronizes the copy stream too before dropping it.
struct SurfDevice {
	FhDetector det;
	DevBuf tabBuf, inBuf, iiBuf, startBuf, angBuf, descBuf, whiteBuf, xysBuf, tmpKp, tmpAng, tmpDesc, tmpWhite, permBuf;
	DevBuf briefTab, wordsBuf;   // BRIEF: [samplePoints | compare] on the device; words of the whole batch, compact [total][briefWords]
	PinnedBuf startsPinned;      // page-locked staging copy of `starts` for its upload
	// host-frame batches are processed in chunks so that the upload of chunk k+1 (copy stream) runs under the kernels of chunk k: the
	// chunks go through `worker` (same configuration, chunk-sized work buffers), whose results are appended to this object's arrays
	std::unique_ptr<bhip_surf> worker;
	HipStream copyStream;
	const int* briefBorrow = nullptr;   // chunk worker: the owner's BRIEF table (not owned: never freed twice)
};

struct bhip_surf : CtxChild<SurfDevice> {
	void onRelease() {   // the chunk worker is owned by this object and is not in the registry: it goes with the SurfDevice
		if (copyStream) (void)hipStreamSynchronize(copyStream);
		haveResult = false;
	}
	int stable = 1;
	bhip_surf_cfg sd;
	bhip_ori_cfg ori;
	SurfTables tables;
	std::vector<int> starts;  // batch+1
	int W = 0, H = 0, batch = 0;
	bool haveResult = false;
	bool iiInt = false;        // the integral images of the last detect (iiBuf, [batch][H][W]; see withIntegral) are GrayS32, from GrayU8 frames, not GrayF32
	int planarBands = 0;       // > 0: the last detect was colour SURF on that many bands (descriptor = planarBands * dof values)
	int dofOut() const { return tables.dof * (planarBands > 0 ? planarBands : 1); }
	// colour SURF: the bands' integral images follow the grey one in iiBuf
	DescPlanar planar() const {
		const long long px = (long long)W * H;
		return planarBands > 0 ? DescPlanar{iiBuf.as<float>() + px, px * (1 + planarBands), px, planarBands} : DescPlanar{};
	}
	const DevBuf* iiOwner = nullptr; int iiFirst = 0;   // worker only: the current chunk's integral images go into the owner's iiBuf, from image iiFirst on
	// describe = BRIEF (DetectDescribeFusion(fastHessian, null, brief), bhip_surf_create_brief): no orientation / SURF stage; every detected
	// point gets its TupleDesc_B words from the input frame itself
	bool brief = false;
	int briefRadius = 0, briefPoints = 0, briefWords = 0;
	bool briefPatch = false;            // the definition fits the LDS-patch kernel
	const int* briefSample() const { return briefBorrow ? briefBorrow : briefTab.as<int>(); }
	const int* briefCompare() const { return briefSample() + briefCompareOff; }
	size_t briefCompareOff = 0;
};

// The one place where the stored integral images' element type becomes a static type again: f(DevImg<const float>) or f(DevImg<const int32_t>)
template <class F>
static int withIntegral(const bhip_surf* s, F f) {
	return s->iiInt ? f(bhip_img_over<const int32_t>(s->iiBuf, s->W, s->W, s->H, s->batch)) : f(bhip_img_over<const float>(s->iiBuf, s->W, s->W, s->H, s->batch));
}
// frame type -> integral image type (GIntegralImageOps.getIntegralType): GrayF32 -> GrayF32, GrayU8 -> GrayS32 (every stage then runs on integer taps)
template <class T> struct SurfTraits;
template <> struct SurfTraits<float> { using II = float; };
template <> struct SurfTraits<uint8_t> { using II = int32_t; };
constexpr int GREY = 0;   // surfRun's `bands` for single-band frames (otherwise the band count of one colour frame)
// SYNCHRONIZED: host-frame callers get their frames (and the upload buffer) back only after a final synchronize.  QUEUED: the caller's device-
// resident batch (bhip_surf_detect_dev_f32) -- the call may return with the describe kernels still queued on the context's stream (its contract)
enum class SurfReturn { SYNCHRONIZED, QUEUED };

static int buildTables(bhip_surf* s) {
	bhip_ctx* ctx = s->ctx;
	SurfTables& t = s->tables;
	memset(&t, 0, sizeof(t));
	const bhip_surf_cfg& c = s->sd;
	const bhip_ori_cfg& o = s->ori;
	if (c.widthLargeGrid < 1 || c.widthSubRegion < 1 || c.widthSample < 1 || c.overLap < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad SURF config");
	if (o.radius < 1 || o.radius > 10) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "orientation radius out of range (1..10 on the GPU)");
	std::vector<double> all;
	auto push = [&](const std::vector<double>& v) { size_t off = all.size(); all.insert(all.end(), v.begin(), v.end()); return off; };
	t.oriStable = s->stable;
	t.oriRadius = o.radius;
	t.oriWidth = 2 * o.radius + 1;
	t.oriKernelWidth = o.sampleWidth;
	t.oriHasWeights = o.weightSigma != 0 ? 1 : 0;
	t.oriPeriod = o.samplePeriod;
	t.oriWindow = o.windowSize;
	t.oriRadiusToScale = o.objectRadiusToScale;
	size_t offOri = 0, offSub = 0, offGrid = 0, offFast = 0;
	// OrientationIntegralBase :85-86 weights = FactoryKernelGaussian.gaussian(2,true,64,weightSigma,sampleRadius)
	if (t.oriHasWeights) offOri = push(bhip_gaussian2d_f64(o.weightSigma, o.radius));
	t.stable = s->stable;
	t.widthLargeGrid = c.widthLargeGrid; t.widthSubRegion = c.widthSubRegion; t.widthSample = c.widthSample; t.overLap = c.overLap;
	t.dof = c.widthLargeGrid * c.widthLargeGrid * 4;
	const int regionSize = c.widthLargeGrid * c.widthSubRegion;
	if (s->stable) {
		// DescribePointSurfMod :76-106
		std::vector<double> wg = bhip_gaussian_width(c.sigmaLargeGrid, c.widthLargeGrid);
		std::vector<double> ws = bhip_gaussian_width(c.sigmaSubRegion, c.widthSubRegion + 2 * c.overLap);
		const int gw = c.widthLargeGrid, sw = c.widthSubRegion + 2 * c.overLap;
		double div = wg[(size_t)(gw / 2) * gw + gw / 2];
		for (double& v : wg) v /= div;
		div = ws[(size_t)(sw / 2) * sw + sw / 2];
		for (double& v : ws) v /= div;
		offGrid = push(wg);
		offSub = push(ws);
		t.radiusDescriptor = regionSize / 2 + c.overLap;
	} else {
		// DescribePointSurf :110-141
		const int radius = regionSize / 2;
		std::vector<double> w = bhip_gaussian_width(c.weightSigma, radius * 2);
		if ((int)w.size() != regionSize * regionSize) return bhip_fail(ctx, BHIP_ERR_INVALID, "Weighting kernel has an unexpected size");
		const double div = w[(size_t)radius * (radius * 2) + radius];
		for (double& v : w) v /= div;
		offFast = push(w);
		t.radiusDescriptor = regionSize / 2;
	}
	BHIP_TRY(s->tabBuf.reserve(ctx, all.size() * 8 + 8));
	BHIP_HIP(ctx, hipMemcpyAsync(s->tabBuf.p, all.data(), all.size() * 8, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const double* base = s->tabBuf.as<double>();
	t.oriWeights = t.oriHasWeights ? base + offOri : nullptr;
	t.weightSub = s->stable ? base + offSub : nullptr;
	t.weightGrid = s->stable ? base + offGrid : nullptr;
	t.weightFast = s->stable ? nullptr : base + offFast;
	return BHIP_OK;
}

// in: a batch of GrayF32 or GrayU8 (dense) frames, bands == GREY; or, bands > 0, one colour frame as [1 + bands] GrayF32 images -- the band
// average first, then the bands
template <class T>
static int surfRun(bhip_surf* s, DevImg<const T> in, int bands, SurfReturn ret) {
	using II = typename SurfTraits<T>::II;
	bhip_ctx* ctx = s->ctx;
	const int W = in.width, H = in.height, batch = bands > 0 ? 1 : in.batch;
	const long long px = (long long)W * H;
	s->haveResult = false;
	BHIP_TRY(s->det.prepare<II>(ctx, W, H, batch));
	if (!s->iiOwner) BHIP_TRY(s->iiBuf.reserve(ctx, (size_t)px * 4 * in.batch));
	II* iiBase = s->iiOwner ? s->iiOwner->as<II>() + px * s->iiFirst : s->iiBuf.as<II>();
	s->W = W; s->H = H; s->batch = batch;
	s->iiInt = std::is_same<II, int32_t>::value; s->planarBands = bands;
	const DevImg<II> iiAll{iiBase, px, W, W, H, in.batch};
	if constexpr (std::is_same<T, uint8_t>::value) BHIP_TRY(bhip_launch_integral_u8(ctx, in, iiAll));
	else BHIP_TRY(bhip_launch_integral(ctx, in, iiAll));
	const DevImg<const II> ii{iiBase, px, W, W, H, batch};
	BHIP_TRY(s->det.run(ctx, ii));
	// exclusive prefix of counts -> start of every image in the compact result arrays
	s->starts.assign(batch + 1, 0);
	for (int i = 0; i < batch; i++) s->starts[i + 1] = s->starts[i] + s->det.counts[i];
	const long long total = s->det.total;
	if (total > 0x7fffffffLL) return bhip_fail(ctx, BHIP_ERR_CAPACITY, "more than 2^31 key points in one batch");
	BHIP_TRY(s->startBuf.reserve(ctx, (size_t)(batch + 1) * 4));
	{
		// through a page-locked staging copy owned by the object: the transfer then reads it in stream order, and nothing rewrites it before the
		// next detect has synchronized on its own count read-back
		const size_t need = (size_t)(batch + 1) * 4;
		if (need > s->startsPinned.cap) BHIP_TRY(s->startsPinned.reserve(ctx, need * 2));
		memcpy(s->startsPinned.p, s->starts.data(), need);
		BHIP_HIP(ctx, hipMemcpyAsync(s->startBuf.p, s->startsPinned.p, need, hipMemcpyHostToDevice, ctx->stream));
	}
	if (s->brief) {
		// DetectDescribeFusion.detect (F:abst/feature/detdesc/DetectDescribeFusion.java:95-127) with orientation == null and
		// describe = WrapDescribeBrief (process always returns true, so every detected point is kept, in detector order):
		// yaw = detector.getOrientation(i) = 0 (WrapFHtoInterestPoint.java:77-79); DescribePointBrief.process samples the frame handed to
		// setImage (:71-75,86-88 -- the blurred copy it makes is never read)
		if (bands > 0) return bhip_fail(ctx, BHIP_ERR_UNSUPPORTED, "BRIEF runs on single-band frames");
		BHIP_TRY(s->angBuf.reserve(ctx, (size_t)std::max<long long>(total, 1) * 8));
		BHIP_TRY(s->whiteBuf.reserve(ctx, (size_t)std::max<long long>(total, 1)));
		BHIP_TRY(s->wordsBuf.reserve(ctx, (size_t)std::max<long long>(total, 1) * 4 * s->briefWords));
		if (total > 0) {
			BHIP_HIP(ctx, hipMemsetAsync(s->angBuf.p, 0, (size_t)total * 8, ctx->stream));
			BHIP_HIP(ctx, hipMemsetAsync(s->whiteBuf.p, 0, (size_t)total, ctx->stream));
			int maxCount = 0;
			for (int c : s->det.counts) maxCount = std::max(maxCount, c);
			BHIP_TRY(bhip_launch_brief(ctx, in, s->briefRadius, s->briefPoints, s->briefSample(), s->briefCompare(), (const double*)s->det.sorted.p, (int)total,
									   s->wordsBuf.as<int>(), s->startBuf.as<int>(), maxCount, (int)(sizeof(KeyPoint) / 8),
									   (long long)s->det.cap * (long long)(sizeof(KeyPoint) / 8), s->briefPatch));
		}
		BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
		s->haveResult = true;
		return BHIP_OK;
	}
	const int dof = s->dofOut();
	BHIP_TRY(s->angBuf.reserve(ctx, (size_t)std::max<long long>(total, 1) * 8));
	BHIP_TRY(s->descBuf.reserve(ctx, (size_t)std::max<long long>(total, 1) * 8 * dof));
	BHIP_TRY(s->whiteBuf.reserve(ctx, (size_t)std::max<long long>(total, 1)));
	// processing order of the describe stage: key points of one image grouped by coarse tile (L2 locality of the gathers)
	const KpOrder* perm = nullptr;
	BHIP_TRY(scratchOf(ctx)->describeQueue.reserve(ctx, BHIP_DESCRIBE_QUEUE_BYTES));
	{
#ifdef BHIP_EXPERIMENTS
		const bool noOrder = bhip_env_flag("BHIP_DESCRIBE_NOORDER");
#else
		const bool noOrder = false;
#endif
		int maxCount = 0;
		for (int c : s->det.counts) maxCount = std::max(maxCount, c);
		if (!noOrder && total > 0) {
			BHIP_TRY(s->permBuf.reserve(ctx, (size_t)total * sizeof(KpOrder) + (size_t)batch * 64 * 4));
			int* hist = (int*)(s->permBuf.as<KpOrder>() + total);
			BHIP_TRY(bhip_launch_kp_spatial_order(ctx, s->det.sorted.as<KeyPoint>(), s->det.cap, s->startBuf.as<int>(), batch, maxCount, W, H, hist,
												  s->permBuf.as<KpOrder>()));
			perm = s->permBuf.as<KpOrder>();
		}
	}
	BHIP_TRY(bhip_launch_describe_ex(ctx, ii, s->det.sorted.as<KeyPoint>(), s->det.cap, s->startBuf.as<int>(), 0, total, s->tables, nullptr,
									 s->angBuf.as<double>(), s->descBuf.as<double>(), s->whiteBuf.as<uint8_t>(), perm, scratchOf(ctx)->describeQueue.as<int>(),
									 s->planar()));
	// host-frame callers may reuse their frames (and the upload buffer) as soon as the call returns; a device-resident batch was consumed before
	// the detector's count read-back, so its call returns with the describe kernels still in flight (stream order covers every later use)
	if (ret == SurfReturn::SYNCHRONIZED) BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	s->haveResult = true;
	return BHIP_OK;
}

static int surfCreateUnregistered(bhip_ctx* ctx, const bhip_fh_cfg* fh, const bhip_surf_cfg* surf, const bhip_ori_cfg* ori, int stable,
								  std::unique_ptr<bhip_surf>& out);

// device buffer growth that keeps the first `keep` bytes (result arrays that chunks are appended to)
static int growKeep(bhip_ctx* ctx, DevBuf& b, size_t bytes, size_t keep) {
	if (bytes <= b.cap) return BHIP_OK;
	DevBuf n;
	BHIP_TRY(n.reserve(ctx, bytes + bytes / 4));
	if (b.p && keep) BHIP_HIP(ctx, hipMemcpyAsync(n.p, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream));
	if (b.p) BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	b = std::move(n);   // the old block (now in n) is freed on return, after the copy out of it has finished
	return BHIP_OK;
}

#define SURF_CHUNK 32   // frames per chunk of a host batch (265 MB of 1080p GrayF32: ~5 ms of PCIe, ~3 ms of kernels)

// Host frames -> device in chunks on the copy stream, each chunk detected + described by the worker object as soon as it has arrived;
// results are appended to the owner's arrays, which end up exactly as one surfRun over the whole batch leaves them.
// upload(i, dst, stream) enqueues the copy of frame i (T: the frames' element type).  Returns BHIP_OK with *done = false when the batch has
// to go through the plain path (small batch, or a key-point list outgrew the owner's capacity half way).
template <class T, class Upload>
static int surfRunChunked(bhip_surf* s, int width, int height, int batch, Upload upload, bool* done) {
	using II = typename SurfTraits<T>::II;
	bhip_ctx* ctx = s->ctx;
	*done = false;
	int chunk = SURF_CHUNK;
	{ const char* e = getenv("BHIP_SURF_CHUNK"); if (e && atoi(e) > 0) chunk = atoi(e); }   // tests: chunk small batches too
	if (batch < 2 * chunk) return BHIP_OK;
	if (!s->worker) {
		BHIP_TRY(surfCreateUnregistered(ctx, &s->det.cfg, &s->sd, &s->ori, s->stable, s->worker));
		if (s->brief) {
			// the worker samples with the owner's definition (it borrows the device table; briefTab stays empty so it is never freed twice)
			bhip_surf* w0 = s->worker.get();
			w0->brief = true; w0->briefRadius = s->briefRadius; w0->briefPoints = s->briefPoints; w0->briefWords = s->briefWords;
			w0->briefBorrow = s->briefTab.as<int>(); w0->briefCompareOff = s->briefCompareOff; w0->briefPatch = s->briefPatch;
		}
		BHIP_HIP(ctx, hipStreamCreateWithFlags(&s->copyStream.h, hipStreamNonBlocking));
	}
	bhip_surf* w = s->worker.get();
	const size_t px = (size_t)width * height;
	s->haveResult = false;
	BHIP_TRY(s->det.prepare<II>(ctx, width, height, batch));
	BHIP_TRY(s->iiBuf.reserve(ctx, px * 4 * batch));
	// everything queued on the compute stream so far (an earlier batch may still read inBuf) precedes the first upload
	const int nchunks = (batch + chunk - 1) / chunk;
	// events are destroyed on every way out of this function
	std::vector<HipEvent> events(nchunks + 1);
	HipEvent& ev = events[nchunks];
	HipEvent* arrived = events.data();
	BHIP_HIP(ctx, hipEventCreateWithFlags(&ev.h, hipEventDisableTiming));
	BHIP_HIP(ctx, hipEventRecord(ev, ctx->stream));
	BHIP_HIP(ctx, hipStreamWaitEvent(s->copyStream, ev, 0));
	int status = BHIP_OK;
	for (int c = 0; c < nchunks && status == BHIP_OK; c++) {
		const int a = c * chunk, n = std::min(chunk, batch - a);
		for (int i = a; i < a + n && status == BHIP_OK; i++) status = upload(i, s->inBuf.as<T>() + px * i, s->copyStream);
		if (status == BHIP_OK && (hipEventCreateWithFlags(&arrived[c].h, hipEventDisableTiming) != hipSuccess || hipEventRecord(arrived[c], s->copyStream) != hipSuccess))
			status = bhip_fail(ctx, BHIP_ERR_HIP, "event");
	}
	const int dof = s->tables.dof;
	s->starts.assign(batch + 1, 0);
	s->det.counts.assign(batch, 0);
	long long total = 0;
	bool fits = true;
	for (int c = 0; c < nchunks && status == BHIP_OK && fits; c++) {
		const int a = c * chunk, n = std::min(chunk, batch - a);
		if (hipStreamWaitEvent(ctx->stream, arrived[c], 0) != hipSuccess) { status = bhip_fail(ctx, BHIP_ERR_HIP, "wait"); break; }
		w->iiOwner = &s->iiBuf; w->iiFirst = a;
		status = surfRun(w, DevImg<const T>{s->inBuf.as<T>() + px * a, (long long)px, width, width, height, n}, GREY, SurfReturn::SYNCHRONIZED);
		if (status != BHIP_OK) break;
		int maxCount = 0;
		for (int i = 0; i < n; i++) maxCount = std::max(maxCount, w->det.counts[i]);
		if (maxCount > s->det.cap) { fits = false; break; }   // the owner's [image][cap] key-point array is too narrow: plain path (it grows there)
		const long long ct = w->det.total;
		status = growKeep(ctx, s->angBuf, (size_t)std::max<long long>(total + ct, 1) * 8, (size_t)total * 8);
		if (status == BHIP_OK && !s->brief) status = growKeep(ctx, s->descBuf, (size_t)std::max<long long>(total + ct, 1) * 8 * dof, (size_t)total * 8 * dof);
		if (status == BHIP_OK) status = growKeep(ctx, s->whiteBuf, (size_t)std::max<long long>(total + ct, 1), (size_t)total);
		if (status == BHIP_OK && s->brief) status = growKeep(ctx, s->wordsBuf, (size_t)std::max<long long>(total + ct, 1) * 4 * s->briefWords, (size_t)total * 4 * s->briefWords);
		if (status != BHIP_OK) break;
		hipError_t e = hipSuccess;
		if (maxCount > 0)
			e = hipMemcpy2DAsync(s->det.sorted.as<KeyPoint>() + (long long)a * s->det.cap, (size_t)s->det.cap * sizeof(KeyPoint), w->det.sorted.p,
								 (size_t)w->det.cap * sizeof(KeyPoint), (size_t)maxCount * sizeof(KeyPoint), n, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess && ct > 0) e = hipMemcpyAsync(s->angBuf.as<double>() + total, w->angBuf.p, (size_t)ct * 8, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess && ct > 0 && !s->brief) e = hipMemcpyAsync(s->descBuf.as<double>() + total * dof, w->descBuf.p, (size_t)ct * 8 * dof, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess && ct > 0 && s->brief) e = hipMemcpyAsync(s->wordsBuf.as<int>() + total * s->briefWords, w->wordsBuf.p, (size_t)ct * 4 * s->briefWords, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess && ct > 0) e = hipMemcpyAsync(s->whiteBuf.as<uint8_t>() + total, w->whiteBuf.p, (size_t)ct, hipMemcpyDeviceToDevice, ctx->stream);
		if (e != hipSuccess) { status = bhip_fail(ctx, BHIP_ERR_HIP, hipGetErrorString(e)); break; }
		for (int i = 0; i < n; i++) {
			s->det.counts[a + i] = w->det.counts[i];
			s->starts[a + i + 1] = s->starts[a + i] + w->det.counts[i];
		}
		total += ct;
	}
	// every upload has to be over before the caller's frames may change (and before the plain path re-uses inBuf)
	(void)hipStreamSynchronize(s->copyStream);
	(void)hipStreamSynchronize(ctx->stream);
	w->iiOwner = nullptr;
	if (status != BHIP_OK) return status;
	if (!fits) {
		// the frames are all on the device: run the whole batch the plain way (its detector grows the key-point capacity as needed)
		*done = true;
		return surfRun(s, bhip_img_over<const T>(s->inBuf, width, width, height, batch), GREY, SurfReturn::SYNCHRONIZED);
	}
	if (total > 0x7fffffffLL) return bhip_fail(ctx, BHIP_ERR_CAPACITY, "more than 2^31 key points in one batch");
	s->det.total = total;
	s->W = width; s->H = height; s->batch = batch;
	s->iiInt = std::is_same<II, int32_t>::value;
	s->planarBands = 0;
	BHIP_TRY(s->startBuf.reserve(ctx, (size_t)(batch + 1) * 4));
	BHIP_HIP(ctx, hipMemcpyAsync(s->startBuf.p, s->starts.data(), (size_t)(batch + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	s->haveResult = true;
	*done = true;
	return BHIP_OK;
}

static int surfCreateUnregistered(bhip_ctx* ctx, const bhip_fh_cfg* fh, const bhip_surf_cfg* surf, const bhip_ori_cfg* ori, int stable,
								  std::unique_ptr<bhip_surf>& out) {
	std::unique_ptr<bhip_surf> s(new (std::nothrow) bhip_surf());
	if (!s) return bhip_fail(ctx, BHIP_ERR_NOMEM, "out of host memory");
	s->ctx = ctx;
	s->stable = stable ? 1 : 0;
	if (fh) s->det.cfg = *fh; else bhip_fh_cfg_default(&s->det.cfg);
	if (surf) s->sd = *surf; else bhip_surf_cfg_default(&s->sd);
	if (ori) s->ori = *ori; else bhip_ori_cfg_default(&s->ori, s->stable);
	BHIP_TRY(buildTables(s.get()));
	out = std::move(s);
	return BHIP_OK;
}

// bhip_surf_detect_f32 (T = float) and bhip_surf_detect_u8 (T = uint8_t: GrayS32 integral images, integer taps)
template <class T>
static int surfDetectHost(bhip_surf* s, const T* const* img, const int* startIndex, const int* stride, int width, int height, int batch) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!img || width <= 0 || height <= 0 || batch <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image batch");
	const size_t px = (size_t)width * height;
	BHIP_TRY(s->inBuf.reserve(ctx, px * sizeof(T) * batch));
	for (int i = 0; i < batch; i++)
		if (!img[i] || (stride ? stride[i] : width) < width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image (null or stride < width)");
	auto put = [&](int i, T* dst, hipStream_t st) {
		return upload(ctx, dst, width, img[i], startIndex ? startIndex[i] : 0, stride ? stride[i] : width, width, height, st);
	};
	bool done = false;
	BHIP_TRY(surfRunChunked<T>(s, width, height, batch, put, &done));
	if (done) return BHIP_OK;
	for (int i = 0; i < batch; i++) BHIP_TRY(put(i, s->inBuf.as<T>() + px * i, ctx->stream));
	return surfRun(s, bhip_img_over<const T>(s->inBuf, width, width, height, batch), GREY, SurfReturn::SYNCHRONIZED);
}

// AssociateDescription over the descriptors still resident from the last detect of `s`: checks the problem table of
// bhip_assoc_l2_surf / bhip_assoc_hamming_surf, has `match` write problem p (source image srcImage[p], destination dstImage[p]) into device
// arrays prefilled with "no match", and downloads them.
template <class Match>
static int assocSurf(bhip_surf* s, int count, const int* srcImage, const int* dstImage, int* pairs, double* fit, Match match) {
	bhip_ctx* ctx = s->ctx;
	if (!s->haveResult) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result");
	if (count < 0 || (count > 0 && (!srcImage || !dstImage || !pairs || !fit))) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad problem table");
	if (count == 0) return BHIP_OK;
	const long long total = s->det.total;
	std::vector<long long> so(count), doff(count);
	std::vector<int> ns(count), nd(count);
	std::vector<char> used(s->batch, 0);
	for (int p = 0; p < count; p++) {
		const int a = srcImage[p], b = dstImage[p];
		if (a < 0 || a >= s->batch || b < 0 || b >= s->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "image index outside the last batch");
		if (used[a]) return bhip_fail(ctx, BHIP_ERR_INVALID, "an image may be the source of one problem per call");
		used[a] = 1;
		so[p] = s->starts[a]; ns[p] = s->det.counts[a];
		doff[p] = s->starts[b]; nd[p] = s->det.counts[b];
	}
	if (total == 0) return BHIP_OK;
	CtxScratch* sc = scratchOf(ctx);
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)total * 4));
	BHIP_TRY(sc->out1.reserve(ctx, (size_t)total * 8));
	// rows of images that are the source of no problem in this call come back as "no match" (-1, 0), not as whatever an earlier call left
	BHIP_HIP(ctx, hipMemsetAsync(sc->out0.p, 0xff, (size_t)total * 4, ctx->stream));
	BHIP_HIP(ctx, hipMemsetAsync(sc->out1.p, 0, (size_t)total * 8, ctx->stream));
	BHIP_TRY(match(so.data(), ns.data(), doff.data(), nd.data(), sc->out0.as<int>(), sc->out1.as<double>()));
	BHIP_HIP(ctx, hipMemcpyAsync(pairs, sc->out0.p, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(fit, sc->out1.p, (size_t)total * 8, hipMemcpyDeviceToHost, ctx->stream));
	return bhip_ctx_synchronize(ctx);
}

// FastHessianFeatureDetector.detect(integral) on a GrayF32 (T = float) or a GrayS32 (T = int32_t, from a GrayU8 frame) integral image
template <class T>
static int fhDetect(bhip_ctx* ctx, const bhip_fh_cfg* cfg, HostImg<const T> hin, double* xy_scale, int cap, int* n) {
	CHECK_CTX(ctx);
	CHECK_IMG(ctx, hin);
	if (!n || cap < 0 || (cap > 0 && !xy_scale)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad output");
	*n = 0;
	FhDetector det;
	if (cfg) det.cfg = *cfg; else bhip_fh_cfg_default(&det.cfg);
	CtxScratch* sc = scratchOf(ctx);
	DevImg<T> din;
	int status = stageIn(ctx, sc->in0, hin, hin.width, din);
	if (status == BHIP_OK) status = det.prepare<T>(ctx, hin.width, hin.height, 1);
	if (status == BHIP_OK) status = det.run(ctx, DevImg<const T>(din));
	if (status == BHIP_OK) {
		*n = det.counts[0];
		const int ncopy = std::min(*n, cap);
		if (ncopy > 0) {
			std::vector<KeyPoint> kps(ncopy);
			hipError_t e = hipMemcpyAsync(kps.data(), det.sorted.p, (size_t)ncopy * sizeof(KeyPoint), hipMemcpyDeviceToHost, ctx->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
			if (e != hipSuccess) status = bhip_fail(ctx, BHIP_ERR_HIP, hipGetErrorString(e));
			else for (int i = 0; i < ncopy; i++) { xy_scale[3 * i] = kps[i].x; xy_scale[3 * i + 1] = kps[i].y; xy_scale[3 * i + 2] = kps[i].scale; }
		}
	}
	(void)hipStreamSynchronize(ctx->stream);   // det's buffers are freed on return
	return status;
}

extern "C" {

const char* bhip_version(void) { return "boofhip 0.1 (gfx950)"; }

void bhip_fh_cfg_default(bhip_fh_cfg* c) {
	c->detectThreshold = 1; c->extractRadius = 2; c->maxFeaturesPerScale = -1; c->initialSampleSize = 1; c->initialSize = 9;
	c->numberScalesPerOctave = 4; c->numberOfOctaves = 4; c->scaleStepSize = 6;
}
void bhip_klt_cfg_default(bhip_klt_cfg* c) {
	c->forbiddenBorder = 0; c->maxPerPixelError = 25; c->maxIterations = 15; c->minDeterminant = 0.001f; c->minPositionDelta = 0.01f;
}
void bhip_bg_basic_cfg_default(bhip_bg_basic_cfg* c) { c->learnRate = 0.05f; c->threshold = 0; c->unknownValue = 0; }
void bhip_bg_gaussian_cfg_default(bhip_bg_gaussian_cfg* c) {
	c->learnRate = 0.05f; c->threshold = 0; c->initialVariance = FLT_TRUE_MIN; c->minimumDifference = 0; c->unknownValue = 0;
}
void bhip_bg_gmm_cfg_default(bhip_bg_gmm_cfg* c) {
	c->learningPeriod = 1000.0f; c->initialVariance = 400; c->decayCoefient = 0.005f; c->maxDistance = 3; c->numberOfGaussian = 5; c->significantWeight = 0.01f;
	c->unknownValue = 0;
}
void bhip_disparity_bm_cfg_default(bhip_disparity_bm_cfg* c) {
	c->minDisparity = 0; c->rangeDisparity = 100; c->regionRadiusX = 3; c->regionRadiusY = 3; c->maxPerPixelError = 0; c->validateRtoL = 1; c->texture = 0.15;
}
void bhip_surf_cfg_default(bhip_surf_cfg* c) {
	c->widthLargeGrid = 4; c->widthSubRegion = 5; c->widthSample = 3; c->weightSigma = 4.5; c->overLap = 2; c->sigmaLargeGrid = 2.5;
	c->sigmaSubRegion = 2.5;
}
void bhip_ori_cfg_default(bhip_ori_cfg* c, int stable) {
	c->objectRadiusToScale = 1.0 / 2.0;
	c->weightSigma = -1;
	c->sampleWidth = 6;
	if (stable) { c->samplePeriod = 0.65; c->windowSize = M_PI / 3.0; c->radius = 8; }
	else { c->samplePeriod = 1; c->windowSize = 0; c->radius = 6; }
}

int bhip_ctx_create(int device, bhip_ctx** out) { return ctxCreate(device, nullptr, false, out); }
int bhip_ctx_create_on_stream(int device, void* hip_stream, bhip_ctx** out) { return ctxCreate(device, hip_stream, true, out); }
int bhip_ctx_destroy(bhip_ctx* c) {
	if (!c) return BHIP_OK;
	HandleRegistry& R = registry();
	std::lock_guard<std::mutex> lock(R.m);
	if (R.exiting) return BHIP_OK;                        // process teardown: the runtime reclaims everything
	if (!R.ctxs.count(c)) return BHIP_ERR_INVALID;        // not a live context (destroyed twice, or never created)
	R.ctxs.erase(c);
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	for (auto& child : R.children) child.second(child.first, c);   // children still alive on this context become inert shells now
	delete static_cast<bhip_ctx_full*>(c);   // scratch, profiling events, staging block, then the stream it owns
	return BHIP_OK;
}
int bhip_ctx_synchronize(bhip_ctx* ctx) {
	if (!ctx) return BHIP_ERR_INVALID;
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}
const char* bhip_last_error(bhip_ctx* ctx) { return ctx ? ctx->error.c_str() : "null context"; }
// Page-locked host memory for the arrays that cross the boundary (results of bhip_surf_fetch, descriptor lists handed to
// bhip_assoc_l2_f64, frames): copies to and from such memory are DMA transfers at PCIe speed, copies from pageable memory go through
// the runtime's staging buffer (1.1 MB of descriptors: ~0.15 ms instead of ~0.03 ms).  The block belongs to the process, not to the
// context: it stays valid after bhip_ctx_destroy and is released by bhip_host_free (after exit has begun: by the runtime).
int bhip_host_alloc(bhip_ctx* ctx, long long bytes, uint8_t** host_mem) {
	if (!ctx || !host_mem) return BHIP_ERR_INVALID;
	*host_mem = nullptr;
	if (bytes <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bhip_host_alloc: size must be positive");
	BHIP_HIP(ctx, hipSetDevice(ctx->device));
	void* p = nullptr;
	const hipError_t e = hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault);
	if (e != hipSuccess) { (void)hipGetLastError(); return bhip_fail(ctx, BHIP_ERR_NOMEM, "bhip_host_alloc: out of page-locked memory"); }
	*host_mem = (uint8_t*)p;
	return BHIP_OK;
}
int bhip_host_free(void* host_mem) {
	if (!host_mem) return BHIP_OK;
	if (registry().exiting) return BHIP_OK;   // process teardown: the runtime reclaims it
	return hipHostFree(host_mem) == hipSuccess ? BHIP_OK : BHIP_ERR_HIP;
}

int bhip_surf_create(bhip_ctx* ctx, const bhip_fh_cfg* fh, const bhip_surf_cfg* surf, const bhip_ori_cfg* ori, int stable, bhip_surf** out) {
	return createChild(ctx, out, [&](std::unique_ptr<bhip_surf>& s) -> int {
		CHECK_CTX(ctx);
		if (!out) return bhip_fail(ctx, BHIP_ERR_INVALID, "null output");
		*out = nullptr;
		return surfCreateUnregistered(ctx, fh, surf, ori, stable, s);
	});
}

int bhip_surf_destroy(bhip_surf* s) { return destroyChild(s); }

int bhip_surf_dof(bhip_surf* s) { return s ? s->dofOut() : 0; }

int bhip_surf_detect_dev_f32(bhip_surf* s, const float* dev_images, long long imageStride, int stride, int width, int height, int batch) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!dev_images || width <= 0 || height <= 0 || batch <= 0 || stride < width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad image batch");
	return surfRun(s, DevImg<const float>{dev_images, imageStride, stride, width, height, batch}, GREY, SurfReturn::QUEUED);
}

int bhip_surf_detect_f32(bhip_surf* s, const float* const* img, const int* startIndex, const int* stride, int width, int height, int batch) {
	return surfDetectHost(s, img, startIndex, stride, width, height, batch);
}

// FactoryDetectDescribe.surfColorStable / surfColorFast on one Planar<GrayF32> frame:
//   SurfPlanar_to_DetectDescribePoint.detect      F:abst/feature/detdesc/SurfPlanar_to_DetectDescribePoint.java:62-77
//   ImplConvertPlanarToGray.average               I:core/image/impl/ImplConvertPlanarToGray.java:296-336
//   DetectDescribeSurfPlanar.detect / describe    F:alg/feature/detdesc/DetectDescribeSurfPlanar.java:91-124
//   DescribePointSurfPlanar.describe              F:alg/feature/describe/DescribePointSurfPlanar.java:100-114
int bhip_surf_detect_planar_f32(bhip_surf* s, const float* const* bands, int numBands, int startIndex, int stride, int width, int height) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!bands || numBands < 1 || numBands > 16 || width <= 0 || height <= 0 || stride < width) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad planar image");
	const size_t px = (size_t)width * height;
	BHIP_TRY(s->inBuf.reserve(ctx, px * 4 * (1 + numBands)));
	for (int b = 0; b < numBands; b++) {
		if (!bands[b]) return bhip_fail(ctx, BHIP_ERR_INVALID, "null band");
		BHIP_TRY(upload(ctx, s->inBuf.as<float>() + px * (1 + b), width, bands[b], startIndex, stride, width, height, ctx->stream));
	}
	BHIP_TRY(bhip_launch_planar_average(ctx, s->inBuf.as<float>() + px, (long long)px, numBands, (long long)px, s->inBuf.as<float>()));
	return surfRun(s, bhip_img_over<const float>(s->inBuf, width, width, height, 1 + numBands), numBands, SurfReturn::SYNCHRONIZED);
}

// FactoryDetectDescribe.surfStable / surfFast on GrayU8 frames (integral type GrayS32, GIntegralImageOps.getIntegralType): same results
// interface as bhip_surf_detect_f32
int bhip_surf_detect_u8(bhip_surf* s, const uint8_t* const* img, const int* startIndex, const int* stride, int width, int height, int batch) {
	return surfDetectHost(s, img, startIndex, stride, width, height, batch);
}

int bhip_surf_count(bhip_surf* s, int image, int* n) {
	if (!s || !n) return BHIP_ERR_INVALID;
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(s->ctx, BHIP_ERR_INVALID, "no detect result for that image");
	*n = s->det.counts[image];
	return BHIP_OK;
}
// getNumberOfFeatures() of every image of the last detect in one call (a batch-level caller's prefix sums)
int bhip_surf_counts(bhip_surf* s, int* counts, int capacity) {
	if (!s || !counts) return BHIP_ERR_INVALID;
	if (!s->haveResult || capacity < s->batch) return bhip_fail(s->ctx, BHIP_ERR_INVALID, "no detect result / counts array too short");
	for (int i = 0; i < s->batch; i++) counts[i] = s->det.counts[i];
	return BHIP_OK;
}
int bhip_surf_total(bhip_surf* s, long long* n) {
	if (!s || !n) return BHIP_ERR_INVALID;
	*n = s->haveResult ? s->det.total : 0;
	return BHIP_OK;
}

int bhip_surf_fetch(bhip_surf* s, int image, double* xy_scale, double* angle, uint8_t* white, double* desc) {
	// (dof below is the full descriptor length: numBands * 64 after a planar detect)
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result for that image");
	if (desc && s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "this object describes with BRIEF: fetch the words with bhip_surf_fetch_brief");
	const int n = s->det.counts[image];
	if (n == 0) return BHIP_OK;
	const long long off = s->starts[image];
	const int dof = s->dofOut();
	std::vector<KeyPoint> kps;
	if (xy_scale) {
		kps.resize(n);
		BHIP_HIP(ctx, hipMemcpyAsync(kps.data(), s->det.sorted.as<KeyPoint>() + (long long)image * s->det.cap, (size_t)n * sizeof(KeyPoint),
									 hipMemcpyDeviceToHost, ctx->stream));
	}
	if (angle) BHIP_HIP(ctx, hipMemcpyAsync(angle, s->angBuf.as<double>() + off, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (white) BHIP_HIP(ctx, hipMemcpyAsync(white, s->whiteBuf.as<uint8_t>() + off, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
	if (desc) BHIP_HIP(ctx, hipMemcpyAsync(desc, s->descBuf.as<double>() + off * dof, (size_t)n * 8 * dof, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	if (xy_scale)
		for (int i = 0; i < n; i++) { xy_scale[3 * i] = kps[i].x; xy_scale[3 * i + 1] = kps[i].y; xy_scale[3 * i + 2] = kps[i].scale; }
	return BHIP_OK;
}

// the whole batch of the last detect in ONE set of copies (per-image slices start at the exclusive prefix of bhip_surf_count):
// what a batched caller (DetectDescribeSurfHip.detectBatch) uses instead of `batch` bhip_surf_fetch calls
int bhip_surf_fetch_all(bhip_surf* s, double* xy_scale, double* angle, uint8_t* white, double* desc) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->haveResult) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result");
	if (desc && s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "this object describes with BRIEF: fetch the words with bhip_surf_fetch_brief");
	const long long total = s->det.total;
	if (total == 0) return BHIP_OK;
	const int dof = s->dofOut();
	if (xy_scale) {
		// key points sit in [image][cap] KeyPoint records: pack x, y, scale of every image into the compact layout on the device first
		BHIP_TRY(s->xysBuf.reserve(ctx, (size_t)total * 24));
		for (int i = 0; i < s->batch; i++) {
			const int n = s->det.counts[i];
			if (n > 0)
				BHIP_HIP(ctx, hipMemcpy2DAsync((char*)s->xysBuf.p + (size_t)s->starts[i] * 24, 24, s->det.sorted.as<KeyPoint>() + (long long)i * s->det.cap,
											   sizeof(KeyPoint), 24, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
		}
		BHIP_HIP(ctx, hipMemcpyAsync(xy_scale, s->xysBuf.p, (size_t)total * 24, hipMemcpyDeviceToHost, ctx->stream));
	}
	if (angle) BHIP_HIP(ctx, hipMemcpyAsync(angle, s->angBuf.p, (size_t)total * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (white) BHIP_HIP(ctx, hipMemcpyAsync(white, s->whiteBuf.p, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
	if (desc) BHIP_HIP(ctx, hipMemcpyAsync(desc, s->descBuf.p, (size_t)total * 8 * dof, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}

int bhip_surf_dev_view(bhip_surf* s, int image, const double** dev_desc, const double** dev_xy_scale, const uint8_t** dev_white, int* n) {
	if (!s) return BHIP_ERR_INVALID;
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(s->ctx, BHIP_ERR_INVALID, "no detect result for that image");
	const long long off = s->starts[image];
	if (dev_desc) *dev_desc = s->descBuf.as<double>() + off * s->dofOut();
	// key points are KeyPoint records {x,y,scale,key,pad}: 32-byte stride, first three doubles are x,y,scale
	if (dev_xy_scale) *dev_xy_scale = (const double*)(s->det.sorted.as<KeyPoint>() + (long long)image * s->det.cap);
	if (dev_white) *dev_white = s->whiteBuf.as<uint8_t>() + off;
	if (n) *n = s->det.counts[image];
	return BHIP_OK;
}

// FactoryDetectDescribe.fuseTogether(FactoryInterestPoint.fastHessian(fh), null, FactoryDescribeRegionPoint.brief(config, imageType))
// (F:factory/feature/detdesc/FactoryDetectDescribe.java:279-284, F:factory/feature/describe/FactoryDescribeRegionPoint.java:187-202 with
// config.fixed): the returned object is driven through the same bhip_surf_detect_* / _count / _fetch calls as the SURF one.
int bhip_surf_create_brief(bhip_ctx* ctx, const bhip_fh_cfg* fh, int radius, int numPoints, const int32_t* samplePoints, const int32_t* compare, bhip_surf** out) {
	return createChild(ctx, out, [&](std::unique_ptr<bhip_surf>& s) -> int {
		CHECK_CTX(ctx);
		if (!out) return bhip_fail(ctx, BHIP_ERR_INVALID, "null output");
		*out = nullptr;
		if (radius < 0 || numPoints <= 0 || !samplePoints || !compare) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad BRIEF definition");
		int maxIdx = 0;
		for (int i = 0; i < 2 * numPoints; i++) {
			if (compare[i] < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "negative sample index");
			maxIdx = std::max(maxIdx, compare[i]);
		}
		BHIP_TRY(surfCreateUnregistered(ctx, fh, nullptr, nullptr, 0, s));   // (the SURF tables of the shell are never used)
		s->brief = true;
		s->briefRadius = radius; s->briefPoints = numPoints; s->briefWords = (numPoints + 31) / 32;
		const size_t nSample = (size_t)(maxIdx + 1) * 2, nCompare = (size_t)numPoints * 2;
		s->briefCompareOff = nSample;
		s->briefPatch = briefPatchOk(samplePoints, maxIdx + 1, radius);
		BHIP_TRY(s->briefTab.reserve(ctx, (nSample + nCompare) * 4));
		if (hipMemcpy(s->briefTab.p, samplePoints, nSample * 4, hipMemcpyHostToDevice) != hipSuccess) return bhip_fail(ctx, BHIP_ERR_HIP, "BRIEF table upload");
		if (hipMemcpy(s->briefTab.as<int>() + nSample, compare, nCompare * 4, hipMemcpyHostToDevice) != hipSuccess) return bhip_fail(ctx, BHIP_ERR_HIP, "BRIEF table upload");
		return BHIP_OK;
	});
}

// getDescription(i).data of every feature of one image (image >= 0: count * words ints) or of the whole batch (image = -1: total * words
// ints, image i's slice at the exclusive prefix of the counts); words = ceil(numPoints / 32) (TupleDesc_B, T:struct/feature/TupleDesc_B.java)
int bhip_surf_fetch_brief(bhip_surf* s, int image, int32_t* words) {
	if (!s || !words) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "not a BRIEF detect+describe object");
	if (!s->haveResult || image < -1 || image >= s->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result for that image");
	const long long off = image < 0 ? 0 : s->starts[image];
	const long long n = image < 0 ? s->det.total : s->det.counts[image];
	if (n == 0) return BHIP_OK;
	BHIP_HIP(ctx, hipMemcpyAsync(words, s->wordsBuf.as<int>() + off * s->briefWords, (size_t)n * 4 * s->briefWords, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}
int bhip_surf_dev_view_brief(bhip_surf* s, int image, const int32_t** dev_words, int* words, int* n) {
	if (!s) return BHIP_ERR_INVALID;
	if (!s->brief) return bhip_fail(s->ctx, BHIP_ERR_INVALID, "not a BRIEF detect+describe object");
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(s->ctx, BHIP_ERR_INVALID, "no detect result for that image");
	if (dev_words) *dev_words = s->wordsBuf.as<int>() + (long long)s->starts[image] * s->briefWords;
	if (words) *words = s->briefWords;
	if (n) *n = s->det.counts[image];
	return BHIP_OK;
}

int bhip_surf_fetch_integral(bhip_surf* s, int image, float* out) {
	if (!s || !out) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result for that image");
	BHIP_HIP(ctx, hipMemcpyAsync(out, s->iiBuf.as<float>() + (long long)image * s->W * s->H, (size_t)s->W * s->H * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}

int bhip_surf_describe_points(bhip_surf* s, int image, const double* xy_scale, int n, double* angle, uint8_t* white, double* desc) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->haveResult || image < 0 || image >= s->batch) return bhip_fail(ctx, BHIP_ERR_INVALID, "no detect result for that image");
	if (s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "this object describes with BRIEF");
	if (n < 0 || (n > 0 && !xy_scale)) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad point list");
	if (n == 0) return BHIP_OK;
	std::vector<KeyPoint> kps(n);
	for (int i = 0; i < n; i++) { kps[i].x = xy_scale[3 * i]; kps[i].y = xy_scale[3 * i + 1]; kps[i].scale = xy_scale[3 * i + 2]; kps[i].key = 0; kps[i].pad = 0; }
	const int dof = s->dofOut();
	BHIP_TRY(s->tmpKp.reserve(ctx, (size_t)n * sizeof(KeyPoint)));
	BHIP_TRY(s->tmpAng.reserve(ctx, (size_t)n * 8));
	BHIP_TRY(s->tmpDesc.reserve(ctx, (size_t)n * 8 * dof));
	BHIP_TRY(s->tmpWhite.reserve(ctx, (size_t)n));
	BHIP_TRY(scratchOf(ctx)->describeQueue.reserve(ctx, BHIP_DESCRIBE_QUEUE_BYTES));
	BHIP_HIP(ctx, hipMemcpyAsync(s->tmpKp.p, kps.data(), (size_t)n * sizeof(KeyPoint), hipMemcpyHostToDevice, ctx->stream));
	BHIP_TRY(withIntegral(s, [&](auto ii) {
		return bhip_launch_describe_ex(ctx, ii, s->tmpKp.as<KeyPoint>(), 0, nullptr, image, n, s->tables, nullptr, s->tmpAng.as<double>(),
									   s->tmpDesc.as<double>(), s->tmpWhite.as<uint8_t>(), nullptr, scratchOf(ctx)->describeQueue.as<int>(), s->planar());
	}));
	if (angle) BHIP_HIP(ctx, hipMemcpyAsync(angle, s->tmpAng.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
	if (white) BHIP_HIP(ctx, hipMemcpyAsync(white, s->tmpWhite.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
	if (desc) BHIP_HIP(ctx, hipMemcpyAsync(desc, s->tmpDesc.p, (size_t)n * 8 * dof, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}

int bhip_fh_detect_f32(bhip_ctx* ctx, const bhip_fh_cfg* cfg, const float* ii, int iiStart, int iiStride, int width, int height, double* xy_scale,
					   int cap, int* n) {
	return fhDetect<float>(ctx, cfg, {ii, iiStart, iiStride, width, height}, xy_scale, cap, n);
}
int bhip_fh_detect_s32(bhip_ctx* ctx, const bhip_fh_cfg* cfg, const int32_t* ii, int iiStart, int iiStride, int width, int height, double* xy_scale,
					   int cap, int* n) {
	return fhDetect<int32_t>(ctx, cfg, {ii, iiStart, iiStride, width, height}, xy_scale, cap, n);
}

// AssociateDescription<TupleDesc_B>.associate() with ScoreAssociateHamming_B on the words still resident from the last detect of a BRIEF
// object: same contract as bhip_assoc_l2_surf, same rules and results as bhip_assoc_hamming, no descriptor upload.
int bhip_assoc_hamming_surf(bhip_surf* s, int count, const int* srcImage, const int* dstImage, double maxErr, int backwards, int* pairs, double* fit) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (!s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "not a BRIEF detect+describe object");
	const int32_t* W = s->wordsBuf.as<int32_t>();
	return assocSurf(s, count, srcImage, dstImage, pairs, fit, [&](const long long* so, const int* ns, const long long* doff, const int* nd, int* dp, double* df) {
		return bhip_assoc_hamming_batched(ctx, W, W, s->briefWords, count, so, ns, doff, nd, maxErr, backwards, dp, df, scratchOf(ctx)->work);
	});
}

// AssociateDescription over descriptors that are still resident from the last detect of `s` (FastQueue<BrightFeature> lists a provider
// recognises as its own): problem p associates image srcImage[p] (source) with image dstImage[p] (destination) -- same rules as
// bhip_assoc_l2_f64, no descriptor upload.  pairs / fit are host arrays over the compact key-point index space of the batch: the results
// of problem p start at the exclusive prefix of the counts of srcImage[p] (every image may be a source at most once per call).
int bhip_assoc_l2_surf(bhip_surf* s, int count, const int* srcImage, const int* dstImage, double maxErr, int backwards, int* pairs, double* fit) {
	if (!s) return BHIP_ERR_INVALID;
	bhip_ctx* ctx = s->ctx;
	CHECK_CTX(ctx);
	if (s->brief) return bhip_fail(ctx, BHIP_ERR_INVALID, "this object describes with BRIEF: use bhip_assoc_hamming_surf");
	const double* D = s->descBuf.as<double>();
	return assocSurf(s, count, srcImage, dstImage, pairs, fit, [&](const long long* so, const int* ns, const long long* doff, const int* nd, int* dp, double* df) {
		return bhip_assoc_l2_dev_batched(ctx, D, D, s->dofOut(), count, so, ns, doff, nd, maxErr, backwards, dp, df);
	});
}

}  // extern "C"
