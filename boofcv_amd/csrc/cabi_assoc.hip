// ---------------------------------------------------------------------------------------------------------------
// association
// ---------------------------------------------------------------------------------------------------------------
// greedy L2 / Hamming on host lists, device lists, batches of problems, and the two phases of the sharded form
#include "cabi.h"

static bool assocExactOnly(bhip_ctx* ctx) {
	CtxScratch* sc = scratchOf(ctx);
	if (sc->assocExactOnly < 0) {
		const char* e = getenv("BHIP_ASSOC_EXACT");
		sc->assocExactOnly = (e && e[0] == '1') ? 1 : 0;
	}
	return sc->assocExactOnly == 1;
}

static int assocL2Exact(bhip_ctx* ctx, const double* dev_src, int ns, const double* dev_dst, int nd, int dof, double maxErr, int backwards,
						int sqrtScore, int* dev_pairs, double* dev_fit) {
	CtxScratch* sc = scratchOf(ctx);
	void* col = nullptr;
	if (backwards && nd > 0) { BHIP_TRY(sc->assocCol.reserve(ctx, (size_t)nd * bhip_assoc_coltop_size())); col = sc->assocCol.p; }
	BHIP_TRY(bhip_assoc_phase1_l2(ctx, dev_src, ns, 0, dev_dst, nd, dof, maxErr, sqrtScore, dev_pairs, dev_fit, col, sc->work));
	if (col) BHIP_TRY(bhip_assoc_phase2(ctx, col, 1, nd, ns, 0, dev_pairs, dev_fit));
	return BHIP_OK;
}

template <class E>
static int assocHost(bhip_ctx* ctx, bool hamming, const E* src, int ns, const E* dst, int nd, int len, double maxErr, int backwards, int sqrtScore,
					 int* pairs, double* fit) {
	if (ns < 0 || nd < 0 || len <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
	if (ns == 0) return BHIP_OK;
	if (!src || (nd > 0 && !dst) || !pairs || !fit) return bhip_fail(ctx, BHIP_ERR_INVALID, "null buffer");
	CtxScratch* sc = scratchOf(ctx);
	BHIP_TRY(sc->in0.reserve(ctx, (size_t)ns * len * sizeof(E)));
	BHIP_TRY(sc->in1.reserve(ctx, (size_t)std::max(nd, 1) * len * sizeof(E)));
	BHIP_TRY(sc->out0.reserve(ctx, (size_t)ns * 4));
	BHIP_TRY(sc->out1.reserve(ctx, (size_t)ns * 8));
	BHIP_HIP(ctx, hipMemcpyAsync(sc->in0.p, src, (size_t)ns * len * sizeof(E), hipMemcpyHostToDevice, ctx->stream));
	if (nd > 0) BHIP_HIP(ctx, hipMemcpyAsync(sc->in1.p, dst, (size_t)nd * len * sizeof(E), hipMemcpyHostToDevice, ctx->stream));
	if (hamming) BHIP_TRY(bhip_assoc_hamming_dev(ctx, sc->in0.as<int32_t>(), ns, sc->in1.as<int32_t>(), nd, len, maxErr, backwards, sc->out0.as<int>(), sc->out1.as<double>()));
	else BHIP_TRY(bhip_assoc_l2_dev(ctx, sc->in0.as<double>(), ns, sc->in1.as<double>(), nd, len, maxErr, backwards, sqrtScore, sc->out0.as<int>(), sc->out1.as<double>()));
	BHIP_HIP(ctx, hipMemcpyAsync(pairs, sc->out0.p, (size_t)ns * 4, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipMemcpyAsync(fit, sc->out1.p, (size_t)ns * 8, hipMemcpyDeviceToHost, ctx->stream));
	BHIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return BHIP_OK;
}

extern "C" {

int bhip_assoc_coltop_bytes(void) { return bhip_assoc_coltop_size(); }

int bhip_assoc_l2_dev(bhip_ctx* ctx, const double* dev_src, int ns, const double* dev_dst, int nd, int dof, double maxErr, int backwards,
					  int sqrtScore, int* dev_pairs, double* dev_fit) {
	CHECK_CTX(ctx);
	if (ns < 0 || nd < 0 || dof <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
	if (ns == 0) return BHIP_OK;
	if (dof == 64 && !sqrtScore && nd > 0 && !assocExactOnly(ctx)) {
		// matrix-core path (fp32 MFMA candidates + exact fp64 re-score); falls through on degenerate inputs
		const long long zero = 0;
		int used = 0;
		BHIP_TRY(bhip_assoc_l2_mfma_batched(ctx, scratchOf(ctx)->mfma, dev_src, dev_dst, 1, &zero, &ns, &zero, &nd, maxErr, backwards, dev_pairs, dev_fit,
											&used));
		if (used) return BHIP_OK;
	}
	return assocL2Exact(ctx, dev_src, ns, dev_dst, nd, dof, maxErr, backwards, sqrtScore, dev_pairs, dev_fit);
}

int bhip_assoc_hamming_dev(bhip_ctx* ctx, const int32_t* dev_src, int ns, const int32_t* dev_dst, int nd, int words, double maxErr, int backwards,
						   int* dev_pairs, double* dev_fit) {
	CHECK_CTX(ctx);
	if (ns < 0 || nd < 0 || words <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
	if (ns == 0) return BHIP_OK;
	CtxScratch* sc = scratchOf(ctx);
	void* col = nullptr;
	if (backwards && nd > 0) { BHIP_TRY(sc->assocCol.reserve(ctx, (size_t)nd * bhip_assoc_coltop_size())); col = sc->assocCol.p; }
	BHIP_TRY(bhip_assoc_phase1_ham(ctx, dev_src, ns, 0, dev_dst, nd, words, maxErr, dev_pairs, dev_fit, col, sc->work));
	if (col) BHIP_TRY(bhip_assoc_phase2(ctx, col, 1, nd, ns, 0, dev_pairs, dev_fit));
	return BHIP_OK;
}

int bhip_assoc_l2_dev_batched(bhip_ctx* ctx, const double* dev_src, const double* dev_dst, int dof, int count, const long long* srcOff, const int* ns,
							  const long long* dstOff, const int* nd, double maxErr, int backwards, int* dev_pairs, double* dev_fit) {
	CHECK_CTX(ctx);
	if (count < 0 || dof <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
	if (count == 0) return BHIP_OK;
	if (!srcOff || !ns || !dstOff || !nd) return bhip_fail(ctx, BHIP_ERR_INVALID, "null problem table");
	if (dof == 64 && !assocExactOnly(ctx)) {
		int used = 0;
		BHIP_TRY(bhip_assoc_l2_mfma_batched(ctx, scratchOf(ctx)->mfma, dev_src, dev_dst, count, srcOff, ns, dstOff, nd, maxErr, backwards, dev_pairs,
											dev_fit, &used));
		if (used) return BHIP_OK;
	}
	for (int p = 0; p < count; p++) {
		if (ns[p] < 0 || nd[p] < 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
		if (ns[p] == 0) continue;
		BHIP_TRY(assocL2Exact(ctx, dev_src + srcOff[p] * dof, ns[p], dev_dst + dstOff[p] * dof, nd[p], dof, maxErr, backwards, 0, dev_pairs + srcOff[p],
							  dev_fit + srcOff[p]));
	}
	return BHIP_OK;
}

// batched device form of bhip_assoc_hamming_dev (contract of bhip_assoc_l2_dev_batched): many small problems in three launches
int bhip_assoc_hamming_dev_batched(bhip_ctx* ctx, const int32_t* dev_src, const int32_t* dev_dst, int words, int count, const long long* srcOff, const int* ns,
								   const long long* dstOff, const int* nd, double maxErr, int backwards, int* dev_pairs, double* dev_fit) {
	CHECK_CTX(ctx);
	if (count < 0 || words <= 0) return bhip_fail(ctx, BHIP_ERR_INVALID, "bad sizes");
	if (count == 0) return BHIP_OK;
	if (!srcOff || !ns || !dstOff || !nd || !dev_pairs || !dev_fit) return bhip_fail(ctx, BHIP_ERR_INVALID, "null problem table");
	return bhip_assoc_hamming_batched(ctx, dev_src, dev_dst, words, count, srcOff, ns, dstOff, nd, maxErr, backwards, dev_pairs, dev_fit, scratchOf(ctx)->work);
}

int bhip_assoc_l2_f64(bhip_ctx* ctx, const double* src, int ns, const double* dst, int nd, int dof, double maxErr, int backwards, int sqrtScore,
					  int* pairs, double* fit) {
	CHECK_CTX(ctx);
	return assocHost<double>(ctx, false, src, ns, dst, nd, dof, maxErr, backwards, sqrtScore, pairs, fit);
}
int bhip_assoc_hamming(bhip_ctx* ctx, const int32_t* src, int ns, const int32_t* dst, int nd, int words, double maxErr, int backwards, int* pairs,
					   double* fit) {
	CHECK_CTX(ctx);
	return assocHost<int32_t>(ctx, true, src, ns, dst, nd, words, maxErr, backwards, 0, pairs, fit);
}

int bhip_assoc_l2_shard_phase1(bhip_ctx* ctx, const double* dev_src, int nsLocal, int srcBegin, const double* dev_dst, int nd, int dof, double maxErr,
							   int* dev_pairs, double* dev_fit, void* dev_colTop) {
	CHECK_CTX(ctx);
	if (!dev_colTop) return bhip_fail(ctx, BHIP_ERR_INVALID, "null column buffer");
	return bhip_assoc_phase1_l2(ctx, dev_src, nsLocal, srcBegin, dev_dst, nd, dof, maxErr, 0, dev_pairs, dev_fit, dev_colTop, scratchOf(ctx)->work);
}
int bhip_assoc_hamming_shard_phase1(bhip_ctx* ctx, const int32_t* dev_src, int nsLocal, int srcBegin, const int32_t* dev_dst, int nd, int words,
									double maxErr, int* dev_pairs, double* dev_fit, void* dev_colTop) {
	CHECK_CTX(ctx);
	if (!dev_colTop) return bhip_fail(ctx, BHIP_ERR_INVALID, "null column buffer");
	return bhip_assoc_phase1_ham(ctx, dev_src, nsLocal, srcBegin, dev_dst, nd, words, maxErr, dev_pairs, dev_fit, dev_colTop, scratchOf(ctx)->work);
}
int bhip_assoc_shard_phase2(bhip_ctx* ctx, const void* dev_colTopAll, int nranks, int nd, int nsLocal, int srcBegin, int* dev_pairs, double* dev_fit) {
	CHECK_CTX(ctx);
	if (nranks < 1) return bhip_fail(ctx, BHIP_ERR_INVALID, "nranks < 1");
	return bhip_assoc_phase2(ctx, dev_colTopAll, nranks, nd, nsLocal, srcBegin, dev_pairs, dev_fit);
}

}  // extern "C"
