// The sequential QuickSelect that detect.hip (N best per scale) and sift.hip (NonMaxLimiter) both run on one lane.
#ifndef BHIP_SELECT_DEV_H
#define BHIP_SELECT_DEV_H
// org.ddogleg.sorting.QuickSelect.selectIndex(data, k, n, indexes) as the oracle restates it (quickSelectIndex): the exchange sequence decides
// the output order and which of several equal keys survive, so it is not parallelised.  Permutes data[0 .. n) and indexes[0 .. n) in place.
static __device__ void quickSelectIndexSeq(float* data, int k, int n, int* indexes) {
	int l = 0, ir = n - 1;
#define QS_SWAP(a_, b_) do { const float tf = data[a_]; data[a_] = data[b_]; data[b_] = tf; const int ti = indexes[a_]; indexes[a_] = indexes[b_]; indexes[b_] = ti; } while (0)
	for (;;) {
		if (ir <= l + 1) {
			if (ir == l + 1 && data[ir] < data[l]) QS_SWAP(l, ir);
			return;
		}
		const int mid = (l + ir) >> 1, lp1 = l + 1;
		QS_SWAP(mid, lp1);
		if (data[l] > data[ir]) QS_SWAP(l, ir);
		if (data[lp1] > data[ir]) QS_SWAP(lp1, ir);
		if (data[l] > data[lp1]) QS_SWAP(l, lp1);
		int i = lp1, j = ir;
		const float a = data[lp1];
		const int indexA = indexes[lp1];
		for (;;) {
			do i++; while (data[i] < a);   // data[ir] >= a and data[l] <= a are the sentinels, as in the sequential routine
			do j--; while (data[j] > a);
			if (j < i) break;
			QS_SWAP(i, j);
		}
		data[lp1] = data[j]; data[j] = a;
		indexes[lp1] = indexes[j]; indexes[j] = indexA;
		if (j >= k) ir = j - 1;
		if (j <= k) l = i;
	}
#undef QS_SWAP
}

#endif
