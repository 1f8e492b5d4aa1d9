// burst_amd/csrc/bhip_mates.hip -- the join of two mates' printed placements into concordant combinations (burst_hip --mates;
// bhip_mates_join, gfx950).  No reference counterpart: the reference lists paired-end alignment as planned and gives the recipe (align both
// mates in ALLPATHS mode, keep the references both map to with acceptable orientation and distance); this is that last step.
//
// Definition (README "Paired-end reads", DESIGN.md section 3 "Mates").  A line is (pair, ref, st, ed, edits): the pair its read belongs
// to, the header it was placed on (both dense numbers of the caller), .b6 columns 9 and 10 as signed numbers, column 11.  It is REVERSE
// when st > ed; lo / hi = the smaller / larger of st and ed.  A combination is a line a of mate 1 and a line b of mate 2 with equal
// (pair, ref).  The orientation names which of the two is the upstream line U and which the downstream line D:
//   fr   exactly one of them is reverse: U = the forward one, D = the reverse one
//   rf   exactly one of them is reverse: U = the reverse one, D = the forward one
//   ff   both forward: U = a, D = b; both reverse: U = b, D = a
// and the combination is concordant when U.lo <= D.lo, U.hi <= D.hi and ins_min <= D.hi - U.lo + 1 <= ins_max.
//
// The device work.  Side b gets 64-bit keys pair << 32 | ref and is sorted by them together with its line numbers (hipcub radix sort:
// stable, so the line numbers ascend inside a key).  Then ONE THREAD PER LINE OF a finds the run of its key by binary search and walks it
// serially.  Why serial: a run is one read's placements on one header -- in ALLPATHS the minimum-edit ties, mostly 1, a handful in a
// repeat -- so there is nothing for a wave to share; what bounds it is the number of placements FORAGE prints for one read on one header,
// which a repeat-rich reference can make long (thousands).  The walk is then only slower: it is bounded by the end of the array and the
// key, never by an assumed length, and a wave waits for its longest walker.
//   all    k_mates_count (concordant combinations per line of a) -> exclusive scan (64-bit) -> k_mates_emit repeats the walk and writes
//          (a, b) at its offset: ascending a, ascending b inside a.
//   best   k_mates_best_key: atomicMin of (edit sum << 32 | a) per pair, as k_best_key does for records -- the minimum is the smallest edit
//          sum and among those the smallest a; k_mates_count then gives 1 to the line of a that holds its pair's minimum and remembers the
//          first b of its run (the smallest) that attains the sum; scan and emit as above.
// Index arithmetic is 64-bit wherever a line number or an offset is formed; every buffer is a grow-only one of the handle.
#include "bhip_handle.h"

#define MATES_BLOCK 256
#define MATES_MAX_GRID 65536u

struct MatesParams { uint64_t na, nb; uint32_t orientation, best; long long ins_min, ins_max; };

__device__ __forceinline__ bool mates_concordant(const BhipMateLine &a, const BhipMateLine &b, const MatesParams &P) {
	const bool ra = a.st > a.ed, rb = b.st > b.ed;
	bool a_up;
	if (P.orientation == BHIP_MATES_FF) { if (ra != rb) return false; a_up = !ra; }
	else { if (ra == rb) return false; a_up = (P.orientation == BHIP_MATES_FR) ? !ra : ra; }
	const BhipMateLine &U = a_up ? a : b, &D = a_up ? b : a;
	const long long ulo = U.st < U.ed ? U.st : U.ed, uhi = U.st < U.ed ? U.ed : U.st;
	const long long dlo = D.st < D.ed ? D.st : D.ed, dhi = D.st < D.ed ? D.ed : D.st;
	const long long len = dhi - ulo + 1;
	return ulo <= dlo && uhi <= dhi && len >= P.ins_min && len <= P.ins_max;
}
__device__ __forceinline__ unsigned long long mates_key(const BhipMateLine &l) { return (unsigned long long)l.pair << 32 | l.ref; }
__device__ __forceinline__ uint32_t mates_edit_sum(const BhipMateLine &a, const BhipMateLine &b) {
	const unsigned long long s = (unsigned long long)a.edits + b.edits;
	return s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
}
// first position of the sorted keys that is not below `key`
__device__ __forceinline__ uint64_t mates_lower_bound(const unsigned long long *__restrict__ keys, uint64_t n, unsigned long long key) {
	uint64_t lo = 0, hi = n;
	while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (keys[mid] < key) lo = mid + 1; else hi = mid; }
	return lo;
}

__global__ __launch_bounds__(MATES_BLOCK) void k_mates_keys(const BhipMateLine *__restrict__ b, uint64_t nb, unsigned long long *__restrict__ key, uint32_t *__restrict__ idx) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nb; i += (uint64_t)gridDim.x * blockDim.x) { key[i] = mates_key(b[i]); idx[i] = (uint32_t)i; }
}

// best[pair] = min over the pair's concordant combinations of (edit sum << 32 | a); best was filled with ones
__global__ __launch_bounds__(MATES_BLOCK) void k_mates_best_key(const BhipMateLine *__restrict__ a, const BhipMateLine *__restrict__ b,
		const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ idx, MatesParams P, unsigned long long *__restrict__ best) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < P.na; i += (uint64_t)gridDim.x * blockDim.x) {
		const BhipMateLine la = a[i];
		const unsigned long long key = mates_key(la);
		uint32_t mn = 0; bool any = false;
		for (uint64_t j = mates_lower_bound(keys, P.nb, key); j < P.nb && keys[j] == key; ++j) {
			const BhipMateLine lb = b[idx[j]];
			if (!mates_concordant(la, lb, P)) continue;
			const uint32_t s = mates_edit_sum(la, lb);
			if (!any || s < mn) { mn = s; any = true; }
		}
		if (any) atomicMin(&best[la.pair], (unsigned long long)mn << 32 | (unsigned long long)i);
	}
}

// cnt[i] = combinations line i of a reports: all = its concordant ones; best = 1 when it holds its pair's minimum, sel[i] = the b to report
__global__ __launch_bounds__(MATES_BLOCK) void k_mates_count(const BhipMateLine *__restrict__ a, const BhipMateLine *__restrict__ b,
		const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ idx, MatesParams P, const unsigned long long *__restrict__ best,
		unsigned long long *__restrict__ cnt, uint32_t *__restrict__ sel) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < P.na; i += (uint64_t)gridDim.x * blockDim.x) {
		const BhipMateLine la = a[i];
		const unsigned long long key = mates_key(la);
		unsigned long long c = 0;
		if (P.best) {
			const unsigned long long w = best[la.pair];
			if ((w & 0xFFFFFFFFull) == i && w != ~0ull) {
				const uint32_t want = (uint32_t)(w >> 32);
				for (uint64_t j = mates_lower_bound(keys, P.nb, key); j < P.nb && keys[j] == key; ++j) {
					const BhipMateLine lb = b[idx[j]];
					if (mates_concordant(la, lb, P) && mates_edit_sum(la, lb) == want) { sel[i] = idx[j]; c = 1; break; }
				}
			}
		} else {
			for (uint64_t j = mates_lower_bound(keys, P.nb, key); j < P.nb && keys[j] == key; ++j) c += mates_concordant(la, b[idx[j]], P) ? 1ull : 0ull;
		}
		cnt[i] = c;
	}
}

// off = the exclusive scan of cnt; the walk again, this time writing
__global__ __launch_bounds__(MATES_BLOCK) void k_mates_emit(const BhipMateLine *__restrict__ a, const BhipMateLine *__restrict__ b,
		const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ idx, MatesParams P, const unsigned long long *__restrict__ off,
		const uint32_t *__restrict__ sel, uint64_t n_total, uint32_t *__restrict__ out_a, uint32_t *__restrict__ out_b) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < P.na; i += (uint64_t)gridDim.x * blockDim.x) {
		unsigned long long o = off[i];
		const unsigned long long end = off[i + 1];
		if (o == end || end > n_total) continue;
		if (P.best) { out_a[o] = (uint32_t)i; out_b[o] = sel[i]; continue; }
		const BhipMateLine la = a[i];
		const unsigned long long key = mates_key(la);
		for (uint64_t j = mates_lower_bound(keys, P.nb, key); j < P.nb && keys[j] == key && o < end; ++j)
			if (mates_concordant(la, b[idx[j]], P)) { out_a[o] = (uint32_t)i; out_b[o] = idx[j]; ++o; }
	}
}

struct MatesState {
	DBuf a, b, key, key_s, idx, idx_s, tmp, best, cnt, off, sel, out_a, out_b;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	uint64_t us_last = 0, us_total = 0, n_lines = 0, n_comb = 0;
};

// (bhip_handle.h: Handle::mates)
void bhip_mates_release(Handle *h) {
	MatesState *st = (MatesState *)h->mates;
	if (!st) return;
	DBuf *all[] = {&st->a, &st->b, &st->key, &st->key_s, &st->idx, &st->idx_s, &st->tmp, &st->best, &st->cnt, &st->off, &st->sel, &st->out_a, &st->out_b};
	for (DBuf *x : all) x->release();
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->mates = nullptr;
}

static inline uint32_t mates_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + MATES_BLOCK - 1) / MATES_BLOCK, MATES_MAX_GRID); }
static inline int bits_of(uint32_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

extern "C" int bhip_mates_join(void *handle, const BhipMateLine *a, uint64_t na, const BhipMateLine *b, uint64_t nb, uint32_t orientation,
		uint32_t ins_min, uint32_t ins_max, uint32_t report, uint32_t *out_a, uint32_t *out_b, uint64_t cap, uint64_t *n_out) {
	Handle *h = (Handle *)handle;
	if (!h || !n_out || (na && !a) || (nb && !b) || (cap && (!out_a || !out_b))) return fail(BHIP_E_ARG, "bhip_mates_join: null argument");
	*n_out = 0;
	if (orientation > BHIP_MATES_FF) return fail(BHIP_E_ARG, "bhip_mates_join: orientation %u (0 fr, 1 rf, 2 ff)", orientation);
	if (report > BHIP_MATES_BEST) return fail(BHIP_E_ARG, "bhip_mates_join: report %u (0 all, 1 best)", report);
	if (ins_min > ins_max) return fail(BHIP_E_ARG, "bhip_mates_join: insert bounds %u > %u", ins_min, ins_max);
	if (na >= (1ull << 32) || nb >= (1ull << 32)) return fail(BHIP_E_ARG, "bhip_mates_join: %llu and %llu lines (fewer than 2^32 each)", (unsigned long long)na, (unsigned long long)nb);
	// pair numbers index the table of the per-pair minimum: dense means not far beyond the number of lines
	uint32_t max_pair_a = 0, max_pair_b = 0;
	for (uint64_t i = 0; i < na; ++i) max_pair_a = std::max(max_pair_a, a[i].pair);
	for (uint64_t i = 0; i < nb; ++i) max_pair_b = std::max(max_pair_b, b[i].pair);
	if (report == BHIP_MATES_BEST && (uint64_t)max_pair_a + 1 > 4 * (na + nb) + (1ull << 20))
		return fail(BHIP_E_ARG, "bhip_mates_join: pair number %u with %llu lines: pair numbers must be dense", max_pair_a, (unsigned long long)(na + nb));
	if (!na || !nb) return BHIP_OK;      // (nothing to join: no launch, the counters of the last call stay)
	HIPCHK(hipSetDevice(h->device));
	MatesState *st = (MatesState *)h->mates;
	if (!st) {
		st = new MatesState();
		h->mates = st;
		if (hipEventCreate(&st->ev0) != hipSuccess || hipEventCreate(&st->ev1) != hipSuccess) { bhip_mates_release(h); return fail(BHIP_E_DEVICE, "hipEventCreate failed"); }
	}
	st->us_last = 0;
	const bool best = report == BHIP_MATES_BEST;
	const uint64_t n_pairs = (uint64_t)max_pair_a + 1;
	int rc = st->a.reserve(na * sizeof(BhipMateLine)); if (rc) return rc;
	rc = st->b.reserve(nb * sizeof(BhipMateLine)); if (rc) return rc;
	rc = st->key.reserve(nb * 8); if (rc) return rc;
	rc = st->key_s.reserve(nb * 8); if (rc) return rc;
	rc = st->idx.reserve(nb * 4); if (rc) return rc;
	rc = st->idx_s.reserve(nb * 4); if (rc) return rc;
	rc = st->cnt.reserve((na + 1) * 8); if (rc) return rc;
	rc = st->off.reserve((na + 1) * 8); if (rc) return rc;
	if (best) { rc = st->best.reserve(n_pairs * 8); if (rc) return rc; rc = st->sel.reserve(na * 4); if (rc) return rc; }
	const int end_bit = 32 + std::max(1, bits_of(max_pair_b));
	size_t tb_sort = 0, tb_scan = 0;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, st->key.as<unsigned long long>(), st->key_s.as<unsigned long long>(), st->idx.as<uint32_t>(), st->idx_s.as<uint32_t>(),
		(size_t)nb, 0, end_bit, h->stream));
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, st->cnt.as<unsigned long long>(), st->off.as<unsigned long long>(), (size_t)(na + 1), h->stream));
	rc = st->tmp.reserve(std::max(tb_sort, tb_scan) + 16); if (rc) return rc;

	MatesParams P;
	P.na = na; P.nb = nb; P.orientation = orientation; P.best = best ? 1u : 0u; P.ins_min = (long long)ins_min; P.ins_max = (long long)ins_max;
	const BhipMateLine *da = st->a.as<BhipMateLine>(), *db = st->b.as<BhipMateLine>();
	const unsigned long long *ks = st->key_s.as<unsigned long long>();
	const uint32_t *is = st->idx_s.as<uint32_t>();
	HIPCHK(hipMemcpyAsync(st->a.p, a, na * sizeof(BhipMateLine), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(st->b.p, b, nb * sizeof(BhipMateLine), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipEventRecord(st->ev0, h->stream));
	hipLaunchKernelGGL(k_mates_keys, dim3(mates_grid(nb)), dim3(MATES_BLOCK), 0, h->stream, db, nb, st->key.as<unsigned long long>(), st->idx.as<uint32_t>());
	HIPCHK(hipGetLastError());
	size_t tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, st->key.as<unsigned long long>(), st->key_s.as<unsigned long long>(), st->idx.as<uint32_t>(), st->idx_s.as<uint32_t>(),
		(size_t)nb, 0, end_bit, h->stream));
	if (best) {
		HIPCHK(hipMemsetAsync(st->best.p, 0xFF, n_pairs * 8, h->stream));
		hipLaunchKernelGGL(k_mates_best_key, dim3(mates_grid(na)), dim3(MATES_BLOCK), 0, h->stream, da, db, ks, is, P, st->best.as<unsigned long long>());
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipMemsetAsync((char *)st->cnt.p + na * 8, 0, 8, h->stream));      // (the scan's extra element: off[na] = the total)
	hipLaunchKernelGGL(k_mates_count, dim3(mates_grid(na)), dim3(MATES_BLOCK), 0, h->stream, da, db, ks, is, P, st->best.as<unsigned long long>(),
		st->cnt.as<unsigned long long>(), st->sel.as<uint32_t>());
	HIPCHK(hipGetLastError());
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(st->tmp.p, tb, st->cnt.as<unsigned long long>(), st->off.as<unsigned long long>(), (size_t)(na + 1), h->stream));
	HIPCHK(hipEventRecord(st->ev1, h->stream));
	unsigned long long total = 0;
	HIPCHK(hipMemcpyAsync(&total, (char *)st->off.p + na * 8, 8, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	st->us_last += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	*n_out = total;
	if (total <= cap && total) {
		rc = st->out_a.reserve(total * 4); if (rc) return rc;
		rc = st->out_b.reserve(total * 4); if (rc) return rc;
		HIPCHK(hipEventRecord(st->ev0, h->stream));
		hipLaunchKernelGGL(k_mates_emit, dim3(mates_grid(na)), dim3(MATES_BLOCK), 0, h->stream, da, db, ks, is, P, st->off.as<unsigned long long>(), st->sel.as<uint32_t>(),
			(uint64_t)total, st->out_a.as<uint32_t>(), st->out_b.as<uint32_t>());
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(st->ev1, h->stream));
		HIPCHK(hipMemcpyAsync(out_a, st->out_a.p, total * 4, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipMemcpyAsync(out_b, st->out_b.p, total * 4, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
		st->us_last += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	}
	st->us_total += st->us_last;
	if (total <= cap) { st->n_lines += na + nb; st->n_comb += total; }
	else return fail(BHIP_E_CAPACITY, "bhip_mates_join: %llu combinations, room for %llu", total, (unsigned long long)cap);
	return BHIP_OK;
}

extern "C" int bhip_mates_info(void *handle, uint64_t info[4]) {
	Handle *h = (Handle *)handle;
	if (!h || !info) return fail(BHIP_E_ARG, "bhip_mates_info: null argument");
	const MatesState *st = (const MatesState *)h->mates;
	info[0] = st ? st->us_last : 0; info[1] = st ? st->us_total : 0; info[2] = st ? st->n_lines : 0; info[3] = st ? st->n_comb : 0;
	return BHIP_OK;
}
