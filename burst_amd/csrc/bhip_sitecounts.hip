// burst_amd/csrc/bhip_sitecounts.hip -- one sample's counts at records the caller names (burst_hip --vcf-study; bhip_site_counts, gfx950).
// No reference counterpart: the reference never says how many of a sample's reads observe a position where they show nothing unusual.
//
// Definition (include/burst_hip.h "Site counts").  A RANGE (header, pos, span, w) is a line of the sample: it covers
// [pos, pos + span - 1] of its header and stands for w reads (span = '=' + X + D of its path; 0 covers nothing).  depth(header, pos) is the
// summed w of the ranges that hold the position.  A SITE RECORD (allele word 0, ref 1..4) takes n[0..3] from the sample's bhip_pile_run(1, 1)
// site at that position, and where there is none every observing read is plain: n[ref - 1] = depth.  An ALLELE RECORD takes the count of the
// sample's bhip_alleles_run(1, 1) entry with that (header, pos, word), or 0.
//
// The work follows ranges + records, never ranges x records:
//   k_sc_bounds        per range the key header << 32 | pos of its first position and of the position behind its last, the weight beside both
//   sort, sort         hipcub radix sorts of the starts and of the one-past-ends with their weights, limited to the bits in use
//   sum, sum           inclusive 64-bit sums of the weights in both orders
//   k_site_counts      one thread per record: the STABBING COUNT of k_pile_finish (weights of the starts <= key minus weights of the
//                      one-past-ends <= key: a range of span 0 is in both or in neither), then one binary search into the sites, or into
//                      the alleles by the 128-bit key (header << 32 | pos, word)
// All sums are 64-bit integers and every look-up is exact: no order of threads, ranges or records changes a byte.
#include "bhip_pile.h"

struct ScState {
	DBuf ranges, k_start, k_end, w_start, w_end, k_start_s, k_end_s, w_start_s, w_end_s, cs, ce, sites, alleles, records, cells, tmp;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	uint64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	void each(void (*f)(DBuf *, void *), void *u) {
		DBuf *all[] = {&ranges, &k_start, &k_end, &w_start, &w_end, &k_start_s, &k_end_s, &w_start_s, &w_end_s, &cs, &ce, &sites, &alleles, &records, &cells, &tmp};
		for (DBuf *x : all) f(x, u);
	}
	uint64_t bytes() { uint64_t b = 0; each([](DBuf *x, void *u) { *(uint64_t *)u += x->cap; }, &b); return b; }
};

__host__ __device__ __forceinline__ unsigned long long sc_key(uint32_t header, uint32_t pos) { return (unsigned long long)header << 32 | pos; }

// the cell of a record whose depth is known: the look-ups (the device and, for a call without ranges, the host)
__host__ __device__ __forceinline__ BhipCountCell sc_cell(const BhipCountRecord &r, unsigned long long depth, const BhipPileSite *__restrict__ sites, uint64_t n_sites,
		const BhipAllele *__restrict__ alleles, uint64_t n_alleles) {
	const unsigned long long key = sc_key(r.header, r.pos);
	BhipCountCell c;
	c.depth = (uint32_t)depth; c.n[0] = c.n[1] = c.n[2] = c.n[3] = 0u; c.count = 0u;
	if (r.allele == 0ull) {
		uint64_t lo = 0, hi = n_sites;
		while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (sc_key(sites[mid].header, sites[mid].pos) < key) lo = mid + 1; else hi = mid; }
		if (lo < n_sites && sc_key(sites[lo].header, sites[lo].pos) == key) { for (int b = 0; b < 4; ++b) c.n[b] = sites[lo].n[b]; }
		else if (r.ref >= 1u && r.ref <= 4u) c.n[r.ref - 1u] = (uint32_t)depth;      // (ref was checked on the host)
	} else {
		uint64_t lo = 0, hi = n_alleles;
		while (lo < hi) {
			const uint64_t mid = lo + ((hi - lo) >> 1);
			const unsigned long long k = sc_key(alleles[mid].header, alleles[mid].pos);
			if (k < key || (k == key && alleles[mid].allele < r.allele)) lo = mid + 1; else hi = mid;
		}
		if (lo < n_alleles && sc_key(alleles[lo].header, alleles[lo].pos) == key && alleles[lo].allele == r.allele) c.count = alleles[lo].count;
	}
	return c;
}

__global__ __launch_bounds__(PILE_BLOCK) void k_sc_bounds(const BhipCountRange *__restrict__ ranges, uint64_t n, unsigned long long *__restrict__ k_start,
		unsigned long long *__restrict__ k_end, unsigned long long *__restrict__ w_start, unsigned long long *__restrict__ w_end) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const BhipCountRange r = ranges[i];
		k_start[i] = sc_key(r.header, r.pos);
		k_end[i] = sc_key(r.header, r.pos + r.span);      // (pos + span <= 2^32 - 1: checked on the host)
		w_start[i] = w_end[i] = r.w;
	}
}

// cs / ce = the inclusive sums of the weights in the order of the sorted starts / one-past-ends
__global__ __launch_bounds__(PILE_BLOCK) void k_site_counts(const BhipCountRecord *__restrict__ records, uint64_t n_records, const unsigned long long *__restrict__ k_start,
		const unsigned long long *__restrict__ cs, const unsigned long long *__restrict__ k_end, const unsigned long long *__restrict__ ce, uint64_t n_ranges,
		const BhipPileSite *__restrict__ sites, uint64_t n_sites, const BhipAllele *__restrict__ alleles, uint64_t n_alleles, BhipCountCell *__restrict__ cells) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_records; i += (uint64_t)gridDim.x * blockDim.x) {
		const BhipCountRecord r = records[i];
		const unsigned long long key = sc_key(r.header, r.pos);
		const uint64_t a = pile_upper_bound(k_start, n_ranges, key), b = pile_upper_bound(k_end, n_ranges, key);
		const unsigned long long depth = (a ? cs[a - 1] : 0ull) - (b ? ce[b - 1] : 0ull);
		cells[i] = sc_cell(r, depth, sites, n_sites, alleles, n_alleles);
	}
}

// (bhip_handle.h: Handle::sitecounts)
void bhip_sitecounts_release(Handle *h) {
	ScState *st = (ScState *)h->sitecounts;
	if (!st) return;
	st->each([](DBuf *x, void *) { x->release(); }, nullptr);
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->sitecounts = nullptr;
}

extern "C" int bhip_site_counts_info(void *handle, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	if (!h || !info) return fail(BHIP_E_ARG, "bhip_site_counts_info: null argument");
	if (h->sitecounts) memcpy(info, ((ScState *)h->sitecounts)->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t));
	return BHIP_OK;
}

extern "C" int bhip_site_counts(void *handle, const BhipCountRange *ranges, uint64_t n_ranges, const BhipPileSite *sites, uint64_t n_sites,
		const BhipAllele *alleles, uint64_t n_alleles, const BhipCountRecord *records, uint64_t n_records, BhipCountCell *cells, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!h || (n_ranges && !ranges) || (n_sites && !sites) || (n_alleles && !alleles) || (n_records && (!records || !cells))) return fail(BHIP_E_ARG, "bhip_site_counts: null argument");
	ScState *st = (ScState *)h->sitecounts;
	if (!st) { st = new ScState(); h->sitecounts = st; }      // (host memory alone: the events and buffers are made by the first call that launches)
	memset(st->info, 0, sizeof st->info);
	// every value the kernels index or add by is checked here, before the device is touched
	if ((n_ranges | n_sites | n_alleles | n_records) >> 32)
		return fail(BHIP_E_ARG, "bhip_site_counts: a count of 2^32 or more (%llu ranges, %llu sites, %llu alleles, %llu records)", (pile_u64)n_ranges, (pile_u64)n_sites, (pile_u64)n_alleles, (pile_u64)n_records);
	uint64_t wsum = 0;
	uint32_t max_header = 0;
	for (uint64_t i = 0; i < n_ranges; ++i) {
		const BhipCountRange &r = ranges[i];
		if (r.pos < 1 || (uint64_t)r.pos + r.span > 0xFFFFFFFFull) return fail(BHIP_E_ARG, "bhip_site_counts: range %llu: position %u + span %u (1 .. 2^32 - 1)", (pile_u64)i, r.pos, r.span);
		if (!r.w) return fail(BHIP_E_ARG, "bhip_site_counts: range %llu has weight 0", (pile_u64)i);
		wsum += r.w;
		if (wsum > 0x7FFFFFFFull) return fail(BHIP_E_ARG, "bhip_site_counts: the ranges stand for more than 2^31 - 1 reads (range %llu)", (pile_u64)i);
		max_header = std::max(max_header, r.header);
	}
	for (uint64_t i = 1; i < n_sites; ++i)
		if (sc_key(sites[i - 1].header, sites[i - 1].pos) >= sc_key(sites[i].header, sites[i].pos)) return fail(BHIP_E_ARG, "bhip_site_counts: sites not strictly ascending by (header, pos) at site %llu", (pile_u64)i);
	for (uint64_t i = 1; i < n_alleles; ++i) {
		const unsigned long long a = sc_key(alleles[i - 1].header, alleles[i - 1].pos), b = sc_key(alleles[i].header, alleles[i].pos);
		if (a > b || (a == b && alleles[i - 1].allele >= alleles[i].allele)) return fail(BHIP_E_ARG, "bhip_site_counts: alleles not strictly ascending by (header, pos, allele) at allele %llu", (pile_u64)i);
	}
	for (uint64_t i = 0; i < n_records; ++i) {
		if (!records[i].pos) return fail(BHIP_E_ARG, "bhip_site_counts: record %llu has position 0", (pile_u64)i);
		if (!records[i].allele && (records[i].ref < 1 || records[i].ref > 4)) return fail(BHIP_E_ARG, "bhip_site_counts: site record %llu has ref %u (1 .. 4)", (pile_u64)i, records[i].ref);
	}
	info[0] = n_ranges; info[1] = n_records;
	info[3] = st->bytes();
	if (!n_records) { memcpy(st->info, info, sizeof st->info); return BHIP_OK; }      // (nothing to fill, no launch)
	if (!n_ranges) {      // (no read anywhere: depth 0 in every cell, the look-ups on the host, no launch)
		for (uint64_t i = 0; i < n_records; ++i) cells[i] = sc_cell(records[i], 0ull, sites, n_sites, alleles, n_alleles);
		memcpy(st->info, info, sizeof st->info);
		return BHIP_OK;
	}
	HIPCHK(hipSetDevice(h->device));
	if (!st->ev0 && hipEventCreate(&st->ev0) != hipSuccess) { st->ev0 = nullptr; return fail(BHIP_E_DEVICE, "hipEventCreate failed"); }
	if (!st->ev1 && hipEventCreate(&st->ev1) != hipSuccess) { st->ev1 = nullptr; return fail(BHIP_E_DEVICE, "hipEventCreate failed"); }
	hipStream_t S = h->stream;
	const uint64_t nr = n_ranges, nq = n_records;
	const int end_bit = 32 + std::max(1, pile_bits(max_header));      // the bits of a key header << 32 | position
	int rc = st->ranges.reserve(nr * sizeof(BhipCountRange)); if (rc) return rc;
	DBuf *per_range[] = {&st->k_start, &st->k_end, &st->w_start, &st->w_end, &st->k_start_s, &st->k_end_s, &st->w_start_s, &st->w_end_s, &st->cs, &st->ce};
	for (DBuf *x : per_range) { rc = x->reserve(nr * 8); if (rc) return rc; }
	rc = st->sites.reserve(n_sites * sizeof(BhipPileSite) + 16); if (rc) return rc;
	rc = st->alleles.reserve(n_alleles * sizeof(BhipAllele) + 16); if (rc) return rc;
	rc = st->records.reserve(nq * sizeof(BhipCountRecord)); if (rc) return rc;
	rc = st->cells.reserve(nq * sizeof(BhipCountCell)); if (rc) return rc;
	size_t tb_sort = 0, tb_sum = 0;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, st->k_start.as<pile_u64>(), st->k_start_s.as<pile_u64>(), st->w_start.as<pile_u64>(), st->w_start_s.as<pile_u64>(), (size_t)nr, 0, end_bit, S));
	HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tb_sum, st->w_start_s.as<pile_u64>(), st->cs.as<pile_u64>(), (size_t)nr, S));
	rc = st->tmp.reserve(std::max(tb_sort, tb_sum) + 16); if (rc) return rc;

	HIPCHK(hipMemcpyAsync(st->ranges.p, ranges, nr * sizeof(BhipCountRange), hipMemcpyHostToDevice, S));
	if (n_sites) HIPCHK(hipMemcpyAsync(st->sites.p, sites, n_sites * sizeof(BhipPileSite), hipMemcpyHostToDevice, S));
	if (n_alleles) HIPCHK(hipMemcpyAsync(st->alleles.p, alleles, n_alleles * sizeof(BhipAllele), hipMemcpyHostToDevice, S));
	HIPCHK(hipMemcpyAsync(st->records.p, records, nq * sizeof(BhipCountRecord), hipMemcpyHostToDevice, S));
	HIPCHK(hipEventRecord(st->ev0, S));
	hipLaunchKernelGGL(k_sc_bounds, dim3(pile_grid(nr)), dim3(PILE_BLOCK), 0, S, st->ranges.as<BhipCountRange>(), nr, st->k_start.as<pile_u64>(), st->k_end.as<pile_u64>(),
		st->w_start.as<pile_u64>(), st->w_end.as<pile_u64>());
	HIPCHK(hipGetLastError());
	size_t tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, st->k_start.as<pile_u64>(), st->k_start_s.as<pile_u64>(), st->w_start.as<pile_u64>(), st->w_start_s.as<pile_u64>(), (size_t)nr, 0, end_bit, S));
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, st->k_end.as<pile_u64>(), st->k_end_s.as<pile_u64>(), st->w_end.as<pile_u64>(), st->w_end_s.as<pile_u64>(), (size_t)nr, 0, end_bit, S));
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::InclusiveSum(st->tmp.p, tb, st->w_start_s.as<pile_u64>(), st->cs.as<pile_u64>(), (size_t)nr, S));
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::InclusiveSum(st->tmp.p, tb, st->w_end_s.as<pile_u64>(), st->ce.as<pile_u64>(), (size_t)nr, S));
	hipLaunchKernelGGL(k_site_counts, dim3(pile_grid(nq)), dim3(PILE_BLOCK), 0, S, st->records.as<BhipCountRecord>(), nq, st->k_start_s.as<pile_u64>(), st->cs.as<pile_u64>(),
		st->k_end_s.as<pile_u64>(), st->ce.as<pile_u64>(), nr, st->sites.as<BhipPileSite>(), (uint64_t)n_sites, st->alleles.as<BhipAllele>(), (uint64_t)n_alleles, st->cells.as<BhipCountCell>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(st->ev1, S));
	HIPCHK(hipMemcpyAsync(cells, st->cells.p, nq * sizeof(BhipCountCell), hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	info[2] = (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f); info[3] = st->bytes();
	memcpy(st->info, info, sizeof st->info);
	return BHIP_OK;
}
