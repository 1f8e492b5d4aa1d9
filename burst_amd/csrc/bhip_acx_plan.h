// burst_amd/csrc/bhip_acx_plan.h -- the host arithmetic of the word-sliced accelerator build (build_accelerator_by_words, bhip_acx.hip) as
// functions of their inputs alone: which word buckets a rank builds, how large the record area's address range is, and how a rank's run of
// buckets is cut into slices that can be sorted inside that range.  These rules decide whether a database fits the device.  No HIP in here:
// tests/csrc/acx_plan_host.cpp compiles it with the host compiler and tests/test_host_cpu.py pins its rows.
#ifndef BHIP_ACX_PLAN_H
#define BHIP_ACX_PLAN_H
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <vector>

#define BHIP_ACX_MAX_SLICES 256u             // slice numbers are bytes (k_acx_wcount's bucket -> slice table), and 0xFF is "not this build's bucket"
#define BHIP_ACX_SORT_MAX 2147483000ull      // tuples one sort call takes

// the sort's part of the range for a slice of n tuples: two 8-byte tuple arrays (the first at offset 0, the second behind it) and the folded
// lane masks (behind both), each rounded up to 256 after adding 16
static inline size_t bhip_acx_key_bytes(uint64_t n) { return (size_t)(n * 8 + 16 + 255) & ~(size_t)255; }
static inline size_t bhip_acx_buf_bytes(uint64_t n) { return 2 * bhip_acx_key_bytes(n) + ((size_t)(n * 2 + 16 + 255) & ~(size_t)255); }

// tuples of the buckets [b0, b1) (*biggest: the largest single bucket among them)
static inline uint64_t bhip_acx_run_tuples(const std::vector<unsigned long long> &hist, uint32_t b0, uint32_t b1, uint64_t *biggest = nullptr) {
	uint64_t n = 0, big = 0;
	for (uint32_t b = b0; b < b1; ++b) { n += hist[b]; big = std::max<uint64_t>(big, hist[b]); }
	if (biggest) *biggest = big;
	return n;
}

// The ranks' runs of buckets, rb[0 .. n_parts]: rank r builds the buckets [rb[r], rb[r + 1]).  Cut from the bucket histogram so that the runs
// hold equal numbers of tuples: rank r starts at the first bucket with at least total * r / n_parts tuples before it; ranks that are left
// over get empty runs at the end.
static inline std::vector<uint32_t> bhip_acx_rank_runs(const std::vector<unsigned long long> &hist, int n_parts) {
	const uint32_t n_buckets = (uint32_t)hist.size();
	const uint64_t total = bhip_acx_run_tuples(hist, 0, n_buckets);
	std::vector<uint32_t> rb((size_t)n_parts + 1, 0);
	uint64_t run = 0; int r = 1;
	for (uint32_t b = 0; b < n_buckets && r < n_parts; ++b) {
		while (r < n_parts && run >= (uint64_t)((double)total * r / n_parts)) rb[r++] = b;      // (run = tuples of the buckets before b)
		run += hist[b];
	}
	for (; r < n_parts; ++r) rb[r] = n_buckets;
	rb[n_parts] = n_buckets;
	return rb;
}

// Bytes to ask DBuf::reserve_growable for, given `avail` bytes of the device beyond what is set aside for everything else: the final size (a
// record per tuple of the whole database at most) and room for the largest slice's sort on top of the own records, as far as the device has
// it.  0: not even the records fit.  (reserve_growable rounds up to whole chunks and adds one: planned with the two chunks taken off)
static inline size_t bhip_acx_range_bytes(double avail, uint64_t total, uint64_t total_own, uint32_t rec_bytes, size_t chunk) {
	const uint64_t biggest_sort = std::min<uint64_t>(total_own, BHIP_ACX_SORT_MAX);
	double want_va = std::max((double)total * rec_bytes + 16.0, (double)total_own * rec_bytes + (double)bhip_acx_buf_bytes(biggest_sort)) + 4096.0;
	if (want_va > avail) want_va = avail;
	if (want_va < (double)total * rec_bytes + 16.0 + 4096.0) return 0;
	return (size_t)want_va > 2 * chunk + ((size_t)total * rec_bytes + 16) ? (size_t)want_va - 2 * chunk : (size_t)total * rec_bytes + 16;
}

// A rank's run of buckets cut into slices: slice s holds the buckets [cuts[s], cuts[s + 1]) and items[s] tuples.  The records fill the range
// from the bottom, the slice at hand is sorted at its top: slice s fits when (tuples before it + its own) records and its sort buffers do.
struct BhipAcxPlan {
	std::vector<uint32_t> cuts;
	std::vector<uint64_t> items;
	uint64_t cap_items = 0;      // the largest slice
	uint32_t n_slices() const { return cuts.empty() ? 0 : (uint32_t)cuts.size() - 1; }
	void start(uint32_t own0) { cuts.assign(1, own0); items.clear(); cap_items = 0; }
	void add(uint32_t b1, uint64_t n) { cuts.push_back(b1); items.push_back(n); cap_items = std::max(cap_items, n); }
};
// a slice spans at most 2^26 words (four sort passes): that many buckets of 2^shift words
static inline uint32_t bhip_acx_max_buckets(uint32_t shift) { return 26 > shift ? 1u << (26 - shift) : 1u; }

// slices of at most `target` tuples (BHIP_MASK_SLICE: slices of a given size); 0 slices: one of them does not fit the range
static inline uint32_t bhip_acx_plan_by_target(const std::vector<unsigned long long> &hist, uint32_t own0, uint32_t own1, uint32_t max_b, size_t va_size, uint64_t target,
		uint32_t rec_bytes, BhipAcxPlan *p) {
	p->start(own0);
	uint64_t before = 0;
	for (uint32_t b0 = own0; b0 < own1;) {
		uint32_t b1 = b0 + 1; uint64_t n = hist[b0];
		while (b1 < own1 && b1 - b0 < max_b && n + hist[b1] <= target) n += hist[b1++];
		if ((before + n) * rec_bytes + 16 + bhip_acx_buf_bytes(n) > va_size) { p->start(own0); return 0; }
		p->add(b1, n); before += n; b0 = b1;
	}
	return p->n_slices();
}
// slices as large as the room between the records so far and the top allows, 4 (before + n) + 18 n <= range: the early slices take what one
// sort call takes, the last ones what is left beside the records; 0 slices: a bucket alone does not fit
static inline uint32_t bhip_acx_plan_by_room(const std::vector<unsigned long long> &hist, uint32_t own0, uint32_t own1, uint32_t max_b, size_t va_size, uint32_t rec_bytes,
		BhipAcxPlan *p) {
	p->start(own0);
	uint64_t before = 0;
	for (uint32_t b0 = own0; b0 < own1;) {
		const double room = (double)va_size - (double)before * rec_bytes - 4096.0;
		const uint64_t target = room > 0 ? (uint64_t)std::min(2147483000.0, room / 22.0) : 0;
		if (hist[b0] > target) { p->start(own0); return 0; }
		uint32_t b1 = b0 + 1; uint64_t n = hist[b0];
		while (b1 < own1 && b1 - b0 < max_b && n + hist[b1] <= target) n += hist[b1++];
		p->add(b1, n); before += n; b0 = b1;
	}
	return p->n_slices();
}
// a plan the build can run: at least one slice, a slice number below 0xFF for every one of them, and no slice beyond one sort call
static inline bool bhip_acx_plan_ok(const BhipAcxPlan &p) { return p.n_slices() && p.n_slices() <= BHIP_ACX_MAX_SLICES - 1u && p.cap_items < BHIP_ACX_SORT_MAX; }

// The plan of the run [own0, own1) of `hist` (buckets of 2^shift words) inside a range of va_size bytes; forced_slice > 0 (BHIP_MASK_SLICE)
// asks for slices of that many tuples, or of the run's biggest bucket where that is more.  false: no plan the build can run.
static inline bool bhip_acx_plan_run(const std::vector<unsigned long long> &hist, uint32_t own0, uint32_t own1, uint32_t shift, size_t va_size, long long forced_slice,
		uint32_t rec_bytes, BhipAcxPlan *p) {
	uint64_t biggest = 0;
	bhip_acx_run_tuples(hist, own0, own1, &biggest);
	const uint32_t max_b = bhip_acx_max_buckets(shift);
	if (forced_slice > 0) bhip_acx_plan_by_target(hist, own0, own1, max_b, va_size, std::max<uint64_t>((uint64_t)forced_slice, biggest), rec_bytes, p);
	else bhip_acx_plan_by_room(hist, own0, own1, max_b, va_size, rec_bytes, p);
	return bhip_acx_plan_ok(*p);
}
#endif
