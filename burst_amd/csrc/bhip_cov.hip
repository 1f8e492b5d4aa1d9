// burst_amd/csrc/bhip_cov.hip -- coverage statistics per reference header and sample from the printed placements (--coverage), and the
// lane extents of the resident database (gfx950).  No reference counterpart on the device: the reference's downstream helper
// (embalmlets/bcov.c) keeps two counters per POSITION of every reference and walks every covered base of every .b6 line on one thread.
//
// Here a placement of weight w over the half-open range [b, e) of header h is two EVENTS, +w at key (h << 32 | b) and -w at
// (h << 32 | e).  Sorted by key, the running sum of the weights is the depth between consecutive events; a column's statistics
// (tot = sum of depth, cov = positions with depth != 0, sq = sum of depth^2, per header) are sums of depth x distance terms.  The cost
// follows the number of lines, never the number of reference positions.
//
//   carry scheme   The running depth is ONE inclusive scan over the whole sorted array (hipcub::DeviceScan, 64-bit integers).  Every
//                  placement puts +w and -w into the SAME header's segment, so the weights of a segment sum to zero and the global
//                  running sum at the first event of a segment is what it would be had the scan started there: the global scan IS the
//                  segmented one, whatever the block size of any kernel and however many events a header has.  k_cov_stats then only
//                  needs event i, its depth and the key of event i + 1 (read across block boundaries like any other element), and adds
//                  into the header's three 64-bit counters: integer additions commute, so the result does not depend on their order.
//   buffer         Each of the two event sets (all placements; the unique ones) is one grow-only array [events of the samples that are
//                  done | events of the sample being added].  Dataset = a column pass over all of it when the study ends.
//   cap            Option cov_event_cap (bytes of the events of both sets together, 16 each).  The sets' arrays grow with half as much
//                  again as headroom, up to the cap for the shared set and half of it for the unique one (a subset): 1.5 x cap.  A
//                  column pass or a compaction holds beside them a sorted copy of the region it works on and the radix sort's own
//                  ping-pong storage, each at most the cap: 3.5 x cap at the peak.  The default is therefore a FIFTH of the memory free
//                  at the first bhip_cov_add: at most 70 % of it is ever taken, the rest is left to the batch buffers a later, larger
//                  sample may reserve.
//   compaction     When a chunk of lines would take the sets beyond the cap: sort, sum the weights of equal keys, drop the zeros, for
//                  both regions of both sets.  The depth function is unchanged and a set is then bounded by two events per DISTINCT
//                  position.  Only if the compacted sets still do not fit does bhip_cov_add fail (BHIP_E_DEVICE).
#include "bhip_handle.h"
#include <map>

#define COV_BLOCK 256
#define COV_ITEMS 8      // consecutive events per thread of k_cov_stats: a block covers COV_BLOCK * COV_ITEMS events

// one thread per line: counts the placement and, unless its range is empty, appends its two events to the set(s) it belongs to
__global__ __launch_bounds__(256) void k_cov_events(const BhipCovLine *__restrict__ ln, uint32_t n, const uint32_t *__restrict__ len, uint32_t n_headers,
		uint32_t pad, unsigned long long *__restrict__ key_sh, long long *__restrict__ val_sh, unsigned long long *__restrict__ key_un,
		long long *__restrict__ val_un, unsigned long long *__restrict__ cnt /* [0] shared, [1] unique, [2] bad lines */,
		unsigned long long *__restrict__ st_sh, unsigned long long *__restrict__ st_un) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const BhipCovLine l = ln[i];
		if (l.ref >= n_headers) { atomicAdd(&cnt[2], 1ull); continue; }
		const long long w = (long long)(l.w & 0x7FFFFFFFu);
		const bool uniq = (l.w >> 31) != 0;
		if (!w) continue;
		atomicAdd(&st_sh[4ull * l.ref + 3], (unsigned long long)w);
		if (uniq) atomicAdd(&st_un[4ull * l.ref + 3], (unsigned long long)w);
		// [max(lo - 1 - pad, 0), min(hi - 1 + pad, L)) in 64-bit signed arithmetic: nothing wraps for coordinates, lengths and pads up to 2^32 - 1
		const long long lo = l.st < l.ed ? l.st : l.ed, hi = l.st < l.ed ? l.ed : l.st, L = len[l.ref];
		long long b = lo - 1 - (long long)pad, e = hi - 1 + (long long)pad;
		if (b < 0) b = 0;
		if (e > L) e = L;
		if (b >= e) continue;
		const unsigned long long kb = ((unsigned long long)l.ref << 32) | (unsigned long long)b, ke = ((unsigned long long)l.ref << 32) | (unsigned long long)e;
		unsigned long long s = atomicAdd(&cnt[0], 2ull);
		key_sh[s] = kb; val_sh[s] = w; key_sh[s + 1] = ke; val_sh[s + 1] = -w;
		if (uniq) {
			s = atomicAdd(&cnt[1], 2ull);
			key_un[s] = kb; val_un[s] = w; key_un[s + 1] = ke; val_un[s + 1] = -w;
		}
	}
}

// The sorted events with their running depth: event i contributes depth[i] x (position of event i + 1 - position of event i) when
// event i + 1 belongs to the same header.  A thread walks COV_ITEMS consecutive events and keeps the sums of the header it is in;
// a block that lies inside ONE header's segment (the long segments) reduces its threads' sums and adds once.
__global__ __launch_bounds__(COV_BLOCK) void k_cov_stats(const unsigned long long *__restrict__ key, const long long *__restrict__ depth, uint64_t n,
		unsigned long long *__restrict__ stats) {
	typedef hipcub::BlockReduce<unsigned long long, COV_BLOCK> Reduce;
	__shared__ typename Reduce::TempStorage tmp;
	const uint64_t blk0 = (uint64_t)blockIdx.x * (COV_BLOCK * COV_ITEMS);
	if (blk0 >= n) return;
	const uint64_t blk1 = blk0 + COV_BLOCK * COV_ITEMS < n ? blk0 + COV_BLOCK * COV_ITEMS : n;
	const bool one_header = (key[blk0] >> 32) == (key[blk1 - 1] >> 32);      // (sorted: equal ends = equal everywhere between)
	const uint64_t i0 = blk0 + (uint64_t)threadIdx.x * COV_ITEMS, i1 = i0 + COV_ITEMS < blk1 ? i0 + COV_ITEMS : blk1;
	unsigned long long tot = 0, cov = 0, sq = 0;
	uint32_t cur = i0 < i1 ? (uint32_t)(key[i0] >> 32) : 0u;
	for (uint64_t i = i0; i < i1; ++i) {
		const unsigned long long k = key[i];
		const uint32_t ref = (uint32_t)(k >> 32);
		if (ref != cur) {      // (never taken in a one-header block)
			if (tot | cov | sq) { atomicAdd(&stats[4ull * cur], tot); atomicAdd(&stats[4ull * cur + 1], cov); atomicAdd(&stats[4ull * cur + 2], sq); }
			tot = cov = sq = 0; cur = ref;
		}
		if (i + 1 < n) {
			const unsigned long long nk = key[i + 1];
			if ((uint32_t)(nk >> 32) == ref) {
				const unsigned long long d = (unsigned long long)depth[i], span = (nk & 0xFFFFFFFFull) - (k & 0xFFFFFFFFull);
				if (d && span) { tot += d * span; cov += span; sq += d * d * span; }
			}
		}
	}
	if (one_header) {
		tot = Reduce(tmp).Sum(tot); __syncthreads();
		cov = Reduce(tmp).Sum(cov); __syncthreads();
		sq = Reduce(tmp).Sum(sq);
		if (threadIdx.x) return;
		cur = (uint32_t)(key[blk0] >> 32);
	}
	if (tot | cov | sq) { atomicAdd(&stats[4ull * cur], tot); atomicAdd(&stats[4ull * cur + 1], cov); atomicAdd(&stats[4ull * cur + 2], sq); }
}

__global__ void k_cov_nonzero(const long long *__restrict__ v, uint64_t n, uint8_t *__restrict__ flag) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) flag[i] = v[i] != 0;
}

// one thread per (clump, lane): the index after the lane's last symbol that is not the pad code 0, walking back from the clump's end
__global__ __launch_bounds__(256) void k_lane_extent(const uint4 *__restrict__ ref, const uint64_t *__restrict__ ref_off, const uint32_t *__restrict__ clump_len,
		uint32_t n_clumps, uint32_t *__restrict__ extent) {
	for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < (uint64_t)n_clumps * 16; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t c = (uint32_t)(t >> 4), z = (uint32_t)(t & 15), nchunks = (clump_len[c] + 31) >> 5;
		const uint4 *rp = ref + ref_off[c] * 16 + (uint64_t)z * nchunks;      // lane-major: [clump][lane][chunk], 32 symbols per chunk, symbol p in bits 4 (p & 7) of word (p & 31) >> 3
		uint32_t ext = 0;
		for (uint32_t k = nchunks; k-- > 0;) {
			const uint4 q = rp[k];
			const uint32_t w[4] = {q.x, q.y, q.z, q.w};
			int hit = -1;
			for (int j = 3; j >= 0; --j) if (w[j]) { hit = j; break; }
			if (hit >= 0) { ext = 32u * k + 8u * (uint32_t)hit + (31u - (uint32_t)__clz((int)w[hit])) / 4u + 1u; break; }
		}
		extent[t] = ext;
	}
}

struct CovSet {
	DBuf keys, vals;
	uint64_t n_done = 0, n_cur = 0;      // events of the finished samples, then those of the sample being added
	uint64_t n() const { return n_done + n_cur; }
};
struct CovState {
	uint32_t n_headers = 0, pad = 0;
	DBuf len, lines, cnt, stats_sh, stats_un, sk, sv, tmp, flag, nsel;
	CovSet sh, un;
	uint64_t cap = 0, peak_bytes = 0, n_compactions = 0, us_last = 0, us_total = 0;
	std::map<uint32_t, std::vector<uint64_t>> sample_sh, sample_un;      // per sample: [n_headers][4] = tot, cov, sq, lines
	std::vector<uint64_t> lines_sh, lines_un;                             // placements per header over all samples
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

// (bhip_handle.h: Handle::cov, Handle::opt_cov_event_cap)
void bhip_cov_release(Handle *h) {
	CovState *st = (CovState *)h->cov;
	if (!st) return;
	DBuf *all[] = {&st->len, &st->lines, &st->cnt, &st->stats_sh, &st->stats_un, &st->sk, &st->sv, &st->tmp, &st->flag, &st->nsel, &st->sh.keys, &st->sh.vals, &st->un.keys, &st->un.vals};
	for (DBuf *b : all) b->release();
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->cov = nullptr;
}

// room for n_events in a set's arrays, what is there kept (DBuf::reserve alone forgets it); half as much again for the samples to come,
// but never more than the cap lets a set hold
static int set_grow(Handle *h, CovSet *S, uint64_t n_events, uint64_t max_events) {
	if (n_events * 8 <= S->keys.cap && n_events * 8 <= S->vals.cap) return 0;
	DBuf nk, nv;
	const uint64_t want = std::max<uint64_t>(n_events, std::min<uint64_t>(n_events + n_events / 2, max_events));
	int rc = nk.reserve_exact(want * 8);
	if (!rc) rc = nv.reserve_exact(want * 8);
	if (rc) { nk.release(); nv.release(); return rc; }
	if (S->n()) {
		HIPCHK(hipMemcpyAsync(nk.p, S->keys.p, S->n() * 8, hipMemcpyDeviceToDevice, h->stream));
		HIPCHK(hipMemcpyAsync(nv.p, S->vals.p, S->n() * 8, hipMemcpyDeviceToDevice, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
	}
	S->keys.release(); S->vals.release();
	S->keys = nk; S->vals = nv;
	return 0;
}

static int key_bits(uint32_t n_headers) { int b = 1; while (b < 32 && ((n_headers - 1) >> b)) ++b; return 32 + b; }

// (keys, vals)[0 .. n) sorted by key into (sk, sv)
static int sort_region(Handle *h, CovState *st, const unsigned long long *keys, const long long *vals, uint64_t n) {
	if (n >= 0x7FFFFFFFull) return fail(BHIP_E_DEVICE, "coverage: %llu events in one pass (limit 2^31 - 1): lower cov_event_cap so that the sets are compacted earlier", (unsigned long long)n);
	int rc = st->sk.reserve(n * 8); if (rc) return rc;
	rc = st->sv.reserve(n * 8); if (rc) return rc;
	size_t tb = 0;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, st->sk.as<unsigned long long>(), vals, st->sv.as<long long>(), (int)n, 0, key_bits(st->n_headers), h->stream));
	rc = st->tmp.reserve(tb + 16); if (rc) return rc;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, keys, st->sk.as<unsigned long long>(), vals, st->sv.as<long long>(), (int)n, 0, key_bits(st->n_headers), h->stream));
	return 0;
}

// one column: tot / cov / sq of the events (keys, vals)[0 .. n) added into d_stats[n_headers][4]
static int cov_column(Handle *h, CovState *st, const unsigned long long *keys, const long long *vals, uint64_t n, unsigned long long *d_stats) {
	if (!n) return 0;
	int rc = sort_region(h, st, keys, vals, n); if (rc) return rc;
	size_t tb = 0;
	HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tb, st->sv.as<long long>(), st->sv.as<long long>(), (int)n, h->stream));
	rc = st->tmp.reserve(tb + 16); if (rc) return rc;
	HIPCHK(hipcub::DeviceScan::InclusiveSum(st->tmp.p, tb, st->sv.as<long long>(), st->sv.as<long long>(), (int)n, h->stream));
	const uint64_t per_block = (uint64_t)COV_BLOCK * COV_ITEMS;
	hipLaunchKernelGGL(k_cov_stats, dim3((uint32_t)((n + per_block - 1) / per_block)), dim3(COV_BLOCK), 0, h->stream, st->sk.as<unsigned long long>(), st->sv.as<long long>(), n, d_stats);
	HIPCHK(hipGetLastError());
	return 0;
}

// (keys, vals)[src .. src + n) of a set -> its compacted form at [dst .. dst + *m), dst <= src: sorted, one event per key, no zero weights
static int compact_region(Handle *h, CovState *st, CovSet *S, uint64_t src, uint64_t n, uint64_t dst, uint64_t *m) {
	*m = 0;
	if (!n) return 0;
	unsigned long long *K = S->keys.as<unsigned long long>() + src; long long *V = S->vals.as<long long>() + src;
	int rc = sort_region(h, st, K, V, n); if (rc) return rc;
	rc = st->nsel.reserve(16); if (rc) return rc;
	rc = st->flag.reserve(n); if (rc) return rc;
	// the region itself is free once it has been sorted away: the sums of the runs of equal keys go back into it ...
	size_t tb = 0;
	HIPCHK(hipcub::DeviceReduce::ReduceByKey(nullptr, tb, st->sk.as<unsigned long long>(), K, st->sv.as<long long>(), V, st->nsel.as<unsigned long long>(), hipcub::Sum(), (int)n, h->stream));
	rc = st->tmp.reserve(tb + 16); if (rc) return rc;
	HIPCHK(hipcub::DeviceReduce::ReduceByKey(st->tmp.p, tb, st->sk.as<unsigned long long>(), K, st->sv.as<long long>(), V, st->nsel.as<unsigned long long>(), hipcub::Sum(), (int)n, h->stream));
	unsigned long long runs = 0, kept = 0;
	HIPCHK(hipMemcpyAsync(&runs, st->nsel.p, 8, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	if (runs > n) return fail(BHIP_E_INTERNAL, "coverage: %llu runs of %llu events", runs, (unsigned long long)n);
	// ... the ones that are not zero into the sorted copy, and from there to their place
	hipLaunchKernelGGL(k_cov_nonzero, dim3((uint32_t)std::min<uint64_t>((runs + 255) / 256, 4096)), dim3(256), 0, h->stream, V, (uint64_t)runs, st->flag.as<uint8_t>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tb, K, st->flag.as<uint8_t>(), st->sk.as<unsigned long long>(), st->nsel.as<unsigned long long>(), (int64_t)runs, h->stream));
	rc = st->tmp.reserve(tb + 16); if (rc) return rc;
	HIPCHK(hipcub::DeviceSelect::Flagged(st->tmp.p, tb, K, st->flag.as<uint8_t>(), st->sk.as<unsigned long long>(), st->nsel.as<unsigned long long>(), (int64_t)runs, h->stream));
	HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tb, V, st->flag.as<uint8_t>(), st->sv.as<long long>(), st->nsel.as<unsigned long long>(), (int64_t)runs, h->stream));
	rc = st->tmp.reserve(tb + 16); if (rc) return rc;
	HIPCHK(hipcub::DeviceSelect::Flagged(st->tmp.p, tb, V, st->flag.as<uint8_t>(), st->sv.as<long long>(), st->nsel.as<unsigned long long>(), (int64_t)runs, h->stream));
	HIPCHK(hipMemcpyAsync(&kept, st->nsel.p, 8, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	if (kept > runs) return fail(BHIP_E_INTERNAL, "coverage: %llu of %llu runs kept", kept, runs);
	if (kept) {
		HIPCHK(hipMemcpyAsync(S->keys.as<unsigned long long>() + dst, st->sk.p, kept * 8, hipMemcpyDeviceToDevice, h->stream));
		HIPCHK(hipMemcpyAsync(S->vals.as<long long>() + dst, st->sv.p, kept * 8, hipMemcpyDeviceToDevice, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
	}
	*m = kept;
	return 0;
}
static int compact_all(Handle *h, CovState *st) {
	for (CovSet *S : {&st->sh, &st->un}) {
		uint64_t m_done = 0, m_cur = 0;
		int rc = compact_region(h, st, S, 0, S->n_done, 0, &m_done); if (rc) return rc;
		rc = compact_region(h, st, S, S->n_done, S->n_cur, m_done, &m_cur); if (rc) return rc;
		S->n_done = m_done; S->n_cur = m_cur;
	}
	++st->n_compactions;
	return 0;
}

extern "C" int bhip_cov_begin(void *handle, uint32_t n_headers, const uint32_t *lengths, uint32_t pad) {
	Handle *h = (Handle *)handle;
	if (!h || !lengths || !n_headers) return fail(BHIP_E_ARG, "bhip_cov_begin: null handle, no headers or no lengths");
	HIPCHK(hipSetDevice(h->device));
	bhip_cov_release(h);
	CovState *st = new CovState();
	h->cov = st;
	st->n_headers = n_headers; st->pad = pad;
	st->lines_sh.assign(n_headers, 0); st->lines_un.assign(n_headers, 0);
	int rc = st->len.reserve((size_t)n_headers * 4);
	if (!rc) rc = st->stats_sh.reserve((size_t)n_headers * 32);
	if (!rc) rc = st->stats_un.reserve((size_t)n_headers * 32);
	if (!rc) rc = st->cnt.reserve(32);
	if (!rc && (hipEventCreate(&st->ev0) != hipSuccess || hipEventCreate(&st->ev1) != hipSuccess)) rc = fail(BHIP_E_DEVICE, "hipEventCreate failed");
	if (rc) { bhip_cov_release(h); return rc; }
	hipError_t e = hipMemcpyAsync(st->len.p, lengths, (size_t)n_headers * 4, hipMemcpyHostToDevice, h->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
	if (e != hipSuccess) { bhip_cov_release(h); return fail(BHIP_E_DEVICE, "bhip_cov_begin: %s", hipGetErrorString(e)); }
	return BHIP_OK;
}

static int cov_add_sample(Handle *h, CovState *st, uint32_t sample, const BhipCovLine *lines, uint64_t n);

extern "C" int bhip_cov_add(void *handle, uint32_t sample, const BhipCovLine *lines, uint64_t n) {
	Handle *h = (Handle *)handle;
	CovState *st = h ? (CovState *)h->cov : nullptr;
	if (!st) return fail(BHIP_E_ARG, "bhip_cov_add: no bhip_cov_begin on this handle");
	const int rc = cov_add_sample(h, st, sample, lines, n);
	if (rc) st->sh.n_cur = st->un.n_cur = 0;      // a sample that failed leaves no events behind: the next one's column and Dataset are its own
	return rc;
}

static int cov_add_sample(Handle *h, CovState *st, uint32_t sample, const BhipCovLine *lines, uint64_t n) {
	if (n && !lines) return fail(BHIP_E_ARG, "bhip_cov_add: null lines");
	if (st->sample_sh.count(sample)) return fail(BHIP_E_ARG, "bhip_cov_add: sample %u has been added already", sample);
	HIPCHK(hipSetDevice(h->device));
	if (h->opt_cov_event_cap > 0) st->cap = (uint64_t)h->opt_cov_event_cap;
	else if (!st->cap) { size_t f = 0, t = 0; HIPCHK(hipMemGetInfo(&f, &t)); st->cap = f / 5; }      // (a fifth: see the head of this file)
	if (st->cap < 4096) st->cap = 4096;
	// one sort pass takes fewer than 2^31 - 1 events (sort_region): a set never holds more than cap / 16, so a cap beyond that many events
	// is lowered to it and the compaction runs where the Dataset pass would otherwise fail at the end of a long study
	st->cap = std::min<uint64_t>(st->cap, 0x7FFFFFF0ull * 16);
	const size_t sbytes = (size_t)st->n_headers * 32;
	HIPCHK(hipMemsetAsync(st->stats_sh.p, 0, sbytes, h->stream));
	HIPCHK(hipMemsetAsync(st->stats_un.p, 0, sbytes, h->stream));
	// chunks of lines whose events (two per set at most) take a quarter of the cap at most: a sample larger than the cap is compacted as it comes
	const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n, st->cap / 256), 1u << 26));
	for (uint64_t l0 = 0; l0 < n; l0 += chunk) {
		const uint64_t c = std::min(chunk, n - l0);
		if ((st->sh.n() + st->un.n() + 4 * c) * 16 > st->cap) {
			int rc = compact_all(h, st); if (rc) return rc;
			if ((st->sh.n() + st->un.n() + 4 * c) * 16 > st->cap)
				return fail(BHIP_E_DEVICE, "coverage: the compacted event buffer (%llu events) and the next %llu lines do not fit cov_event_cap = %llu bytes",
				            (unsigned long long)(st->sh.n() + st->un.n()), (unsigned long long)c, (unsigned long long)st->cap);
		}
		int rc = set_grow(h, &st->sh, st->sh.n() + 2 * c, st->cap / 16 + 1); if (rc) return rc;      // (the unique events are a subset of the shared ones: at most half the cap)
		rc = set_grow(h, &st->un, st->un.n() + 2 * c, st->cap / 32 + 1); if (rc) return rc;
		rc = st->lines.reserve(c * sizeof(BhipCovLine)); if (rc) return rc;
		HIPCHK(hipMemcpyAsync(st->lines.p, lines + l0, c * sizeof(BhipCovLine), hipMemcpyHostToDevice, h->stream));
		HIPCHK(hipMemsetAsync(st->cnt.p, 0, 32, h->stream));
		hipLaunchKernelGGL(k_cov_events, dim3((uint32_t)std::min<uint64_t>((c + 255) / 256, 8192)), dim3(256), 0, h->stream, st->lines.as<BhipCovLine>(), (uint32_t)c,
			st->len.as<uint32_t>(), st->n_headers, st->pad, st->sh.keys.as<unsigned long long>() + st->sh.n(), st->sh.vals.as<long long>() + st->sh.n(),
			st->un.keys.as<unsigned long long>() + st->un.n(), st->un.vals.as<long long>() + st->un.n(), st->cnt.as<unsigned long long>(),
			st->stats_sh.as<unsigned long long>(), st->stats_un.as<unsigned long long>());
		HIPCHK(hipGetLastError());
		unsigned long long cnt[3] = {0, 0, 0};
		HIPCHK(hipMemcpyAsync(cnt, st->cnt.p, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
		if (cnt[0] > 2 * c || cnt[1] > 2 * c) return fail(BHIP_E_INTERNAL, "coverage: %llu / %llu events from %llu lines", cnt[0], cnt[1], (unsigned long long)c);
		st->sh.n_cur += cnt[0]; st->un.n_cur += cnt[1];
		st->peak_bytes = std::max<uint64_t>(st->peak_bytes, (st->sh.n() + st->un.n()) * 16);
		if (cnt[2]) return fail(BHIP_E_ARG, "bhip_cov_add: %llu lines name a header beyond the %u of bhip_cov_begin", cnt[2], st->n_headers);
	}
	// the sample's two columns
	HIPCHK(hipEventRecord(st->ev0, h->stream));
	int rc = cov_column(h, st, st->sh.keys.as<unsigned long long>() + st->sh.n_done, st->sh.vals.as<long long>() + st->sh.n_done, st->sh.n_cur, st->stats_sh.as<unsigned long long>());
	if (!rc) rc = cov_column(h, st, st->un.keys.as<unsigned long long>() + st->un.n_done, st->un.vals.as<long long>() + st->un.n_done, st->un.n_cur, st->stats_un.as<unsigned long long>());
	if (rc) return rc;
	HIPCHK(hipEventRecord(st->ev1, h->stream));
	std::vector<uint64_t> a((size_t)st->n_headers * 4), b((size_t)st->n_headers * 4);
	HIPCHK(hipMemcpyAsync(a.data(), st->stats_sh.p, sbytes, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(b.data(), st->stats_un.p, sbytes, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	st->us_last = (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f); st->us_total += st->us_last;
	for (uint32_t r = 0; r < st->n_headers; ++r) { st->lines_sh[r] += a[4 * (size_t)r + 3]; st->lines_un[r] += b[4 * (size_t)r + 3]; }
	st->sample_sh[sample] = std::move(a); st->sample_un[sample] = std::move(b);
	st->sh.n_done += st->sh.n_cur; st->sh.n_cur = 0;
	st->un.n_done += st->un.n_cur; st->un.n_cur = 0;
	return BHIP_OK;
}

extern "C" int bhip_cov_sample_stats(void *handle, uint32_t sample, uint64_t *shared, uint64_t *unique) {
	Handle *h = (Handle *)handle;
	CovState *st = h ? (CovState *)h->cov : nullptr;
	if (!st) return fail(BHIP_E_ARG, "bhip_cov_sample_stats: no bhip_cov_begin on this handle");
	const size_t bytes = (size_t)st->n_headers * 32;
	auto it = st->sample_sh.find(sample);      // (a sample that was never added -- one that failed -- is an all-zero column)
	if (shared) { if (it == st->sample_sh.end()) memset(shared, 0, bytes); else memcpy(shared, it->second.data(), bytes); }
	if (unique) { if (it == st->sample_sh.end()) memset(unique, 0, bytes); else memcpy(unique, st->sample_un[sample].data(), bytes); }
	return BHIP_OK;
}

extern "C" int bhip_cov_dataset_stats(void *handle, uint64_t *shared, uint64_t *unique) {
	Handle *h = (Handle *)handle;
	CovState *st = h ? (CovState *)h->cov : nullptr;
	if (!st) return fail(BHIP_E_ARG, "bhip_cov_dataset_stats: no bhip_cov_begin on this handle");
	HIPCHK(hipSetDevice(h->device));
	const size_t sbytes = (size_t)st->n_headers * 32;
	HIPCHK(hipMemsetAsync(st->stats_sh.p, 0, sbytes, h->stream));
	HIPCHK(hipMemsetAsync(st->stats_un.p, 0, sbytes, h->stream));
	int rc = cov_column(h, st, st->sh.keys.as<unsigned long long>(), st->sh.vals.as<long long>(), st->sh.n_done, st->stats_sh.as<unsigned long long>());
	if (!rc) rc = cov_column(h, st, st->un.keys.as<unsigned long long>(), st->un.vals.as<long long>(), st->un.n_done, st->stats_un.as<unsigned long long>());
	if (rc) return rc;
	if (shared) HIPCHK(hipMemcpyAsync(shared, st->stats_sh.p, sbytes, hipMemcpyDeviceToHost, h->stream));
	if (unique) HIPCHK(hipMemcpyAsync(unique, st->stats_un.p, sbytes, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	for (uint32_t r = 0; r < st->n_headers; ++r) {
		if (shared) shared[4 * (size_t)r + 3] = st->lines_sh[r];
		if (unique) unique[4 * (size_t)r + 3] = st->lines_un[r];
	}
	return BHIP_OK;
}

extern "C" int bhip_cov_info(void *handle, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	CovState *st = h ? (CovState *)h->cov : nullptr;
	if (!st || !info) return fail(BHIP_E_ARG, "bhip_cov_info: no bhip_cov_begin on this handle");
	info[0] = st->sh.n() + st->un.n(); info[1] = st->peak_bytes; info[2] = st->n_compactions; info[3] = st->cap;
	info[4] = st->us_last; info[5] = (uint64_t)COV_BLOCK * COV_ITEMS; info[6] = st->us_total; info[7] = st->sample_sh.size();
	return BHIP_OK;
}

extern "C" int bhip_cov_end(void *handle) {
	Handle *h = (Handle *)handle;
	if (!h) return fail(BHIP_E_ARG, "null handle");
	(void)hipSetDevice(h->device);
	if (h->stream) (void)hipStreamSynchronize(h->stream);
	bhip_cov_release(h);
	return BHIP_OK;
}

extern "C" int bhip_lane_extents(void *handle, uint32_t *extents) {
	Handle *h = (Handle *)handle;
	if (!h || !extents) return fail(BHIP_E_ARG, "bhip_lane_extents: null argument");
	HIPCHK(hipSetDevice(h->device));
	DBuf d;
	const uint64_t n = (uint64_t)h->n_clumps * 16;
	if (!n) return BHIP_OK;
	int rc = d.reserve(n * 4); if (rc) return rc;
	hipLaunchKernelGGL(k_lane_extent, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)h->n_cu * 16)), dim3(256), 0, h->stream, h->ref_lane.as<uint4>(), h->ref_off.as<uint64_t>(),
		h->clump_len.as<uint32_t>(), h->n_clumps, d.as<uint32_t>());
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(extents, d.p, n * 4, hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
	d.release();
	if (e != hipSuccess) return fail(BHIP_E_DEVICE, "bhip_lane_extents: %s", hipGetErrorString(e));
	return BHIP_OK;
}
