// burst_amd/csrc/bhip_consensus.hip -- the consensus of one sample on every reference position its printed lines cover (burst_hip
// --consensus; bhip_consensus_run, gfx950).  No reference counterpart: the definition is this project's own (include/burst_hip.h
// "Consensus"), a pure function of the sample's lines in integer arithmetic.
//
// The lines, observations, classes, Depth, the counts and Ref are those of the variant sites (bhip_pile.hip).  A position is COVERED when
// Depth >= 1, a SEGMENT is a maximal run of consecutive covered positions of a header, and every covered position gets a letter: N under
// min_depth, the reference's own letter where Ref is not A/C/G/T, else the largest of the counts A C G T Del (Ref first among equals, then
// that order; '-' for Del).
//
// The work follows lines + events + covered positions.  No kernel here loops over the columns of a line.
//   pile_stage_lines    (bhip_pile.hip) events counted; starts and one-past-ends sorted with the running sums of their weights
//   pile_stage_cands    (bhip_pile.hip) the events sorted and reduced to candidate sites: the only positions whose call can differ from Ref
//   sort                the line numbers by start key header << 32 | pos (the same stable sort of the same keys as the sorted starts: entry i
//                       of both belongs to one line)
//   k_cons_reach, scan  inclusive MAX-scan of (one-past-end key, line) in that order: how far the lines up to i reach, and one line that
//                       reaches there.  pos + span <= 2^32 - 1 keeps every end key of header h below every start key of header h + 1, so
//                       the unsegmented scan starts anew at a header change by itself
//   k_cons_heads, scan  line i opens a segment when i == 0 or its start key is GREATER than the reach before it (equal = adjacent = the same
//                       segment); the scan numbers the segments
//   k_cons_segs, scan   start key and reach of every segment; the exclusive sum of the lengths gives the letter offsets and the total
//   k_cons_fill         one thread per CONS_RUN consecutive output slots: the STABBING COUNT of bhip_pile.hip's k_pile_finish, (weights of
//                       the starts <= key) - (weights of the one-past-ends <= key), with two binary searches for the thread's first slot and
//                       two cursors that only move forwards after it; the line that reaches furthest among the starts <= key covers the
//                       position (the position is covered and that line ends last), and the reference code is read from its lane column.
//                       Letter: N under min_depth, else the reference's; 16 letters leave in one store.  Called / Same / Ambig are summed
//                       per wave where the wave lies in one segment, else per thread, and added to the segment with integer atomics
//   k_cons_call         one thread per candidate site: its slot by a binary search of the segment starts, its depth as k_pile_finish takes
//                       it, rules 2 and 3 on the full counts; it replaces the letter and moves the position between Same / Subst / Del /
//                       Ambig, and counts InsMajor
// Nothing depends on the order of threads: every slot and every candidate is written by one thread, the figures are integer sums, the
// sorts are stable and the scans' operators associative.  The one choice that depends on the order of the LINES is which of several lines
// that reach equally far lends its lane column for the reference code; lanes that share a position agree there (the variants' assumption).
#include "bhip_pile.h"

#define CONS_RUN 16u

struct ConsReach { unsigned long long end; unsigned long long line; };
struct ConsReachMax {      // associative; the earlier of two that reach equally far
	__host__ __device__ __forceinline__ ConsReach operator()(const ConsReach &a, const ConsReach &b) const { return b.end > a.end ? b : a; }
};

__global__ __launch_bounds__(PILE_BLOCK) void k_cons_iota(pile_u64 *__restrict__ v, uint64_t n) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) v[i] = i;
}

// order = the line numbers sorted by start key; k_end = the one-past-end keys in the order of the lines
__global__ __launch_bounds__(PILE_BLOCK) void k_cons_reach(const pile_u64 *__restrict__ order, const pile_u64 *__restrict__ k_end, uint64_t n, ConsReach *__restrict__ reach) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const pile_u64 ln = order[i];
		ConsReach r; r.end = ln < n ? k_end[ln] : 0ull; r.line = ln;
		reach[i] = r;
	}
}

// reach = the inclusive max-scan.  (head[n] = 0: the scan's extra element holds the number of segments)
__global__ __launch_bounds__(PILE_BLOCK) void k_cons_heads(const pile_u64 *__restrict__ k_start_s, const ConsReach *__restrict__ reach, uint64_t n, pile_u64 *__restrict__ head) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x)
		head[i] = (i < n && (i == 0 || k_start_s[i] > reach[i - 1].end)) ? 1ull : 0ull;
}

// ix = the exclusive scan of head.  seg_key[s] = the start key of segment s; seg_len[s] = its length; (seg_len[n_segs] = 0 for the scan's total)
__global__ __launch_bounds__(PILE_BLOCK) void k_cons_segs(const pile_u64 *__restrict__ k_start_s, const ConsReach *__restrict__ reach, const pile_u64 *__restrict__ head,
		const pile_u64 *__restrict__ ix, uint64_t n, uint64_t n_segs, pile_u64 *__restrict__ seg_key, pile_u64 *__restrict__ seg_end) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const pile_u64 s = ix[i] - (head[i] ? 0ull : 1ull);      // the segment line i belongs to
		if (s >= n_segs) continue;
		if (head[i]) seg_key[s] = k_start_s[i];
		if (i + 1 == n || head[i + 1]) seg_end[s] = reach[i].end;      // the last line of its segment
	}
}

__global__ __launch_bounds__(PILE_BLOCK) void k_cons_lens(const pile_u64 *__restrict__ seg_key, const pile_u64 *__restrict__ seg_end, uint64_t n_segs, pile_u64 *__restrict__ seg_len) {
	for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s <= n_segs; s += (uint64_t)gridDim.x * blockDim.x)
		seg_len[s] = s < n_segs ? seg_end[s] - seg_key[s] : 0ull;
}

// seg_off = the exclusive sum of the lengths; the figures start at 0
__global__ __launch_bounds__(PILE_BLOCK) void k_cons_seg_init(const pile_u64 *__restrict__ seg_key, const pile_u64 *__restrict__ seg_len, const pile_u64 *__restrict__ seg_off,
		uint64_t n_segs, BhipConsSeg *__restrict__ segs) {
	for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < n_segs; s += (uint64_t)gridDim.x * blockDim.x) {
		BhipConsSeg g;
		g.header = (uint32_t)(seg_key[s] >> 32); g.pos = (uint32_t)seg_key[s]; g.len = (uint32_t)seg_len[s];
		g.called = g.same = g.subst = g.del = g.ambig = g.ins_major = g.pad = 0u;
		g.off = seg_off[s];
		segs[s] = g;
	}
}

__device__ __forceinline__ void cons_add(BhipConsSeg *__restrict__ g, uint32_t called, uint32_t same, uint32_t ambig) {
	if (called) atomicAdd(&g->called, called);
	if (same) atomicAdd(&g->same, same);
	if (ambig) atomicAdd(&g->ambig, ambig);
}
__device__ __forceinline__ uint32_t cons_wave_sum(uint32_t v) {
	for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
	return v;
}

// one thread per CONS_RUN consecutive slots (the grid covers all of them: no stride, so that the threads of a wave hold neighbouring runs)
__global__ __launch_bounds__(PILE_BLOCK) void k_cons_fill(uint64_t n_slots, BhipConsSeg *__restrict__ segs, uint64_t n_segs, const pile_u64 *__restrict__ seg_key,
		const pile_u64 *__restrict__ seg_off, const pile_u64 *__restrict__ k_start_s, const pile_u64 *__restrict__ cs, const pile_u64 *__restrict__ k_end_s,
		const pile_u64 *__restrict__ ce, const ConsReach *__restrict__ reach, uint64_t n_lines, const PileLine *__restrict__ lines, const uint32_t *__restrict__ refw,
		const uint64_t *__restrict__ ref_off, const uint32_t *__restrict__ clump_len, uint32_t min_depth, char *__restrict__ letters) {
	const uint64_t s0 = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) * CONS_RUN;
	const bool valid = s0 < n_slots;
	uint64_t seg = 0;
	uint32_t called = 0, same = 0, ambig = 0;
	if (valid) {
		const uint64_t e = s0 + CONS_RUN < n_slots ? s0 + CONS_RUN : n_slots;
		seg = pile_upper_bound(seg_off, n_segs, s0) - 1;      // (seg_off[0] = 0 <= s0; the lengths are >= 1, so the offsets ascend strictly)
		pile_u64 key0 = seg_key[seg], off0 = seg_off[seg], off1 = seg_off[seg + 1];
		uint64_t a = 0, b = 0, cur = ~0ull;
		uint64_t base = 0; long long col0 = 0; pile_u64 cov_end = 0;
		uint32_t word[CONS_RUN / 4] = {0, 0, 0, 0};
#pragma unroll
		for (uint32_t t = 0; t < CONS_RUN; ++t) {      // (unrolled: word[] stays in registers)
			const uint64_t s = s0 + t;
			if (s >= e) break;
			if (s >= off1) {      // the next segment (one step: every segment has a slot)
				cons_add(&segs[seg], called, same, ambig);
				called = same = ambig = 0;
				++seg; key0 = seg_key[seg]; off0 = off1; off1 = seg_off[seg + 1];
			}
			const pile_u64 key = key0 + (s - off0);      // (pos + len <= 2^32 - 1: no carry into the header)
			if (t == 0) { a = pile_upper_bound(k_start_s, n_lines, key); b = pile_upper_bound(k_end_s, n_lines, key); }
			else {
				while (a < n_lines && k_start_s[a] <= key) ++a;
				while (b < n_lines && k_end_s[b] <= key) ++b;
			}
			char letter = 'N';
			if (a) {
				const pile_u64 depth = cs[a - 1] - (b ? ce[b - 1] : 0ull);
				if (a != cur) {      // the line that reaches furthest among the starts <= key
					cur = a;
					const ConsReach r = reach[a - 1];
					cov_end = r.end;
					if (r.line < n_lines) {
						const PileLine ln = lines[r.line];
						const uint32_t c = ln.refIx >> 4, z = ln.refIx & 15u, nchunks = (clump_len[c] + 31u) >> 5;
						base = (ref_off[c] * 16 + (uint64_t)z * nchunks) * 4;
						col0 = (long long)ln.ref_first - 1 - (long long)ln.pos;
					} else cov_end = 0;
				}
				if (key < cov_end && depth >= min_depth) {      // (key < cov_end: the position is inside that line, whose columns were checked on the host)
					const uint32_t ref = pile_ref(refw, base, (uint32_t)(col0 + (long long)(uint32_t)key));
					letter = "NACGTNKMRYSWBVHD"[ref];
					++called;
					if (ref >= 1u && ref <= 4u) ++same; else ++ambig;
				}
			}
			word[t >> 2] |= (uint32_t)(uint8_t)letter << (8u * (t & 3u));
		}
		if (e - s0 == CONS_RUN) *(uint4 *)(letters + s0) = make_uint4(word[0], word[1], word[2], word[3]);      // (s0 is a multiple of 16, the buffer aligned)
		else for (uint64_t s = s0; s < e; ++s) { const uint32_t t = (uint32_t)(s - s0); letters[s] = (char)(word[t >> 2] >> (8u * (t & 3u))); }
	}
	// the figures of the thread's last segment: one sum per wave where all its threads end in one segment
	const unsigned long long seg_first = __shfl((unsigned long long)seg, 0, 64);      // (lane 0 holds the smallest slots: when it has none, no lane has)
	if (__all(!valid || seg == seg_first)) {
		called = cons_wave_sum(valid ? called : 0u); same = cons_wave_sum(valid ? same : 0u); ambig = cons_wave_sum(valid ? ambig : 0u);
		if ((threadIdx.x & 63u) == 0u && valid) cons_add(&segs[seg], called, same, ambig);
	} else if (valid) cons_add(&segs[seg], called, same, ambig);
}

// one thread per candidate site: rules 2 and 3 on the full counts
__global__ __launch_bounds__(PILE_BLOCK) void k_cons_call(const PileCand *__restrict__ cand, uint64_t n_cand, BhipConsSeg *__restrict__ segs, uint64_t n_segs,
		const pile_u64 *__restrict__ seg_key, const pile_u64 *__restrict__ k_start_s, const pile_u64 *__restrict__ cs, const pile_u64 *__restrict__ k_end_s,
		const pile_u64 *__restrict__ ce, uint64_t n_lines, uint32_t min_depth, uint64_t n_slots, char *__restrict__ letters) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_cand; i += (uint64_t)gridDim.x * blockDim.x) {
		const PileCand cd = cand[i];
		const uint64_t sg = pile_upper_bound(seg_key, n_segs, cd.key);
		if (!sg) continue;
		BhipConsSeg *g = &segs[sg - 1];
		const pile_u64 within = cd.key - seg_key[sg - 1];
		if (within >= g->len) continue;      // (every event lies on a covered position)
		const uint64_t slot = g->off + within;
		if (slot >= n_slots) continue;
		const uint64_t a = pile_upper_bound(k_start_s, n_lines, cd.key), b = pile_upper_bound(k_end_s, n_lines, cd.key);
		const pile_u64 depth = (a ? cs[a - 1] : 0ull) - (b ? ce[b - 1] : 0ull);
		if (depth < min_depth) continue;
		if (2ull * cd.ins > depth) atomicAdd(&g->ins_major, 1u);
		// what k_cons_fill counted here: Same for a letter A/C/G/T, else Ambig
		const char was = letters[slot];
		uint32_t *from = (was == 'A' || was == 'C' || was == 'G' || was == 'T') ? &g->same : &g->ambig, *to;
		char letter;
		if (cd.ref >= 1u && cd.ref <= 4u) {
			pile_u64 n[5], seen = 0;
			for (int c = 0; c < 6; ++c) seen += cd.n[c];
			for (int c = 0; c < 5; ++c) n[c] = cd.n[c];
			n[cd.ref - 1u] += depth - seen;      // the plain observations
			uint32_t win = cd.ref - 1u;
			for (uint32_t c = 0; c < 5u; ++c) if (n[c] > n[win]) win = c;      // only a larger count moves it: Ref among equal largest counts, else the first in the order A C G T Del
			letter = "ACGT-"[win];
			to = win == cd.ref - 1u ? &g->same : win == 4u ? &g->del : &g->subst;
		} else { letter = "NACGTNKMRYSWBVHD"[cd.ref]; to = &g->ambig; }
		if (to != from) { atomicSub(from, 1u); atomicAdd(to, 1u); }
		letters[slot] = letter;
	}
}

struct ConsState {
	DBuf ord_in, ord, reach_in, reach, head, ix, seg_key, seg_end, seg_len, seg_off, segs, letters, tmp;
	uint64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint64_t bytes() const {
		const DBuf *all[] = {&ord_in, &ord, &reach_in, &reach, &head, &ix, &seg_key, &seg_end, &seg_len, &seg_off, &segs, &letters, &tmp};
		uint64_t b = 0;
		for (const DBuf *x : all) b += x->cap;
		return b;
	}
};

// (bhip_handle.h: Handle::cons)
void bhip_consensus_release(Handle *h) {
	ConsState *cs = (ConsState *)h->cons;
	if (!cs) return;
	DBuf *all[] = {&cs->ord_in, &cs->ord, &cs->reach_in, &cs->reach, &cs->head, &cs->ix, &cs->seg_key, &cs->seg_end, &cs->seg_len, &cs->seg_off, &cs->segs, &cs->letters, &cs->tmp};
	for (DBuf *x : all) x->release();
	delete cs;
	h->cons = nullptr;
}

extern "C" int bhip_consensus_info(void *handle, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	if (!h || !info) return fail(BHIP_E_ARG, "bhip_consensus_info: null argument");
	if (h->cons) memcpy(info, ((ConsState *)h->cons)->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t));
	return BHIP_OK;
}

extern "C" int bhip_consensus_run(void *handle, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
		const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, BhipConsSeg *segs, uint64_t seg_cap, uint64_t *n_segs, char *letters, uint64_t letter_cap,
		uint64_t *n_letters, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!h || !n_segs || !n_letters || (n_lines && (!lines || !q_codes || !q_off)) || (n_ops && !ops) || (seg_cap && !segs) || (letter_cap && !letters))
		return fail(BHIP_E_ARG, "bhip_consensus_run: null argument");
	*n_segs = *n_letters = 0;
	if (h->cons) memset(((ConsState *)h->cons)->info, 0, 8 * sizeof(uint64_t));
	if (!min_depth || min_depth > 0x7FFFFFFFu) return fail(BHIP_E_ARG, "bhip_consensus_run: min_depth %u (1 .. 2^31 - 1)", min_depth);
	PileInput in;
	int rc = pile_check_lines("bhip_consensus_run", h, q_codes, q_off, n_queries, lines, n_lines, ops, n_ops, in);
	if (rc) return rc;
	if (!n_lines) return BHIP_OK;      // (no segments, no launch)
	HIPCHK(hipSetDevice(h->device));
	PileState *st = nullptr;
	rc = pile_state(h, &st); if (rc) return rc;
	ConsState *cn = (ConsState *)h->cons;
	if (!cn) { cn = new ConsState(); h->cons = cn; }
	hipStream_t S = h->stream;
	const uint64_t nl = n_lines;
	const int end_bit = in.end_bit();
	uint64_t us = 0;
	pile_u64 n_events = 0, n_cand = 0;
	// 1. events and candidate sites, as the variants take them
	rc = pile_stage_lines(h, st, in, ops, n_ops, &n_events, &us); if (rc) return rc;
	if (n_events) { rc = pile_stage_cands(h, st, in, n_events, "bhip_consensus_run", &n_cand, &us); if (rc) return rc; }
	// 2. segments
	DBuf *per_line[] = {&cn->ord_in, &cn->ord};
	for (DBuf *x : per_line) { rc = x->reserve(nl * 8); if (rc) return rc; }
	rc = cn->reach_in.reserve(nl * sizeof(ConsReach)); if (rc) return rc;
	rc = cn->reach.reserve(nl * sizeof(ConsReach)); if (rc) return rc;
	rc = cn->head.reserve((nl + 1) * 8); if (rc) return rc;
	rc = cn->ix.reserve((nl + 1) * 8); if (rc) return rc;
	size_t tb_sort = 0, tb_max = 0, tb_sum = 0;
	// (the keys go to st->w_start_s, which nobody reads any more: st->k_start_s stays as pile_stage_lines left it, and holds the same values)
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, st->k_start.as<pile_u64>(), st->w_start_s.as<pile_u64>(), cn->ord_in.as<pile_u64>(), cn->ord.as<pile_u64>(), (size_t)nl, 0, end_bit, S));
	HIPCHK(hipcub::DeviceScan::InclusiveScan(nullptr, tb_max, cn->reach_in.as<ConsReach>(), cn->reach.as<ConsReach>(), ConsReachMax(), (size_t)nl, S));
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_sum, cn->head.as<pile_u64>(), cn->ix.as<pile_u64>(), (size_t)(nl + 1), S));
	rc = cn->tmp.reserve(std::max(tb_sort, std::max(tb_max, tb_sum)) + 16); if (rc) return rc;
	HIPCHK(hipEventRecord(st->ev0, S));
	hipLaunchKernelGGL(k_cons_iota, dim3(pile_grid(nl)), dim3(PILE_BLOCK), 0, S, cn->ord_in.as<pile_u64>(), nl);
	HIPCHK(hipGetLastError());
	size_t tb = cn->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(cn->tmp.p, tb, st->k_start.as<pile_u64>(), st->w_start_s.as<pile_u64>(), cn->ord_in.as<pile_u64>(), cn->ord.as<pile_u64>(), (size_t)nl, 0, end_bit, S));
	hipLaunchKernelGGL(k_cons_reach, dim3(pile_grid(nl)), dim3(PILE_BLOCK), 0, S, cn->ord.as<pile_u64>(), st->k_end.as<pile_u64>(), nl, cn->reach_in.as<ConsReach>());
	HIPCHK(hipGetLastError());
	tb = cn->tmp.cap;
	HIPCHK(hipcub::DeviceScan::InclusiveScan(cn->tmp.p, tb, cn->reach_in.as<ConsReach>(), cn->reach.as<ConsReach>(), ConsReachMax(), (size_t)nl, S));
	hipLaunchKernelGGL(k_cons_heads, dim3(pile_grid(nl + 1)), dim3(PILE_BLOCK), 0, S, st->k_start_s.as<pile_u64>(), cn->reach.as<ConsReach>(), nl, cn->head.as<pile_u64>());
	HIPCHK(hipGetLastError());
	tb = cn->tmp.cap;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(cn->tmp.p, tb, cn->head.as<pile_u64>(), cn->ix.as<pile_u64>(), (size_t)(nl + 1), S));
	HIPCHK(hipEventRecord(st->ev1, S));
	pile_u64 ns = 0;
	HIPCHK(hipMemcpyAsync(&ns, (char *)cn->ix.p + nl * 8, 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	if (!ns || ns > nl) return fail(BHIP_E_INTERNAL, "bhip_consensus_run: %llu segments of %llu lines", ns, (pile_u64)nl);
	DBuf *per_seg[] = {&cn->seg_key, &cn->seg_end, &cn->seg_len, &cn->seg_off};
	for (DBuf *x : per_seg) { rc = x->reserve((ns + 1) * 8); if (rc) return rc; }
	rc = cn->segs.reserve(ns * sizeof(BhipConsSeg)); if (rc) return rc;
	tb_sum = 0;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_sum, cn->seg_len.as<pile_u64>(), cn->seg_off.as<pile_u64>(), (size_t)(ns + 1), S));
	rc = cn->tmp.reserve(tb_sum + 16); if (rc) return rc;
	HIPCHK(hipEventRecord(st->ev0, S));
	hipLaunchKernelGGL(k_cons_segs, dim3(pile_grid(nl)), dim3(PILE_BLOCK), 0, S, st->k_start_s.as<pile_u64>(), cn->reach.as<ConsReach>(), cn->head.as<pile_u64>(), cn->ix.as<pile_u64>(),
		nl, (uint64_t)ns, cn->seg_key.as<pile_u64>(), cn->seg_end.as<pile_u64>());
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_cons_lens, dim3(pile_grid(ns + 1)), dim3(PILE_BLOCK), 0, S, cn->seg_key.as<pile_u64>(), cn->seg_end.as<pile_u64>(), (uint64_t)ns, cn->seg_len.as<pile_u64>());
	HIPCHK(hipGetLastError());
	tb = cn->tmp.cap;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(cn->tmp.p, tb, cn->seg_len.as<pile_u64>(), cn->seg_off.as<pile_u64>(), (size_t)(ns + 1), S));
	HIPCHK(hipEventRecord(st->ev1, S));
	pile_u64 total = 0;
	HIPCHK(hipMemcpyAsync(&total, (char *)cn->seg_off.p + ns * 8, 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	if (total > 0x7FFFFFFFull) return fail(BHIP_E_ARG, "bhip_consensus_run: the lines cover %llu positions (at most 2^31 - 1 in one call)", total);
	if (total < ns) return fail(BHIP_E_INTERNAL, "bhip_consensus_run: %llu segments hold %llu positions", ns, total);
	info[0] = n_events; info[1] = n_cand; info[2] = ns; info[3] = total;
	*n_segs = ns; *n_letters = total;
	if (ns > seg_cap || total > letter_cap) {
		info[4] = us; info[5] = st->bytes() + cn->bytes();
		memcpy(cn->info, info, sizeof cn->info);
		return fail(BHIP_E_CAPACITY, "bhip_consensus_run: %llu segments and %llu letters, room for %llu and %llu", ns, total, (pile_u64)seg_cap, (pile_u64)letter_cap);
	}
	// 3. + 4. + 5. depth, letter and figures of every covered position; then the candidate sites
	rc = cn->letters.reserve(((size_t)total + 15) / 16 * 16 + 16); if (rc) return rc;
	HIPCHK(hipEventRecord(st->ev0, S));
	hipLaunchKernelGGL(k_cons_seg_init, dim3(pile_grid(ns)), dim3(PILE_BLOCK), 0, S, cn->seg_key.as<pile_u64>(), cn->seg_len.as<pile_u64>(), cn->seg_off.as<pile_u64>(), (uint64_t)ns,
		cn->segs.as<BhipConsSeg>());
	HIPCHK(hipGetLastError());
	const uint64_t n_runs = (total + CONS_RUN - 1) / CONS_RUN;
	hipLaunchKernelGGL(k_cons_fill, dim3((uint32_t)((n_runs + PILE_BLOCK - 1) / PILE_BLOCK)), dim3(PILE_BLOCK), 0, S, (uint64_t)total, cn->segs.as<BhipConsSeg>(), (uint64_t)ns,
		cn->seg_key.as<pile_u64>(), cn->seg_off.as<pile_u64>(), st->k_start_s.as<pile_u64>(), st->cs.as<pile_u64>(), st->k_end_s.as<pile_u64>(), st->ce.as<pile_u64>(),
		cn->reach.as<ConsReach>(), nl, st->lines.as<PileLine>(), h->ref_lane.as<uint32_t>(), h->ref_off.as<uint64_t>(), h->clump_len.as<uint32_t>(), min_depth, cn->letters.as<char>());
	HIPCHK(hipGetLastError());
	if (n_cand) {
		rc = pile_launch_reduce(h, st, n_events, n_cand); if (rc) return rc;
		hipLaunchKernelGGL(k_cons_call, dim3(pile_grid(n_cand)), dim3(PILE_BLOCK), 0, S, st->cand.as<PileCand>(), (uint64_t)n_cand, cn->segs.as<BhipConsSeg>(), (uint64_t)ns,
			cn->seg_key.as<pile_u64>(), st->k_start_s.as<pile_u64>(), st->cs.as<pile_u64>(), st->k_end_s.as<pile_u64>(), st->ce.as<pile_u64>(), nl, min_depth, (uint64_t)total,
			cn->letters.as<char>());
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipEventRecord(st->ev1, S));
	HIPCHK(hipMemcpyAsync(segs, cn->segs.p, ns * sizeof(BhipConsSeg), hipMemcpyDeviceToHost, S));
	HIPCHK(hipMemcpyAsync(letters, cn->letters.p, total, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	info[4] = us; info[5] = st->bytes() + cn->bytes();
	memcpy(cn->info, info, sizeof cn->info);
	return BHIP_OK;
}
