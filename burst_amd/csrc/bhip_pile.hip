// burst_amd/csrc/bhip_pile.hip -- variant sites of one sample from the alignment paths of its printed lines (burst_hip --variants;
// bhip_pile_run, gfx950).  No reference counterpart: the reference prints how many edits a placement has, never which bases a sample shows
// at a reference position.
//
// Definition (include/burst_hip.h "Variant sites", DESIGN.md section 3 "Pile-up").  A line is a path (bhip_trace_paths' ops and first lane
// column) of a query entry on a lane, placed at position `pos` of header `header`, standing for `w` reads.  Walking its ops forwards with
// reference position p = pos and query index j = 0: '=' or X gives one observation (header, p, class of query[j]) per symbol, D one
// observation (header, p, Del) per column, an I run that is neither the first nor the last op one insertion mark (header, p - 1).  A site
// (header, position) has the weighted counts A C G T Del Other of its observations, Depth = their sum, Ins = its marks, Ref = the code of the
// lane column the observing paths consumed there.  It is returned when Ref is A/C/G/T, Depth >= min_depth and Depth - count[Ref] >= min_alt
// or Ins >= min_alt.
//
// The device work follows the lines and their edits, never lines x read length.  An observation is PLAIN when its op is '=' and its query
// code is A/C/G/T: at a site whose Ref is A/C/G/T it is a Ref observation, and a site with plain observations only is never returned.
//   k_pile_walk<false>  one thread per line walks its ops and COUNTS its events: every observation that is not plain, every insertion mark.
//                       Runs of '=' are only scanned for ambiguous query codes, four symbols per word where the address allows.
//   scan                exclusive sum of the counts (64-bit)
//   k_pile_walk<true>   the walk again, writing key = header << 32 | position and value = weight | class << 32 | ref code << 36
//   sort                hipcub radix sort of the events by key
//   k_pile_heads, scan  an event that differs from its predecessor opens a candidate site; the scan numbers the candidates
//   k_pile_reduce       the opening event's thread walks its run (bounded by the end of the array and the key) and sums the classes, the
//                       marks and the smallest ref code: 64-bit integer sums, so the order inside a run changes nothing
//   k_pile_bounds, sort per line the keys of its first position and of the position behind its last, each sorted with the weights; inclusive
//                       sums of the weights in both orders
//   k_pile_finish       per candidate the STABBING COUNT: the weight of the lines whose range [pos, pos + ('=' + X + D) - 1] holds the site
//                       = (weights of the starts <= key) - (weights of the one-past-ends <= key): lines of a smaller header are in both
//                       sums, lines of a larger header in neither, a line of this header that starts at or before the site is in the first
//                       and leaves through the second once the site is behind it.  Every covering line observes the site exactly once
//                       ('=', X and D consume one column each), so the count IS the depth, and depth - (observations that are not plain)
//                       = the plain ones, which go to count[Ref].  Then the thresholds.
//   select, copy        hipcub flagged selection keeps the order of the candidates, which is ascending (header, position)
// Lanes that share header positions are taken to agree there (they are cuts of one original sequence): Ref is the smallest ref code among
// the events of a site, and plain observations count as Ref.
#include "bhip_pile.h"

__device__ __forceinline__ uint32_t pile_class(uint32_t code) { return code >= 1u && code <= 4u ? code - 1u : PILE_CLS_OTHER; }
__device__ __forceinline__ unsigned long long pile_value(uint32_t w, uint32_t cls, uint32_t ref) { return (unsigned long long)w | (unsigned long long)cls << 32 | (unsigned long long)ref << 36; }

// EMIT = false: cnt[i] = events of line i.  EMIT = true: off = the exclusive scan of cnt; the events at their offsets
template <bool EMIT>
__global__ __launch_bounds__(PILE_BLOCK) void k_pile_walk(const PileLine *__restrict__ lines, uint64_t n_lines, const uint32_t *__restrict__ ops, const uint8_t *__restrict__ codes,
		const uint32_t *__restrict__ refw, const uint64_t *__restrict__ ref_off, const uint32_t *__restrict__ clump_len,
		unsigned long long *__restrict__ cnt, const unsigned long long *__restrict__ off, uint64_t n_events,
		unsigned long long *__restrict__ ev_key, unsigned long long *__restrict__ ev_val) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_lines; i += (uint64_t)gridDim.x * blockDim.x) {
		const PileLine ln = lines[i];
		const uint32_t c = ln.refIx >> 4, z = ln.refIx & 15u, nchunks = (clump_len[c] + 31u) >> 5;
		const uint64_t base = (ref_off[c] * 16 + (uint64_t)z * nchunks) * 4;
		const unsigned long long hkey = (unsigned long long)ln.header << 32;
		uint32_t p = ln.pos, col = ln.ref_first - 1u;      // position on the header; 0-based lane column
		unsigned long long j = ln.qbase, o = EMIT ? off[i] : 0ull, n_ev = 0;
		const unsigned long long end = EMIT ? off[i + 1] : 0ull;
		if (EMIT && (o == end || end > n_events)) continue;
#define PILE_EVENT(at, cls, rc) do { if (EMIT) { if (o < end) { ev_key[o] = hkey | (unsigned long long)(at); ev_val[o] = pile_value(ln.w, (cls), (rc)); ++o; } } else ++n_ev; } while (0)
		for (uint32_t k = 0; k < ln.n_ops; ++k) {
			const uint32_t word = ops[ln.op_off + k], len = word >> 4, code = word & 15u;
			if (code == BHIP_OP_EQ) {
				uint32_t t = 0;
				while (t < len) {
					if (((j + t) & 3ull) == 0 && len - t >= 4u) {      // four symbols: all of them A/C/G/T iff every byte + 3 is 4 .. 7
						const uint32_t four = *(const uint32_t *)(codes + j + t) & 0x0F0F0F0Fu;
						if (((four + 0x03030303u) & 0xFCFCFCFCu) == 0x04040404u) { t += 4; continue; }
					}
					const uint32_t q = codes[j + t] & 15u;
					if (q < 1u || q > 4u) PILE_EVENT(p + t, PILE_CLS_OTHER, pile_ref(refw, base, col + t));
					++t;
				}
				p += len; col += len; j += len;
			} else if (code == BHIP_OP_X) {
				for (uint32_t t = 0; t < len; ++t) PILE_EVENT(p + t, pile_class(codes[j + t] & 15u), pile_ref(refw, base, col + t));
				p += len; col += len; j += len;
			} else if (code == BHIP_OP_D) {
				for (uint32_t t = 0; t < len; ++t) PILE_EVENT(p + t, PILE_CLS_DEL, pile_ref(refw, base, col + t));
				p += len; col += len;
			} else {      // I: the column before it was consumed by the op before it
				if (k > 0 && k + 1 < ln.n_ops) PILE_EVENT(p - 1u, PILE_CLS_INS, pile_ref(refw, base, col - 1u));
				j += len;
			}
		}
#undef PILE_EVENT
		if (!EMIT) cnt[i] = n_ev;
	}
}

__global__ __launch_bounds__(PILE_BLOCK) void k_pile_heads(const unsigned long long *__restrict__ key, uint64_t n, unsigned long long *__restrict__ head) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x)
		head[i] = (i < n && (i == 0 || key[i] != key[i - 1])) ? 1ull : 0ull;      // (head[n] = 0: the scan's extra element holds the total)
}

// idx = the exclusive scan of head: the candidate an event belongs to
__global__ __launch_bounds__(PILE_BLOCK) void k_pile_reduce(const unsigned long long *__restrict__ key, const unsigned long long *__restrict__ val, uint64_t n,
		const unsigned long long *__restrict__ head, const unsigned long long *__restrict__ idx, uint64_t n_cand, PileCand *__restrict__ cand) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		if (!head[i] || idx[i] >= n_cand) continue;
		const unsigned long long k = key[i];
		unsigned long long s[7] = {0, 0, 0, 0, 0, 0, 0};
		uint32_t rmin = 15u;
		for (uint64_t e = i; e < n && key[e] == k; ++e) {
			const unsigned long long v = val[e];
			const uint32_t cls = (uint32_t)(v >> 32) & 15u, r = (uint32_t)(v >> 36) & 15u;
			if (cls <= PILE_CLS_INS) s[cls] += v & 0xFFFFFFFFull;
			rmin = r < rmin ? r : rmin;
		}
		PileCand cd;
		cd.key = k;
		for (int a = 0; a < 6; ++a) cd.n[a] = (uint32_t)s[a];      // (the summed weights of a call are below 2^31)
		cd.ins = (uint32_t)s[PILE_CLS_INS]; cd.ref = rmin;
		cand[idx[i]] = cd;
	}
}

// per line: the key of its first position and of the position behind its last, the weight beside both
__global__ __launch_bounds__(PILE_BLOCK) void k_pile_bounds(const PileLine *__restrict__ lines, const uint32_t *__restrict__ span, uint64_t n_lines,
		unsigned long long *__restrict__ k_start, unsigned long long *__restrict__ k_end, unsigned long long *__restrict__ w_start, unsigned long long *__restrict__ w_end) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_lines; i += (uint64_t)gridDim.x * blockDim.x) {
		const unsigned long long hkey = (unsigned long long)lines[i].header << 32;
		k_start[i] = hkey | lines[i].pos;
		k_end[i] = hkey | (unsigned long long)(lines[i].pos + span[i]);      // (pos + span <= 2^32 - 1: checked on the host)
		w_start[i] = w_end[i] = lines[i].w;
	}
}

// cs / ce = the inclusive sums of the weights in the order of the sorted starts / one-past-ends
__global__ __launch_bounds__(PILE_BLOCK) void k_pile_finish(const PileCand *__restrict__ cand, uint64_t n_cand, const unsigned long long *__restrict__ k_start,
		const unsigned long long *__restrict__ cs, const unsigned long long *__restrict__ k_end, const unsigned long long *__restrict__ ce, uint64_t n_lines,
		uint32_t min_depth, uint32_t min_alt, BhipPileSite *__restrict__ site, uint8_t *__restrict__ keep) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_cand; i += (uint64_t)gridDim.x * blockDim.x) {
		const PileCand cd = cand[i];
		const uint64_t a = pile_upper_bound(k_start, n_lines, cd.key), b = pile_upper_bound(k_end, n_lines, cd.key);
		const unsigned long long depth = (a ? cs[a - 1] : 0ull) - (b ? ce[b - 1] : 0ull);
		unsigned long long n[6], seen = 0;
		for (int c = 0; c < 6; ++c) { n[c] = cd.n[c]; seen += n[c]; }
		const bool acgt = cd.ref >= 1u && cd.ref <= 4u;
		if (acgt) n[cd.ref - 1u] += depth - seen;
		BhipPileSite s;
		s.header = (uint32_t)(cd.key >> 32); s.pos = (uint32_t)cd.key; s.ref = cd.ref; s.depth = (uint32_t)depth;
		for (int c = 0; c < 6; ++c) s.n[c] = (uint32_t)n[c];
		s.ins = cd.ins;
		site[i] = s;
		keep[i] = (acgt && depth >= min_depth && (depth - n[cd.ref - 1u] >= min_alt || cd.ins >= min_alt)) ? 1 : 0;
	}
}

// (bhip_handle.h: Handle::pile)
void bhip_pile_release(Handle *h) {
	PileState *st = (PileState *)h->pile;
	if (!st) return;
	DBuf *all[] = {&st->lines, &st->span, &st->ops, &st->codes, &st->cnt, &st->off, &st->ev_key, &st->ev_val, &st->ev_key_s, &st->ev_val_s, &st->head, &st->idx, &st->cand,
		&st->k_start, &st->k_end, &st->w_start, &st->w_end, &st->k_start_s, &st->k_end_s, &st->w_start_s, &st->w_end_s, &st->cs, &st->ce, &st->site, &st->keep, &st->out, &st->n_sel, &st->tmp};
	for (DBuf *x : all) x->release();
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->pile = nullptr;
}

// ---- the stages bhip_pile_run and bhip_consensus_run share (bhip_pile.h) ----
// every line is checked on the host before the device is touched: the kernels index by these values alone
int pile_check_lines(const char *who, Handle *h, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
		const uint32_t *ops, uint64_t n_ops, PileInput &in) {
	if (n_lines >= (1ull << 32)) return fail(BHIP_E_ARG, "%s: %llu lines (fewer than 2^32)", who, (pile_u64)n_lines);
	in.dl.assign((size_t)n_lines, PileLine());
	in.span.assign((size_t)n_lines, 0u);
	in.codes.clear();
	in.max_header = 0;
	std::vector<uint64_t> qpos;
	if (n_lines) qpos.assign(n_queries, ~0ull);
	uint64_t wsum = 0;
	for (uint64_t i = 0; i < n_lines; ++i) {
		const BhipPileLine &u = lines[i];
		if (u.q >= n_queries) return fail(BHIP_E_ARG, "%s: line %llu names query %u of %u", who, (pile_u64)i, u.q, n_queries);
		if (q_off[u.q + 1] < q_off[u.q]) return fail(BHIP_E_ARG, "%s: line %llu: query %u has descending offsets", who, (pile_u64)i, u.q);
		if (u.refIx >= 16ull * h->n_clumps || u.refIx >= h->tot_refs) return fail(BHIP_E_ARG, "%s: line %llu names reference %u of %u", who, (pile_u64)i, u.refIx, h->tot_refs);
		if (u.op_off > n_ops || u.n_ops > n_ops - u.op_off) return fail(BHIP_E_ARG, "%s: line %llu owns ops %llu + %u of %llu", who, (pile_u64)i, (pile_u64)u.op_off, u.n_ops, (pile_u64)n_ops);
		uint64_t on_q = 0, on_r = 0;
		uint32_t last_code = 0;
		for (uint32_t k = 0; k < u.n_ops; ++k) {
			const uint32_t word = ops[u.op_off + k], len = word >> 4, code = word & 15u;
			if (!len || code == last_code || (code != BHIP_OP_I && code != BHIP_OP_D && code != BHIP_OP_EQ && code != BHIP_OP_X))      // (merged runs: an I that is not the first op follows a column)
				return fail(BHIP_E_ARG, "%s: line %llu, op %u: word 0x%x is not a run of I, D, = or X, or repeats the op before it", who, (pile_u64)i, k, word);
			last_code = code;
			if (code != BHIP_OP_D) on_q += len;
			if (code != BHIP_OP_I) on_r += len;
		}
		if (on_q != q_off[u.q + 1] - q_off[u.q])
			return fail(BHIP_E_ARG, "%s: line %llu: its ops consume %llu query symbols, query %u has %llu", who, (pile_u64)i, (pile_u64)on_q, u.q, (pile_u64)(q_off[u.q + 1] - q_off[u.q]));
		if (u.ref_first < 1 || (uint64_t)u.ref_first - 1 + on_r > h->h_clump_len[u.refIx >> 4])
			return fail(BHIP_E_ARG, "%s: line %llu: columns %u + %llu leave a clump of %u", who, (pile_u64)i, u.ref_first, (pile_u64)on_r, h->h_clump_len[u.refIx >> 4]);
		if (u.pos < 1 || (uint64_t)u.pos + on_r > 0xFFFFFFFFull) return fail(BHIP_E_ARG, "%s: line %llu: position %u + %llu columns (1 .. 2^32 - 1)", who, (pile_u64)i, u.pos, (pile_u64)on_r);
		if (!u.w) return fail(BHIP_E_ARG, "%s: line %llu has weight 0", who, (pile_u64)i);
		wsum += u.w;
		if (wsum > 0x7FFFFFFFull) return fail(BHIP_E_ARG, "%s: the lines stand for more than 2^31 - 1 reads (line %llu)", who, (pile_u64)i);
		if (qpos[u.q] == ~0ull) {      // (a query entry is uploaded once, word-aligned, however many lines it has)
			in.codes.resize((in.codes.size() + 3) & ~(size_t)3);
			qpos[u.q] = in.codes.size();
			in.codes.insert(in.codes.end(), q_codes + q_off[u.q], q_codes + q_off[u.q + 1]);
		}
		PileLine &d = in.dl[i];
		d.qbase = qpos[u.q]; d.op_off = u.op_off; d.refIx = u.refIx; d.ref_first = u.ref_first; d.header = u.header; d.pos = u.pos; d.w = u.w; d.n_ops = u.n_ops;
		in.span[i] = (uint32_t)on_r;
		in.max_header = std::max(in.max_header, u.header);
	}
	return BHIP_OK;
}

int pile_state(Handle *h, PileState **out) {
	PileState *st = (PileState *)h->pile;
	if (!st) {
		st = new PileState();
		h->pile = st;
		if (hipEventCreate(&st->ev0) != hipSuccess || hipEventCreate(&st->ev1) != hipSuccess) { bhip_pile_release(h); return fail(BHIP_E_DEVICE, "hipEventCreate failed"); }
	}
	*out = st;
	return BHIP_OK;
}

int pile_stage_lines(Handle *h, PileState *st, const PileInput &in, const uint32_t *ops, uint64_t n_ops, pile_u64 *n_events, uint64_t *us) {
	hipStream_t S = h->stream;
	const uint64_t nl = in.dl.size();
	const int end_bit = in.end_bit();
	int rc = st->lines.reserve(nl * sizeof(PileLine)); if (rc) return rc;
	rc = st->span.reserve(nl * 4); if (rc) return rc;
	rc = st->ops.reserve(n_ops * 4 + 16); if (rc) return rc;
	rc = st->codes.reserve(in.codes.size() + 16); if (rc) return rc;
	rc = st->cnt.reserve((nl + 1) * 8); if (rc) return rc;
	rc = st->off.reserve((nl + 1) * 8); if (rc) return rc;
	DBuf *per_line[] = {&st->k_start, &st->k_end, &st->w_start, &st->w_end, &st->k_start_s, &st->k_end_s, &st->w_start_s, &st->w_end_s, &st->cs, &st->ce};
	for (DBuf *x : per_line) { rc = x->reserve(nl * 8); if (rc) return rc; }
	size_t tb_scan = 0, tb_sort = 0, tb_sum = 0;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, st->cnt.as<pile_u64>(), st->off.as<pile_u64>(), (size_t)(nl + 1), S));
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, st->k_start.as<pile_u64>(), st->k_start_s.as<pile_u64>(), st->w_start.as<pile_u64>(), st->w_start_s.as<pile_u64>(), (size_t)nl, 0, end_bit, S));
	HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tb_sum, st->w_start_s.as<pile_u64>(), st->cs.as<pile_u64>(), (size_t)nl, S));
	rc = st->tmp.reserve(std::max(tb_scan, std::max(tb_sort, tb_sum)) + 16); if (rc) return rc;

	const PileLine *d_lines = st->lines.as<PileLine>();
	HIPCHK(hipMemcpyAsync(st->lines.p, in.dl.data(), nl * sizeof(PileLine), hipMemcpyHostToDevice, S));
	HIPCHK(hipMemcpyAsync(st->span.p, in.span.data(), nl * 4, hipMemcpyHostToDevice, S));
	if (n_ops) HIPCHK(hipMemcpyAsync(st->ops.p, ops, n_ops * 4, hipMemcpyHostToDevice, S));
	if (!in.codes.empty()) HIPCHK(hipMemcpyAsync(st->codes.p, in.codes.data(), in.codes.size(), hipMemcpyHostToDevice, S));
	HIPCHK(hipEventRecord(st->ev0, S));
	// 1. the events of every line: count, scan, and (pile_stage_cands) emit
	HIPCHK(hipMemsetAsync((char *)st->cnt.p + nl * 8, 0, 8, S));      // (the scan's extra element: off[n_lines] = the total)
	hipLaunchKernelGGL(k_pile_walk<false>, dim3(pile_grid(nl)), dim3(PILE_BLOCK), 0, S, d_lines, nl, st->ops.as<uint32_t>(), st->codes.as<uint8_t>(), h->ref_lane.as<uint32_t>(),
		h->ref_off.as<uint64_t>(), h->clump_len.as<uint32_t>(), st->cnt.as<pile_u64>(), (const pile_u64 *)nullptr, (uint64_t)0, (pile_u64 *)nullptr, (pile_u64 *)nullptr);
	HIPCHK(hipGetLastError());
	size_t tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(st->tmp.p, tb, st->cnt.as<pile_u64>(), st->off.as<pile_u64>(), (size_t)(nl + 1), S));
	// 3a. the starts and one-past-ends of the lines, sorted, with the running sums of their weights (independent of the events)
	hipLaunchKernelGGL(k_pile_bounds, dim3(pile_grid(nl)), dim3(PILE_BLOCK), 0, S, d_lines, st->span.as<uint32_t>(), nl, st->k_start.as<pile_u64>(), st->k_end.as<pile_u64>(),
		st->w_start.as<pile_u64>(), st->w_end.as<pile_u64>());
	HIPCHK(hipGetLastError());
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, st->k_start.as<pile_u64>(), st->k_start_s.as<pile_u64>(), st->w_start.as<pile_u64>(), st->w_start_s.as<pile_u64>(), (size_t)nl, 0, end_bit, S));
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, st->k_end.as<pile_u64>(), st->k_end_s.as<pile_u64>(), st->w_end.as<pile_u64>(), st->w_end_s.as<pile_u64>(), (size_t)nl, 0, end_bit, S));
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::InclusiveSum(st->tmp.p, tb, st->w_start_s.as<pile_u64>(), st->cs.as<pile_u64>(), (size_t)nl, S));
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::InclusiveSum(st->tmp.p, tb, st->w_end_s.as<pile_u64>(), st->ce.as<pile_u64>(), (size_t)nl, S));
	HIPCHK(hipEventRecord(st->ev1, S));
	*n_events = 0;
	HIPCHK(hipMemcpyAsync(n_events, (char *)st->off.p + nl * 8, 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	*us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	return BHIP_OK;
}

int pile_stage_cands(Handle *h, PileState *st, const PileInput &in, uint64_t ne, const char *who, pile_u64 *n_cand, uint64_t *us) {
	hipStream_t S = h->stream;
	const uint64_t nl = in.dl.size();
	const int end_bit = in.end_bit();
	int rc;
	DBuf *per_event[] = {&st->ev_key, &st->ev_val, &st->ev_key_s, &st->ev_val_s};
	for (DBuf *x : per_event) { rc = x->reserve(ne * 8); if (rc) return rc; }
	rc = st->head.reserve((ne + 1) * 8); if (rc) return rc;
	rc = st->idx.reserve((ne + 1) * 8); if (rc) return rc;
	size_t tb_sort = 0, tb_scan = 0;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, st->ev_key.as<pile_u64>(), st->ev_key_s.as<pile_u64>(), st->ev_val.as<pile_u64>(), st->ev_val_s.as<pile_u64>(), (size_t)ne, 0, end_bit, S));
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, st->head.as<pile_u64>(), st->idx.as<pile_u64>(), (size_t)(ne + 1), S));
	rc = st->tmp.reserve(std::max(tb_sort, tb_scan) + 16); if (rc) return rc;
	HIPCHK(hipEventRecord(st->ev0, S));
	hipLaunchKernelGGL(k_pile_walk<true>, dim3(pile_grid(nl)), dim3(PILE_BLOCK), 0, S, st->lines.as<PileLine>(), nl, st->ops.as<uint32_t>(), st->codes.as<uint8_t>(), h->ref_lane.as<uint32_t>(),
		h->ref_off.as<uint64_t>(), h->clump_len.as<uint32_t>(), (pile_u64 *)nullptr, st->off.as<pile_u64>(), ne, st->ev_key.as<pile_u64>(), st->ev_val.as<pile_u64>());
	HIPCHK(hipGetLastError());
	// 2. sort, open a candidate at every new key, reduce the runs (pile_launch_reduce)
	size_t tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, st->ev_key.as<pile_u64>(), st->ev_key_s.as<pile_u64>(), st->ev_val.as<pile_u64>(), st->ev_val_s.as<pile_u64>(), (size_t)ne, 0, end_bit, S));
	hipLaunchKernelGGL(k_pile_heads, dim3(pile_grid(ne + 1)), dim3(PILE_BLOCK), 0, S, st->ev_key_s.as<pile_u64>(), ne, st->head.as<pile_u64>());
	HIPCHK(hipGetLastError());
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(st->tmp.p, tb, st->head.as<pile_u64>(), st->idx.as<pile_u64>(), (size_t)(ne + 1), S));
	HIPCHK(hipEventRecord(st->ev1, S));
	*n_cand = 0;
	HIPCHK(hipMemcpyAsync(n_cand, (char *)st->idx.p + ne * 8, 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	*us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	if (*n_cand > 0x7FFFFFFFull) return fail(BHIP_E_INTERNAL, "%s: %llu candidate sites (at most 2^31 - 1 in one call)", who, *n_cand);      // (>= 1: there are events)
	return st->cand.reserve(*n_cand * sizeof(PileCand));
}

int pile_launch_reduce(Handle *h, PileState *st, uint64_t ne, uint64_t nc) {
	hipLaunchKernelGGL(k_pile_reduce, dim3(pile_grid(ne)), dim3(PILE_BLOCK), 0, h->stream, st->ev_key_s.as<pile_u64>(), st->ev_val_s.as<pile_u64>(), ne, st->head.as<pile_u64>(),
		st->idx.as<pile_u64>(), nc, st->cand.as<PileCand>());
	HIPCHK(hipGetLastError());
	return BHIP_OK;
}

extern "C" int bhip_pile_run(void *handle, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
		const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, uint32_t min_alt, BhipPileSite *sites, uint64_t cap, uint64_t *n_sites, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!h || !n_sites || (n_lines && (!lines || !q_codes || !q_off)) || (n_ops && !ops) || (cap && !sites)) return fail(BHIP_E_ARG, "bhip_pile_run: null argument");
	*n_sites = 0;
	if (!min_depth || !min_alt) return fail(BHIP_E_ARG, "bhip_pile_run: min_depth %u, min_alt %u (1 .. 2^31 - 1 each)", min_depth, min_alt);
	PileInput in;
	int rc = pile_check_lines("bhip_pile_run", h, q_codes, q_off, n_queries, lines, n_lines, ops, n_ops, in);
	if (rc) return rc;
	if (!n_lines) return BHIP_OK;      // (no sites, no launch)
	HIPCHK(hipSetDevice(h->device));
	PileState *st = nullptr;
	rc = pile_state(h, &st); if (rc) return rc;
	hipStream_t S = h->stream;
	const uint64_t nl = n_lines;
	uint64_t us = 0;
	pile_u64 n_events = 0, n_cand = 0, n_keep = 0;
	rc = pile_stage_lines(h, st, in, ops, n_ops, &n_events, &us); if (rc) return rc;
	info[0] = n_events;
	if (n_events) {
		const uint64_t ne = n_events;
		rc = pile_stage_cands(h, st, in, ne, "bhip_pile_run", &n_cand, &us); if (rc) return rc;
		const uint64_t nc = n_cand;
		rc = st->site.reserve(nc * sizeof(BhipPileSite)); if (rc) return rc;
		rc = st->out.reserve(nc * sizeof(BhipPileSite)); if (rc) return rc;
		rc = st->keep.reserve(nc + 16); if (rc) return rc;
		rc = st->n_sel.reserve(16); if (rc) return rc;
		size_t tb_sel = 0;
		HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tb_sel, st->site.as<BhipPileSite>(), st->keep.as<uint8_t>(), st->out.as<BhipPileSite>(), st->n_sel.as<pile_u64>(), (int)nc, S));
		rc = st->tmp.reserve(tb_sel + 16); if (rc) return rc;
		HIPCHK(hipEventRecord(st->ev0, S));
		rc = pile_launch_reduce(h, st, ne, nc); if (rc) return rc;
		// 3b. the stabbing count per candidate, the plain observations to count[Ref];  4. the thresholds, the selection in order
		hipLaunchKernelGGL(k_pile_finish, dim3(pile_grid(nc)), dim3(PILE_BLOCK), 0, S, st->cand.as<PileCand>(), nc, st->k_start_s.as<pile_u64>(), st->cs.as<pile_u64>(),
			st->k_end_s.as<pile_u64>(), st->ce.as<pile_u64>(), nl, min_depth, min_alt, st->site.as<BhipPileSite>(), st->keep.as<uint8_t>());
		HIPCHK(hipGetLastError());
		size_t tb = st->tmp.cap;
		HIPCHK(hipcub::DeviceSelect::Flagged(st->tmp.p, tb, st->site.as<BhipPileSite>(), st->keep.as<uint8_t>(), st->out.as<BhipPileSite>(), st->n_sel.as<pile_u64>(), (int)nc, S));
		HIPCHK(hipEventRecord(st->ev1, S));
		HIPCHK(hipMemcpyAsync(&n_keep, st->n_sel.p, 8, hipMemcpyDeviceToHost, S));
		HIPCHK(hipStreamSynchronize(S));
		us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	}
	info[1] = n_cand; info[3] = us; info[4] = st->bytes();
	*n_sites = n_keep;
	if (n_keep > cap) return fail(BHIP_E_CAPACITY, "bhip_pile_run: %llu sites, room for %llu", n_keep, (pile_u64)cap);
	if (n_keep) {
		HIPCHK(hipMemcpyAsync(sites, st->out.p, n_keep * sizeof(BhipPileSite), hipMemcpyDeviceToHost, S));
		HIPCHK(hipStreamSynchronize(S));
	}
	info[2] = n_keep;
	return BHIP_OK;
}

