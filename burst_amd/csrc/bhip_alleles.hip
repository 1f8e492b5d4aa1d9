// burst_amd/csrc/bhip_alleles.hip -- the indel alleles of one sample from the alignment paths of its printed lines (burst_hip --vcf;
// bhip_alleles_run, gfx950).  No reference counterpart: the reference prints how many edits a placement has, never which bases a sample
// inserts or which reference columns it deletes.
//
// Definition (include/burst_hip.h "Indel alleles").  Lines, the walk (reference position p, query index j), Depth and
// the reference codes are those of the variant sites (bhip_pile.hip).  An ALLELE RUN is an I or D run whose preceding op is '=' or X and
// which is not the last op of its path; its ANCHOR is (header, p - 1), the column the preceding op consumed.  Del(n): a D allele run of n
// columns.  Ins(c1..cn): an I allele run of 1 <= n <= 15 query codes.  The count of (anchor, allele) is the summed weight of the lines that
// carry it; it is returned when Depth(anchor) >= min_depth and count >= min_alt.  A run that is the first or the last op (END), one
// directly behind the other indel kind (ADJACENT) and an I run of more than 15 symbols (LONG) give no allele and are counted.
//
// The work follows lines + allele events, never lines x read length, and never the depth of a pile-up serially.
//   pile_stage_lines    (bhip_pile.hip) upload; the starts and one-past-ends sorted with the running sums of their weights
//   k_al_walk<false>    one thread per line walks its ops and COUNTS its allele events and its three kinds of skipped runs (summed per wave,
//                       one integer atomic per wave and kind)
//   scan                exclusive sum of the counts (64-bit)
//   k_al_walk<true>     the walk again, per event: key1 = header << 32 | anchor; key2 = the allele word -- top 4 bits 0 for Del with n in the
//                       low 32 bits, or n for Ins with c1 in the next 4 bits and so on -- so that plain integer order of (key1, key2) is the
//                       defined order; value = weight | line << 32
//   sort                two stable radix passes over a permutation, by key2 then by key1, each limited to the bits in use
//   k_al_pack, reduce   hipcub ReduceByKey over the runs of equal (key1, key2): the sum of the weights and the SMALLEST line: a deep pile-up
//                       that puts tens of thousands of lines on one allele is reduced in parallel, not by one thread walking its run
//   k_al_finish         per distinct allele the STABBING COUNT of k_pile_finish for Depth(anchor), the anchor's code from the lane column of
//                       the representative line, the thresholds
//   select              hipcub flagged selection keeps the order
//   k_al_dcount, scan   the deleted columns of every kept Del: where its codes start in the code buffer
//   k_al_codes          per kept allele: the offset; for a Del the representative line is walked again to the run and its n lane columns read
// All sums are 64-bit integers and every choice is a minimum: no order of threads matters.  Lanes that share header positions agree there
// (the variants' assumption), so the codes of one carrying line stand for all.
#include "bhip_pile.h"

#define AL_MAX_INS 15u

struct AlKey {
	unsigned long long k1, k2;
	__host__ __device__ __forceinline__ bool operator==(const AlKey &o) const { return k1 == o.k1 && k2 == o.k2; }
	__host__ __device__ __forceinline__ bool operator!=(const AlKey &o) const { return !(*this == o); }
};
struct AlVal { unsigned long long count, line; };
struct AlSumMin {      // associative and commutative
	__host__ __device__ __forceinline__ AlVal operator()(const AlVal &a, const AlVal &b) const { AlVal r; r.count = a.count + b.count; r.line = b.line < a.line ? b.line : a.line; return r; }
};

__device__ __forceinline__ unsigned long long al_wave_sum(unsigned long long v) {
	for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
	return v;
}

// EMIT = false: cnt[i] = allele events of line i; skipped[0..2] += its END, ADJACENT and LONG runs.  EMIT = true: off = the exclusive scan of
// cnt; the events at their offsets
template <bool EMIT>
__global__ __launch_bounds__(PILE_BLOCK) void k_al_walk(const PileLine *__restrict__ lines, uint64_t n_lines, const uint32_t *__restrict__ ops, const uint8_t *__restrict__ codes,
		unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ skipped, const unsigned long long *__restrict__ off, uint64_t n_events,
		unsigned long long *__restrict__ key1, unsigned long long *__restrict__ key2, unsigned long long *__restrict__ val) {
	unsigned long long s_end = 0, s_adj = 0, s_long = 0;
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_lines; i += (uint64_t)gridDim.x * blockDim.x) {
		const PileLine ln = lines[i];
		const unsigned long long hkey = (unsigned long long)ln.header << 32;
		uint32_t p = ln.pos, prev = 0;
		unsigned long long j = ln.qbase, o = EMIT ? off[i] : 0ull, n_ev = 0;
		const unsigned long long end = EMIT ? off[i + 1] : 0ull;
		if (EMIT && (o == end || end > n_events)) continue;
		for (uint32_t k = 0; k < ln.n_ops; ++k) {
			const uint32_t word = ops[ln.op_off + k], len = word >> 4, code = word & 15u;
			if (code == BHIP_OP_I || code == BHIP_OP_D) {
				if (k == 0 || k + 1 == ln.n_ops) ++s_end;
				else if (prev == BHIP_OP_I || prev == BHIP_OP_D) ++s_adj;
				else if (code == BHIP_OP_I && len > AL_MAX_INS) ++s_long;
				else if (EMIT) {
					if (o < end) {
						unsigned long long a = len;      // Del(n)
						if (code == BHIP_OP_I) {
							a = (unsigned long long)len << 60;
							for (uint32_t t = 0; t < len; ++t) a |= (unsigned long long)(codes[j + t] & 15u) << (56u - 4u * t);
						}
						key1[o] = hkey | (unsigned long long)(p - 1u);      // (p - 1 >= pos: the op before consumed a column)
						key2[o] = a;
						val[o] = (unsigned long long)ln.w | (unsigned long long)i << 32;
						++o;
					}
				} else ++n_ev;
			}
			if (code != BHIP_OP_I) p += len;
			if (code != BHIP_OP_D) j += len;
			prev = code;
		}
		if (!EMIT) cnt[i] = n_ev;
	}
	if (!EMIT) {      // (every thread of the block arrives here)
		s_end = al_wave_sum(s_end); s_adj = al_wave_sum(s_adj); s_long = al_wave_sum(s_long);
		if ((threadIdx.x & 63u) == 0u) {
			if (s_end) atomicAdd(&skipped[0], s_end);
			if (s_adj) atomicAdd(&skipped[1], s_adj);
			if (s_long) atomicAdd(&skipped[2], s_long);
		}
	}
}

__global__ __launch_bounds__(PILE_BLOCK) void k_al_iota(unsigned long long *__restrict__ v, uint64_t n) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) v[i] = i;
}

// out[i] = in[perm[i]]
__global__ __launch_bounds__(PILE_BLOCK) void k_al_gather(const unsigned long long *__restrict__ in, const unsigned long long *__restrict__ perm, uint64_t n, unsigned long long *__restrict__ out) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) { const unsigned long long s = perm[i]; out[i] = s < n ? in[s] : 0ull; }
}

// the events in their final order: perm = the permutation both sorts left
__global__ __launch_bounds__(PILE_BLOCK) void k_al_pack(const unsigned long long *__restrict__ key1, const unsigned long long *__restrict__ key2, const unsigned long long *__restrict__ val,
		const unsigned long long *__restrict__ perm, uint64_t n, AlKey *__restrict__ keys, AlVal *__restrict__ vals) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const unsigned long long s = perm[i];
		AlKey k; AlVal v;
		if (s < n) { k.k1 = key1[s]; k.k2 = key2[s]; v.count = val[s] & 0xFFFFFFFFull; v.line = val[s] >> 32; }
		else { k.k1 = k.k2 = ~0ull; v.count = 0; v.line = ~0ull; }
		keys[i] = k; vals[i] = v;
	}
}

// per distinct allele: Depth(anchor), the anchor's code, the thresholds.  code_off holds the representative line until k_al_codes replaces it
__global__ __launch_bounds__(PILE_BLOCK) void k_al_finish(const AlKey *__restrict__ keys, const AlVal *__restrict__ vals, uint64_t n, const unsigned long long *__restrict__ k_start,
		const unsigned long long *__restrict__ cs, const unsigned long long *__restrict__ k_end, const unsigned long long *__restrict__ ce, uint64_t n_lines,
		const PileLine *__restrict__ lines, const uint32_t *__restrict__ span, const uint32_t *__restrict__ refw, const uint64_t *__restrict__ ref_off,
		const uint32_t *__restrict__ clump_len, uint32_t min_depth, uint32_t min_alt, BhipAllele *__restrict__ out, uint8_t *__restrict__ keep) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const AlKey k = keys[i]; const AlVal v = vals[i];
		const uint64_t a = pile_upper_bound(k_start, n_lines, k.k1), b = pile_upper_bound(k_end, n_lines, k.k1);
		const unsigned long long depth = (a ? cs[a - 1] : 0ull) - (b ? ce[b - 1] : 0ull);
		BhipAllele r;
		r.header = (uint32_t)(k.k1 >> 32); r.pos = (uint32_t)k.k1; r.allele = k.k2; r.ref = 0; r.depth = (uint32_t)depth; r.count = (uint32_t)v.count; r.pad = 0; r.code_off = v.line;
		bool ok = v.line < n_lines;
		if (ok) {
			const PileLine ln = lines[v.line];
			ok = r.pos >= ln.pos && r.pos - ln.pos < span[v.line];      // (the carrying line observes the anchor: its columns were checked on the host)
			if (ok) {
				const uint32_t c = ln.refIx >> 4, z = ln.refIx & 15u, nchunks = (clump_len[c] + 31u) >> 5;
				const uint64_t base = (ref_off[c] * 16 + (uint64_t)z * nchunks) * 4;
				r.ref = pile_ref(refw, base, ln.ref_first - 1u + (r.pos - ln.pos));
			}
		}
		out[i] = r;
		keep[i] = (ok && depth >= min_depth && v.count >= min_alt) ? 1 : 0;
	}
}

// dc[i] = the columns kept allele i deletes; (dc[n] = 0: the scan's extra element holds the total)
__global__ __launch_bounds__(PILE_BLOCK) void k_al_dcount(const BhipAllele *__restrict__ al, uint64_t n, unsigned long long *__restrict__ dc) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x)
		dc[i] = (i < n && (al[i].allele >> 60) == 0ull) ? (al[i].allele & 0xFFFFFFFFull) : 0ull;
}

// doff = the exclusive scan of dc.  Per kept allele: its offset; for a Del the representative line walked to the run, the lane columns read
__global__ __launch_bounds__(PILE_BLOCK) void k_al_codes(BhipAllele *__restrict__ al, uint64_t n, const unsigned long long *__restrict__ doff, uint64_t n_codes,
		const PileLine *__restrict__ lines, uint64_t n_lines, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ refw, const uint64_t *__restrict__ ref_off,
		const uint32_t *__restrict__ clump_len, uint8_t *__restrict__ codes) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const BhipAllele r = al[i];
		const unsigned long long line = r.code_off, o = doff[i], nd = doff[i + 1] - o;
		al[i].code_off = o;
		if ((r.allele >> 60) != 0ull || line >= n_lines || o + nd > n_codes) continue;
		const PileLine ln = lines[line];
		const uint32_t c = ln.refIx >> 4, z = ln.refIx & 15u, nchunks = (clump_len[c] + 31u) >> 5;
		const uint64_t base = (ref_off[c] * 16 + (uint64_t)z * nchunks) * 4;
		uint32_t p = ln.pos, col = ln.ref_first - 1u;
		for (uint32_t k = 0; k < ln.n_ops; ++k) {
			const uint32_t word = ops[ln.op_off + k], len = word >> 4, code = word & 15u;
			if (code == BHIP_OP_I) continue;
			if (code == BHIP_OP_D && k > 0 && p - 1u == r.pos) {      // (positions ascend strictly over '=', X and D: one run starts behind the anchor)
				for (uint32_t t = 0; t < len && t < nd; ++t) codes[o + t] = (uint8_t)pile_ref(refw, base, col + t);
				break;
			}
			p += len; col += len;
			if (p - 1u > r.pos) break;
		}
	}
}

struct AlState {
	DBuf cnt, off, skipped, key1, key2, val, iota, k2s, perm1, k1g, k1s, perm2, keys, vals, ukeys, uvals, n_runs, cand, keep, out, n_sel, dc, doff, codes, tmp;
	uint64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	void each(void (*f)(DBuf *, void *), void *u) {
		DBuf *all[] = {&cnt, &off, &skipped, &key1, &key2, &val, &iota, &k2s, &perm1, &k1g, &k1s, &perm2, &keys, &vals, &ukeys, &uvals, &n_runs, &cand, &keep, &out, &n_sel, &dc, &doff, &codes, &tmp};
		for (DBuf *x : all) f(x, u);
	}
	uint64_t bytes() { uint64_t b = 0; each([](DBuf *x, void *u) { *(uint64_t *)u += x->cap; }, &b); return b; }
};

// (bhip_handle.h: Handle::alleles)
void bhip_alleles_release(Handle *h) {
	AlState *al = (AlState *)h->alleles;
	if (!al) return;
	al->each([](DBuf *x, void *) { x->release(); }, nullptr);
	delete al;
	h->alleles = nullptr;
}

extern "C" int bhip_alleles_info(void *handle, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	if (!h || !info) return fail(BHIP_E_ARG, "bhip_alleles_info: null argument");
	if (h->alleles) memcpy(info, ((AlState *)h->alleles)->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t));
	return BHIP_OK;
}

extern "C" int bhip_alleles_run(void *handle, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
		const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, uint32_t min_alt, BhipAllele *alleles, uint64_t cap, uint64_t *n_alleles,
		uint8_t *codes, uint64_t code_cap, uint64_t *n_codes, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!h || !n_alleles || !n_codes || (n_lines && (!lines || !q_codes || !q_off)) || (n_ops && !ops) || (cap && !alleles) || (code_cap && !codes))
		return fail(BHIP_E_ARG, "bhip_alleles_run: null argument");
	*n_alleles = *n_codes = 0;
	if (h->alleles) memset(((AlState *)h->alleles)->info, 0, 8 * sizeof(uint64_t));
	if (!min_depth || min_depth > 0x7FFFFFFFu || !min_alt || min_alt > 0x7FFFFFFFu) return fail(BHIP_E_ARG, "bhip_alleles_run: min_depth %u, min_alt %u (1 .. 2^31 - 1 each)", min_depth, min_alt);
	PileInput in;
	int rc = pile_check_lines("bhip_alleles_run", h, q_codes, q_off, n_queries, lines, n_lines, ops, n_ops, in);
	if (rc) return rc;
	if (!n_lines) return BHIP_OK;      // (no alleles, no launch)
	// the bits of the allele words in use: a Del holds n in its low bits, an Ins of n symbols the bits from 60 - 4 n up
	uint32_t max_del = 0, max_ins = 0;
	for (uint64_t i = 0; i < n_lines; ++i) for (uint32_t k = 0; k < lines[i].n_ops; ++k) {
		const uint32_t word = ops[lines[i].op_off + k], len = word >> 4, code = word & 15u;
		if (code == BHIP_OP_D) max_del = std::max(max_del, len);
		else if (code == BHIP_OP_I && len <= AL_MAX_INS) max_ins = std::max(max_ins, len);
	}
	int k2_begin = max_del ? 0 : 60 - 4 * (int)max_ins, k2_end = max_ins ? 64 : std::max(1, pile_bits(max_del));
	if (k2_begin >= k2_end) { k2_begin = 0; k2_end = 64; }      // (no indel run at all: there will be no event to sort)
	HIPCHK(hipSetDevice(h->device));
	PileState *st = nullptr;
	rc = pile_state(h, &st); if (rc) return rc;
	AlState *al = (AlState *)h->alleles;
	if (!al) { al = new AlState(); h->alleles = al; }
	hipStream_t S = h->stream;
	const uint64_t nl = n_lines;
	const int end_bit = in.end_bit();
	uint64_t us = 0;
	pile_u64 pile_events = 0;
	// 0. upload; the sorted starts and one-past-ends with their running weights
	rc = pile_stage_lines(h, st, in, ops, n_ops, &pile_events, &us); if (rc) return rc;
	// 1. the allele events and the skipped runs of every line: count, scan
	rc = al->cnt.reserve((nl + 1) * 8); if (rc) return rc;
	rc = al->off.reserve((nl + 1) * 8); if (rc) return rc;
	rc = al->skipped.reserve(32); if (rc) return rc;
	size_t tb_scan = 0;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, al->cnt.as<pile_u64>(), al->off.as<pile_u64>(), (size_t)(nl + 1), S));
	rc = al->tmp.reserve(tb_scan + 16); if (rc) return rc;
	HIPCHK(hipEventRecord(st->ev0, S));
	HIPCHK(hipMemsetAsync((char *)al->cnt.p + nl * 8, 0, 8, S));      // (the scan's extra element: off[n_lines] = the total)
	HIPCHK(hipMemsetAsync(al->skipped.p, 0, 32, S));
	hipLaunchKernelGGL(k_al_walk<false>, dim3(pile_grid(nl)), dim3(PILE_BLOCK), 0, S, st->lines.as<PileLine>(), nl, st->ops.as<uint32_t>(), st->codes.as<uint8_t>(),
		al->cnt.as<pile_u64>(), al->skipped.as<pile_u64>(), (const pile_u64 *)nullptr, (uint64_t)0, (pile_u64 *)nullptr, (pile_u64 *)nullptr, (pile_u64 *)nullptr);
	HIPCHK(hipGetLastError());
	size_t tb = al->tmp.cap;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(al->tmp.p, tb, al->cnt.as<pile_u64>(), al->off.as<pile_u64>(), (size_t)(nl + 1), S));
	HIPCHK(hipEventRecord(st->ev1, S));
	pile_u64 n_events = 0, skipped[4] = {0, 0, 0, 0};
	HIPCHK(hipMemcpyAsync(&n_events, (char *)al->off.p + nl * 8, 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipMemcpyAsync(skipped, al->skipped.p, 32, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	info[0] = n_events; info[3] = skipped[0]; info[4] = skipped[1]; info[5] = skipped[2];
	pile_u64 n_distinct = 0, n_keep = 0, total_codes = 0;
	if (n_events) {
		if (n_events > 0x7FFFFFFFull) return fail(BHIP_E_ARG, "bhip_alleles_run: %llu allele events (at most 2^31 - 1 in one call)", n_events);
		const uint64_t ne = n_events;
		// 2. + 3. emit; two stable passes over a permutation, by the allele word, then by the anchor
		DBuf *per_event[] = {&al->key1, &al->key2, &al->val, &al->iota, &al->k2s, &al->perm1, &al->k1g, &al->k1s, &al->perm2};
		for (DBuf *x : per_event) { rc = x->reserve(ne * 8); if (rc) return rc; }
		DBuf *per_pair[] = {&al->keys, &al->vals, &al->ukeys, &al->uvals};
		for (DBuf *x : per_pair) { rc = x->reserve(ne * 16); if (rc) return rc; }
		rc = al->n_runs.reserve(16); if (rc) return rc;
		size_t tb_s2 = 0, tb_s1 = 0, tb_red = 0;
		HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_s2, al->key2.as<pile_u64>(), al->k2s.as<pile_u64>(), al->iota.as<pile_u64>(), al->perm1.as<pile_u64>(), (size_t)ne, k2_begin, k2_end, S));
		HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_s1, al->k1g.as<pile_u64>(), al->k1s.as<pile_u64>(), al->perm1.as<pile_u64>(), al->perm2.as<pile_u64>(), (size_t)ne, 0, end_bit, S));
		HIPCHK(hipcub::DeviceReduce::ReduceByKey(nullptr, tb_red, al->keys.as<AlKey>(), al->ukeys.as<AlKey>(), al->vals.as<AlVal>(), al->uvals.as<AlVal>(), al->n_runs.as<pile_u64>(), AlSumMin(), (int)ne, S));
		rc = al->tmp.reserve(std::max(tb_s2, std::max(tb_s1, tb_red)) + 16); if (rc) return rc;
		HIPCHK(hipEventRecord(st->ev0, S));
		hipLaunchKernelGGL(k_al_walk<true>, dim3(pile_grid(nl)), dim3(PILE_BLOCK), 0, S, st->lines.as<PileLine>(), nl, st->ops.as<uint32_t>(), st->codes.as<uint8_t>(),
			(pile_u64 *)nullptr, (pile_u64 *)nullptr, al->off.as<pile_u64>(), ne, al->key1.as<pile_u64>(), al->key2.as<pile_u64>(), al->val.as<pile_u64>());
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_al_iota, dim3(pile_grid(ne)), dim3(PILE_BLOCK), 0, S, al->iota.as<pile_u64>(), ne);
		HIPCHK(hipGetLastError());
		tb = al->tmp.cap;
		HIPCHK(hipcub::DeviceRadixSort::SortPairs(al->tmp.p, tb, al->key2.as<pile_u64>(), al->k2s.as<pile_u64>(), al->iota.as<pile_u64>(), al->perm1.as<pile_u64>(), (size_t)ne, k2_begin, k2_end, S));
		hipLaunchKernelGGL(k_al_gather, dim3(pile_grid(ne)), dim3(PILE_BLOCK), 0, S, al->key1.as<pile_u64>(), al->perm1.as<pile_u64>(), ne, al->k1g.as<pile_u64>());
		HIPCHK(hipGetLastError());
		tb = al->tmp.cap;
		HIPCHK(hipcub::DeviceRadixSort::SortPairs(al->tmp.p, tb, al->k1g.as<pile_u64>(), al->k1s.as<pile_u64>(), al->perm1.as<pile_u64>(), al->perm2.as<pile_u64>(), (size_t)ne, 0, end_bit, S));
		// 4. the runs of equal (anchor, allele) reduced to their count and their smallest line
		hipLaunchKernelGGL(k_al_pack, dim3(pile_grid(ne)), dim3(PILE_BLOCK), 0, S, al->key1.as<pile_u64>(), al->key2.as<pile_u64>(), al->val.as<pile_u64>(), al->perm2.as<pile_u64>(), ne,
			al->keys.as<AlKey>(), al->vals.as<AlVal>());
		HIPCHK(hipGetLastError());
		tb = al->tmp.cap;
		HIPCHK(hipcub::DeviceReduce::ReduceByKey(al->tmp.p, tb, al->keys.as<AlKey>(), al->ukeys.as<AlKey>(), al->vals.as<AlVal>(), al->uvals.as<AlVal>(), al->n_runs.as<pile_u64>(), AlSumMin(), (int)ne, S));
		HIPCHK(hipEventRecord(st->ev1, S));
		HIPCHK(hipMemcpyAsync(&n_distinct, al->n_runs.p, 8, hipMemcpyDeviceToHost, S));
		HIPCHK(hipStreamSynchronize(S));
		us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
		if (!n_distinct || n_distinct > ne) return fail(BHIP_E_INTERNAL, "bhip_alleles_run: %llu distinct alleles of %llu events", n_distinct, n_events);
		const uint64_t nd = n_distinct;
		// 5. depth, anchor code, thresholds;  6. the selection in order
		rc = al->cand.reserve(nd * sizeof(BhipAllele)); if (rc) return rc;
		rc = al->out.reserve(nd * sizeof(BhipAllele)); if (rc) return rc;
		rc = al->keep.reserve(nd + 16); if (rc) return rc;
		rc = al->n_sel.reserve(16); if (rc) return rc;
		size_t tb_sel = 0;
		HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tb_sel, al->cand.as<BhipAllele>(), al->keep.as<uint8_t>(), al->out.as<BhipAllele>(), al->n_sel.as<pile_u64>(), (int)nd, S));
		rc = al->tmp.reserve(tb_sel + 16); if (rc) return rc;
		HIPCHK(hipEventRecord(st->ev0, S));
		hipLaunchKernelGGL(k_al_finish, dim3(pile_grid(nd)), dim3(PILE_BLOCK), 0, S, al->ukeys.as<AlKey>(), al->uvals.as<AlVal>(), nd, st->k_start_s.as<pile_u64>(), st->cs.as<pile_u64>(),
			st->k_end_s.as<pile_u64>(), st->ce.as<pile_u64>(), nl, st->lines.as<PileLine>(), st->span.as<uint32_t>(), h->ref_lane.as<uint32_t>(), h->ref_off.as<uint64_t>(),
			h->clump_len.as<uint32_t>(), min_depth, min_alt, al->cand.as<BhipAllele>(), al->keep.as<uint8_t>());
		HIPCHK(hipGetLastError());
		tb = al->tmp.cap;
		HIPCHK(hipcub::DeviceSelect::Flagged(al->tmp.p, tb, al->cand.as<BhipAllele>(), al->keep.as<uint8_t>(), al->out.as<BhipAllele>(), al->n_sel.as<pile_u64>(), (int)nd, S));
		HIPCHK(hipEventRecord(st->ev1, S));
		HIPCHK(hipMemcpyAsync(&n_keep, al->n_sel.p, 8, hipMemcpyDeviceToHost, S));
		HIPCHK(hipStreamSynchronize(S));
		us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
		if (n_keep > nd) return fail(BHIP_E_INTERNAL, "bhip_alleles_run: %llu alleles kept of %llu", n_keep, n_distinct);
		if (n_keep) {      // where the deleted columns of every kept Del start
			const uint64_t nk = n_keep;
			rc = al->dc.reserve((nk + 1) * 8); if (rc) return rc;
			rc = al->doff.reserve((nk + 1) * 8); if (rc) return rc;
			tb_scan = 0;
			HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, al->dc.as<pile_u64>(), al->doff.as<pile_u64>(), (size_t)(nk + 1), S));
			rc = al->tmp.reserve(tb_scan + 16); if (rc) return rc;
			HIPCHK(hipEventRecord(st->ev0, S));
			hipLaunchKernelGGL(k_al_dcount, dim3(pile_grid(nk + 1)), dim3(PILE_BLOCK), 0, S, al->out.as<BhipAllele>(), nk, al->dc.as<pile_u64>());
			HIPCHK(hipGetLastError());
			tb = al->tmp.cap;
			HIPCHK(hipcub::DeviceScan::ExclusiveSum(al->tmp.p, tb, al->dc.as<pile_u64>(), al->doff.as<pile_u64>(), (size_t)(nk + 1), S));
			HIPCHK(hipEventRecord(st->ev1, S));
			HIPCHK(hipMemcpyAsync(&total_codes, (char *)al->doff.p + nk * 8, 8, hipMemcpyDeviceToHost, S));
			HIPCHK(hipStreamSynchronize(S));
			us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
		}
	}
	info[1] = n_distinct; info[6] = us; info[7] = st->bytes() + al->bytes();
	*n_alleles = n_keep; *n_codes = total_codes;
	if (n_keep > cap || total_codes > code_cap) {
		memcpy(al->info, info, sizeof al->info);
		return fail(BHIP_E_CAPACITY, "bhip_alleles_run: %llu alleles and %llu deleted codes, room for %llu and %llu", n_keep, total_codes, (pile_u64)cap, (pile_u64)code_cap);
	}
	if (n_keep) {
		const uint64_t nk = n_keep;
		rc = al->codes.reserve(total_codes + 16); if (rc) return rc;
		HIPCHK(hipEventRecord(st->ev0, S));
		hipLaunchKernelGGL(k_al_codes, dim3(pile_grid(nk)), dim3(PILE_BLOCK), 0, S, al->out.as<BhipAllele>(), nk, al->doff.as<pile_u64>(), (uint64_t)total_codes, st->lines.as<PileLine>(), nl,
			st->ops.as<uint32_t>(), h->ref_lane.as<uint32_t>(), h->ref_off.as<uint64_t>(), h->clump_len.as<uint32_t>(), al->codes.as<uint8_t>());
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(st->ev1, S));
		HIPCHK(hipMemcpyAsync(alleles, al->out.p, nk * sizeof(BhipAllele), hipMemcpyDeviceToHost, S));
		if (total_codes) HIPCHK(hipMemcpyAsync(codes, al->codes.p, total_codes, hipMemcpyDeviceToHost, S));
		HIPCHK(hipStreamSynchronize(S));
		us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	}
	info[2] = n_keep; info[6] = us; info[7] = st->bytes() + al->bytes();
	memcpy(al->info, info, sizeof al->info);
	return BHIP_OK;
}
