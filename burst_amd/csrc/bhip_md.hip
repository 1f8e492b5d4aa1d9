// burst_amd/csrc/bhip_md.hip -- the MD strings and NM counts of alignment paths (burst_hip --sam; bhip_md_tags, gfx950).  No reference
// counterpart: the reference prints how many edits a placement has, never which reference bases lie under them.
//
// Definition (include/burst_hip.h "MD tags"): samtools calmd's walk over the ops bhip_trace_paths returns, a match
// being an '=' op.  With counter u = 0 and 0-based lane column col = ref_first - 1: '=' of n: u += n, col += n; X of n, per column: u in
// decimal, the letter of the lane column, u = 0, col++; D of n: u, '^', the n letters, u = 0, col += n; I: nothing; at the end u, also
// when it is 0.  NM = X + I + D symbols.
//
// The MD text names the reference base under every X and D column, and the packed lanes are resident here only, next to the tracer that
// produced the ops.  The work follows the edits, never requests x read length: an '=' run costs one addition.
//   k_md_walk<false>  one thread per request walks its ops and COUNTS the bytes of its string and its NM; no lane is read
//   scan              exclusive sum of the counts (64-bit): md_off
//   k_md_walk<true>   the walk again, writing the bytes at the request's offset; the lane is read under X and D only, a dword (8 columns)
//                     kept while the columns stay inside it
// A wave per long request has not been measured and is not built.
#include "bhip_handle.h"

#define MD_BLOCK 256
#define MD_MAX_GRID 65536u

struct MdReq { unsigned long long op_off; uint32_t n_ops, refIx, ref_first, pad; };

__device__ __forceinline__ uint32_t md_digits(uint32_t v) { uint32_t d = 1; while (v >= 10u) { v /= 10u; ++d; } return d; }

// EMIT = false: cnt[i] = bytes of request i's string, nm[i] = its X + I + D.  EMIT = true: off = the exclusive scan of cnt; the bytes at their offsets
template <bool EMIT>
__global__ __launch_bounds__(MD_BLOCK) void k_md_walk(const MdReq *__restrict__ req, uint64_t n_req, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ refw,
		const uint64_t *__restrict__ ref_off, const uint32_t *__restrict__ clump_len, unsigned long long *__restrict__ cnt, uint32_t *__restrict__ nm,
		const unsigned long long *__restrict__ off, uint64_t n_bytes, char *__restrict__ md) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_req; i += (uint64_t)gridDim.x * blockDim.x) {
		const MdReq r = req[i];
		uint64_t base = 0;
		unsigned long long o = 0, end = 0;
		if (EMIT) {
			const uint32_t c = r.refIx >> 4, z = r.refIx & 15u, nchunks = (clump_len[c] + 31u) >> 5;
			base = (ref_off[c] * 16 + (uint64_t)z * nchunks) * 4;      // (the addressing of pile_ref: 8 nibbles per dword)
			o = off[i]; end = off[i + 1];
			if (end > n_bytes) continue;
		}
#define MD_PUT(ch) do { if (EMIT) { if (o < end) md[o] = (char)(ch); } ++o; } while (0)
#define MD_NUM(v) do { const uint32_t d_ = md_digits(v); if (EMIT) { uint32_t t_ = (v); for (uint32_t k_ = d_; k_ > 0; --k_) { if (o + k_ - 1 < end) md[o + k_ - 1] = (char)('0' + t_ % 10u); t_ /= 10u; } } o += d_; } while (0)
		uint32_t u = 0, col = r.ref_first - 1u, edits = 0, word_at = 0xFFFFFFFFu, word = 0;
		for (uint32_t k = 0; k < r.n_ops; ++k) {
			const uint32_t w = ops[r.op_off + k], len = w >> 4, code = w & 15u;
			if (code == BHIP_OP_EQ) { u += len; col += len; continue; }
			edits += len;
			if (code == BHIP_OP_I) continue;
			if (code == BHIP_OP_D) { MD_NUM(u); MD_PUT('^'); u = 0; }
			for (uint32_t t = 0; t < len; ++t, ++col) {
				if (code == BHIP_OP_X) { MD_NUM(u); u = 0; }
				if (EMIT) {
					if ((col >> 3) != word_at) { word_at = col >> 3; word = refw[base + word_at]; }
					MD_PUT("NACGTNKMRYSWBVHD"[(word >> (4u * (col & 7u))) & 15u]);
				} else ++o;
			}
		}
		MD_NUM(u);
#undef MD_PUT
#undef MD_NUM
		if (!EMIT) { cnt[i] = o; nm[i] = edits; }
	}
}

struct MdState {
	DBuf req, ops, cnt, off, nm, md, tmp;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	uint64_t bytes() const { return req.cap + ops.cap + cnt.cap + off.cap + nm.cap + md.cap + tmp.cap; }
};

// (bhip_handle.h: Handle::md)
void bhip_md_release(Handle *h) {
	MdState *st = (MdState *)h->md;
	if (!st) return;
	DBuf *all[] = {&st->req, &st->ops, &st->cnt, &st->off, &st->nm, &st->md, &st->tmp};
	for (DBuf *x : all) x->release();
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->md = nullptr;
}

static inline uint32_t md_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + MD_BLOCK - 1) / MD_BLOCK, MD_MAX_GRID); }

typedef unsigned long long md_u64;

extern "C" int bhip_md_tags(void *handle, const BhipPathReq *requests, const uint32_t *ref_first, const uint64_t *op_off, const uint32_t *ops, uint64_t n_requests,
		char *md, uint64_t md_cap, uint64_t *md_off, uint32_t *nm, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!h || !md_off || (n_requests && (!requests || !ref_first || !op_off || !nm)) || (md_cap && !md)) return fail(BHIP_E_ARG, "bhip_md_tags: null argument");
	md_off[0] = 0;
	if (!n_requests) return BHIP_OK;      // (no strings, no launch)
	// every request is checked on the host before the device is touched: the kernels index by these values alone
	std::vector<MdReq> dr((size_t)n_requests);
	const uint64_t first_op = op_off[0];
	for (uint64_t i = 0; i < n_requests; ++i) {
		const BhipPathReq &u = requests[i];
		if (op_off[i + 1] < op_off[i]) return fail(BHIP_E_ARG, "bhip_md_tags: request %llu: op_off descends (%llu after %llu)", (md_u64)i, (md_u64)op_off[i + 1], (md_u64)op_off[i]);
		if (!ops && op_off[i + 1] != op_off[i]) return fail(BHIP_E_ARG, "bhip_md_tags: null argument");
		if (op_off[i + 1] - op_off[i] > 0xFFFFFFFFull) return fail(BHIP_E_ARG, "bhip_md_tags: request %llu owns %llu ops", (md_u64)i, (md_u64)(op_off[i + 1] - op_off[i]));
		if (u.refIx >= 16ull * h->n_clumps || u.refIx >= h->tot_refs) return fail(BHIP_E_ARG, "bhip_md_tags: request %llu names reference %u of %u", (md_u64)i, u.refIx, h->tot_refs);
		uint64_t on_r = 0;
		for (uint64_t k = op_off[i]; k < op_off[i + 1]; ++k) {
			const uint32_t word = ops[k], len = word >> 4, code = word & 15u;
			if (!len || (code != BHIP_OP_I && code != BHIP_OP_D && code != BHIP_OP_EQ && code != BHIP_OP_X))
				return fail(BHIP_E_ARG, "bhip_md_tags: request %llu, op %llu: word 0x%x is not a run of I, D, = or X", (md_u64)i, (md_u64)(k - op_off[i]), word);
			if (code != BHIP_OP_I) on_r += len;
		}
		if (ref_first[i] < 1 || (uint64_t)ref_first[i] - 1 + on_r > h->h_clump_len[u.refIx >> 4])
			return fail(BHIP_E_ARG, "bhip_md_tags: request %llu: columns %u + %llu leave a clump of %u", (md_u64)i, ref_first[i], (md_u64)on_r, h->h_clump_len[u.refIx >> 4]);
		MdReq &d = dr[i];
		d.op_off = op_off[i] - first_op; d.n_ops = (uint32_t)(op_off[i + 1] - op_off[i]); d.refIx = u.refIx; d.ref_first = ref_first[i]; d.pad = 0;
	}
	const uint64_t nr = n_requests, n_ops = op_off[nr] - first_op;
	HIPCHK(hipSetDevice(h->device));
	MdState *st = (MdState *)h->md;
	if (!st) {
		st = new MdState();
		h->md = st;
		if (hipEventCreate(&st->ev0) != hipSuccess || hipEventCreate(&st->ev1) != hipSuccess) { bhip_md_release(h); return fail(BHIP_E_DEVICE, "hipEventCreate failed"); }
	}
	hipStream_t S = h->stream;
	int rc = st->req.reserve(nr * sizeof(MdReq)); if (rc) return rc;
	rc = st->ops.reserve(n_ops * 4 + 16); if (rc) return rc;
	rc = st->cnt.reserve((nr + 1) * 8); if (rc) return rc;
	rc = st->off.reserve((nr + 1) * 8); if (rc) return rc;
	rc = st->nm.reserve(nr * 4); if (rc) return rc;
	size_t tb_scan = 0;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, st->cnt.as<md_u64>(), st->off.as<md_u64>(), (size_t)(nr + 1), S));
	rc = st->tmp.reserve(tb_scan + 16); if (rc) return rc;
	HIPCHK(hipMemcpyAsync(st->req.p, dr.data(), nr * sizeof(MdReq), hipMemcpyHostToDevice, S));
	if (n_ops) HIPCHK(hipMemcpyAsync(st->ops.p, ops + first_op, n_ops * 4, hipMemcpyHostToDevice, S));
	HIPCHK(hipEventRecord(st->ev0, S));
	// 1. the bytes and the NM of every request: count, scan
	HIPCHK(hipMemsetAsync((char *)st->cnt.p + nr * 8, 0, 8, S));      // (the scan's extra element: off[n_requests] = the total)
	hipLaunchKernelGGL(k_md_walk<false>, dim3(md_grid(nr)), dim3(MD_BLOCK), 0, S, st->req.as<MdReq>(), nr, st->ops.as<uint32_t>(), h->ref_lane.as<uint32_t>(),
		h->ref_off.as<uint64_t>(), h->clump_len.as<uint32_t>(), st->cnt.as<md_u64>(), st->nm.as<uint32_t>(), (const md_u64 *)nullptr, (uint64_t)0, (char *)nullptr);
	HIPCHK(hipGetLastError());
	size_t tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(st->tmp.p, tb, st->cnt.as<md_u64>(), st->off.as<md_u64>(), (size_t)(nr + 1), S));
	HIPCHK(hipEventRecord(st->ev1, S));
	static_assert(sizeof(md_u64) == sizeof(uint64_t), "md_off is copied as it is");
	HIPCHK(hipMemcpyAsync(md_off, st->off.p, (nr + 1) * 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipMemcpyAsync(nm, st->nm.p, nr * 4, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	uint64_t us = (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	const uint64_t total = md_off[nr];      // (>= n_requests: every string ends in a number)
	info[0] = us; info[1] = nr; info[2] = total; info[3] = st->bytes();
	if (total > md_cap) return fail(BHIP_E_CAPACITY, "bhip_md_tags: %llu bytes, room for %llu", (md_u64)total, (md_u64)md_cap);
	// 2. the strings at their offsets
	rc = st->md.reserve(total + 16); if (rc) return rc;
	HIPCHK(hipEventRecord(st->ev0, S));
	hipLaunchKernelGGL(k_md_walk<true>, dim3(md_grid(nr)), dim3(MD_BLOCK), 0, S, st->req.as<MdReq>(), nr, st->ops.as<uint32_t>(), h->ref_lane.as<uint32_t>(),
		h->ref_off.as<uint64_t>(), h->clump_len.as<uint32_t>(), (md_u64 *)nullptr, (uint32_t *)nullptr, st->off.as<md_u64>(), total, st->md.as<char>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(st->ev1, S));
	HIPCHK(hipMemcpyAsync(md, st->md.p, total, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	info[0] = us; info[3] = st->bytes();
	return BHIP_OK;
}
