// burst_amd/csrc/bhip_chimera.hip -- de-novo two-parent chimera check of reads from their FORAGE self-hits and the hits' alignment
// paths (burst_hip --chimeras; bhip_chimera_run, gfx950).  No reference counterpart: the definition is this project's own
// (include/burst_hip.h, README "Chimera check"), a pure integer function of the printed lines and their paths.
//
// The device work.
//   rank      keys ~weight << 32 | node, hipcub radix sort: order[p] = the p-th node in priority, rank[node] = p (as bhip_cluster.hip).
//   clean     a line with r == q or weight[r] < skew * weight[q] (64-bit product) gets the key of all ones and sorts behind everything;
//             the others get q << 32 | r and are sorted with the value edits << 32 | input index.  The first of every run of equal keys
//             is flagged, the flags scanned, and every line of a run takes atomicMin of its value into the run's cell: per (q, r) the
//             line with the fewest edits, the one given first among equals -- a minimum of packed keys, so no order of threads matters.
//             A binary search per node over the sorted q gives the run offsets: the kept lines of read q are pair[off[q] .. off[q + 1]).
//   profile   the hot path, k_ch_profile: ONE WAVE PER READ in a block of 64 threads.  Lanes own cuts: in a pass lane l owns the cuts
//             base + 64 t + l, t < CH_CUTS, and keeps their two running minima (L << 32 | rank, R << 32 | rank) in registers.  Per kept
//             line the wave stages the line's sorted doubled edit positions in LDS (256 x 2 bytes: at most 254 edits, positions at most
//             2 x 4095): the op words are taken 64 at a time, a wave scan of their query symbols and edits gives every word its j and its
//             place in the list, and the lane of an X, I or D word writes its positions -- those of a reverse line mirrored
//             (2 len - p) and written from the list's far end, so the list ascends again.  Each lane then takes L[c] = the positions
//             <= 2c by a binary search of the list (at most 8 steps).  After the last line the lane turns its cuts into
//             Model << 32 | c, a wave minimum of that key picks the cut (c is in the key: the smallest c among equal models, one lane
//             only holds it) and that lane writes the BhipChimera.  A read with more than 64 * CH_CUTS cuts takes further passes, which
//             stage its lines again.  O(lines x (edits + cuts / 64 x log edits)) per read, no LDS atomics.
// Index arithmetic is 64-bit wherever a line number or an offset is formed; every buffer is a grow-only one of the handle.
#include "bhip_handle.h"

#define CH_BLOCK 256
#define CH_MAX_GRID 65536u
#define CH_CUTS 4            // cuts a lane owns in one pass: 256 cuts per pass cover amplicon reads (250 .. 300 bases) in one or two
#define CH_MAX_EDITS 254u    // bhip_trace_paths' limit, and what the staged list holds

typedef unsigned long long u64;

__global__ __launch_bounds__(CH_BLOCK) void k_ch_rank_keys(const uint32_t *__restrict__ w, uint64_t n, u64 *__restrict__ key) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) key[i] = (u64)(~w[i]) << 32 | (u64)i;
}
__global__ __launch_bounds__(CH_BLOCK) void k_ch_rank(const u64 *__restrict__ key_s, uint64_t n, uint32_t *__restrict__ order, uint32_t *__restrict__ rank) {
	for (uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t node = (uint32_t)key_s[p];
		order[p] = node; rank[node] = (uint32_t)p;
	}
}
// a line that can matter: q << 32 | r; a self line or one towards a read that is no candidate parent: all ones (q <= 2^32 - 2, so no real key is that)
__global__ __launch_bounds__(CH_BLOCK) void k_ch_line_keys(const BhipChimLine *__restrict__ ln, const uint32_t *__restrict__ edits, uint64_t m, const uint32_t *__restrict__ w,
		uint32_t skew, u64 *__restrict__ key, u64 *__restrict__ val) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t q = ln[i].q, r = ln[i].r;
		key[i] = q != r && (u64)w[r] >= (u64)skew * (u64)w[q] ? (u64)q << 32 | r : ~0ull;
		val[i] = (u64)edits[i] << 32 | i;
	}
}
// sorted keys: 1 for the first of every run of equal real keys
__global__ __launch_bounds__(CH_BLOCK) void k_ch_heads(const u64 *__restrict__ key, uint64_t m, uint32_t *__restrict__ flag) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
		const u64 k = key[i];
		flag[i] = k != ~0ull && (!i || key[i - 1] != k);
	}
}
// pos = the inclusive scan of flag: line i belongs to pair pos[i] - 1; p_best was filled with ones
__global__ __launch_bounds__(CH_BLOCK) void k_ch_compact(const u64 *__restrict__ key, const u64 *__restrict__ val, const uint32_t *__restrict__ flag,
		const uint32_t *__restrict__ pos, uint64_t m, uint32_t *__restrict__ p_q, uint32_t *__restrict__ p_r, u64 *__restrict__ p_best) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
		const u64 k = key[i];
		if (k == ~0ull) continue;
		const uint64_t o = (uint64_t)pos[i] - 1;
		if (flag[i]) { p_q[o] = (uint32_t)(k >> 32); p_r[o] = (uint32_t)k; }
		atomicMin(&p_best[o], val[i]);
	}
}
// off[q] = the first pair whose read is not below q (q = 0 .. n: off[n] = kept)
__global__ __launch_bounds__(CH_BLOCK) void k_ch_offsets(const uint32_t *__restrict__ p_q, uint64_t kept, uint64_t n, u64 *__restrict__ off) {
	for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q <= n; q += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t lo = 0, hi = kept;
		while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)p_q[mid] < q) lo = mid + 1; else hi = mid; }
		off[q] = lo;
	}
}

// one wave per read (the block IS the wave: q, its lines and every trip count below are the same in all 64 lanes, so the barriers are met by all)
__global__ __launch_bounds__(64) void k_ch_profile(const u64 *__restrict__ off, const uint32_t *__restrict__ p_r, const u64 *__restrict__ p_best,
		const BhipChimLine *__restrict__ lines, const uint32_t *__restrict__ ops, const uint32_t *__restrict__ len, const uint32_t *__restrict__ rank,
		const uint32_t *__restrict__ order, uint64_t n, uint32_t min_seg, uint32_t min_gain, BhipChimera *__restrict__ out) {
	__shared__ uint16_t s_pos[256];
	const uint32_t lane = threadIdx.x;
	for (uint64_t q = blockIdx.x; q < n; q += gridDim.x) {
		const uint64_t a = off[q], b = off[q + 1];
		const uint32_t m = len[q];
		if (b - a < 2 || (u64)m < 2ull * min_seg) {      // fewer than two candidate parents with a line, or no cut: not evaluated
			if (!lane) { BhipChimera z; z.role = z.single = z.model = z.cut = z.a = z.ea = z.b = z.eb = 0; out[q] = z; }
			continue;
		}
		const uint32_t c_last = m - min_seg;      // cuts min_seg .. c_last
		u64 best_key = ~0ull, best_l = 0, best_r = 0;
		uint32_t single = ~0u;
		for (uint32_t base = min_seg; base <= c_last; base += 64 * CH_CUTS) {      // (m <= 4095: no overflow)
			u64 kl[CH_CUTS], kr[CH_CUTS];
			#pragma unroll
			for (int t = 0; t < CH_CUTS; ++t) kl[t] = kr[t] = ~0ull;
			for (uint64_t i = a; i < b; ++i) {
				const u64 pb = p_best[i];
				const uint32_t E = (uint32_t)(pb >> 32);
				const BhipChimLine ln = lines[(uint32_t)pb];
				const uint32_t rk = rank[p_r[i]];
				const bool rev = ln.flags & 1u;
				single = E < single ? E : single;
				__syncthreads();      // the searches of the line before are over
				uint32_t j_base = 0, e_base = 0;
				for (uint32_t w0 = 0; w0 < ln.n_ops; w0 += 64) {
					const uint32_t w = w0 + lane < ln.n_ops ? ops[ln.op_off + w0 + lane] : 0u;
					const uint32_t code = w & 15u, run = w >> 4;
					const uint32_t dj = code == BHIP_OP_EQ || code == BHIP_OP_X || code == BHIP_OP_I ? run : 0u;
					const uint32_t de = code == BHIP_OP_X || code == BHIP_OP_I || code == BHIP_OP_D ? run : 0u;
					uint32_t sj = dj, se = de;      // inclusive wave scans
					for (int o = 1; o < 64; o <<= 1) {
						const uint32_t tj = __shfl_up(sj, o, 64), te = __shfl_up(se, o, 64);
						if (lane >= (uint32_t)o) { sj += tj; se += te; }
					}
					const uint32_t j = j_base + sj - dj, e = e_base + se - de;
					for (uint32_t t = 0; t < de; ++t) {
						uint32_t p = code == BHIP_OP_D ? 2 * j : 2 * (j + t) + 1, k = e + t;
						if (rev) { p = 2 * m - p; k = E - 1 - k; }
						if (k < 256u) s_pos[k] = (uint16_t)p;      // (the host has checked E <= 254 and k < E; the list is never left)
					}
					j_base += __shfl(sj, 63, 64); e_base += __shfl(se, 63, 64);
				}
				__syncthreads();
				#pragma unroll
				for (int t = 0; t < CH_CUTS; ++t) {
					const uint32_t c = base + 64 * t + lane;
					if (c > c_last) continue;
					uint32_t lo = 0, hi = E < 256u ? E : 256u;      // L = the positions <= 2c
					while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint32_t)s_pos[mid] <= 2 * c) lo = mid + 1; else hi = mid; }
					const u64 l = (u64)lo << 32 | rk, r = (u64)(E - lo) << 32 | rk;
					kl[t] = l < kl[t] ? l : kl[t];
					kr[t] = r < kr[t] ? r : kr[t];
				}
			}
			#pragma unroll
			for (int t = 0; t < CH_CUTS; ++t) {
				const uint32_t c = base + 64 * t + lane;
				if (c > c_last) continue;
				const u64 key = ((kl[t] >> 32) + (kr[t] >> 32)) << 32 | c;
				if (key < best_key) { best_key = key; best_l = kl[t]; best_r = kr[t]; }
			}
		}
		u64 k = best_key;
		for (int o = 32; o; o >>= 1) { const u64 x = __shfl_xor(k, o, 64); k = x < k ? x : k; }      // (every lane of the wave is here)
		if (best_key == k) {      // one lane: c is part of the key, and lane min_seg's key is a real one
			BhipChimera res;
			res.single = single; res.model = (uint32_t)(k >> 32); res.cut = (uint32_t)k;
			res.a = order[(uint32_t)best_l]; res.ea = (uint32_t)(best_l >> 32);
			res.b = order[(uint32_t)best_r]; res.eb = (uint32_t)(best_r >> 32);
			res.role = single - res.model >= min_gain ? 2u : 1u;
			out[q] = res;
		}
	}
}

struct ChimeraState {
	DBuf w, len, lines, ops, edits, key, key_s, val, val_s, tmp, order, rank, flag, pos, p_q, p_r, p_best, off, out;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
};
#define CH_ALL_BUFS(st) {&st->w, &st->len, &st->lines, &st->ops, &st->edits, &st->key, &st->key_s, &st->val, &st->val_s, &st->tmp, &st->order, &st->rank, &st->flag, \
                         &st->pos, &st->p_q, &st->p_r, &st->p_best, &st->off, &st->out}

// (bhip_handle.h: Handle::chimera)
void bhip_chimera_release(Handle *h) {
	ChimeraState *st = (ChimeraState *)h->chimera;
	if (!st) return;
	DBuf *all[] = CH_ALL_BUFS(st);
	for (DBuf *x : all) x->release();
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->chimera = nullptr;
}

static inline uint32_t ch_grid(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + CH_BLOCK - 1) / CH_BLOCK, CH_MAX_GRID)); }

extern "C" int bhip_chimera_run(void *handle, uint32_t n_nodes, const uint32_t *weights, const uint32_t *len, const BhipChimLine *lines, uint64_t n_lines,
		const uint32_t *ops, uint64_t n_ops, uint32_t skew, uint32_t min_seg, uint32_t min_gain, BhipChimera *out) {
	Handle *h = (Handle *)handle;
	if (!h || (n_nodes && (!weights || !len || !out)) || (n_lines && !lines) || (n_ops && !ops)) return fail(BHIP_E_ARG, "bhip_chimera_run: null argument");
	if (!skew || !min_seg || !min_gain) return fail(BHIP_E_ARG, "bhip_chimera_run: skew %u, min_seg %u, min_gain %u (each at least 1)", skew, min_seg, min_gain);
	if (n_nodes == 0xFFFFFFFFu || n_lines >= (1ull << 32)) return fail(BHIP_E_ARG, "bhip_chimera_run: %u nodes and %llu lines (fewer than 2^32 - 1 nodes, fewer than 2^32 lines)", n_nodes, (unsigned long long)n_lines);
	std::vector<uint32_t> edits((size_t)n_lines);
	for (uint64_t i = 0; i < n_lines; ++i) {
		const BhipChimLine &l = lines[i];
		if (l.q >= n_nodes || l.r >= n_nodes) return fail(BHIP_E_ARG, "bhip_chimera_run: line %llu names node %u -> %u of %u", (unsigned long long)i, l.q, l.r, n_nodes);
		if (!len[l.q] || len[l.q] > BHIP_MAX_QLEN) return fail(BHIP_E_ARG, "bhip_chimera_run: line %llu: read %u has %u symbols (1 .. %d)", (unsigned long long)i, l.q, len[l.q], BHIP_MAX_QLEN);
		if (l.op_off > n_ops || l.n_ops > n_ops - l.op_off) return fail(BHIP_E_ARG, "bhip_chimera_run: line %llu: ops %llu + %u leave the %llu given", (unsigned long long)i, (unsigned long long)l.op_off, l.n_ops, (unsigned long long)n_ops);
		uint64_t used = 0, ed = 0;
		for (uint32_t k = 0; k < l.n_ops; ++k) {
			const uint32_t w = ops[l.op_off + k], code = w & 15u, run = w >> 4;
			if (!run || (code != BHIP_OP_EQ && code != BHIP_OP_X && code != BHIP_OP_I && code != BHIP_OP_D)) return fail(BHIP_E_ARG, "bhip_chimera_run: line %llu: op word %u (0x%x) is no run of I/D/=/X", (unsigned long long)i, k, w);
			if (code != BHIP_OP_D) used += run;
			if (code != BHIP_OP_EQ) ed += run;
		}
		if (used != len[l.q]) return fail(BHIP_E_ARG, "bhip_chimera_run: line %llu: its ops consume %llu symbols, read %u has %u", (unsigned long long)i, (unsigned long long)used, l.q, len[l.q]);
		if (ed > CH_MAX_EDITS) return fail(BHIP_E_ARG, "bhip_chimera_run: line %llu: %llu edits (at most %u)", (unsigned long long)i, (unsigned long long)ed, CH_MAX_EDITS);
		edits[i] = (uint32_t)ed;
	}
	memset(h->chimera_info, 0, sizeof h->chimera_info);
	h->chimera_info[5] = n_lines; h->chimera_info[6] = n_nodes;
	if (n_nodes) memset(out, 0, (size_t)n_nodes * sizeof(*out));
	if (!n_lines || !n_nodes) return BHIP_OK;      // (nothing to evaluate: every role is 0, nothing is launched)
	HIPCHK(hipSetDevice(h->device));
	ChimeraState *st = (ChimeraState *)h->chimera;
	if (!st) {
		st = new ChimeraState();
		h->chimera = st;
		if (hipEventCreate(&st->ev0) != hipSuccess || hipEventCreate(&st->ev1) != hipSuccess) { bhip_chimera_release(h); return fail(BHIP_E_DEVICE, "hipEventCreate failed"); }
	}
	const uint64_t n = n_nodes, m = n_lines, nm = std::max(n, m);
	int rc;
	#define CH_RESERVE(buf, bytes) do { rc = st->buf.reserve(bytes); if (rc) return rc; } while (0)
	CH_RESERVE(w, n * 4); CH_RESERVE(len, n * 4); CH_RESERVE(lines, m * sizeof(BhipChimLine)); CH_RESERVE(ops, std::max<uint64_t>(n_ops, 1) * 4); CH_RESERVE(edits, m * 4);
	CH_RESERVE(key, nm * 8); CH_RESERVE(key_s, nm * 8); CH_RESERVE(val, m * 8); CH_RESERVE(val_s, m * 8);
	CH_RESERVE(order, n * 4); CH_RESERVE(rank, n * 4);
	CH_RESERVE(flag, m * 4); CH_RESERVE(pos, m * 4); CH_RESERVE(p_q, m * 4); CH_RESERVE(p_r, m * 4); CH_RESERVE(p_best, m * 8);
	CH_RESERVE(off, (n + 1) * 8); CH_RESERVE(out, n * sizeof(BhipChimera));
	u64 *key = st->key.as<u64>(), *key_s = st->key_s.as<u64>(), *val = st->val.as<u64>(), *val_s = st->val_s.as<u64>(), *p_best = st->p_best.as<u64>();
	uint32_t *flag = st->flag.as<uint32_t>(), *pos = st->pos.as<uint32_t>();
	size_t tb_rank = 0, tb_sort = 0, tb_scan = 0;
	HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb_rank, key, key_s, (size_t)n, 0, 64, h->stream));
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, key, key_s, val, val_s, (size_t)m, 0, 64, h->stream));
	HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tb_scan, flag, pos, (size_t)m, h->stream));
	CH_RESERVE(tmp, std::max(tb_rank, std::max(tb_sort, tb_scan)) + 16);
	#undef CH_RESERVE
	uint32_t *order = st->order.as<uint32_t>(), *rank = st->rank.as<uint32_t>(), *p_q = st->p_q.as<uint32_t>(), *p_r = st->p_r.as<uint32_t>();
	u64 *off = st->off.as<u64>();

	HIPCHK(hipMemcpyAsync(st->w.p, weights, n * 4, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(st->len.p, len, n * 4, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(st->lines.p, lines, m * sizeof(BhipChimLine), hipMemcpyHostToDevice, h->stream));
	if (n_ops) HIPCHK(hipMemcpyAsync(st->ops.p, ops, n_ops * 4, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(st->edits.p, edits.data(), m * 4, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipEventRecord(st->ev0, h->stream));
	// rank
	hipLaunchKernelGGL(k_ch_rank_keys, dim3(ch_grid(n)), dim3(CH_BLOCK), 0, h->stream, st->w.as<uint32_t>(), n, key);
	HIPCHK(hipGetLastError());
	size_t tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortKeys(st->tmp.p, tb, key, key_s, (size_t)n, 0, 64, h->stream));
	hipLaunchKernelGGL(k_ch_rank, dim3(ch_grid(n)), dim3(CH_BLOCK), 0, h->stream, key_s, n, order, rank);
	HIPCHK(hipGetLastError());
	// clean: per (q, r) towards a candidate parent the line with the fewest edits, the run offsets
	hipLaunchKernelGGL(k_ch_line_keys, dim3(ch_grid(m)), dim3(CH_BLOCK), 0, h->stream, st->lines.as<BhipChimLine>(), st->edits.as<uint32_t>(), m, st->w.as<uint32_t>(), skew, key, val);
	HIPCHK(hipGetLastError());
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, key, key_s, val, val_s, (size_t)m, 0, 64, h->stream));
	hipLaunchKernelGGL(k_ch_heads, dim3(ch_grid(m)), dim3(CH_BLOCK), 0, h->stream, key_s, m, flag);
	HIPCHK(hipGetLastError());
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::InclusiveSum(st->tmp.p, tb, flag, pos, (size_t)m, h->stream));
	uint32_t kept32 = 0;
	HIPCHK(hipMemcpyAsync(&kept32, pos + (m - 1), 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemsetAsync(p_best, 0xFF, m * 8, h->stream));
	hipLaunchKernelGGL(k_ch_compact, dim3(ch_grid(m)), dim3(CH_BLOCK), 0, h->stream, key_s, val_s, flag, pos, m, p_q, p_r, p_best);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(h->stream));
	const uint64_t kept = kept32;
	if (kept > m) return fail(BHIP_E_INTERNAL, "bhip_chimera_run: %llu pairs out of %llu lines", (unsigned long long)kept, (unsigned long long)m);
	hipLaunchKernelGGL(k_ch_offsets, dim3(ch_grid(n + 1)), dim3(CH_BLOCK), 0, h->stream, p_q, kept, n, off);
	HIPCHK(hipGetLastError());
	// profile: one wave per read
	hipLaunchKernelGGL(k_ch_profile, dim3((uint32_t)std::min<uint64_t>(n, 1u << 20)), dim3(64), 0, h->stream, off, p_r, p_best, st->lines.as<BhipChimLine>(), st->ops.as<uint32_t>(),
	                   st->len.as<uint32_t>(), rank, order, n, min_seg, min_gain, st->out.as<BhipChimera>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(st->ev1, h->stream));
	HIPCHK(hipMemcpyAsync(out, st->out.p, n * sizeof(BhipChimera), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	uint64_t evaluated = 0, chimeric = 0, bytes = 0;
	for (uint64_t i = 0; i < n; ++i) { evaluated += out[i].role != 0; chimeric += out[i].role == 2; }
	DBuf *all[] = CH_ALL_BUFS(st);
	for (DBuf *x : all) bytes += x->cap;
	uint64_t *info = h->chimera_info;
	info[0] = kept; info[1] = evaluated; info[2] = chimeric; info[3] = (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	info[4] = bytes; info[5] = m; info[6] = n; info[7] = 0;
	return BHIP_OK;
}

extern "C" int bhip_chimera_info(void *handle, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	if (!h || !info) return fail(BHIP_E_ARG, "bhip_chimera_info: null argument");
	memcpy(info, h->chimera_info, sizeof h->chimera_info);
	return BHIP_OK;
}
