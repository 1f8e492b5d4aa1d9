// burst_amd/csrc/bhip_em.hip -- abundance: the reads of multi-mapped lines split over their references by expectation-maximisation
// (burst_hip --abundance; bhip_em_run, gfx950).  No reference counterpart: the reference's README leaves "EM interpolation" of ALLPATHS
// output to its users, and its COMMUNIST mode ("min. ref. set, taxa interpolation, and fair redistribution") is a stub.
//
// Definition (include/burst_hip.h).  ONE = 2^30.  A group g has W_g reads and a candidate set S_g, the distinct
// headers among its lines.  c0[h] = ONE; per iteration every group hands out exactly ONE per read: q_h = floor((double)c[h] / (double)d
// * 2^30) to each candidate, d the integer sum of c over the set, and the rest ONE - sum q to the candidate with the largest c (lowest
// header among equals).  Everything but that one IEEE division is 64-bit integer addition, so the order in which classes, waves and
// atomics arrive cannot change a bit of the result.
//
// The device work.
//   pairs     keys group << 32 | ref (a line of a group without reads gets the group number n_groups, one past the last, and sorts behind
//             everything), hipcub radix sort over the bits that can be set, flag the first of every run of equal keys, select: the
//             distinct pairs, headers ascending inside a group.  The first pair of every group starts a SEGMENT = one candidate set.
//   classes   per segment a 64-bit hash of (size, headers); the segments sorted by it; ONE WAVE PER NEIGHBOUR PAIR compares size and
//             headers element by element, and only segments proven equal merge (scan of the run heads = class numbers, weights summed
//             per class).  A hash collision can only keep two equal sets apart -- one class more, no other count.  Option em_weak_hash
//             cuts the hash to two bits so that the comparison decides (tests).
//   base      a class of ONE candidate gives W x ONE to it in every iteration: added once into base[h]; every iteration starts from a copy.
//   steps     the classes with more candidates, in three lists by set size (order inside a list: as the atomics fell, irrelevant):
//             k_em_step_thread one thread per class, k_em_step_wave one wave per class (lanes stride the set; shuffles reduce d, the
//             argmax and sum q), k_em_step_block one block per class.  c(t-1) is read-only, ct gets 64-bit atomicAdd in global memory.
//   delta     k_em_delta: max |ct - c(t-1)| by atomicMax into the iteration's cell, and in the same pass c(t-1)'s buffer becomes the
//             copy of base the NEXT iteration adds into: two buffers swap roles.
//   stopping  iterations are enqueued EM_POLL at a time; every kernel of an iteration first reads the cell of the iteration before it
//             (complete: the kernel boundary orders it) and returns at once when that delta is <= tol -- a skipped iteration leaves its
//             own cell 0, so everything behind it skips too.  The host reads the cells once per chunk: the first one <= tol is the
//             iteration whose counts are returned, and its buffer has not been touched since.  No graph: a stream of plain launches.
#include "bhip_handle.h"

#define EM_BLOCK 256
#define EM_MAX_GRID 8192u
#define EM_POLL 8            // iterations enqueued between two reads of the delta cells
// Largest set a thread / a wave takes (options em_thread_max, em_wave_max; 0 = these).  Measured on an MI355X, microseconds per iteration
// (step kernels + k_em_delta) with EVERY class on one path, 100 000 random sets of one size on 65 536 headers beside as many single-candidate
// groups (profiles/abundance_thresholds.json):
//   set size        3     4     8    12    16    28    48          set size      256   1024   2048   4096  16384  65536
//   thread       33.2  46.9  49.2  70.1  89.7 147.6 240.2          wave        222.3  242.1  250.0  278.4  527.8 1468.8
//   wave         71.6  71.7  71.7  81.7  98.1 144.3 224.9          block       224.7  243.6  235.8  229.2  284.4  480.8
// A thread's serial walk wins up to 16 candidates and ties at 28; a block's four waves win from 2 048 and tie at 1 024 and below.
#define EM_THREAD_MAX 16
#define EM_WAVE_MAX 1024
#define EM_ONE (1ull << 30)

typedef unsigned long long u64;
struct EmClass { uint32_t start, size, w; };

__device__ __forceinline__ u64 em_wave_sum(u64 v) { for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
__device__ __forceinline__ u64 em_wave_max(u64 v) { for (int o = 32; o; o >>= 1) { const u64 x = __shfl_xor(v, o, 64); v = x > v ? x : v; } return v; }
// the candidate with the largest count, the lowest header among equals (a lane without a candidate holds (0, 0xFFFFFFFF): every real one beats it)
__device__ __forceinline__ void em_top_merge(u64 &c, uint32_t &h, u64 oc, uint32_t oh) { if (oc > c || (oc == c && oh < h)) { c = oc; h = oh; } }
__device__ __forceinline__ void em_wave_top(u64 &c, uint32_t &h) {
	for (int o = 32; o; o >>= 1) { const u64 oc = __shfl_xor(c, o, 64); const uint32_t oh = __shfl_xor(h, o, 64); em_top_merge(c, h, oc, oh); }
}
// the one floating-point step: u64 -> f64 conversions round to nearest, the division is IEEE, the scale is a power of two
__device__ __forceinline__ u64 em_share(u64 c, u64 d) { return (u64)(((double)c / (double)d) * 1073741824.0); }
__device__ __forceinline__ u64 em_mix(u64 x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x; }

// one thread per line: its key; a line outside the tables is counted (bad[0] group, bad[1] ref) and, like a line of a group without reads, sorts last
__global__ __launch_bounds__(EM_BLOCK) void k_em_keys(const BhipEmLine *__restrict__ ln, uint64_t n, const uint32_t *__restrict__ gw, uint32_t n_groups, uint32_t n_headers,
		u64 *__restrict__ key, u64 *__restrict__ bad) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const BhipEmLine l = ln[i];
		uint32_t g = l.group;
		if (g >= n_groups) { atomicAdd(&bad[0], 1ull); g = n_groups; }
		else if (l.ref >= n_headers) { atomicAdd(&bad[1], 1ull); g = n_groups; }
		else if (!gw[g]) g = n_groups;
		key[i] = (u64)g << 32 | (g == n_groups ? 0u : l.ref);
	}
}
// sorted keys: 1 for the first of every run of equal keys that belongs to a participating group
__global__ __launch_bounds__(EM_BLOCK) void k_em_first(const u64 *__restrict__ key, uint64_t n, uint32_t n_groups, uint8_t *__restrict__ flag) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const u64 k = key[i];
		flag[i] = (uint32_t)(k >> 32) != n_groups && (!i || key[i - 1] != k);
	}
}
// distinct pairs: the header of each, and 1 where a group's segment starts
__global__ __launch_bounds__(EM_BLOCK) void k_em_segflag(const u64 *__restrict__ pk, uint64_t n, uint32_t *__restrict__ ref, uint8_t *__restrict__ flag) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const u64 k = pk[i];
		ref[i] = (uint32_t)k;
		flag[i] = !i || (pk[i - 1] >> 32) != (k >> 32);
	}
}
// one thread per segment: size, reads, sort key (hash of size and headers; two bits of it with the weak hash); the reads of all segments summed
__global__ __launch_bounds__(EM_BLOCK) void k_em_segments(const u64 *__restrict__ pk, const uint32_t *__restrict__ seg_start, uint32_t n_seg, uint32_t n_pairs,
		const uint32_t *__restrict__ gw, u64 hash_mask, uint32_t *__restrict__ seg_size, uint32_t *__restrict__ seg_w, u64 *__restrict__ skey, uint32_t *__restrict__ sidx,
		u64 *__restrict__ total_w) {
	u64 wsum = 0;
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_seg; s += gridDim.x * blockDim.x) {
		const uint32_t a = seg_start[s], b = s + 1 < n_seg ? seg_start[s + 1] : n_pairs;
		const uint32_t w = gw[(uint32_t)(pk[a] >> 32)];
		u64 hsh = em_mix((u64)(b - a));
		for (uint32_t i = a; i < b; ++i) hsh = em_mix(hsh ^ (u64)(uint32_t)pk[i]);
		seg_size[s] = b - a; seg_w[s] = w; skey[s] = hsh & hash_mask; sidx[s] = s;
		wsum += w;
	}
	wsum = em_wave_sum(wsum);      // (every lane of the wave is here: the loop has ended for all of them)
	if (!(threadIdx.x & 63) && wsum) atomicAdd(total_w, wsum);
}
// one wave per sorted position j: head[j] = 0 only when segment j and segment j - 1 are PROVEN the same set (key, size, every header)
__global__ __launch_bounds__(EM_BLOCK) void k_em_same(const u64 *__restrict__ skey, const uint32_t *__restrict__ sidx, uint32_t n_seg, const uint32_t *__restrict__ seg_start,
		const uint32_t *__restrict__ seg_size, const uint32_t *__restrict__ ref, uint32_t *__restrict__ head) {
	const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * (EM_BLOCK / 64);
	for (uint32_t j = blockIdx.x * (EM_BLOCK / 64) + (threadIdx.x >> 6); j < n_seg; j += waves) {
		bool same = j > 0 && skey[j] == skey[j - 1];      // (wave-uniform)
		if (same) {
			const uint32_t s = sidx[j], p = sidx[j - 1], n = seg_size[s];
			same = n == seg_size[p];
			if (same) {
				const uint32_t *x = ref + seg_start[s], *y = ref + seg_start[p];
				bool eq = true;
				for (uint32_t i = lane; i < n; i += 64) eq &= x[i] == y[i];
				same = __all(eq);
			}
		}
		if (!lane) head[j] = same ? 0u : 1u;
	}
}
// cid = inclusive scan of head (class number + 1): the class's reads summed, its first segment noted as the one that describes it
__global__ __launch_bounds__(EM_BLOCK) void k_em_class_w(const uint32_t *__restrict__ cid, const uint32_t *__restrict__ head, const uint32_t *__restrict__ sidx, uint32_t n_seg,
		const uint32_t *__restrict__ seg_w, uint32_t *__restrict__ cls_w, uint32_t *__restrict__ cls_rep) {
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_seg; j += gridDim.x * blockDim.x) {
		const uint32_t c = cid[j] - 1, s = sidx[j];
		atomicAdd(&cls_w[c], seg_w[s]);      // (the sum of all of them is at most 2^31 - 1, checked before anything reads this)
		if (head[j]) cls_rep[c] = s;
	}
}
// one thread per class: a single candidate goes into base once and for all, the others into the list of their set size
__global__ __launch_bounds__(EM_BLOCK) void k_em_classify(const uint32_t *__restrict__ cls_w, const uint32_t *__restrict__ cls_rep, uint32_t n_cls, const uint32_t *__restrict__ seg_start,
		const uint32_t *__restrict__ seg_size, const uint32_t *__restrict__ ref, uint32_t thread_max, uint32_t wave_max, u64 *__restrict__ base,
		EmClass *__restrict__ list /* [3][n_cls] */, uint32_t *__restrict__ cnt /* [3] */) {
	for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cls; c += gridDim.x * blockDim.x) {
		const uint32_t s = cls_rep[c];
		const EmClass k = {seg_start[s], seg_size[s], cls_w[c]};
		if (k.size == 1) { atomicAdd(&base[ref[k.start]], (u64)k.w << 30); continue; }
		const uint32_t kind = k.size <= thread_max ? 0u : k.size <= wave_max ? 1u : 2u;
		list[(uint64_t)kind * n_cls + atomicAdd(&cnt[kind], 1u)] = k;
	}
}
__global__ __launch_bounds__(EM_BLOCK) void k_em_fill(u64 *__restrict__ a, u64 v, u64 *__restrict__ b, const u64 *__restrict__ src, uint32_t n) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { a[i] = v; b[i] = src[i]; }
}

// ---- the step: c = counts of the iteration before (read-only), out = this iteration's (preset to base) ----
#define EM_SKIP(prev_cell, tol) if ((prev_cell) && *(prev_cell) <= (tol)) return      /* (the same answer in every thread of the grid) */

__global__ __launch_bounds__(EM_BLOCK) void k_em_step_thread(const EmClass *__restrict__ cls, uint32_t n, const uint32_t *__restrict__ ref, const u64 *__restrict__ c,
		u64 *__restrict__ out, const u64 *__restrict__ prev_cell, u64 tol) {
	EM_SKIP(prev_cell, tol);
	for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
		const EmClass K = cls[k];
		const uint32_t *r = ref + K.start;
		u64 d = 0, tc = 0; uint32_t th = 0xFFFFFFFFu;
		for (uint32_t i = 0; i < K.size; ++i) { const uint32_t h = r[i]; const u64 v = c[h]; d += v; em_top_merge(tc, th, v, h); }
		u64 sq = 0;
		for (uint32_t i = 0; i < K.size; ++i) {
			const uint32_t h = r[i];
			const u64 q = em_share(c[h], d);
			sq += q;
			if (q) atomicAdd(&out[h], (u64)K.w * q);
		}
		if (EM_ONE - sq) atomicAdd(&out[th], (u64)K.w * (EM_ONE - sq));
	}
}
__global__ __launch_bounds__(EM_BLOCK) void k_em_step_wave(const EmClass *__restrict__ cls, uint32_t n, const uint32_t *__restrict__ ref, const u64 *__restrict__ c,
		u64 *__restrict__ out, const u64 *__restrict__ prev_cell, u64 tol) {
	EM_SKIP(prev_cell, tol);
	const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * (EM_BLOCK / 64);
	for (uint32_t k = blockIdx.x * (EM_BLOCK / 64) + (threadIdx.x >> 6); k < n; k += waves) {
		const EmClass K = cls[k];
		const uint32_t *r = ref + K.start;
		u64 d = 0, tc = 0; uint32_t th = 0xFFFFFFFFu;
		for (uint32_t i = lane; i < K.size; i += 64) { const uint32_t h = r[i]; const u64 v = c[h]; d += v; em_top_merge(tc, th, v, h); }
		d = em_wave_sum(d); em_wave_top(tc, th);
		u64 sq = 0;
		for (uint32_t i = lane; i < K.size; i += 64) {
			const uint32_t h = r[i];
			const u64 q = em_share(c[h], d);
			sq += q;
			if (q) atomicAdd(&out[h], (u64)K.w * q);
		}
		sq = em_wave_sum(sq);
		if (!lane && EM_ONE - sq) atomicAdd(&out[th], (u64)K.w * (EM_ONE - sq));
	}
}
__global__ __launch_bounds__(EM_BLOCK) void k_em_step_block(const EmClass *__restrict__ cls, uint32_t n, const uint32_t *__restrict__ ref, const u64 *__restrict__ c,
		u64 *__restrict__ out, const u64 *__restrict__ prev_cell, u64 tol) {
	EM_SKIP(prev_cell, tol);
	__shared__ u64 s_sum[EM_BLOCK / 64], s_tc[EM_BLOCK / 64]; __shared__ uint32_t s_th[EM_BLOCK / 64];
	const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {      // (block-uniform loop: every barrier below is met by the whole block)
		const EmClass K = cls[k];
		const uint32_t *r = ref + K.start;
		u64 d = 0, tc = 0; uint32_t th = 0xFFFFFFFFu;
		for (uint32_t i = threadIdx.x; i < K.size; i += EM_BLOCK) { const uint32_t h = r[i]; const u64 v = c[h]; d += v; em_top_merge(tc, th, v, h); }
		d = em_wave_sum(d); em_wave_top(tc, th);
		if (!lane) { s_sum[wv] = d; s_tc[wv] = tc; s_th[wv] = th; }
		__syncthreads();
		d = 0; tc = 0; th = 0xFFFFFFFFu;
		for (uint32_t x = 0; x < EM_BLOCK / 64; ++x) { d += s_sum[x]; em_top_merge(tc, th, s_tc[x], s_th[x]); }
		__syncthreads();
		u64 sq = 0;
		for (uint32_t i = threadIdx.x; i < K.size; i += EM_BLOCK) {
			const uint32_t h = r[i];
			const u64 q = em_share(c[h], d);
			sq += q;
			if (q) atomicAdd(&out[h], (u64)K.w * q);
		}
		sq = em_wave_sum(sq);
		if (!lane) s_sum[wv] = sq;
		__syncthreads();
		if (!threadIdx.x) {
			sq = 0;
			for (uint32_t x = 0; x < EM_BLOCK / 64; ++x) sq += s_sum[x];
			if (EM_ONE - sq) atomicAdd(&out[th], (u64)K.w * (EM_ONE - sq));
		}
		__syncthreads();
	}
}
// delta of the iteration into its cell; the buffer of the iteration before becomes the copy of base the next one adds into
__global__ __launch_bounds__(EM_BLOCK) void k_em_delta(const u64 *__restrict__ cur, u64 *__restrict__ old, const u64 *__restrict__ base, uint32_t n, u64 *__restrict__ cell,
		const u64 *__restrict__ prev_cell, u64 tol) {
	EM_SKIP(prev_cell, tol);
	u64 m = 0;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const u64 a = cur[i], b = old[i], dl = a > b ? a - b : b - a;
		m = dl > m ? dl : m;
		old[i] = base[i];
	}
	m = em_wave_max(m);
	if (!(threadIdx.x & 63) && m) atomicMax(cell, m);
}

struct EmState {
	DBuf lines, gw, key, key2, flag, pk, ref, nsel, bad, tmp, seg_start, seg_size, seg_w, skey, skey2, sidx, sidx2, head, cid, cls_w, cls_rep, list, cnt, base, c0, c1, cells;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	uint64_t bytes() {
		uint64_t b = 0;
		for (DBuf *x : all()) b += x->cap;
		return b;
	}
	std::vector<DBuf *> all() {
		return {&lines, &gw, &key, &key2, &flag, &pk, &ref, &nsel, &bad, &tmp, &seg_start, &seg_size, &seg_w, &skey, &skey2, &sidx, &sidx2, &head, &cid, &cls_w, &cls_rep, &list, &cnt,
		        &base, &c0, &c1, &cells};
	}
};

// (bhip_handle.h: Handle::em, Handle::opt_em_weak_hash, opt_em_thread_max, opt_em_wave_max)
void bhip_em_release(Handle *h) {
	EmState *st = (EmState *)h->em;
	if (!st) return;
	for (DBuf *b : st->all()) b->release();
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->em = nullptr;
}

static inline dim3 em_grid(uint64_t n) { return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + EM_BLOCK - 1) / EM_BLOCK, EM_MAX_GRID))); }
static inline dim3 em_grid_waves(uint64_t n) { return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + EM_BLOCK / 64 - 1) / (EM_BLOCK / 64), EM_MAX_GRID))); }
static int bits_of(uint32_t v) { int b = 1; while (b < 32 && (v >> b)) ++b; return b; }

static int em_run(Handle *h, EmState *st, uint32_t n_headers, uint32_t n_groups, const uint32_t *group_w, const BhipEmLine *lines, uint64_t n_lines, uint32_t max_iters,
                  uint64_t tol, uint64_t *counts, uint64_t *info) {
	hipStream_t S = h->stream;
	const uint32_t n = (uint32_t)n_lines;
	int rc;
	#define RES(buf, bytes) do { if ((rc = st->buf.reserve((size_t)(bytes) + 16))) return rc; } while (0)
	RES(lines, (size_t)n * 8); RES(gw, (size_t)n_groups * 4); RES(key, (size_t)n * 8); RES(key2, (size_t)n * 8); RES(flag, n); RES(pk, (size_t)n * 8); RES(ref, (size_t)n * 4);
	RES(nsel, 16); RES(bad, 32); RES(cnt, 16); RES(cells, (EM_POLL + 1) * 8);
	RES(base, (size_t)n_headers * 8); RES(c0, (size_t)n_headers * 8); RES(c1, (size_t)n_headers * 8);
	HIPCHK(hipMemcpyAsync(st->lines.p, lines, (size_t)n * 8, hipMemcpyHostToDevice, S));
	HIPCHK(hipMemcpyAsync(st->gw.p, group_w, (size_t)n_groups * 4, hipMemcpyHostToDevice, S));
	HIPCHK(hipMemsetAsync(st->bad.p, 0, 32, S));
	HIPCHK(hipEventRecord(st->ev0, S));
	// ---- pairs ----
	hipLaunchKernelGGL(k_em_keys, em_grid(n), dim3(EM_BLOCK), 0, S, st->lines.as<BhipEmLine>(), (uint64_t)n, st->gw.as<uint32_t>(), n_groups, n_headers, st->key.as<u64>(), st->bad.as<u64>());
	HIPCHK(hipGetLastError());
	const int end_bit = 32 + bits_of(n_groups);      // (n_groups itself is the group of the lines that take no part)
	size_t tb = 0;
	HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, st->key.as<u64>(), st->key2.as<u64>(), (int)n, 0, end_bit, S));
	RES(tmp, tb);
	HIPCHK(hipcub::DeviceRadixSort::SortKeys(st->tmp.p, tb, st->key.as<u64>(), st->key2.as<u64>(), (int)n, 0, end_bit, S));
	hipLaunchKernelGGL(k_em_first, em_grid(n), dim3(EM_BLOCK), 0, S, st->key2.as<u64>(), (uint64_t)n, n_groups, st->flag.as<uint8_t>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tb, st->key2.as<u64>(), st->flag.as<uint8_t>(), st->pk.as<u64>(), st->nsel.as<uint32_t>(), (int)n, S));
	RES(tmp, tb);
	HIPCHK(hipcub::DeviceSelect::Flagged(st->tmp.p, tb, st->key2.as<u64>(), st->flag.as<uint8_t>(), st->pk.as<u64>(), st->nsel.as<uint32_t>(), (int)n, S));
	uint32_t n_pairs = 0; u64 bad[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(&n_pairs, st->nsel.p, 4, hipMemcpyDeviceToHost, S));
	HIPCHK(hipMemcpyAsync(bad, st->bad.p, 16, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	if (bad[0]) return fail(BHIP_E_ARG, "bhip_em_run: %llu lines name a group beyond the %u given", bad[0], n_groups);
	if (bad[1]) return fail(BHIP_E_ARG, "bhip_em_run: %llu lines name a header beyond the %u given", bad[1], n_headers);
	if (n_pairs > n) return fail(BHIP_E_INTERNAL, "abundance: %u pairs from %u lines", n_pairs, n);
	info[1] = n_pairs;
	if (!n_pairs) return BHIP_OK;      // (no group takes part: zeros, 0 iterations)
	// ---- segments (one candidate set each) ----
	hipLaunchKernelGGL(k_em_segflag, em_grid(n_pairs), dim3(EM_BLOCK), 0, S, st->pk.as<u64>(), (uint64_t)n_pairs, st->ref.as<uint32_t>(), st->flag.as<uint8_t>());
	HIPCHK(hipGetLastError());
	RES(seg_start, (size_t)n_pairs * 4);
	hipcub::CountingInputIterator<uint32_t> iota(0u);
	HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tb, iota, st->flag.as<uint8_t>(), st->seg_start.as<uint32_t>(), st->nsel.as<uint32_t>(), (int)n_pairs, S));
	RES(tmp, tb);
	HIPCHK(hipcub::DeviceSelect::Flagged(st->tmp.p, tb, iota, st->flag.as<uint8_t>(), st->seg_start.as<uint32_t>(), st->nsel.as<uint32_t>(), (int)n_pairs, S));
	uint32_t n_seg = 0;
	HIPCHK(hipMemcpyAsync(&n_seg, st->nsel.p, 4, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	if (!n_seg || n_seg > n_pairs) return fail(BHIP_E_INTERNAL, "abundance: %u candidate sets from %u pairs", n_seg, n_pairs);
	RES(seg_size, (size_t)n_seg * 4); RES(seg_w, (size_t)n_seg * 4); RES(skey, (size_t)n_seg * 8); RES(skey2, (size_t)n_seg * 8); RES(sidx, (size_t)n_seg * 4); RES(sidx2, (size_t)n_seg * 4);
	RES(head, (size_t)n_seg * 4); RES(cid, (size_t)n_seg * 4); RES(cls_w, (size_t)n_seg * 4); RES(cls_rep, (size_t)n_seg * 4);
	HIPCHK(hipMemsetAsync(st->bad.p, 0, 32, S));      // ([2]: the reads of all sets)
	const u64 hash_mask = h->opt_em_weak_hash ? 3ull : ~0ull;
	hipLaunchKernelGGL(k_em_segments, em_grid(n_seg), dim3(EM_BLOCK), 0, S, st->pk.as<u64>(), st->seg_start.as<uint32_t>(), n_seg, n_pairs, st->gw.as<uint32_t>(), hash_mask,
		st->seg_size.as<uint32_t>(), st->seg_w.as<uint32_t>(), st->skey.as<u64>(), st->sidx.as<uint32_t>(), st->bad.as<u64>() + 2);
	HIPCHK(hipGetLastError());
	// ---- classes ----
	const int hbits = h->opt_em_weak_hash ? 2 : 64;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, st->skey.as<u64>(), st->skey2.as<u64>(), st->sidx.as<uint32_t>(), st->sidx2.as<uint32_t>(), (int)n_seg, 0, hbits, S));
	RES(tmp, tb);
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, st->skey.as<u64>(), st->skey2.as<u64>(), st->sidx.as<uint32_t>(), st->sidx2.as<uint32_t>(), (int)n_seg, 0, hbits, S));
	hipLaunchKernelGGL(k_em_same, em_grid_waves(n_seg), dim3(EM_BLOCK), 0, S, st->skey2.as<u64>(), st->sidx2.as<uint32_t>(), n_seg, st->seg_start.as<uint32_t>(), st->seg_size.as<uint32_t>(),
		st->ref.as<uint32_t>(), st->head.as<uint32_t>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tb, st->head.as<uint32_t>(), st->cid.as<uint32_t>(), (int)n_seg, S));
	RES(tmp, tb);
	HIPCHK(hipcub::DeviceScan::InclusiveSum(st->tmp.p, tb, st->head.as<uint32_t>(), st->cid.as<uint32_t>(), (int)n_seg, S));
	uint32_t n_cls = 0; u64 total_w = 0;
	HIPCHK(hipMemcpyAsync(&n_cls, st->cid.as<uint32_t>() + (n_seg - 1), 4, hipMemcpyDeviceToHost, S));
	HIPCHK(hipMemcpyAsync(&total_w, st->bad.as<u64>() + 2, 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	if (total_w > 0x7FFFFFFFull) return fail(BHIP_E_ARG, "bhip_em_run: the participating groups hold %llu reads (limit 2^31 - 1)", total_w);
	if (!n_cls || n_cls > n_seg) return fail(BHIP_E_INTERNAL, "abundance: %u classes from %u candidate sets", n_cls, n_seg);
	info[2] = n_cls;
	RES(list, (size_t)n_cls * 3 * sizeof(EmClass));
	HIPCHK(hipMemsetAsync(st->cls_w.p, 0, (size_t)n_cls * 4, S));
	HIPCHK(hipMemsetAsync(st->cnt.p, 0, 16, S));
	HIPCHK(hipMemsetAsync(st->base.p, 0, (size_t)n_headers * 8, S));
	hipLaunchKernelGGL(k_em_class_w, em_grid(n_seg), dim3(EM_BLOCK), 0, S, st->cid.as<uint32_t>(), st->head.as<uint32_t>(), st->sidx2.as<uint32_t>(), n_seg, st->seg_w.as<uint32_t>(),
		st->cls_w.as<uint32_t>(), st->cls_rep.as<uint32_t>());
	HIPCHK(hipGetLastError());
	const uint32_t thread_max = h->opt_em_thread_max ? (uint32_t)h->opt_em_thread_max : EM_THREAD_MAX;
	const uint32_t wave_max = std::max<uint32_t>(h->opt_em_wave_max ? (uint32_t)h->opt_em_wave_max : EM_WAVE_MAX, thread_max);
	hipLaunchKernelGGL(k_em_classify, em_grid(n_cls), dim3(EM_BLOCK), 0, S, st->cls_w.as<uint32_t>(), st->cls_rep.as<uint32_t>(), n_cls, st->seg_start.as<uint32_t>(), st->seg_size.as<uint32_t>(),
		st->ref.as<uint32_t>(), thread_max, wave_max, st->base.as<u64>(), st->list.as<EmClass>(), st->cnt.as<uint32_t>());
	HIPCHK(hipGetLastError());
	uint32_t cnt[3] = {0, 0, 0};
	HIPCHK(hipMemcpyAsync(cnt, st->cnt.p, 12, hipMemcpyDeviceToHost, S));
	// c0 = ONE everywhere in buffer 0; buffer 1 = base, what iteration 1 adds into
	u64 *buf[2] = {st->c0.as<u64>(), st->c1.as<u64>()};
	hipLaunchKernelGGL(k_em_fill, em_grid(n_headers), dim3(EM_BLOCK), 0, S, buf[0], (u64)EM_ONE, buf[1], st->base.as<u64>(), n_headers);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(S));
	if ((uint64_t)cnt[0] + cnt[1] + cnt[2] > n_cls) return fail(BHIP_E_INTERNAL, "abundance: %u + %u + %u listed classes of %u", cnt[0], cnt[1], cnt[2], n_cls);
	// ---- iterations ----
	const EmClass *lst = st->list.as<EmClass>();
	u64 *cells = st->cells.as<u64>();
	uint64_t t = 0, delta = 0; bool conv = false;
	while (t < max_iters && !conv) {
		const uint32_t m = (uint32_t)std::min<uint64_t>(EM_POLL, max_iters - t);
		HIPCHK(hipMemsetAsync(cells, 0, (EM_POLL + 1) * 8, S));
		for (uint32_t k = 1; k <= m; ++k) {
			const u64 *prev = k > 1 ? cells + (k - 1) : nullptr;
			const u64 *c = buf[(t + k - 1) & 1]; u64 *out = buf[(t + k) & 1];
			if (cnt[0]) hipLaunchKernelGGL(k_em_step_thread, em_grid(cnt[0]), dim3(EM_BLOCK), 0, S, lst, cnt[0], st->ref.as<uint32_t>(), c, out, prev, (u64)tol);
			if (cnt[1]) hipLaunchKernelGGL(k_em_step_wave, em_grid_waves(cnt[1]), dim3(EM_BLOCK), 0, S, lst + n_cls, cnt[1], st->ref.as<uint32_t>(), c, out, prev, (u64)tol);
			if (cnt[2]) hipLaunchKernelGGL(k_em_step_block, dim3(std::min(cnt[2], EM_MAX_GRID)), dim3(EM_BLOCK), 0, S, lst + 2ull * n_cls, cnt[2], st->ref.as<uint32_t>(), c, out, prev, (u64)tol);
			hipLaunchKernelGGL(k_em_delta, em_grid(n_headers), dim3(EM_BLOCK), 0, S, out, (u64 *)c, st->base.as<u64>(), n_headers, cells + k, prev, (u64)tol);
			HIPCHK(hipGetLastError());
		}
		u64 hc[EM_POLL + 1];
		HIPCHK(hipMemcpyAsync(hc, cells, sizeof hc, hipMemcpyDeviceToHost, S));
		HIPCHK(hipStreamSynchronize(S));
		for (uint32_t k = 1; k <= m && !conv; ++k) { ++t; delta = hc[k]; conv = delta <= tol; }
	}
	HIPCHK(hipEventRecord(st->ev1, S));
	HIPCHK(hipMemcpyAsync(counts, buf[t & 1], (size_t)n_headers * 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	info[0] = t; info[3] = delta; info[4] = conv ? 1 : 0;
	info[5] = (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	#undef RES
	return BHIP_OK;
}

extern "C" int bhip_em_run(void *handle, uint32_t n_headers, uint32_t n_groups, const uint32_t *group_w, const BhipEmLine *lines, uint64_t n_lines, uint32_t max_iters, uint64_t tol,
                           uint64_t *counts, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!h || !counts || !n_headers) return fail(BHIP_E_ARG, "bhip_em_run: null handle, no headers or no place for the counts");
	if (!max_iters) return fail(BHIP_E_ARG, "bhip_em_run: max_iters must be at least 1");
	if (n_lines >= 0x80000000ull) return fail(BHIP_E_ARG, "bhip_em_run: %llu lines (limit 2^31 - 1)", (unsigned long long)n_lines);
	if (n_lines && (!lines || !group_w)) return fail(BHIP_E_ARG, "bhip_em_run: lines without a line array or without group weights");
	memset(counts, 0, (size_t)n_headers * 8);
	if (!n_lines) return BHIP_OK;
	if (!n_groups) return fail(BHIP_E_ARG, "bhip_em_run: %llu lines name a group beyond the 0 given", (unsigned long long)n_lines);
	bool any_w = false;
	for (uint32_t g = 0; g < n_groups && !any_w; ++g) any_w = group_w[g] != 0;
	if (!any_w) {      // (no group can take part: nothing is launched -- but a line outside the tables is still an error)
		for (uint64_t i = 0; i < n_lines; ++i) {
			if (lines[i].group >= n_groups) return fail(BHIP_E_ARG, "bhip_em_run: line %llu names group %u of %u", (unsigned long long)i, lines[i].group, n_groups);
			if (lines[i].ref >= n_headers) return fail(BHIP_E_ARG, "bhip_em_run: line %llu names header %u of %u", (unsigned long long)i, lines[i].ref, n_headers);
		}
		return BHIP_OK;
	}
	HIPCHK(hipSetDevice(h->device));
	EmState *st = (EmState *)h->em;
	if (!st) {
		st = new EmState();
		if (hipEventCreate(&st->ev0) != hipSuccess || hipEventCreate(&st->ev1) != hipSuccess) {
			if (st->ev0) (void)hipEventDestroy(st->ev0);
			delete st;
			return fail(BHIP_E_DEVICE, "hipEventCreate failed");
		}
		h->em = st;
	}
	const int rc = em_run(h, st, n_headers, n_groups, group_w, lines, n_lines, max_iters, tol, counts, info);
	if (rc) { memset(info, 0, 8 * sizeof(uint64_t)); memset(counts, 0, (size_t)n_headers * 8); }
	info[6] = st->bytes();
	return rc;
}
