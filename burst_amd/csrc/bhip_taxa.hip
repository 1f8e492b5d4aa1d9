// burst_amd/csrc/bhip_taxa.hip -- taxon tables: every group of reads goes to the lowest common ancestor of its candidates' taxonomy nodes
// (burst_hip --taxa; bhip_taxa_run, bhip_taxa_rollup, gfx950).  The reference's embalmulate.c counts column 13 of BEST output; its README
// leaves the tied references of ALLPATHS output to the user.
//
// Definition (include/burst_hip.h).  The tree comes numbered in preorder (a subtree is a range of numbers), every
// header has a node, a group's candidates are the distinct headers of its lines, n of them; t = (agree * n + 999) / 1000 and the group's
// taxon is the deepest node whose subtree holds the nodes of at least t candidates.  own[v] = the reads of the groups at v, clade[v] = own
// summed over v's subtree.  Integers only: the sums are 64-bit atomic additions, which commute.
//
// The device work.
//   pairs     keys group << 32 | header (a line outside the tables is counted and gets the group number n_groups, which sorts behind
//             everything), hipcub radix sort over the bits in use, the first of every run of equal keys selected: the distinct pairs.
//   nodes     each pair's header replaced by its node -- in preorder also its DFS index -- and the keys sorted again: inside a group the
//             candidates stand in DFS order.  The first pair of every group starts its SEGMENT.
//   taxon     in DFS order the t candidates under one node are neighbours, and the lowest common ancestor of a window of neighbours is
//             that of its two ends: the taxon is the deepest LCA(x[i], x[i + t - 1]) over the n - t + 1 windows.  An LCA is a walk over
//             `parent` that lifts the deeper end (at most 2 x 64 steps).  k_taxa_thread takes the segments of up to TAXA_THREAD_MAX
//             candidates, one thread each, and lists the longer ones; k_taxa_wave gives each of those a wave whose lanes stride the windows
//             and reduce (depth, node) by shuffles.  Either adds the group's reads to own[taxon].
//   clade     a subtree is the range [v, last[v]] of preorder numbers: an inclusive prefix sum of own (hipcub) and one subtraction per
//             node, k_taxa_clade.  No atomics: every read would otherwise be added to the root's cell.  (A first version that added each
//             count to every ancestor took 22 ms of device time per call for a million groups; the record of that run was not kept.  This
//             form: profiles/taxa_e2e.json.)
// The tree is checked on the host before anything is launched (one pass over `parent`, which also yields the depths and every subtree's
// last node) and stays on the device: a later call with the same parent and header_node, compared byte by byte, skips check and upload.
#include "bhip_handle.h"

#define TAXA_BLOCK 256
#define TAXA_MAX_GRID 8192u
#define TAXA_MAX_DEPTH 64u
#define TAXA_THREAD_MAX 64u      // candidates of the largest segment a single thread walks; not measured (bhip_cluster.hip hands runs of 64 and more to a wave: its split lies one lower)

typedef unsigned long long u64;

__device__ __forceinline__ u64 taxa_wave_sum(u64 v) { for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
__device__ __forceinline__ u64 taxa_wave_max(u64 v) { for (int o = 32; o; o >>= 1) { const u64 x = __shfl_xor(v, o, 64); v = x > v ? x : v; } return v; }

// the lowest common ancestor of two nodes: the deeper one is lifted until they meet (both below n_nodes, parent[v] < v: it ends at the root at the latest)
__device__ __forceinline__ uint32_t taxa_lca(uint32_t a, uint32_t b, const uint32_t *__restrict__ parent, const uint32_t *__restrict__ depth) {
	uint32_t da = depth[a], db = depth[b];
	while (a != b) {
		if (da > db) { a = parent[a]; --da; }
		else { b = parent[b]; --db; }
	}
	return a;
}
// depth << 32 | node of the deepest window LCA among the windows i = first, first + step, ... of a segment x[0 .. n) with windows of t
__device__ __forceinline__ u64 taxa_windows(const u64 *__restrict__ x, uint32_t n, uint32_t t, uint32_t first, uint32_t step, const uint32_t *__restrict__ parent,
		const uint32_t *__restrict__ depth) {
	u64 best = 0;
	for (uint32_t i = first; i + t <= n; i += step) {
		const uint32_t v = taxa_lca((uint32_t)x[i], (uint32_t)x[i + t - 1], parent, depth);
		const u64 k = (u64)depth[v] << 32 | v;
		best = k > best ? k : best;
	}
	return best;
}

// one thread per line: its key; a line outside the tables is counted (bad[0] group, bad[1] header) and sorts last
__global__ __launch_bounds__(TAXA_BLOCK) void k_taxa_keys(const BhipEmLine *__restrict__ ln, uint32_t n, uint32_t n_groups, uint32_t n_headers, u64 *__restrict__ key,
		u64 *__restrict__ bad) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const BhipEmLine l = ln[i];
		uint32_t g = l.group;
		if (g >= n_groups) { atomicAdd(&bad[0], 1ull); g = n_groups; }
		else if (l.ref >= n_headers) { atomicAdd(&bad[1], 1ull); g = n_groups; }
		key[i] = (u64)g << 32 | (g == n_groups ? 0u : l.ref);
	}
}
// sorted keys: 1 for the first of every run of equal keys
__global__ __launch_bounds__(TAXA_BLOCK) void k_taxa_first(const u64 *__restrict__ key, uint32_t n, uint32_t n_groups, uint8_t *__restrict__ flag) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const u64 k = key[i];
		flag[i] = (uint32_t)(k >> 32) != n_groups && (!i || key[i - 1] != k);
	}
}
// distinct pairs (every header below n_headers: the bad lines were not selected): the header becomes its node
__global__ __launch_bounds__(TAXA_BLOCK) void k_taxa_nodes(const u64 *__restrict__ pk, uint32_t n, const uint32_t *__restrict__ header_node, u64 *__restrict__ out) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const u64 k = pk[i];
		out[i] = (k & 0xFFFFFFFF00000000ull) | header_node[(uint32_t)k];
	}
}
// pairs sorted by (group, node): 1 where a group's segment starts
__global__ __launch_bounds__(TAXA_BLOCK) void k_taxa_segflag(const u64 *__restrict__ x, uint32_t n, uint8_t *__restrict__ flag) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) flag[i] = !i || (x[i - 1] >> 32) != (x[i] >> 32);
}
// a group's result: its node, its reads into own[node].  The totals (tot[0] reads, tot[1] deepest level) are reduced per wave by the callers:
// one atomic per group on a single cell would serialise the whole kernel
__device__ __forceinline__ void taxa_assign(uint32_t g, u64 best, const uint32_t *__restrict__ gw, uint32_t *__restrict__ group_node, u64 *__restrict__ own) {
	const uint32_t v = (uint32_t)best, w = gw[g];
	group_node[g] = v;
	if (w) atomicAdd(&own[v], (u64)w);
}
// one thread per segment: the short ones solved, the long ones listed
__global__ __launch_bounds__(TAXA_BLOCK) void k_taxa_thread(const u64 *__restrict__ x, const uint32_t *__restrict__ seg_start, uint32_t n_seg, uint32_t n_pairs, uint32_t agree,
		const uint32_t *__restrict__ parent, const uint32_t *__restrict__ depth, const uint32_t *__restrict__ gw, uint32_t *__restrict__ group_node, u64 *__restrict__ own,
		u64 *__restrict__ tot, uint32_t *__restrict__ long_list, uint32_t *__restrict__ n_long) {
	u64 wsum = 0, deep = 0;
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_seg; s += gridDim.x * blockDim.x) {
		const uint32_t a = seg_start[s], b = s + 1 < n_seg ? seg_start[s + 1] : n_pairs, n = b - a;
		const uint32_t g = (uint32_t)(x[a] >> 32);
		wsum += gw[g];
		if (n > TAXA_THREAD_MAX) { long_list[atomicAdd(n_long, 1u)] = s; continue; }
		const uint32_t t = (uint32_t)(((u64)agree * n + 999) / 1000);
		const u64 best = taxa_windows(x + a, n, t, 0, 1, parent, depth);
		taxa_assign(g, best, gw, group_node, own);
		deep = (best >> 32) > deep ? best >> 32 : deep;
	}
	wsum = taxa_wave_sum(wsum); deep = taxa_wave_max(deep);      // (every lane of the wave is here: the loop has ended for all of them)
	if (!(threadIdx.x & 63)) { if (wsum) atomicAdd(&tot[0], wsum); if (deep) atomicMax(&tot[1], deep); }
}
// one wave per listed segment
__global__ __launch_bounds__(TAXA_BLOCK) void k_taxa_wave(const u64 *__restrict__ x, const uint32_t *__restrict__ seg_start, uint32_t n_seg, uint32_t n_pairs, uint32_t agree,
		const uint32_t *__restrict__ parent, const uint32_t *__restrict__ depth, const uint32_t *__restrict__ gw, uint32_t *__restrict__ group_node, u64 *__restrict__ own,
		u64 *__restrict__ tot, const uint32_t *__restrict__ long_list, const uint32_t *__restrict__ n_long) {
	const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * (TAXA_BLOCK / 64), nl = min(*n_long, n_seg);
	u64 deep = 0;
	for (uint32_t j = blockIdx.x * (TAXA_BLOCK / 64) + (threadIdx.x >> 6); j < nl; j += waves) {      // (wave-uniform loop)
		const uint32_t s = long_list[j];
		if (s >= n_seg) continue;
		const uint32_t a = seg_start[s], b = s + 1 < n_seg ? seg_start[s + 1] : n_pairs, n = b - a;
		const uint32_t t = (uint32_t)(((u64)agree * n + 999) / 1000);
		const u64 best = taxa_wave_max(taxa_windows(x + a, n, t, lane, 64, parent, depth));
		if (!lane) taxa_assign((uint32_t)(x[a] >> 32), best, gw, group_node, own);
		deep = (best >> 32) > deep ? best >> 32 : deep;
	}
	if (!lane && deep) atomicMax(&tot[1], deep);
}
// psum = inclusive prefix sum of own in preorder, last[v] = the last node of v's subtree (v <= last[v] < n_nodes): clade[v] = own summed over [v, last[v]]
__global__ __launch_bounds__(TAXA_BLOCK) void k_taxa_clade(const u64 *__restrict__ psum, uint32_t n_nodes, const uint32_t *__restrict__ last, u64 *__restrict__ clade) {
	for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n_nodes; v += gridDim.x * blockDim.x) clade[v] = psum[last[v]] - (v ? psum[v - 1] : 0ull);
}
// roll-up: own[node of h] += count[h]
__global__ __launch_bounds__(TAXA_BLOCK) void k_taxa_rollup(const u64 *__restrict__ count, uint32_t n_headers, const uint32_t *__restrict__ header_node, u64 *__restrict__ own) {
	for (uint32_t h = blockIdx.x * blockDim.x + threadIdx.x; h < n_headers; h += gridDim.x * blockDim.x) {
		const u64 c = count[h];
		if (c) atomicAdd(&own[header_node[h]], c);
	}
}

struct TaxaState {
	DBuf parent, depth, last, hnode, lines, gw, key, key2, flag, pk, nsel, bad, tmp, seg_start, long_list, gnode, own, psum, clade, count;
	// the tree that is on the device (parent, depth, last, hnode): a call that brings the same parent and header_node again -- every sample of
	// a study does -- finds it by comparing the bytes, and is spared the check and the four uploads
	std::vector<uint32_t> cparent, chnode;
	bool resident = false;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	std::vector<DBuf *> all() { return {&parent, &depth, &last, &hnode, &lines, &gw, &key, &key2, &flag, &pk, &nsel, &bad, &tmp, &seg_start, &long_list, &gnode, &own, &psum, &clade, &count}; }
	uint64_t bytes() {
		uint64_t b = 0;
		for (DBuf *x : all()) b += x->cap;
		return b;
	}
};

// (bhip_handle.h: Handle::taxa)
void bhip_taxa_release(Handle *h) {
	TaxaState *st = (TaxaState *)h->taxa;
	if (!st) return;
	for (DBuf *b : st->all()) b->release();
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->taxa = nullptr;
}

static inline dim3 taxa_grid(uint64_t n) { return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + TAXA_BLOCK - 1) / TAXA_BLOCK, TAXA_MAX_GRID))); }
static inline dim3 taxa_grid_waves(uint64_t n) { return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + TAXA_BLOCK / 64 - 1) / (TAXA_BLOCK / 64), TAXA_MAX_GRID))); }
static int taxa_bits_of(uint32_t v) { int b = 1; while (b < 32 && (v >> b)) ++b; return b; }

// the checks on the tree, on the host; depth[] and last[] (the last node of every subtree) filled
static int taxa_check_tree(const char *who, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, std::vector<uint32_t> &depth,
                           std::vector<uint32_t> &last) {
	if (!n_nodes || !parent || n_nodes > 0x7FFFFFFFu) return fail(BHIP_E_ARG, "%s: no tree", who);
	if (n_headers && !header_node) return fail(BHIP_E_ARG, "%s: headers without their nodes", who);
	if (parent[0]) return fail(BHIP_E_ARG, "%s: node 0 is the root and its own parent", who);
	depth.assign(n_nodes, 0);
	for (uint32_t v = 1; v < n_nodes; ++v) {
		const uint32_t p = parent[v];
		if (p >= v) return fail(BHIP_E_ARG, "%s: node %u has parent %u: not a preorder numbering", who, v, p);
		uint32_t x = v - 1;
		while (x > p) x = parent[x];
		if (x != p) return fail(BHIP_E_ARG, "%s: the parent %u of node %u is no ancestor of node %u: not a preorder numbering", who, p, v, v - 1);
		depth[v] = depth[p] + 1;
		if (depth[v] > TAXA_MAX_DEPTH) return fail(BHIP_E_ARG, "%s: node %u lies %u levels deep (limit %u)", who, v, depth[v], TAXA_MAX_DEPTH);
	}
	for (uint32_t h = 0; h < n_headers; ++h)
		if (header_node[h] >= n_nodes) return fail(BHIP_E_ARG, "%s: header %u names node %u of %u", who, h, header_node[h], n_nodes);
	last.resize(n_nodes);
	for (uint32_t v = 0; v < n_nodes; ++v) last[v] = v;
	for (uint32_t v = n_nodes - 1; v > 0; --v) if (last[v] > last[parent[v]]) last[parent[v]] = last[v];      // (children have larger numbers than their parent)
	return BHIP_OK;
}

// clade from own (both on the device, own complete in stream order); st->last holds the tree's
static int taxa_clade(Handle *h, TaxaState *st, uint32_t n_nodes) {
	hipStream_t S = h->stream;
	int rc;
	size_t tb = 0;
	HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tb, st->own.as<u64>(), st->psum.as<u64>(), (int)n_nodes, S));
	if ((rc = st->tmp.reserve(tb + 16))) return rc;
	HIPCHK(hipcub::DeviceScan::InclusiveSum(st->tmp.p, tb, st->own.as<u64>(), st->psum.as<u64>(), (int)n_nodes, S));
	hipLaunchKernelGGL(k_taxa_clade, taxa_grid(n_nodes), dim3(TAXA_BLOCK), 0, S, st->psum.as<u64>(), n_nodes, st->last.as<uint32_t>(), st->clade.as<u64>());
	HIPCHK(hipGetLastError());
	return BHIP_OK;
}

static int taxa_state(Handle *h, TaxaState **out) {
	HIPCHK(hipSetDevice(h->device));
	TaxaState *st = (TaxaState *)h->taxa;
	if (!st) {
		st = new TaxaState();
		if (hipEventCreate(&st->ev0) != hipSuccess || hipEventCreate(&st->ev1) != hipSuccess) {
			if (st->ev0) (void)hipEventDestroy(st->ev0);
			delete st;
			return fail(BHIP_E_DEVICE, "hipEventCreate failed");
		}
		h->taxa = st;
	}
	*out = st;
	return BHIP_OK;
}

#define RES(buf, bytes) do { if ((rc = st->buf.reserve((size_t)(bytes) + 16))) return rc; } while (0)

static bool taxa_tree_same(const TaxaState *st, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node) {
	return st && st->resident && parent && (!n_headers || header_node) && st->cparent.size() == n_nodes && st->chnode.size() == n_headers && !memcmp(st->cparent.data(), parent, (size_t)n_nodes * 4) &&
	       (!n_headers || !memcmp(st->chnode.data(), header_node, (size_t)n_headers * 4));
}
// a checked tree to the device, with the depths and subtree ends the check found; complete when this returns
static int taxa_tree_put(Handle *h, TaxaState *st, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, const std::vector<uint32_t> &depth,
                         const std::vector<uint32_t> &last) {
	hipStream_t S = h->stream;
	int rc;
	st->resident = false;
	st->cparent.assign(parent, parent + n_nodes);
	st->chnode.assign(header_node, header_node + n_headers);
	RES(parent, (size_t)n_nodes * 4); RES(depth, (size_t)n_nodes * 4); RES(last, (size_t)n_nodes * 4); RES(hnode, (size_t)n_headers * 4);
	HIPCHK(hipMemcpyAsync(st->parent.p, parent, (size_t)n_nodes * 4, hipMemcpyHostToDevice, S));
	HIPCHK(hipMemcpyAsync(st->depth.p, depth.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, S));
	HIPCHK(hipMemcpyAsync(st->last.p, last.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, S));
	if (n_headers) HIPCHK(hipMemcpyAsync(st->hnode.p, header_node, (size_t)n_headers * 4, hipMemcpyHostToDevice, S));
	HIPCHK(hipStreamSynchronize(S));
	st->resident = true;
	return BHIP_OK;
}

static int taxa_run(Handle *h, TaxaState *st, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, uint32_t n_groups,
                    const uint32_t *group_w, const BhipEmLine *lines, uint32_t n, uint32_t agree, uint32_t *group_node, uint64_t *own, uint64_t *clade, uint64_t *info) {
	hipStream_t S = h->stream;
	int rc;
	RES(lines, (size_t)n * 8); RES(gw, (size_t)n_groups * 4);      // (the tree is on the device: taxa_tree_put)
	RES(key, (size_t)n * 8); RES(key2, (size_t)n * 8); RES(flag, n); RES(pk, (size_t)n * 8); RES(nsel, 16); RES(bad, 64);
	RES(gnode, (size_t)n_groups * 4); RES(own, (size_t)n_nodes * 8); RES(psum, (size_t)n_nodes * 8); RES(clade, (size_t)n_nodes * 8);
	HIPCHK(hipMemcpyAsync(st->lines.p, lines, (size_t)n * 8, hipMemcpyHostToDevice, S));
	HIPCHK(hipMemcpyAsync(st->gw.p, group_w, (size_t)n_groups * 4, hipMemcpyHostToDevice, S));
	HIPCHK(hipMemsetAsync(st->bad.p, 0, 64, S));      // ([0] [1] lines outside the tables, [2] reads, [3] deepest level, [4] listed segments)
	HIPCHK(hipMemsetAsync(st->gnode.p, 0xFF, (size_t)n_groups * 4, S));
	HIPCHK(hipMemsetAsync(st->own.p, 0, (size_t)n_nodes * 8, S));
	HIPCHK(hipEventRecord(st->ev0, S));
	// ---- pairs ----
	hipLaunchKernelGGL(k_taxa_keys, taxa_grid(n), dim3(TAXA_BLOCK), 0, S, st->lines.as<BhipEmLine>(), n, n_groups, n_headers, st->key.as<u64>(), st->bad.as<u64>());
	HIPCHK(hipGetLastError());
	const int end_bit = 32 + taxa_bits_of(n_groups);      // (n_groups itself is the group of the lines outside the tables)
	size_t tb = 0;
	HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, st->key.as<u64>(), st->key2.as<u64>(), (int)n, 0, end_bit, S));
	RES(tmp, tb);
	HIPCHK(hipcub::DeviceRadixSort::SortKeys(st->tmp.p, tb, st->key.as<u64>(), st->key2.as<u64>(), (int)n, 0, end_bit, S));
	hipLaunchKernelGGL(k_taxa_first, taxa_grid(n), dim3(TAXA_BLOCK), 0, S, st->key2.as<u64>(), n, n_groups, st->flag.as<uint8_t>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tb, st->key2.as<u64>(), st->flag.as<uint8_t>(), st->pk.as<u64>(), st->nsel.as<uint32_t>(), (int)n, S));
	RES(tmp, tb);
	HIPCHK(hipcub::DeviceSelect::Flagged(st->tmp.p, tb, st->key2.as<u64>(), st->flag.as<uint8_t>(), st->pk.as<u64>(), st->nsel.as<uint32_t>(), (int)n, S));
	uint32_t n_pairs = 0; u64 bad[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(&n_pairs, st->nsel.p, 4, hipMemcpyDeviceToHost, S));
	HIPCHK(hipMemcpyAsync(bad, st->bad.p, 16, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	if (bad[0]) return fail(BHIP_E_ARG, "bhip_taxa_run: %llu lines name a group beyond the %u given", bad[0], n_groups);
	if (bad[1]) return fail(BHIP_E_ARG, "bhip_taxa_run: %llu lines name a header beyond the %u given", bad[1], n_headers);
	if (!n_pairs || n_pairs > n) return fail(BHIP_E_INTERNAL, "taxa: %u pairs from %u lines", n_pairs, n);
	// ---- nodes in DFS order inside every group (key: the pairs' nodes, key2: sorted) ----
	hipLaunchKernelGGL(k_taxa_nodes, taxa_grid(n_pairs), dim3(TAXA_BLOCK), 0, S, st->pk.as<u64>(), n_pairs, st->hnode.as<uint32_t>(), st->key.as<u64>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, st->key.as<u64>(), st->key2.as<u64>(), (int)n_pairs, 0, end_bit, S));
	RES(tmp, tb);
	HIPCHK(hipcub::DeviceRadixSort::SortKeys(st->tmp.p, tb, st->key.as<u64>(), st->key2.as<u64>(), (int)n_pairs, 0, end_bit, S));
	hipLaunchKernelGGL(k_taxa_segflag, taxa_grid(n_pairs), dim3(TAXA_BLOCK), 0, S, st->key2.as<u64>(), n_pairs, st->flag.as<uint8_t>());
	HIPCHK(hipGetLastError());
	RES(seg_start, (size_t)n_pairs * 4); RES(long_list, (size_t)n_pairs * 4);
	hipcub::CountingInputIterator<uint32_t> iota(0u);
	HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tb, iota, st->flag.as<uint8_t>(), st->seg_start.as<uint32_t>(), st->nsel.as<uint32_t>(), (int)n_pairs, S));
	RES(tmp, tb);
	HIPCHK(hipcub::DeviceSelect::Flagged(st->tmp.p, tb, iota, st->flag.as<uint8_t>(), st->seg_start.as<uint32_t>(), st->nsel.as<uint32_t>(), (int)n_pairs, S));
	uint32_t n_seg = 0;
	HIPCHK(hipMemcpyAsync(&n_seg, st->nsel.p, 4, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	if (!n_seg || n_seg > n_pairs) return fail(BHIP_E_INTERNAL, "taxa: %u groups from %u pairs", n_seg, n_pairs);
	// ---- the groups' taxa, own, clade ----
	u64 *tot = st->bad.as<u64>() + 2; uint32_t *n_long = (uint32_t *)(st->bad.as<u64>() + 4);
	hipLaunchKernelGGL(k_taxa_thread, taxa_grid(n_seg), dim3(TAXA_BLOCK), 0, S, st->key2.as<u64>(), st->seg_start.as<uint32_t>(), n_seg, n_pairs, agree, st->parent.as<uint32_t>(),
		st->depth.as<uint32_t>(), st->gw.as<uint32_t>(), st->gnode.as<uint32_t>(), st->own.as<u64>(), tot, st->long_list.as<uint32_t>(), n_long);
	HIPCHK(hipGetLastError());
	// (a segment of more than TAXA_THREAD_MAX pairs: there are at most n_pairs / (TAXA_THREAD_MAX + 1) of them; the kernel reads how many)
	hipLaunchKernelGGL(k_taxa_wave, taxa_grid_waves(n_pairs / (TAXA_THREAD_MAX + 1) + 1), dim3(TAXA_BLOCK), 0, S, st->key2.as<u64>(), st->seg_start.as<uint32_t>(), n_seg, n_pairs, agree,
		st->parent.as<uint32_t>(), st->depth.as<uint32_t>(), st->gw.as<uint32_t>(), st->gnode.as<uint32_t>(), st->own.as<u64>(), tot, st->long_list.as<uint32_t>(), n_long);
	HIPCHK(hipGetLastError());
	if ((rc = taxa_clade(h, st, n_nodes))) return rc;
	HIPCHK(hipEventRecord(st->ev1, S));
	u64 t2[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(t2, tot, 16, hipMemcpyDeviceToHost, S));
	HIPCHK(hipMemcpyAsync(own, st->own.p, (size_t)n_nodes * 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipMemcpyAsync(clade, st->clade.p, (size_t)n_nodes * 8, hipMemcpyDeviceToHost, S));
	if (group_node) HIPCHK(hipMemcpyAsync(group_node, st->gnode.p, (size_t)n_groups * 4, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	info[0] = n_pairs; info[1] = n_seg; info[2] = t2[0]; info[3] = own[0]; info[4] = t2[1];
	info[5] = (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	return BHIP_OK;
}

extern "C" int bhip_taxa_run(void *handle, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, uint32_t n_groups, const uint32_t *group_w,
                             const BhipEmLine *lines, uint64_t n_lines, uint32_t agree, uint32_t *group_node, uint64_t *own, uint64_t *clade, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!h || !own || !clade) return fail(BHIP_E_ARG, "bhip_taxa_run: null handle or no place for the counts");
	if (agree < 501 || agree > 1000) return fail(BHIP_E_ARG, "bhip_taxa_run: agree %u outside 501 .. 1000", agree);
	if (n_lines >= 0x80000000ull) return fail(BHIP_E_ARG, "bhip_taxa_run: %llu lines (limit 2^31 - 1)", (unsigned long long)n_lines);
	if (n_lines && (!lines || !group_w)) return fail(BHIP_E_ARG, "bhip_taxa_run: lines without a line array or without group weights");
	std::vector<uint32_t> depth, last;
	const bool same = taxa_tree_same((TaxaState *)h->taxa, n_nodes, parent, n_headers, header_node);      // (checked when it came first)
	int rc = same ? BHIP_OK : taxa_check_tree("bhip_taxa_run", n_nodes, parent, n_headers, header_node, depth, last);
	if (rc) return rc;
	memset(own, 0, (size_t)n_nodes * 8); memset(clade, 0, (size_t)n_nodes * 8);
	if (group_node) memset(group_node, 0xFF, (size_t)n_groups * 4);
	if (!n_lines) return BHIP_OK;      // (nothing is launched)
	if (!n_groups) return fail(BHIP_E_ARG, "bhip_taxa_run: %llu lines name a group beyond the 0 given", (unsigned long long)n_lines);
	if (!n_headers) return fail(BHIP_E_ARG, "bhip_taxa_run: %llu lines name a header beyond the 0 given", (unsigned long long)n_lines);
	TaxaState *st = nullptr;
	if ((rc = taxa_state(h, &st))) return rc;
	if (!same && (rc = taxa_tree_put(h, st, n_nodes, parent, n_headers, header_node, depth, last))) return rc;
	rc = taxa_run(h, st, n_nodes, parent, n_headers, header_node, n_groups, group_w, lines, (uint32_t)n_lines, agree, group_node, own, clade, info);
	if (rc) {
		memset(info, 0, 8 * sizeof(uint64_t)); memset(own, 0, (size_t)n_nodes * 8); memset(clade, 0, (size_t)n_nodes * 8);
		if (group_node) memset(group_node, 0xFF, (size_t)n_groups * 4);
	}
	info[6] = st->bytes();
	return rc;
}

extern "C" int bhip_taxa_rollup(void *handle, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, const uint64_t *header_count,
                                uint64_t *own, uint64_t *clade) {
	Handle *h = (Handle *)handle;
	if (!h || !own || !clade || (n_headers && !header_count)) return fail(BHIP_E_ARG, "bhip_taxa_rollup: null handle, no counts or no place for the sums");
	std::vector<uint32_t> depth, last;
	const bool same = taxa_tree_same((TaxaState *)h->taxa, n_nodes, parent, n_headers, header_node);
	int rc = same ? BHIP_OK : taxa_check_tree("bhip_taxa_rollup", n_nodes, parent, n_headers, header_node, depth, last);
	if (rc) return rc;
	memset(own, 0, (size_t)n_nodes * 8); memset(clade, 0, (size_t)n_nodes * 8);
	if (!n_headers) return BHIP_OK;
	TaxaState *st = nullptr;
	if ((rc = taxa_state(h, &st))) return rc;
	if (!same && (rc = taxa_tree_put(h, st, n_nodes, parent, n_headers, header_node, depth, last))) return rc;
	hipStream_t S = h->stream;
	RES(psum, (size_t)n_nodes * 8); RES(count, (size_t)n_headers * 8); RES(own, (size_t)n_nodes * 8); RES(clade, (size_t)n_nodes * 8);
	HIPCHK(hipMemcpyAsync(st->count.p, header_count, (size_t)n_headers * 8, hipMemcpyHostToDevice, S));
	HIPCHK(hipMemsetAsync(st->own.p, 0, (size_t)n_nodes * 8, S));
	hipLaunchKernelGGL(k_taxa_rollup, taxa_grid(n_headers), dim3(TAXA_BLOCK), 0, S, st->count.as<u64>(), n_headers, st->hnode.as<uint32_t>(), st->own.as<u64>());
	HIPCHK(hipGetLastError());
	if ((rc = taxa_clade(h, st, n_nodes))) return rc;
	HIPCHK(hipMemcpyAsync(own, st->own.p, (size_t)n_nodes * 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipMemcpyAsync(clade, st->clade.p, (size_t)n_nodes * 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipStreamSynchronize(S));
	return BHIP_OK;
}
#undef RES
