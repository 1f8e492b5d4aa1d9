// burst_amd/csrc/bhip_cluster.hip -- greedy centroid clustering of reads from their FORAGE self-hits (burst_hip --cluster;
// bhip_cluster_run, gfx950).  No reference counterpart: the reference's README lists clustering "as an output mode" as planned and gives
// the recipe (run the queries as their own references in FORAGE, pick clusters from that hit graph); this is the picking.
//
// Definition (include/burst_hip.h, README "Clustering").  Nodes 0 .. n-1 with weights; node a is BEFORE node b when
// its weight is larger, or the weights are equal and its number is smaller.  An edge q -> r with `edits` reads "r can represent q".  The
// nodes are taken in that order: a node with an edge to a centroid before it is a member of the one with the fewest edits (the earliest
// among equals), any other node is a centroid.  Edges towards later nodes never matter.
//
// The device work.
//   rank      keys ~weight << 32 | node, hipcub radix sort: order[p] = the p-th node in priority, rank[node] = p.
//   clean     an edge with q == r or rank[r] >= rank[q] gets the key of all ones and sorts behind everything; the others get
//             q << 32 | rank[r] and are sorted with their edits.  The first of every run of equal keys is flagged, the flags scanned, and
//             every edge of a run takes atomicMin of its edits into the run's cell: the distinct edges, each with its smallest edits.  A
//             binary search per node over the sorted q gives the run offsets -- a CSR whose targets ascend in priority.
//   rounds    state[rank] is one 32-bit word: undecided, centroid or member.  An undecided node walks its run: a centroid among the
//             targets makes it a member; all targets members (or no target) makes it a centroid; otherwise it waits and appends itself to
//             the next round's work list.  Runs shorter than 64, the wave's width, get one thread (k_cl_round_thread); longer runs get
//             one wave (k_cl_round_wave), which strides the run, ballots, and leaves at the first centroid.  The two lists' new lengths
//             come back to the host after every round: zero ends the loop.
//             WHY THE ORDER OF THREADS CANNOT MATTER: a node only ever moves from undecided to its final state, and only on final
//             information -- "member" needs one target that IS a centroid, "centroid" needs every target to BE a member, and neither
//             fact can change later.  A state that another thread writes during the same round is either seen (and is final) or not
//             seen (and reads as undecided, which only makes the reader wait).  So the result is the same whatever the order of threads
//             and whatever a round sees of itself.  The first undecided node in priority order has only decided targets (they are all
//             before it, and the kernel boundary has made their states visible), so every round decides at least one node: a round that
//             decides none is BHIP_E_INTERNAL, never a spin.  The worst case, a chain, takes one round per node: correct and slow.
//   assign    one pass over all nodes: a member takes the smallest (edits << 32 | rank) among its centroid targets, a centroid itself.
// Index arithmetic is 64-bit wherever an edge number or an offset is formed; every buffer is a grow-only one of the handle.
#include "bhip_handle.h"

#define CL_BLOCK 256
#define CL_MAX_GRID 65536u
#define CL_WAVE_MIN 64u      // a run of this many targets or more gets a wave (the wave's width)

typedef unsigned long long u64;
enum { CL_UNDECIDED = 0u, CL_CENTROID = 1u, CL_MEMBER = 2u };

// (a state may be written by another thread of the same launch: one 32-bit access that the compiler may neither split nor keep in a register)
__device__ __forceinline__ uint32_t cl_state_load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void cl_state_store(uint32_t *p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

__global__ __launch_bounds__(CL_BLOCK) void k_cl_rank_keys(const uint32_t *__restrict__ w, uint64_t n, u64 *__restrict__ key) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) key[i] = (u64)(~w[i]) << 32 | (u64)i;
}
__global__ __launch_bounds__(CL_BLOCK) void k_cl_rank(const u64 *__restrict__ key_s, uint64_t n, uint32_t *__restrict__ order, uint32_t *__restrict__ rank,
		uint32_t *__restrict__ state) {
	for (uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t node = (uint32_t)key_s[p];
		order[p] = node; rank[node] = (uint32_t)p; state[p] = CL_UNDECIDED;
	}
}
// an edge that can matter: q << 32 | rank[r]; a self edge or one towards a later node: all ones (q <= 2^32 - 2, so no real key is that)
__global__ __launch_bounds__(CL_BLOCK) void k_cl_edge_keys(const BhipClusterEdge *__restrict__ e, uint64_t m, const uint32_t *__restrict__ rank, u64 *__restrict__ key,
		uint32_t *__restrict__ val) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
		const BhipClusterEdge x = e[i];
		const uint32_t rq = rank[x.q], rr = rank[x.r];
		key[i] = x.q != x.r && rr < rq ? (u64)x.q << 32 | rr : ~0ull;
		val[i] = x.edits;
	}
}
// sorted keys: 1 for the first of every run of equal real keys
__global__ __launch_bounds__(CL_BLOCK) void k_cl_heads(const u64 *__restrict__ key, uint64_t m, uint32_t *__restrict__ flag) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
		const u64 k = key[i];
		flag[i] = k != ~0ull && (!i || key[i - 1] != k);
	}
}
// pos = the inclusive scan of flag: edge i belongs to distinct edge pos[i] - 1; e_ed was filled with ones
__global__ __launch_bounds__(CL_BLOCK) void k_cl_compact(const u64 *__restrict__ key, const uint32_t *__restrict__ val, const uint32_t *__restrict__ flag,
		const uint32_t *__restrict__ pos, uint64_t m, uint32_t *__restrict__ e_q, uint32_t *__restrict__ e_t, uint32_t *__restrict__ e_ed) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
		const u64 k = key[i];
		if (k == ~0ull) continue;
		const uint64_t o = (uint64_t)pos[i] - 1;
		if (flag[i]) { e_q[o] = (uint32_t)(k >> 32); e_t[o] = (uint32_t)k; }
		atomicMin(&e_ed[o], val[i]);
	}
}
// off[q] = the first distinct edge whose source is not below q (q = 0 .. n: off[n] = kept)
__global__ __launch_bounds__(CL_BLOCK) void k_cl_offsets(const uint32_t *__restrict__ e_q, uint64_t kept, uint64_t n, u64 *__restrict__ off) {
	for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q <= n; q += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t lo = 0, hi = kept;
		while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)e_q[mid] < q) lo = mid + 1; else hi = mid; }
		off[q] = lo;
	}
}
// the two work lists of the first round (and of the assignment): nodes by the length of their run
__global__ __launch_bounds__(CL_BLOCK) void k_cl_split(const u64 *__restrict__ off, uint64_t n, uint32_t *__restrict__ list_t, uint32_t *__restrict__ list_w,
		uint32_t *__restrict__ cnt /* [2] */) {
	for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < n; q += (uint64_t)gridDim.x * blockDim.x) {
		if (off[q + 1] - off[q] < CL_WAVE_MIN) list_t[atomicAdd(&cnt[0], 1u)] = (uint32_t)q;
		else list_w[atomicAdd(&cnt[1], 1u)] = (uint32_t)q;
	}
}

// one thread per undecided node with a short run
__global__ __launch_bounds__(CL_BLOCK) void k_cl_round_thread(const uint32_t *__restrict__ list, uint32_t n_list, const u64 *__restrict__ off, const uint32_t *__restrict__ e_t,
		const uint32_t *__restrict__ rank, uint32_t *state, uint32_t *__restrict__ next, uint32_t *__restrict__ cnt) {
	for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < n_list; k += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t q = list[k];
		const uint64_t a = off[q], b = off[q + 1];
		bool centroid = false, waiting = false;
		for (uint64_t i = a; i < b; ++i) {
			const uint32_t s = cl_state_load(&state[e_t[i]]);
			if (s == CL_CENTROID) { centroid = true; break; }
			waiting |= s == CL_UNDECIDED;
		}
		if (centroid) cl_state_store(&state[rank[q]], CL_MEMBER);
		else if (!waiting) cl_state_store(&state[rank[q]], CL_CENTROID);
		else next[atomicAdd(cnt, 1u)] = q;
	}
}
// one wave per undecided node with a long run
__global__ __launch_bounds__(CL_BLOCK) void k_cl_round_wave(const uint32_t *__restrict__ list, uint32_t n_list, const u64 *__restrict__ off, const uint32_t *__restrict__ e_t,
		const uint32_t *__restrict__ rank, uint32_t *state, uint32_t *__restrict__ next, uint32_t *__restrict__ cnt) {
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t waves = (uint64_t)gridDim.x * (CL_BLOCK / 64);
	for (uint64_t k = blockIdx.x * (uint64_t)(CL_BLOCK / 64) + (threadIdx.x >> 6); k < n_list; k += waves) {      // (k is wave-uniform)
		const uint32_t q = list[k];
		const uint64_t a = off[q], b = off[q + 1];
		bool centroid = false, waiting = false;
		for (uint64_t i0 = a; i0 < b; i0 += 64) {
			const uint64_t i = i0 + lane;
			const uint32_t s = i < b ? cl_state_load(&state[e_t[i]]) : (uint32_t)CL_MEMBER;
			if (__ballot(s == CL_CENTROID)) { centroid = true; break; }
			waiting |= __ballot(s == CL_UNDECIDED) != 0;
		}
		if (lane) continue;
		if (centroid) cl_state_store(&state[rank[q]], CL_MEMBER);
		else if (!waiting) cl_state_store(&state[rank[q]], CL_CENTROID);
		else next[atomicAdd(cnt, 1u)] = q;
	}
}

// every state is final: a member's centroid is the smallest (edits, rank) among its centroid targets
__global__ __launch_bounds__(CL_BLOCK) void k_cl_assign_thread(const uint32_t *__restrict__ list, uint32_t n_list, const u64 *__restrict__ off, const uint32_t *__restrict__ e_t,
		const uint32_t *__restrict__ e_ed, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ order, const uint32_t *__restrict__ state,
		uint32_t *__restrict__ centroid, uint32_t *__restrict__ edits) {
	for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < n_list; k += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t q = list[k];
		u64 best = ~0ull;
		if (state[rank[q]] == CL_MEMBER) {
			const uint64_t a = off[q], b = off[q + 1];
			for (uint64_t i = a; i < b; ++i) {
				const uint32_t t = e_t[i];
				if (state[t] == CL_CENTROID) { const u64 c = (u64)e_ed[i] << 32 | t; best = c < best ? c : best; }
			}
		}
		if (best == ~0ull) { centroid[q] = q; edits[q] = 0; }
		else { centroid[q] = order[(uint32_t)best]; edits[q] = (uint32_t)(best >> 32); }
	}
}
__global__ __launch_bounds__(CL_BLOCK) void k_cl_assign_wave(const uint32_t *__restrict__ list, uint32_t n_list, const u64 *__restrict__ off, const uint32_t *__restrict__ e_t,
		const uint32_t *__restrict__ e_ed, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ order, const uint32_t *__restrict__ state,
		uint32_t *__restrict__ centroid, uint32_t *__restrict__ edits) {
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t waves = (uint64_t)gridDim.x * (CL_BLOCK / 64);
	for (uint64_t k = blockIdx.x * (uint64_t)(CL_BLOCK / 64) + (threadIdx.x >> 6); k < n_list; k += waves) {
		const uint32_t q = list[k];
		u64 best = ~0ull;
		if (state[rank[q]] == CL_MEMBER) {
			const uint64_t a = off[q], b = off[q + 1];
			for (uint64_t i = a + lane; i < b; i += 64) {
				const uint32_t t = e_t[i];
				if (state[t] == CL_CENTROID) { const u64 c = (u64)e_ed[i] << 32 | t; best = c < best ? c : best; }
			}
		}
		for (int o = 32; o; o >>= 1) { const u64 x = __shfl_xor(best, o, 64); best = x < best ? x : best; }      // (every lane of the wave is here)
		if (lane) continue;
		if (best == ~0ull) { centroid[q] = q; edits[q] = 0; }
		else { centroid[q] = order[(uint32_t)best]; edits[q] = (uint32_t)(best >> 32); }
	}
}

struct ClusterState {
	DBuf w, edges, key, key_s, val, val_s, tmp, order, rank, state, flag, pos, e_q, e_t, e_ed, off, list0_t, list0_w, list_t[2], list_w[2], cnt, centroid, edits;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

// (bhip_handle.h: Handle::cluster)
void bhip_cluster_release(Handle *h) {
	ClusterState *st = (ClusterState *)h->cluster;
	if (!st) return;
	DBuf *all[] = {&st->w, &st->edges, &st->key, &st->key_s, &st->val, &st->val_s, &st->tmp, &st->order, &st->rank, &st->state, &st->flag, &st->pos, &st->e_q, &st->e_t,
	               &st->e_ed, &st->off, &st->list0_t, &st->list0_w, &st->list_t[0], &st->list_t[1], &st->list_w[0], &st->list_w[1], &st->cnt, &st->centroid, &st->edits};
	for (DBuf *x : all) x->release();
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->cluster = nullptr;
}

static inline uint32_t cl_grid(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + CL_BLOCK - 1) / CL_BLOCK, CL_MAX_GRID)); }
static inline uint32_t cl_grid_waves(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + CL_BLOCK / 64 - 1) / (CL_BLOCK / 64), CL_MAX_GRID)); }

extern "C" int bhip_cluster_run(void *handle, uint32_t n_nodes, const uint32_t *weights, const BhipClusterEdge *edges, uint64_t n_edges, uint32_t *centroid_out,
		uint32_t *edits_out) {
	Handle *h = (Handle *)handle;
	if (!h || (n_nodes && (!weights || !centroid_out || !edits_out)) || (n_edges && !edges)) return fail(BHIP_E_ARG, "bhip_cluster_run: null argument");
	if (n_nodes == 0xFFFFFFFFu || n_edges >= (1ull << 32)) return fail(BHIP_E_ARG, "bhip_cluster_run: %u nodes and %llu edges (fewer than 2^32 - 1 nodes, fewer than 2^32 edges)", n_nodes, (unsigned long long)n_edges);
	for (uint64_t i = 0; i < n_edges; ++i) if (edges[i].q >= n_nodes || edges[i].r >= n_nodes)
		return fail(BHIP_E_ARG, "bhip_cluster_run: edge %llu names node %u -> %u of %u", (unsigned long long)i, edges[i].q, edges[i].r, n_nodes);
	ClusterState *st = (ClusterState *)h->cluster;
	if (!n_edges) {      // (nothing to resolve: every read is a centroid, nothing is launched)
		for (uint32_t i = 0; i < n_nodes; ++i) { centroid_out[i] = i; edits_out[i] = 0; }
		memset(h->cluster_info, 0, sizeof h->cluster_info);
		h->cluster_info[2] = n_nodes; h->cluster_info[6] = n_nodes;
		return BHIP_OK;
	}
	HIPCHK(hipSetDevice(h->device));
	if (!st) {
		st = new ClusterState();
		h->cluster = st;
		if (hipEventCreate(&st->ev0) != hipSuccess || hipEventCreate(&st->ev1) != hipSuccess) { bhip_cluster_release(h); return fail(BHIP_E_DEVICE, "hipEventCreate failed"); }
	}
	memset(h->cluster_info, 0, sizeof h->cluster_info);
	const uint64_t n = n_nodes, m = n_edges, nm = std::max(n, m);
	int rc;
	#define CL_RESERVE(buf, bytes) do { rc = st->buf.reserve(bytes); if (rc) return rc; } while (0)
	CL_RESERVE(w, n * 4); CL_RESERVE(edges, m * sizeof(BhipClusterEdge));
	CL_RESERVE(key, nm * 8); CL_RESERVE(key_s, nm * 8); CL_RESERVE(val, m * 4); CL_RESERVE(val_s, m * 4);
	CL_RESERVE(order, n * 4); CL_RESERVE(rank, n * 4); CL_RESERVE(state, n * 4);
	CL_RESERVE(flag, m * 4); CL_RESERVE(pos, m * 4); CL_RESERVE(e_q, m * 4); CL_RESERVE(e_t, m * 4); CL_RESERVE(e_ed, m * 4);
	CL_RESERVE(off, (n + 1) * 8);
	CL_RESERVE(list0_t, n * 4); CL_RESERVE(list0_w, n * 4);
	for (int k = 0; k < 2; ++k) { CL_RESERVE(list_t[k], n * 4); CL_RESERVE(list_w[k], n * 4); }
	CL_RESERVE(cnt, 16); CL_RESERVE(centroid, n * 4); CL_RESERVE(edits, n * 4);
	u64 *key = st->key.as<u64>(), *key_s = st->key_s.as<u64>();
	uint32_t *val = st->val.as<uint32_t>(), *val_s = st->val_s.as<uint32_t>(), *flag = st->flag.as<uint32_t>(), *pos = st->pos.as<uint32_t>();
	size_t tb_rank = 0, tb_sort = 0, tb_scan = 0;
	HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb_rank, key, key_s, (size_t)n, 0, 64, h->stream));
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, key, key_s, val, val_s, (size_t)m, 0, 64, h->stream));
	HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tb_scan, flag, pos, (size_t)m, h->stream));
	CL_RESERVE(tmp, std::max(tb_rank, std::max(tb_sort, tb_scan)) + 16);
	#undef CL_RESERVE
	uint32_t *order = st->order.as<uint32_t>(), *rank = st->rank.as<uint32_t>(), *state = st->state.as<uint32_t>(), *cnt = st->cnt.as<uint32_t>();
	uint32_t *e_q = st->e_q.as<uint32_t>(), *e_t = st->e_t.as<uint32_t>(), *e_ed = st->e_ed.as<uint32_t>();
	u64 *off = st->off.as<u64>();

	HIPCHK(hipMemcpyAsync(st->w.p, weights, n * 4, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(st->edges.p, edges, m * sizeof(BhipClusterEdge), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipEventRecord(st->ev0, h->stream));
	// rank
	hipLaunchKernelGGL(k_cl_rank_keys, dim3(cl_grid(n)), dim3(CL_BLOCK), 0, h->stream, st->w.as<uint32_t>(), n, key);
	HIPCHK(hipGetLastError());
	size_t tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortKeys(st->tmp.p, tb, key, key_s, (size_t)n, 0, 64, h->stream));
	hipLaunchKernelGGL(k_cl_rank, dim3(cl_grid(n)), dim3(CL_BLOCK), 0, h->stream, key_s, n, order, rank, state);
	HIPCHK(hipGetLastError());
	// clean: the distinct edges towards earlier nodes, their smallest edits, the run offsets
	hipLaunchKernelGGL(k_cl_edge_keys, dim3(cl_grid(m)), dim3(CL_BLOCK), 0, h->stream, st->edges.as<BhipClusterEdge>(), m, rank, key, val);
	HIPCHK(hipGetLastError());
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, key, key_s, val, val_s, (size_t)m, 0, 64, h->stream));
	hipLaunchKernelGGL(k_cl_heads, dim3(cl_grid(m)), dim3(CL_BLOCK), 0, h->stream, key_s, m, flag);
	HIPCHK(hipGetLastError());
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::InclusiveSum(st->tmp.p, tb, flag, pos, (size_t)m, h->stream));
	uint32_t kept32 = 0;
	HIPCHK(hipMemcpyAsync(&kept32, pos + (m - 1), 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemsetAsync(e_ed, 0xFF, m * 4, h->stream));
	hipLaunchKernelGGL(k_cl_compact, dim3(cl_grid(m)), dim3(CL_BLOCK), 0, h->stream, key_s, val_s, flag, pos, m, e_q, e_t, e_ed);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(h->stream));
	const uint64_t kept = kept32;
	if (kept > m) return fail(BHIP_E_INTERNAL, "bhip_cluster_run: %llu distinct edges out of %llu", (unsigned long long)kept, (unsigned long long)m);
	hipLaunchKernelGGL(k_cl_offsets, dim3(cl_grid(n + 1)), dim3(CL_BLOCK), 0, h->stream, e_q, kept, n, off);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemsetAsync(cnt, 0, 16, h->stream));
	hipLaunchKernelGGL(k_cl_split, dim3(cl_grid(n)), dim3(CL_BLOCK), 0, h->stream, off, n, st->list0_t.as<uint32_t>(), st->list0_w.as<uint32_t>(), cnt);
	HIPCHK(hipGetLastError());
	uint32_t c[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(c, cnt, 8, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	const uint32_t n0_t = c[0], n0_w = c[1];
	if ((uint64_t)n0_t + n0_w != n) return fail(BHIP_E_INTERNAL, "bhip_cluster_run: %u + %u nodes listed out of %u", n0_t, n0_w, n_nodes);
	// rounds: the undecided nodes of each list walk their runs; the lists of those that wait come back with their lengths
	const uint32_t *cur_t = st->list0_t.as<uint32_t>(), *cur_w = st->list0_w.as<uint32_t>();
	uint32_t n_t = n0_t, n_w = n0_w;
	uint64_t rounds = 0;
	while ((uint64_t)n_t + n_w) {
		uint32_t *nx_t = st->list_t[rounds & 1].as<uint32_t>(), *nx_w = st->list_w[rounds & 1].as<uint32_t>();
		HIPCHK(hipMemsetAsync(cnt, 0, 8, h->stream));
		if (n_t) { hipLaunchKernelGGL(k_cl_round_thread, dim3(cl_grid(n_t)), dim3(CL_BLOCK), 0, h->stream, cur_t, n_t, off, e_t, rank, state, nx_t, cnt); HIPCHK(hipGetLastError()); }
		if (n_w) { hipLaunchKernelGGL(k_cl_round_wave, dim3(cl_grid_waves(n_w)), dim3(CL_BLOCK), 0, h->stream, cur_w, n_w, off, e_t, rank, state, nx_w, cnt + 1); HIPCHK(hipGetLastError()); }
		HIPCHK(hipMemcpyAsync(c, cnt, 8, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
		++rounds;
		if (c[0] > n_t || c[1] > n_w || (uint64_t)c[0] + c[1] == (uint64_t)n_t + n_w)      // (the first undecided node in priority order can always be decided)
			return fail(BHIP_E_INTERNAL, "bhip_cluster_run: round %llu decided no node (%u + %u undecided before, %u + %u after)", (unsigned long long)rounds, n_t, n_w, c[0], c[1]);
		cur_t = nx_t; cur_w = nx_w; n_t = c[0]; n_w = c[1];
	}
	// assign
	uint32_t *d_cen = st->centroid.as<uint32_t>(), *d_ed = st->edits.as<uint32_t>();
	if (n0_t) { hipLaunchKernelGGL(k_cl_assign_thread, dim3(cl_grid(n0_t)), dim3(CL_BLOCK), 0, h->stream, st->list0_t.as<uint32_t>(), n0_t, off, e_t, e_ed, rank, order, state, d_cen, d_ed); HIPCHK(hipGetLastError()); }
	if (n0_w) { hipLaunchKernelGGL(k_cl_assign_wave, dim3(cl_grid_waves(n0_w)), dim3(CL_BLOCK), 0, h->stream, st->list0_w.as<uint32_t>(), n0_w, off, e_t, e_ed, rank, order, state, d_cen, d_ed); HIPCHK(hipGetLastError()); }
	HIPCHK(hipEventRecord(st->ev1, h->stream));
	HIPCHK(hipMemcpyAsync(centroid_out, d_cen, n * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(edits_out, d_ed, n * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	uint64_t n_centroids = 0, bytes = 0;
	for (uint64_t i = 0; i < n; ++i) n_centroids += centroid_out[i] == (uint32_t)i;
	DBuf *all[] = {&st->w, &st->edges, &st->key, &st->key_s, &st->val, &st->val_s, &st->tmp, &st->order, &st->rank, &st->state, &st->flag, &st->pos, &st->e_q, &st->e_t,
	               &st->e_ed, &st->off, &st->list0_t, &st->list0_w, &st->list_t[0], &st->list_t[1], &st->list_w[0], &st->list_w[1], &st->cnt, &st->centroid, &st->edits};
	for (DBuf *x : all) bytes += x->cap;
	uint64_t *info = h->cluster_info;
	info[0] = rounds; info[1] = kept; info[2] = n_centroids; info[3] = (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	info[4] = bytes; info[5] = m; info[6] = n; info[7] = 0;
	return BHIP_OK;
}

extern "C" int bhip_cluster_info(void *handle, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	if (!h || !info) return fail(BHIP_E_ARG, "bhip_cluster_info: null argument");
	memcpy(info, h->cluster_info, sizeof h->cluster_info);
	return BHIP_OK;
}
