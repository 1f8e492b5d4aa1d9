// burst_amd/csrc/bhip_align.hip -- the alignment chain of a staged batch (include/burst_hip.h: bhip_align_staged, bhip_align_batch,
// bhip_reserve) and the kernel-level entry points (bhip_align_pairs, bhip_prefilter): what replaces the bodies of the two OpenMP
// loops of do_alignments (burst.c:4077-4289, 4343-4484).  HIP-event timing of every phase on the stream it runs on.
#include "bhip_handle.h"
#include "bhip_pf_select.h"

// ---- ordering of the output records: (q, refIx) ascending, done on the device.  A query has one or two records, rarely
// more, so a counting sort by query (rank inside the query from the counting atomic, offsets from one exclusive scan)
// followed by a tiny in-place sort of the few multi-record groups replaces a 7-pass radix sort of 64-bit keys ----
// (n_dev: the record count still lives on the device -- the sort is enqueued behind the re-scorer before the host has seen it)
__global__ void k_hit_count(const BhipHit *__restrict__ hits, uint32_t n, const uint32_t *__restrict__ n_dev, uint32_t *__restrict__ cnt, uint32_t *__restrict__ rank) {
	if (n_dev) n = *n_dev < n ? *n_dev : n;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) rank[i] = atomicAdd(&cnt[hits[i].q], 1u);
}
__global__ void k_hit_scatter(const BhipHit *__restrict__ in, uint32_t n, const uint32_t *__restrict__ n_dev, const uint32_t *__restrict__ off, const uint32_t *__restrict__ rank,
                              BhipHit *__restrict__ out, const uint32_t *__restrict__ qmap) {      // qmap: batch entry -> query number reported to the caller
	if (n_dev) n = *n_dev < n ? *n_dev : n;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		BhipHit h = in[i];
		const uint32_t dst = off[h.q] + rank[i];
		if (qmap) h.q = qmap[h.q];
		out[dst] = h;
	}
}
// Batches with query symbols of code 0 (see Handle::qcodes_s): the sweeps ran on the queries without those symbols; every
// such symbol costs exactly one edit more (it can only face a gap), so its count goes onto the raw hits and onto the
// running minima before the re-scorer -- which sees the original queries -- takes over.
__global__ void k_junk_adjust_raw(BhipRawHit *__restrict__ raw, const uint32_t *__restrict__ n_raw_dev, uint32_t raw_cap, const uint8_t *__restrict__ nx) {
	uint32_t n = *n_raw_dev;
	if (n > raw_cap) n = raw_cap;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { const uint32_t x = nx[raw[i].q]; raw[i].ed += x; raw[i].m += x; }
}
__global__ void k_junk_adjust_best(uint32_t *__restrict__ best, const uint8_t *__restrict__ nx_six, uint32_t s0, uint32_t s1) {
	for (uint32_t s = s0 + blockIdx.x * blockDim.x + threadIdx.x; s < s1; s += gridDim.x * blockDim.x)
		if (nx_six[s] && best[s] != 0xFFFFFFFFu) best[s] += nx_six[s];
}

// The records of a query, scattered in arrival order, into reference order.  Round 5: one WAVE per group that needs it, a rank sort --
// lane l holds record l, its place is the number of records of the group with a smaller reference number ((query, reference) pairs are
// unique) -- instead of one thread per query shell-sorting 20-byte records in global memory: with strain-level redundancy every read
// has twenty equally good references (and some hundreds), and a wave took as long as its longest query: 330 of a batch's 410 ms.
// Groups of up to 64 records are permuted through registers; larger ones go through `scratch` (a buffer of their own,
// same size, same offsets) 64 records at a time, each ranked against the whole group.
__global__ __launch_bounds__(256) void k_hit_fix(BhipHit *__restrict__ out, const uint32_t *__restrict__ off, const uint32_t *__restrict__ cnt, uint32_t n_q,
                                               BhipHit *__restrict__ scratch, uint32_t scratch_cap) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
	struct Rec { uint32_t w[5]; };
	static_assert(sizeof(BhipHit) == 20, "BhipHit is five dwords");
	for (uint32_t q0 = wave * 64u; q0 < n_q; q0 += n_waves * 64u) {
		const uint32_t q = q0 + lane;
		const uint32_t n_mine = q < n_q ? cnt[q] : 0u, o_mine = q < n_q ? off[q] : 0u;
		unsigned long long todo = __ballot(n_mine >= 2u);
		while (todo) {
			const int b = __builtin_ctzll(todo);
			todo &= todo - 1ull;
			const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)n_mine, b), o = (uint32_t)__builtin_amdgcn_readlane((int)o_mine, b);
			Rec *grp = (Rec *)(out + o);
			if (n <= 64u) {
				Rec r = {};
				if (lane < n) r = grp[lane];
				const uint32_t key = lane < n ? r.w[1] : 0xFFFFFFFFu;          // refIx
				uint32_t rank = 0;
				// (stable: equal keys -- which the (query, reference) uniqueness of the records rules out -- would keep their order instead of colliding)
				for (uint32_t j = 0; j < n; ++j) { const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)j); rank += (kj < key || (kj == key && j < lane)) ? 1u : 0u; }
				if (lane < n) grp[rank] = r;                                   // (every lane's load is complete before the first store: the rank depends on all keys)
			} else if ((uint64_t)o + n <= scratch_cap) {
				Rec *tmp = (Rec *)(scratch + o);
				for (uint32_t i = lane; i < n; i += 64u) tmp[i] = grp[i];
				__threadfence();
				for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
					const uint32_t i = i0 + lane;
					Rec r = {};
					if (i < n) r = tmp[i];
					const uint32_t key = i < n ? r.w[1] : 0xFFFFFFFFu;
					uint32_t rank = 0;
					for (uint32_t j0 = 0; j0 < n; j0 += 64u) {
						const uint32_t kj = j0 + lane < n ? tmp[j0 + lane].w[1] : 0xFFFFFFFFu;
						const uint32_t m = n - j0 < 64u ? n - j0 : 64u;
						for (uint32_t j = 0; j < m; ++j) { const uint32_t kk = (uint32_t)__builtin_amdgcn_readlane((int)kj, (int)j); rank += (kk < key || (kk == key && j0 + j < i)) ? 1u : 0u; }
					}
					if (i < n) grp[rank] = r;
				}
			} else if (lane == 0) {                                            // (no scratch of that size: the serial sort)
				BhipHit *a = out + o;
				uint32_t gap = 1;
				while (gap < n / 3) gap = 3 * gap + 1;
				for (; gap >= 1; gap /= 3)
					for (uint32_t i = gap; i < n; ++i) {
						const BhipHit v = a[i];
						uint32_t j = i;
						for (; j >= gap && a[j - gap].refIx > v.refIx; j -= gap) a[j] = a[j - gap];
						a[j] = v;
					}
			}
		}
	}
}
__global__ void k_set_rank_ptrs(SharedCtr *sc, uint32_t *cnt, uint32_t *rank) { sc->cnt = cnt; sc->rank = rank; }

// ---- BEST on the device (all_hits = BHIP_HITS_BEST) ----------------------------------------------------------------
// The reference's BEST keeps, of a query's hits, the one with the fewest edits, then the higher f32 identity, then the lower original
// reference number RefIxSrt[refIx] (burst.c:4847-4891).  With the minimum-only semantics every record of an entry carries the same edit
// distance (k_rescore_classify lets ed == best[six] through and nothing else), so the choice inside an ENTRY is the minimum of the 64-bit
// key (~score bits, order[refIx]) -- scores are non-negative floats, their bit patterns order like their values; (entry, refIx) pairs
// are unique, so no two records of an entry share a key.  With strain-level redundancy a read has twenty equally good references:
// one record per entry leaves the device instead of all of them, and the counting sort of the records (a scatter of 20-byte records
// and a rank sort per group) is replaced by two streaming passes.  The choice between the two strands of a query (one entry each)
// stays with the host's consolidation, which knows the list order the reference would have met them in.
__device__ __forceinline__ unsigned long long best_key_of(const BhipHit &h, const uint32_t *__restrict__ order) {
	return (unsigned long long)(~__float_as_uint(h.score)) << 32 | order[h.refIx];
}
// (an entry with ONE record -- the rule on a low-redundancy database -- has nothing to choose: no table look-up, no atomic, for it)
__global__ void k_best_key(const BhipHit *__restrict__ hits, uint32_t n, const uint32_t *__restrict__ n_dev, const uint32_t *__restrict__ order, const uint32_t *__restrict__ cnt,
                           unsigned long long *__restrict__ key) {
	if (n_dev) n = *n_dev < n ? *n_dev : n;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const BhipHit h = hits[i];
		if (cnt[h.q] > 1u) atomicMin(&key[h.q], best_key_of(h, order));
	}
}
__global__ void k_best_flag(const uint32_t *__restrict__ cnt, uint32_t n_q, uint32_t *__restrict__ flag) {      // records per entry -> 1 where the entry has any (flag[n_q] = 0: the scan's total)
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n_q; i += gridDim.x * blockDim.x) flag[i] = i < n_q && cnt[i] ? 1u : 0u;
}
__global__ void k_best_emit(const BhipHit *__restrict__ hits, uint32_t n, const uint32_t *__restrict__ n_dev, const uint32_t *__restrict__ order, const uint32_t *__restrict__ cnt,
                            const unsigned long long *__restrict__ key, const uint32_t *__restrict__ off, BhipHit *__restrict__ out, const uint32_t *__restrict__ qmap) {
	if (n_dev) n = *n_dev < n ? *n_dev : n;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		BhipHit h = hits[i];
		if (cnt[h.q] > 1u && best_key_of(h, order) != key[h.q]) continue;
		const uint32_t dst = off[h.q];
		if (qmap) h.q = qmap[h.q];
		out[dst] = h;
	}
}
extern "C" int bhip_set_ref_order(void *handle, const uint32_t *order, uint32_t n) {
	Handle *h = (Handle *)handle;
	if (!h) return fail(BHIP_E_ARG, "null handle");
	if (!order) return h->n_order ? 1 : 0;
	if (n < h->tot_refs) return fail(BHIP_E_ARG, "reference order table holds %u entries, the database has %u references", n, h->tot_refs);
	HIPCHK(hipSetDevice(h->device));
	int rc;
	h->n_order = 0;
	if ((rc = h->ref_order.reserve((size_t)h->tot_refs * 4 + 16))) return rc;
	HIPCHK(hipMemcpy(h->ref_order.p, order, (size_t)h->tot_refs * 4, hipMemcpyHostToDevice));
	h->n_order = h->tot_refs;
	return BHIP_OK;
}

// ---- kernel launch helpers (st = stream to launch on) ---------------------------------------------------------------
// A run-time word count as a template argument.  dispatch_int: f(std::integral_constant<int, N>) for the N of the list that equals v, for
// the last N of the list when none does (the widest kernel takes the rest); for_each_int: f for every N, in list order.  One list per
// template parameter: exactly the instances bhip_kernels.hip and bhip_prefilter.hip define.
template <int... Ns> struct IntList {};
using NwList = IntList<2, 4, 6, 8, 10, 16, 32>;      // k_myers<NW>, k_myers_window<NW>: words of the query vector
using NwpList = IntList<1, 2, 3, 4, 6>;              // k_myers_prefix<NWP>, k_myers_prefix_task<NWP>: words of the prefix
using BwList = IntList<2, 3, 4>;                     // k_myers_window_band<BW>: words of the band
using HtbList = IntList<9, 10, 11>;                  // k_prefilter_mask<HTB>: log2 of the hash table
// k_rescore_reg<SET>, in launch order.  3 = 12 diagonals: a kernel of its own, so that the 4 / 6 / 8 variants run at 80 registers (6 waves per
// SIMD instead of 4); 2 = 32 / 40 / 48 diagonals (usually empty lists: large budgets, or repeats that stretch the end-column range)
using SetList = IntList<0, 3, 1, 2>;
template <int N, class F> static void dispatch_int(IntList<N>, int, F &&f) { f(std::integral_constant<int, N>{}); }
template <int N, int M, int... Ns, class F> static void dispatch_int(IntList<N, M, Ns...>, int v, F &&f) {
	if (v == N) f(std::integral_constant<int, N>{}); else dispatch_int(IntList<M, Ns...>{}, v, f);
}
template <int... Ns, class F> static void for_each_int(IntList<Ns...>, F &&f) { (f(std::integral_constant<int, Ns>{}), ...); }

// argument groups many launches share: shared-slot numbers and strand flags of the current batch (null: it has none), the reference arrays
static const uint32_t *six_or_null(const Handle *h) { return h->cur->st_has_six ? h->cur->qsix.as<uint32_t>() : nullptr; }
static const uint8_t *rc_or_null(const Handle *h) { return h->cur->st_has_rc ? h->cur->qrc.as<uint8_t>() : nullptr; }
struct RefArgs {
	const void *lanes; const uint64_t *off; const uint32_t *len;      // ref_lane, ref_off, clump_len
	const uint4 *chunks() const { return (const uint4 *)lanes; }      // as the sweeps read them: 16-byte chunks of 32 columns
	const uint8_t *bytes() const { return (const uint8_t *)lanes; }   // as the re-scorers do
};
static RefArgs ref_args(const Handle *h) { return {h->ref_lane.p, h->ref_off.as<uint64_t>(), h->clump_len.as<uint32_t>()}; }

static void launch_myers(Handle *h, Lane *L, hipStream_t st, int NW, uint32_t grid, const uint2 *pairs, const uint32_t *n_pairs_dev,
		uint64_t n_pairs_host, uint32_t li_base, const uint32_t *qlist, BhipRawHit *raw, uint32_t *n_raw, uint32_t raw_cap, uint32_t *best,
		uint8_t *mins, Counters *dc) {
	const RefArgs R = ref_args(h);
	const uint32_t *six = best ? six_or_null(h) : nullptr;
	if (NW > 32) {      // queries beyond 1 024 symbols: the vector lives in LDS (2 x NW words per thread, one wave per block)
		hipLaunchKernelGGL(k_myers_long, dim3(grid * 4u), dim3(64), (size_t)NW * 512u, st, pairs, n_pairs_dev, n_pairs_host, h->n_clumps, li_base, qlist,
			L->peq.as<uint32_t>(), h->s_off(), h->s_emac(), six, R.chunks(), R.off, R.len, h->tot_refs, raw, n_raw, raw_cap, best, mins, &dc->col_sum, &dc->qlen_sum, (uint32_t)NW);
		return;
	}
	dispatch_int(NwList{}, NW, [&](auto nw) {
		hipLaunchKernelGGL(k_myers<decltype(nw)::value>, dim3(grid), dim3(256), 0, st, pairs, n_pairs_dev, n_pairs_host, h->n_clumps, li_base, qlist,
			L->peq.as<uint32_t>(), h->s_off(), h->s_emac(), six, R.chunks(), R.off, R.len, h->tot_refs, raw, n_raw, raw_cap, best, mins, &dc->col_sum, &dc->qlen_sum);
	});
}
static void launch_prefix(Handle *h, Lane *L, hipStream_t st, int NWP, uint32_t grid, const uint2 *pairs, const uint32_t *n_pairs_dev,
		uint64_t n_pairs_host, uint32_t li_base, const uint32_t *qlist, uint32_t *n_wins, Counters *dc) {
	const RefArgs R = ref_args(h);
	dispatch_int(NwpList{}, NWP, [&](auto nwp) {
		hipLaunchKernelGGL(k_myers_prefix<decltype(nwp)::value>, dim3(grid), dim3(256), 0, st, pairs, n_pairs_dev, n_pairs_host, h->n_clumps, li_base, qlist,
			L->peqp.as<uint32_t>(), h->s_off(), h->s_emac(), R.chunks(), R.off, R.len, h->tot_refs, L->wins.as<BhipWin>(), n_wins, (uint32_t)L->win_cap,
			&dc->col_sum, &dc->qlen_sum, dc->win_class_seen, six_or_null(h));
	});
}
static void launch_prefix_task(Handle *h, Lane *L, hipStream_t st, int NWP, uint32_t grid, const uint2 *tasks, const uint32_t *n_tasks_dev, const uint32_t *qlist,
		BhipWin *wins, uint32_t *n_wins, Counters *dc, const uint4 *qmeta) {
	const RefArgs R = ref_args(h);
	dispatch_int(NwpList{}, NWP, [&](auto nwp) {
		hipLaunchKernelGGL(k_myers_prefix_task<decltype(nwp)::value>, dim3(grid), dim3(64), 0, st, tasks, n_tasks_dev, (uint32_t)L->task_cap, qlist,
			L->peqp.as<uint32_t>(), h->s_off(), h->s_emac(), R.chunks(), R.off, R.len, wins, n_wins, (uint32_t)L->win_cap, &dc->tcol_sum, dc->win_class_seen, qmeta, six_or_null(h));
	});
}
// Resident blocks per CU of a kernel from its static register / LDS use (512 VGPRs per SIMD lane granted in steps of 8, at
// most 8 waves per SIMD; about 148 KB of the 160 KB of LDS -- measured on gfx950: 11 single-wave blocks of 13 144 B fit a CU and 12 do
// not, 10 of 14 168 B fit and 11 do not): the persistent grid-stride kernels are launched with exactly that many blocks, a block that
// has to wait for a free slot would run its whole share after the others.  fa_out: what the runtime said about the kernel.
static uint32_t blocks_per_cu(const void *fn, uint32_t threads, size_t dyn_lds, hipFuncAttributes *fa_out = nullptr) {
	hipFuncAttributes fa_here, &fa = fa_out ? *fa_out : fa_here;
	memset(&fa, 0, sizeof fa);
	if (hipFuncGetAttributes(&fa, fn) != hipSuccess) return 4;
	return bhip_resident_blocks(threads, {fa.numRegs, fa.sharedSizeBytes}, dyn_lds);      // (the arithmetic: bhip_fetch_plan.h)
}
// registers and static LDS of a kernel, asked once per kernel (bhip_fetch_plan.h plans with them at every launch); {0, 0}: the runtime does not say
template <auto FN> static BhipKernelRes kernel_res() {      // (one instance, and one cached answer, per kernel)
	static const BhipKernelRes res = [] { hipFuncAttributes fa; memset(&fa, 0, sizeof fa);
		return hipFuncGetAttributes(&fa, (const void *)FN) == hipSuccess ? BhipKernelRes{fa.numRegs, fa.sharedSizeBytes} : BhipKernelRes{0, 0}; }();
	return res;
}

static void launch_window(Handle *h, Lane *L, hipStream_t wst, int cls, int NWP, uint32_t grid_cap, const BhipWin *wins, const uint32_t *n_wins, Counters *dc) {
	const uint32_t *six = six_or_null(h);
	const uint4 *ref = ref_args(h).chunks();
	const int NWc = kClasses[cls];
	// the windows whose flagged diagonals fit a band of 2, 3 or 4 words (class 0 .. 2 in the record, set by the prefix kernels) go to
	// k_myers_window_band<2 .. 4> where the query has more words than that; the full-column kernel takes the rest
	const int min_class = h->opt_no_band ? 0 : NWc >= 8 ? 3 : NWc >= 6 ? 2 : NWc >= 4 ? 1 : 0;
	for_each_int(BwList{}, [&](auto bw) {
		constexpr int BW = decltype(bw)::value;
		if (min_class < BW - 1) return;
		uint32_t per_cu = blocks_per_cu((const void *)k_myers_window_band<BW>, 64u, 0);
		if (h->opt_band_blocks > 0) per_cu = (uint32_t)h->opt_band_blocks;
		const uint32_t grid = (uint32_t)h->n_cu * per_cu * (uint32_t)h->opt_oversub;
		hipLaunchKernelGGL(k_myers_window_band<BW>, dim3(grid), dim3(64), 0, wst, wins, n_wins, (uint32_t)L->win_cap, NWP, NWc, L->peq.as<uint32_t>(), six,
			ref, L->raw.as<BhipRawHit>(), &dc->n_raw, (uint32_t)L->raw_cap, h->best.as<uint32_t>(), &dc->wcol_sum, dc->win_class_seen);
	});
	dispatch_int(NwList{}, NWc, [&](auto nw) {
		constexpr int N = decltype(nw)::value;
		const uint32_t thr = N <= 8 ? 64u : 256u;      // NW <= 8: per-thread A/C/G/T profile rows in LDS, 64-thread blocks
		const uint32_t grid = std::min<uint32_t>(grid_cap * (256u / thr), (uint32_t)h->n_cu * blocks_per_cu((const void *)k_myers_window<N>, thr, 0));
		hipLaunchKernelGGL(k_myers_window<N>, dim3(grid), dim3(thr), 0, wst, wins, n_wins, (uint32_t)L->win_cap, NWP, min_class, L->peq.as<uint32_t>(), six,
			ref, L->raw.as<BhipRawHit>(), &dc->n_raw, (uint32_t)L->raw_cap, h->best.as<uint32_t>(), &dc->wcol_sum, dc->win_class_seen);
	});
}


static int upload_queries(Handle *h, const uint8_t *q_codes, const uint64_t *q_off, const uint16_t *q_emac,
                          const uint32_t *q_six, const uint8_t *q_rc, uint32_t n_q) {
	const uint64_t nb = q_off[n_q];
	int rc;
	h->cur->st_has_junk = false;      // bhip_stage_queries builds the search view after this upload when the batch needs one
	h->cur->st_maxlen = 0; h->cur->st_maxE = 0;
	for (uint32_t i = 0; i < n_q; ++i) {
		h->cur->st_maxlen = std::max<uint32_t>(h->cur->st_maxlen, (uint32_t)(q_off[i + 1] - q_off[i]));
		h->cur->st_maxE = std::max<uint32_t>(h->cur->st_maxE, q_emac[i]);
	}
	if ((rc = h->cur->qcodes.reserve(nb + 16))) return rc;
	if ((rc = h->cur->qoff.reserve((n_q + 1) * sizeof(uint64_t)))) return rc;
	if ((rc = h->cur->qemac.reserve((n_q + 1) * sizeof(uint16_t)))) return rc;
	if ((rc = h->cur->qsix.reserve((n_q + 1) * sizeof(uint32_t)))) return rc;
	if ((rc = h->cur->qrc.reserve(n_q + 1))) return rc;
	HIPCHK(hipMemcpyAsync(h->cur->qcodes.p, q_codes, nb, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->cur->qoff.p, q_off, (n_q + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->cur->qemac.p, q_emac, n_q * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
	if (q_six) HIPCHK(hipMemcpyAsync(h->cur->qsix.p, q_six, n_q * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
	if (q_rc) HIPCHK(hipMemcpyAsync(h->cur->qrc.p, q_rc, n_q, hipMemcpyHostToDevice, h->stream));
	return 0;
}

static int upload_plan(Handle *h, uint32_t n_q, std::vector<uint32_t> &plan) {
	int rc;
	if ((rc = h->cur->plan.reserve((size_t)n_q * 4 + 16))) return rc;
	HIPCHK(hipMemcpyAsync(h->cur->plan.p, plan.data(), (size_t)n_q * 4, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	return 0;
}

// The overflow lists of a lane's prefilter: the list positions of the queries whose tables overflowed a pass, and how many.  Both prefilters
// of a lane (clump-level: launch_prefilter; lane-resolved: launch_prefilter_mask) keep them in L->fb_list and count them in Counters::n_fb /
// n_fb2, class after class.  INVARIANT: a second pass and the dense fallback only ever read the list and the counter that the first pass of
// the SAME class wrote.  (Round 6's fuzzer under BHIP_POISON met a second pass that took the list positions of a 2-word class, counted by
// the clump-level prefilter in n_fb, for those of the 4-word class behind it.)  So the counters are zero when a class begins -- by
// enqueue_lane's reset of the whole counter block for the lane's first lane-resolved launch of a call, by a memset here otherwise; an
// unconditional memset would be one more stream operation in front of every prefilter of the headline chain.
struct PfOverflow {
	uint32_t *fb1 = nullptr, *n_fb1 = nullptr;      // queries that overflowed the first pass
	uint32_t *fb2 = nullptr, *n_fb2 = nullptr;      // ... and the second (lane-resolved prefilter only)
	int begin(Lane *L, Counters *dc, hipStream_t st, uint32_t n_list, bool lane_resolved) {
		int rc;
		if ((rc = L->fb_list.reserve(lane_resolved ? (size_t)n_list * 8 + 64 : (size_t)n_list * 4 + 16))) return rc;
		fb1 = L->fb_list.as<uint32_t>(); n_fb1 = &dc->n_fb;
		if (lane_resolved) {
			fb2 = fb1 + n_list + 8; n_fb2 = &dc->n_fb2;
			if (L->pf_launches || L->fb_dirty) HIPCHK(hipMemsetAsync(&dc->n_fb, 0, 8, st));      // (n_fb, n_fb2)
			L->fb_dirty = false;
		} else {
			HIPCHK(hipMemsetAsync(&dc->n_fb, 0, 4, st));
			L->fb_dirty = true;      // (a later lane-resolved class of this lane must not find this count)
		}
		return 0;
	}
};

// fallback pass for the (rare) queries of the overflow list `fb` (*n_fb of them): dense per-clump counters, LDS if they fit, else global
// memory; (list position, clump) pairs into `cand`.  12 ms per launch at 6.8 M clumps whatever the number of queries.
static int launch_dense_fallback(Handle *h, Lane *L, hipStream_t st, const uint32_t *d_qlist, uint32_t n_list, const uint32_t *bad, uint32_t n_bad,
                                 uint2 *cand, uint32_t *candcnt, uint32_t *n_cand_dev, uint32_t cand_cap, Counters *dc, const uint32_t *fb, const uint32_t *n_fb) {
	const uint32_t *plan = h->cur->plan.as<uint32_t>();
	const bool narrow = h->cur->st_maxlen < 255u + (uint32_t)h->K;
	const size_t lds_w = ((size_t)(h->n_clumps + (narrow ? 3 : 1)) / (narrow ? 4 : 2)) * 4 + 1536u * 4 + 512u * 8 + 512u * 4 + 16;
	const uint32_t nw32 = (h->n_clumps + 1) / 2;
	if (lds_w <= 64 * 1024) {
		const uint32_t per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(16, (160 * 1024) / lds_w));
		const uint32_t grid = std::min<uint32_t>(n_list, (uint32_t)h->n_cu * per_cu);
		if (narrow) hipLaunchKernelGGL(k_prefilter_wave<uint8_t>, dim3(grid), dim3(64), lds_w, st, h->s_codes(), h->s_off(),
			h->s_emac(), d_qlist, n_list, h->acx_view(), h->K, h->n_clumps, bad, n_bad, cand, candcnt,
			n_cand_dev, cand_cap, &dc->ent_read, plan, fb, n_fb);
		else hipLaunchKernelGGL(k_prefilter_wave<uint16_t>, dim3(grid), dim3(64), lds_w, st, h->s_codes(), h->s_off(),
			h->s_emac(), d_qlist, n_list, h->acx_view(), h->K, h->n_clumps, bad, n_bad, cand, candcnt,
			n_cand_dev, cand_cap, &dc->ent_read, plan, fb, n_fb);
	} else {
		// dense counters in global memory, one workgroup per query (very large databases only)
		int rc;
		const uint32_t grid = std::min<uint32_t>(n_list, (uint32_t)h->n_cu * 2);
		if ((rc = L->gcnt.reserve((size_t)grid * nw32 * 4))) return rc;
		hipLaunchKernelGGL(k_prefilter<false>, dim3(grid), dim3(256), 0, st, h->s_codes(), h->s_off(),
			h->s_emac(), d_qlist, n_list, h->acx_view(), h->K, h->n_clumps,
			L->gcnt.as<uint32_t>(), bad, n_bad, cand, candcnt, n_cand_dev, cand_cap, &dc->ent_read, fb, n_fb, plan);
	}
	HIPCHK(hipGetLastError());
	return 0;
}

// clump-level prefilter of list positions [0, n_list) of `d_qlist` on the lane's stream
static int launch_prefilter(Handle *h, Lane *L, hipStream_t st, const uint32_t *d_qlist, uint32_t n_list, uint2 *cand, uint32_t *candcnt, uint32_t cand_cap,
                            bool with_bad, uint32_t *n_cand_dev, Counters *dc) {
	const uint32_t *bad = with_bad ? h->bad.as<uint32_t>() : nullptr;
	const uint32_t n_bad = with_bad ? h->n_bad : 0;
	int rc;
	PfOverflow ov;
	if ((rc = ov.begin(L, dc, st, n_list, false))) return rc;
	{	// main pass: hashed counters, four queries per wave (any database size)
		const uint32_t n_quads = (n_list + 3) / 4;
		const uint32_t grid = std::min<uint32_t>(n_quads, (uint32_t)h->n_cu * 6);
		hipLaunchKernelGGL(k_prefilter_hash, dim3(grid), dim3(64), 0, st, h->s_codes(), h->s_off(), h->s_emac(),
			d_qlist, n_list, h->acx_view(), h->K, bad, n_bad, cand, candcnt, n_cand_dev, cand_cap, &dc->ent_read,
			h->cur->plan.as<uint32_t>(), ov.fb1, ov.n_fb1);
		HIPCHK(hipGetLastError());
	}
	return launch_dense_fallback(h, L, st, d_qlist, n_list, bad, n_bad, cand, candcnt, n_cand_dev, cand_cap, dc, ov.fb1, ov.n_fb1);
}

// words per query row of the range table (8 when no query of the class samples more)
static uint32_t seed_row_words(uint32_t maxwords) { return maxwords <= 8 ? 8u : std::max<uint32_t>(16u, (maxwords + 15u) & ~15u); }
// prefix words of the two-stage sweep for a class (0 = one-stage sweep): about 6 prefix symbols per allowed edit, shorter than the query vector
static int class_prefix_words(const Handle *h, uint32_t maxE, int NW) {
	if (!h->opt_two_stage || NW > 32) return 0;      // (beyond 1 024 symbols: single stage, k_myers_long)
	const uint32_t want = (6 * maxE + 31) / 32;
	int NWP = want <= 1 ? 1 : (want <= 2 ? 2 : (want <= 3 ? 3 : (want <= 4 ? 4 : (want <= 6 ? 6 : 0))));
	if (NWP >= NW) NWP = 0;
	return NWP;
}
// match profiles (k_build_peq) of one (lane, class) list of staged batch S: full-length rows into `peq`, prefix rows into `peqp`
static int launch_peq(Handle *h, hipStream_t st, StageSlot *S, const uint32_t *d_qlist, uint32_t n_list, int NW, int NWP, DBuf &peq, DBuf &peqp, uint32_t blocks_per_cu = 16) {
	int rc;
	if ((rc = peq.reserve((size_t)n_list * 16 * NW * 4))) return rc;
	if ((rc = peqp.reserve((size_t)n_list * 16 * 6 * 4))) return rc;
	const bool junk = S->st_has_junk;
	const uint8_t *codes = junk ? S->qcodes_s.as<uint8_t>() : S->qcodes.as<uint8_t>();
	const uint64_t *off = junk ? S->qoff_s.as<uint64_t>() : S->qoff.as<uint64_t>();
	const uint32_t *pack = junk ? S->qpack_s.as<uint32_t>() : S->qpack.as<uint32_t>();
	{
		const uint32_t qb = 256u / (uint32_t)NW;
		const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n_list + qb - 1) / qb, (uint64_t)h->n_cu * blocks_per_cu);
		hipLaunchKernelGGL(k_build_peq, dim3(grid), dim3(256), 0, st, codes, off, d_qlist, n_list, NW, 0, h->mm, peq.as<uint32_t>(), pack, (S->st_maxlen + 7) / 8, h->peq_rows);
		HIPCHK(hipGetLastError());
	}
	if (NWP) {
		const uint32_t qb = 256u / (uint32_t)NWP;
		const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n_list + qb - 1) / qb, (uint64_t)h->n_cu * blocks_per_cu);
		hipLaunchKernelGGL(k_build_peq, dim3(grid), dim3(256), 0, st, codes, off, d_qlist, n_list, NWP, 32 * NWP, h->mm, peqp.as<uint32_t>(), pack, (S->st_maxlen + 7) / 8, h->peq_rows);
		HIPCHK(hipGetLastError());
	}
	return 0;
}
// whether k_seed_ranges leaves out a query's longest list: the rule, and what was measured, in bhip_pf_select.h
static uint32_t seed_min_need_for(const Handle *h, double mean_words, uint32_t W16) {
	return bhip_seed_min_need(h->opt_seed_min_need, h->opt_pf_cw, h->opt_pf_table, h->opt_pf_bytes, h->acx_wmean, mean_words, W16);
}
// k_seed_ranges for one (lane, class) list of staged batch S into the lane's per-class buffers
static int launch_seed(Handle *h, Lane *L, hipStream_t st, StageSlot *S, int cls, const uint32_t *d_qlist, uint32_t n_list, uint32_t maxwords, double mean_words, bool ahead = false) {
	int rc;
	const uint32_t W16 = seed_row_words(maxwords);
	L->seeded_ok[cls] = false;
	if ((rc = L->ranges_c[cls].reserve((size_t)n_list * W16 * 8 + 16))) return rc;
	if ((rc = L->hdr_c[cls].reserve((size_t)n_list * 8 + 16))) return rc;
	DBuf &qm = L->qmeta_c[S->seq & 1][cls];
	if ((rc = qm.reserve((size_t)n_list * 16 + 16))) return rc;
	L->qmeta_seq[S->seq & 1][cls] = 0;
	const uint64_t n_thr = (uint64_t)n_list * W16;
	hipEvent_t *ev = L->ev_seed[S->seq & 1][cls];
	const bool junk = S->st_has_junk;
	HIPCHK(hipEventRecord(ev[SPAN_START], st));
	// ahead of its batch the kernel shares the device with the sweeps of the batch before: a few blocks per CU leave them their
	// wave slots (option "seed_ahead_blocks"), and it still ends long before it is needed
	const uint64_t full = (n_thr + 255) / 256;
	const uint32_t grid = (uint32_t)(ahead && h->opt_seed_ahead_blocks > 0 ? std::min<uint64_t>(full, (uint64_t)h->n_cu * (uint64_t)h->opt_seed_ahead_blocks) : full);
	hipLaunchKernelGGL(k_seed_ranges, dim3(grid), dim3(256), 0, st,
		junk ? S->qcodes_s.as<uint8_t>() : S->qcodes.as<uint8_t>(), junk ? S->qoff_s.as<uint64_t>() : S->qoff.as<uint64_t>(), d_qlist, n_list,
		h->acx_view(), h->K, S->plan.as<uint32_t>(), W16, L->ranges_c[cls].as<uint2>(), L->hdr_c[cls].as<uint2>(),
		junk ? S->qpack_s.as<uint32_t>() : S->qpack.as<uint32_t>(), (S->st_maxlen + 7) / 8, junk ? S->qemac_s.as<uint16_t>() : S->qemac.as<uint16_t>(), qm.as<uint4>(), S->st_has_six ? S->qsix.as<uint32_t>() : nullptr,
		seed_min_need_for(h, mean_words, W16), (uint32_t)h->opt_seed_drop_len, h->alt);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(ev[SPAN_DONE], st));
	L->qmeta_seq[S->seq & 1][cls] = S->seq + 1;
	L->seeded_ok[cls] = true; L->seeded_seq[cls] = S->seq; L->seeded_n[cls] = n_list; L->seeded_W16[cls] = W16;
	return 0;
}

// the counting-filter kernel of a choice (bhip_pf_select.h), first pass (big = 0) or second pass over the queries that overflowed it
// (big = 1: the largest tables); gw: lanes per query of the first pass (bhip_pf_group: 8 only for k_prefilter_cq in slot mode 0); null: a
// superseded kernel and no test-only library in the process
static bhip_pf_kernel_t pf_kernel(const BhipPfChoice &c, int big, int gw = 16) {
	if (c.legacy) return bhip_legacy_pf_kernel ? bhip_legacy_pf_kernel(c.kind, big ? 11 : c.htb, big ? 4 : c.rb, c.cw_mode, big) : nullptr;
	if (c.kind == BHIP_PF_CQ) return c.cw_mode == 0 ? (big ? k_prefilter_cq<0, 1, 16> : gw == 8 ? k_prefilter_cq<0, 0, 8> : k_prefilter_cq<0, 0, 16>) : (big ? k_prefilter_cq<1, 1, 16> : k_prefilter_cq<1, 0, 16>);
	return big ? k_prefilter_cw<2, 1> : k_prefilter_cw<2, 0>;      // plans beyond 16 lists per query: one query per wave
}

// lane-resolved prefilter of a class (algo: bhip_pf_algo): tasks (list position, reference lane) into L->tasks; the queries that overflow its
// tables go through the dense clump-level kernels into L->cand as (list position, clump) pairs
static int launch_prefilter_mask(Handle *h, Lane *L, hipStream_t st, int cls, const uint32_t *d_qlist, uint32_t n_list, uint32_t maxwords, uint32_t *n_tasks_dev,
                                 uint32_t *n_cand_dev, Counters *dc, int algo, int prune) {
	int rc;
	PfOverflow ov;
	if ((rc = ov.begin(L, dc, st, n_list, true))) return rc;
	const uint32_t W16 = seed_row_words(maxwords);
	const double mean_words = n_list ? (double)L->seed_words[cls] / (double)n_list : (double)maxwords;
	// the lookups of this batch may have run ahead (seed_next_batch, during the previous call)
	if (!(L->seeded_ok[cls] && L->seeded_seq[cls] == h->cur->seq && L->seeded_n[cls] == n_list && L->seeded_W16[cls] == W16))
		if ((rc = launch_seed(h, L, st, h->cur, cls, d_qlist, n_list, maxwords, mean_words))) return rc;
	// expected number of distinct clumps of a query: sampled words x occurrence-weighted mean list length
	const double expect = mean_words * h->acx_wmean;
	const BhipPfChoice c = bhip_pf_choose(algo, h->opt_pf_cw, h->opt_pf_table, h->opt_pf_rb, W16, expect);
	const bool filter = c.kind != BHIP_PF_MASK, cw = c.kind == BHIP_PF_CW || c.kind == BHIP_PF_CQ;
	// lanes per query of the first pass, queries per wave (k_prefilter_cq only: every other kernel's grid is sized as before)
	const int gw = bhip_pf_group(h->opt_pf_group, c, W16, expect, L->pf_surv_per_query);
	const uint32_t qw = 64u / (uint32_t)gw;
	const bhip_pf_kernel_t fp = filter ? pf_kernel(c, 0, gw) : nullptr, fp2 = filter && c.two_pass ? pf_kernel(c, 1) : nullptr;
	if (filter && (!fp || (c.two_pass && !fp2)))
		return fail(BHIP_E_ARG, "option prefilter_cw = %d selects a superseded prefilter kernel that is not part of libburst_hip.so (tests: libburst_hip_legacy.so is loaded first)", h->opt_pf_cw);
	// As many single-wave blocks per CU as are resident at once: the kernel is a persistent loop over a static partition of the list, one
	// block too many per CU would run after the others and double the time.  (Should the runtime not know the kernel: 4.)
	hipFuncAttributes fa;
	const void *fn = filter ? (const void *)fp : c.htb == 9 ? (const void *)k_prefilter_mask<9> : c.htb == 10 ? (const void *)k_prefilter_mask<10> : (const void *)k_prefilter_mask<11>;
	const uint32_t fit = std::min<uint32_t>(cw ? 32u : 12u, blocks_per_cu(fn, 64u, 0, &fa));
	if (getenv("BHIP_DEBUG")) {
		if (cw) fprintf(stderr, "[bhip] prefilter kernel: %s, slot mode %d, %zu B LDS, %d VGPRs -> %u blocks per CU (expected stream %.0f records, %.1f survivors per query in the lane's last chain)\n", c.kind != BHIP_PF_CQ ? "one query per wave" : gw == 8 ? "eight queries per wave, 8 lanes each, streams by the whole wave" : "four queries per wave, 16 lanes each, streams by the whole wave", c.cw_mode, fa.sharedSizeBytes, fa.numRegs, fit, expect, L->pf_surv_per_query);
		else fprintf(stderr, "[bhip] prefilter kernel: table 2^%d, %d record blocks in registers, %zu B LDS, %d VGPRs -> %u blocks per CU\n", c.htb, c.rb, fa.sharedSizeBytes, fa.numRegs, fit);
	}
	const uint32_t waves = h->opt_pf_waves ? std::min<uint32_t>((uint32_t)h->opt_pf_waves, fit) : fit;
	const uint32_t grid = std::min<uint32_t>(c.kind == BHIP_PF_CW ? n_list : (n_list + qw - 1) / qw, (uint32_t)h->n_cu * waves);
	HIPCHK(hipEventRecord(L->ev_pf[cls][PF_HASH_START], st));
	const uint32_t *fb_dense = ov.fb1, *n_fb_dense = ov.n_fb1;
	if (filter) {
		auto launch = [&](bhip_pf_kernel_t k, uint32_t g, uint32_t *fb, uint32_t *n_fb, const uint32_t *sel, const uint32_t *n_sel) {
			hipLaunchKernelGGL(k, dim3(g), dim3(64), 0, st, L->ranges_c[cls].as<uint2>(), L->hdr_c[cls].as<uint2>(), W16, n_list,
				h->acx_view().rec, h->bad.as<uint32_t>(), h->n_bad,
				h->clump_len.as<uint32_t>(), h->tot_refs, L->tasks.as<uint2>(), n_tasks_dev, (uint32_t)L->task_cap, &dc->ent_read,
				fb, n_fb, &dc->unit_sum, &dc->col_sum, &dc->qlen_sum, &dc->surv_sum,
				L->tasks2.as<uint2>(), &dc->n_tasks2_cls[cls], prune, sel, n_sel, c.kind == BHIP_PF_CF ? h->opt_pf_bytes : 0);
		};
		// first pass, then the queries whose survivors overflowed its exact lane table once more with the largest tables (BIG / <11, 4>);
		// an empty second pass costs ~10 us, the dense per-clump fallback behind it 12 ms per launch at 6.8 M clumps whatever the number of queries
		launch(fp, grid, ov.fb1, ov.n_fb1, nullptr, nullptr);
		if (c.two_pass) {
			HIPCHK(hipGetLastError());
			// the second pass of a strain-rich batch is not a handful of queries (round 5 gave it one block per CU): k_prefilter_cq gets as many
			// blocks as fit, up to 4; the one-query-per-wave kernels one per CU
			const uint32_t g2 = (uint32_t)h->n_cu * (c.kind == BHIP_PF_CQ ? std::min<uint32_t>(4u, blocks_per_cu((const void *)fp2, 64u, 0)) : 1u);
			launch(fp2, g2, ov.fb2, ov.n_fb2, ov.fb1, ov.n_fb1);
			fb_dense = ov.fb2; n_fb_dense = ov.n_fb2;
		}
	} else {
		dispatch_int(HtbList{}, c.htb, [&](auto htb) {
			hipLaunchKernelGGL(k_prefilter_mask<decltype(htb)::value>, dim3(grid), dim3(64), 0, st, L->ranges_c[cls].as<uint2>(), L->hdr_c[cls].as<uint2>(), W16, n_list,
				h->acx_view().rec, h->bad.as<uint32_t>(), h->n_bad,
				h->clump_len.as<uint32_t>(), h->tot_refs, L->tasks.as<uint2>(), n_tasks_dev, (uint32_t)L->task_cap, &dc->ent_read,
				ov.fb1, ov.n_fb1, &dc->unit_sum, &dc->col_sum, &dc->qlen_sum, L->cand.as<uint2>(), n_cand_dev, (uint32_t)L->cand_cap);
		});
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(L->ev_pf[cls][PF_HASH_DONE], st));
	++L->pf_launches;
	L->pf_algo_used = c.kind;
	// dense fallback for the queries that overflowed the last pass (clump-level pairs)
	return launch_dense_fallback(h, L, st, d_qlist, n_list, h->bad.as<uint32_t>(), h->n_bad, L->cand.as<uint2>(), nullptr, n_cand_dev, (uint32_t)L->cand_cap, dc, fb_dense, n_fb_dense);
}

// the work buffers of a lane's chain at the lane's present capacities (candidates, tasks, windows, raw hits, re-scorer lists)
static int lane_reserve_work(Lane *L) {
	int rc;
	if ((rc = L->cand.reserve(L->cand_cap * sizeof(uint2))) || (rc = L->raw.reserve(L->raw_cap * sizeof(BhipRawHit))) || (rc = L->wide.reserve(L->raw_cap * sizeof(uint32_t))) ||
	    (rc = L->rs_lists.reserve(L->raw_cap * sizeof(uint32_t) * 10)) || (rc = L->scratch.reserve(L->scratch_cap * sizeof(uint32_t))) || (rc = L->wins.reserve(L->win_cap * sizeof(BhipWin))) ||
	    (rc = L->tasks.reserve(L->task_cap * sizeof(uint2))) || (rc = L->tasks2.reserve(L->task_cap * sizeof(uint2))) || (rc = L->tasks2k.reserve(L->task_cap * sizeof(uint2))) ||
	    (rc = L->wins2.reserve(L->win_cap * sizeof(BhipWin)))) return rc;
	return 0;
}
// Allocate, ahead of the first batch, what batches of up to n_entries entries of up to max_len symbols need (both staging slots,
// the scratch of the alignment kernels, the record buffers): a batch scheduler calls it once so that no allocation -- each one
// synchronises the device -- falls into its first batches.
extern "C" int bhip_reserve(void *handle, uint32_t n_entries, uint32_t max_len) { return bhip_reserve_symbols(handle, n_entries, max_len, 0); }
// total_symbols > 0: the symbols of the largest batch that will be staged (sum of its entries' lengths).  Buffers that hold the
// symbols themselves and the match profiles are then sized from it -- one 1 000-symbol read among millions of 100-symbol ones
// must not make every buffer n_entries x max_len large -- while the fixed-stride tables keep their max_len stride.
extern "C" int bhip_reserve_symbols(void *handle, uint32_t n_entries, uint32_t max_len, uint64_t total_symbols) {
	Handle *h = (Handle *)handle;
	if (!h) return fail(BHIP_E_ARG, "null handle");
	if (!n_entries) return BHIP_OK;
	if (!max_len || max_len > BHIP_MAX_QLEN) max_len = BHIP_MAX_QLEN;
	HIPCHK(hipSetDevice(h->device));
	int rc;
	if (getenv("BHIP_DEBUG")) { size_t f_ = 0, t_ = 0; if (hipMemGetInfo(&f_, &t_) == hipSuccess) fprintf(stderr, "[bhip] reserve for %u entries of up to %u symbols: %.2f GB of the device's %.2f free\n", n_entries, max_len, f_ / 1e9, t_ / 1e9); }
	const size_t n = n_entries, nb = total_symbols ? (size_t)std::min<uint64_t>(total_symbols + 64, (uint64_t)n * max_len) : n * max_len, qw = (max_len + 7) / 8;
	// profile words: an entry of len symbols has a vector of at most 2 x (len / 32 + 1) words (class rounding), 16 rows of them
	const size_t cw = (size_t)class_words(class_of_len(max_len), max_len);
	const size_t peq_words = total_symbols ? std::min<size_t>(n * cw, 2 * (nb / 32 + n)) : n * cw;
	for (StageSlot &S : h->slots) {
		if ((rc = slot_init(&S))) return rc;
		if ((rc = S.qcodes4.reserve(nb / 2 + 128)) || (rc = S.qcodes.reserve(nb + 128)) || (rc = S.qoff.reserve((n + 1) * 8)) || (rc = S.qemac.reserve((n + 1) * 2)) ||
		    (rc = S.qsix.reserve((n + 1) * 4)) || (rc = S.qrc.reserve(n + 1)) || (rc = S.qflags.reserve(n + 1)) || (rc = S.qmap.reserve((n + 1) * 4)) ||
		    (rc = S.off_raw.reserve((n + 8) * 8)) || (rc = S.plan.reserve(n * 4 + 16)) || (rc = S.qpack.reserve(n * qw * 4 + 64)) || (rc = S.key.reserve(n + 16)) ||
		    (rc = S.key_sorted.reserve(n + 16)) || (rc = S.idx.reserve(n * 4 + 16)) || (rc = S.idx_sorted.reserve(n * 4 + 16))) return rc;
		size_t tb = 0;
		HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, S.key.as<uint8_t>(), S.key_sorted.as<uint8_t>(), S.idx.as<uint32_t>(), S.idx_sorted.as<uint32_t>(), (int)n, 0, 8, h->stage_stream));
		if ((rc = S.sort_tmp.reserve(tb + 16))) return rc;
	}
	if (getenv("BHIP_DEBUG")) { size_t f_ = 0, t_ = 0; if (hipMemGetInfo(&f_, &t_) == hipSuccess) fprintf(stderr, "[bhip] ... staging slots reserved: %.2f GB free\n", f_ / 1e9); }
	if ((rc = ensure_lanes(h, 1))) return rc;
	Lane *L = h->lanes[0];
	lane_capacity_floor(h, L, n);
	const int cls = class_of_len(max_len);
	if ((rc = lane_reserve_work(L)) || (rc = L->peq.reserve(peq_words * 16 * 4)) || (rc = L->peqp.reserve(n * 16 * 6 * 4)) ||
	    (rc = L->peq_alt.reserve(peq_words * 16 * 4)) || (rc = L->peqp_alt.reserve(n * 16 * 6 * 4)) ||
	    (rc = L->fb_list.reserve(n * 8 + 64)) || (rc = L->ranges_c[cls].reserve(n * 16 * 8 + 16)) || (rc = L->hdr_c[cls].reserve(n * 8 + 16))) return rc;
	// (BEST on the device: its per-entry keys and the read-back word as well -- nothing is allocated inside the first batch)
	if (h->n_order) { if ((rc = h->best_key.reserve((n + 1) * 8)) || (rc = h->sort_idx.reserve(std::max<size_t>((size_t)h->out_cap, n + 1) * 4))) return rc; if (!h->nsel_pinned) HIPCHK(hipHostMalloc((void **)&h->nsel_pinned, 64, hipHostMallocDefault)); }
	if ((rc = h->best.reserve((n + 1) * 4)) || (rc = h->out.reserve(h->out_cap * sizeof(BhipHit))) || (rc = h->shared_ctr.reserve(sizeof(SharedCtr))) ||
	    (rc = h->sort_idx.reserve(h->out_cap * 4)) || (rc = h->sort_keys.reserve((n + 1) * 4)) || (rc = h->sort_keys2.reserve((n + 1) * 4)) ||
	    (rc = h->out_sorted.reserve(h->out_cap * sizeof(BhipHit))) || (rc = h->out_sorted2.reserve(h->out_cap * sizeof(BhipHit)))) return rc;
	{
		size_t tb = 0;
		HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, h->sort_keys.as<uint32_t>(), h->sort_keys2.as<uint32_t>(), (int)(n + 1), h->stream));
		if ((rc = h->sort_tmp.reserve(tb))) return rc;
	}
	if (getenv("BHIP_DEBUG")) { size_t f_ = 0, t_ = 0; if (hipMemGetInfo(&f_, &t_) == hipSuccess) fprintf(stderr, "[bhip] ... lane and record buffers reserved: %.2f GB free\n", f_ / 1e9); }
	if (!h->copy_stream) { HIPCHK(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking)); HIPCHK(hipEventCreateWithFlags(&h->ev_sorted, hipEventDisableTiming));
		for (auto &e : h->ev_copied) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
	{	// A synthetic batch through the whole path, the way a batch scheduler drives it (page-locked arrays, asynchronous copies
		// in and out): the first launch of every kernel, the first use of the copy engines from the staging and hand-over
		// streams and the first touch of the new buffers cost tens of milliseconds that would otherwise land in the caller's
		// first real batch; an idle device also clocks down, and a few milliseconds of work bring it back up.
		const uint32_t nw = std::min<uint32_t>(n_entries, 1u << 17), len = std::min<uint32_t>(max_len, 100u);
		const size_t nb_w = (size_t)nw * len + 16;
		uint8_t *pin = nullptr;
		const size_t bytes = nb_w + nb_w / 2 + 16 + ((size_t)nw + 1) * 8 + (size_t)nw * 2 + 64 + (size_t)nw * 4 * sizeof(BhipHit);
		HIPCHK(hipHostMalloc((void **)&pin, bytes, hipHostMallocPortable));
		uint8_t *codes = pin, *codes4 = pin + nb_w;
		uint64_t *off = (uint64_t *)(pin + ((nb_w + nb_w / 2 + 16 + 7) & ~(size_t)7));
		uint16_t *emac = (uint16_t *)(off + nw + 1);
		BhipHit *hbuf = (BhipHit *)(((uintptr_t)(emac + nw) + 63) & ~(uintptr_t)63);
		uint64_t x = 88172645463325252ull;
		for (size_t i = 0; i < nb_w; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; codes[i] = (uint8_t)(1 + (x & 3)); }
		for (size_t i = 0; i < nb_w / 2; ++i) codes4[i] = (uint8_t)(codes[2 * i] | codes[2 * i + 1] << 4);
		for (uint32_t i = 0; i <= nw; ++i) off[i] = (uint64_t)i * len;
		for (uint32_t i = 0; i < nw; ++i) emac[i] = (uint16_t)(len / 40);
		BhipQuerySpan sp;
		memset(&sp, 0, sizeof sp);
		sp.codes = codes; sp.codes4 = codes4; sp.off = off; sp.emac = emac; sp.n = nw;
		uint64_t n_out = 0;
		const int async = h->opt_async_d2h;
		h->opt_async_d2h = 1;
		for (StageSlot &S : h->slots) { S.state = 0; S.st_valid = false; }
		rc = 0;
		for (int rep = 0; rep < 4 && !rc; ++rep) {
			rc = bhip_stage_spans(h, &sp, 1, nw, len);
			if (!rc) rc = bhip_align_staged(h, 0, hbuf, (uint64_t)nw * 4, &n_out);
		}
		(void)bhip_sync_hits(h);
		{	// the first LARGE asynchronous copy in each direction takes another path through the runtime than the small ones above
			// and blocks its caller for ~19 ms once per process (measured in front of the first 43 MB hand-over copy): make it here
			// ... and so does the first copy that is enqueued while another one is still in flight on the same stream (measured: 16 ms in
			// front of the second hand-over copy of a process): two of each, back to back
			const size_t big = std::min<size_t>(64u << 20, std::min(h->out_sorted.cap, h->out_sorted2.cap));
			void *tmp = nullptr;
			if (big && hipHostMalloc(&tmp, 2 * big, hipHostMallocPortable) == hipSuccess) {
				(void)hipMemcpyAsync(tmp, h->out_sorted.p, big, hipMemcpyDeviceToHost, h->copy_stream);
				(void)hipMemcpyAsync((char *)tmp + big, h->out_sorted2.p, big, hipMemcpyDeviceToHost, h->copy_stream);
				(void)hipMemcpyAsync(tmp, h->out_sorted.p, big, hipMemcpyDeviceToHost, h->copy_stream);
				(void)hipStreamSynchronize(h->copy_stream);
				(void)hipMemcpyAsync(h->out_sorted.p, tmp, big, hipMemcpyHostToDevice, h->stage_stream);
				(void)hipMemcpyAsync(h->out_sorted2.p, (char *)tmp + big, big, hipMemcpyHostToDevice, h->stage_stream);
				(void)hipMemcpyAsync(h->out_sorted.p, tmp, big, hipMemcpyHostToDevice, h->stage_stream);
				(void)hipStreamSynchronize(h->stage_stream);
				// ... and a hand-over copy enqueued while the staging copies of two batches are still queued (15-17 ms once, measured
				// in front of the second batch's hand-over of the first call that stages two batches ahead)
				const size_t piece = big / 16;
				if (piece) {
					for (int i = 0; i < 12; ++i) (void)hipMemcpyAsync((char *)h->out_sorted.p + (size_t)i * piece, (char *)tmp + (size_t)i * piece, piece, hipMemcpyHostToDevice, h->stage_stream);
					(void)hipMemcpyAsync((char *)tmp + big, h->out_sorted2.p, big, hipMemcpyDeviceToHost, h->copy_stream);
					(void)hipStreamSynchronize(h->copy_stream);
					(void)hipStreamSynchronize(h->stage_stream);
				}
				(void)hipHostFree(tmp);
			}
			(void)hipGetLastError();
		}
		h->opt_async_d2h = async;
		for (StageSlot &S : h->slots) { S.state = 0; S.st_valid = false; S.spans.clear(); }
		h->res_valid = false;
		(void)hipHostFree(pin);
		if (rc) return rc;
	}
	return BHIP_OK;
}
// ---- one batch call (bhip_align_staged) ------------------------------------------------------------------------------
// What the steps of a call share.  A step returns BHIP_OK, an error (< 0) or STEP_REDO: a buffer was too small for what the chain
// produced, it has grown, the chain is enqueued again.
enum { STEP_REDO = 1 };
struct BatchCall {
	StageSlot *slot = nullptr;
	int mode = 0;                        // all_hits as the caller gave it (BHIP_HITS_*)
	int all_hits = 0;                    // what the kernels are told: every hit within budget, or the minimum per shared slot
	bool sel_best = false;               // ... and of those one record per entry, chosen on the device
	BhipHit *hits = nullptr; uint64_t cap = 0; uint64_t *n_hits = nullptr;      // the caller's buffer
	uint32_t n_q = 0, n_shared = 0, nl = 0;
	uint32_t band_rows = 0, qw = 0, rw = 0;      // LDS plan of the re-scorer: band rows, query and reference staging (dwords per thread)
	SharedCtr hsc = {};                  // the shared counters behind the last re-scorer
	uint32_t n_deliver = 0;              // records the caller gets: all of them, or one per entry (sel_best)
	bool sorted_ahead = false; int o_ahead = 0;      // the records were grouped behind the re-scorer, into out_sorted (0) or out_sorted2 (1)
	size_t tmp_bytes = 0;                // scratch of the scan over the per-entry counters
	std::chrono::steady_clock::time_point t0; double t_host[4] = {0, 0, 0, 0};      // delivery, host side (BHIP_DEBUG_TIMES)
	void mark(int i) { t_host[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Enqueue one length class of a lane (no host synchronisation): match profiles on the sweep stream, the prefilter on its own, the sweeps of the
// prefiltered and of the exhaustive queries behind it, the window stage on the post stream and -- with pruning -- the second sweep.
static int enqueue_class(Handle *h, Lane *L, int cls, int all_hits) {
	int rc;
	hipStream_t pf = h->pf_stream, sw = h->sweep_stream, po = h->post_stream;
	Counters *dc = L->counters.as<Counters>();
	const uint32_t n_pf = L->npf[cls], n_ex = L->nex[cls], n_list = n_pf + n_ex;
	const uint32_t grid_my = (uint32_t)h->n_cu * (uint32_t)h->opt_sweep_blocks;   // < 8 leaves wave slots for the other stages' kernels
	const uint32_t grid_task = (uint32_t)h->n_cu * 4u * (uint32_t)h->opt_sweep_blocks * (uint32_t)h->opt_oversub;      // 64-thread blocks of the task sweeps
	const int NW = class_words(cls, L->maxlen);
	const uint32_t *qlist = L->qlist[cls];
	hipEvent_t *ce = L->ev_cls[cls];
	// the lane's peq buffers are reused class after class: do not rebuild them before the previous class's window stage is done
	// (the profiles are built on the sweep stream, which is idle while this class's seeds and prefilter run on theirs)
	if (L->launches) { HIPCHK(hipStreamWaitEvent(pf, L->ev_rs[RS_START], 0)); HIPCHK(hipStreamWaitEvent(sw, L->ev_rs[RS_START], 0)); }
	const int NWP = class_prefix_words(h, L->maxE[cls], NW);   // two-stage edit distance when a prefix of 32*NWP symbols is selective for this class's budgets
	HIPCHK(hipEventRecord(ce[CE_START], sw));
	L->peq_ahead[cls] = false;
	if (L->alt_ok && L->alt_seq == h->cur->seq && L->alt_cls == cls && L->alt_n == n_list && L->alt_nwp == NWP && !L->launches) {
		// built ahead during the previous batch (seed_next_batch): that batch is through, its profiles are not needed any more
		std::swap(L->peq, L->peq_alt); std::swap(L->peqp, L->peqp_alt);
		std::swap(L->ev_peq_cur[SPAN_START], L->ev_peq_alt[SPAN_START]); std::swap(L->ev_peq_cur[SPAN_DONE], L->ev_peq_alt[SPAN_DONE]);
		L->alt_ok = false; L->peq_ahead[cls] = true;
	} else if ((rc = launch_peq(h, sw, h->cur, qlist, n_list, NW, NWP, L->peq, L->peqp))) return rc;
	L->prefix_words = (uint32_t)NWP;
	HIPCHK(hipEventRecord(ce[CE_PEQ_DONE], sw));
	HIPCHK(hipEventRecord(ce[CE_PF_START], pf));
	const bool masked = NWP && n_pf && h->has_masks && h->opt_lane_masks;
	// lower-bound pruning (second sweep) only when the minimum per shared slot is all that is wanted, with the counting-filter
	// kernel (it sees all lane counts of a query at once) and while a list position fits the 24 bits next to the bound
	const int pf_algo = bhip_pf_algo(h->opt_pf_algo, L->pf_algo);
	const int prune = masked && !all_hits && h->opt_prune && n_list < (1u << 24) && pf_algo == 0;
	if (n_pf) {
		if (masked) { if ((rc = launch_prefilter_mask(h, L, pf, cls, qlist, n_pf, L->maxwords[cls], &dc->n_tasks_cls[cls], &dc->n_cand_cls[cls], dc, pf_algo, prune))) return rc; }
		else if ((rc = launch_prefilter(h, L, pf, qlist, n_pf, L->cand.as<uint2>(), nullptr, (uint32_t)L->cand_cap, true, &dc->n_cand_cls[cls], dc))) return rc;
	}
	// (query, length, budget) per list position, written by this batch's k_seed_ranges: what the prefix sweeps of the tasks start from
	const uint4 *qmeta_cls = (masked && L->qmeta_seq[h->cur->seq & 1][cls] == h->cur->seq + 1) ? L->qmeta_c[h->cur->seq & 1][cls].as<uint4>() : nullptr;
	L->masked = masked;
	L->pf_masked[cls] = masked && n_pf;
	HIPCHK(hipEventRecord(ce[CE_PF_DONE], pf));
	// column sweep on the sweep stream, behind this lane's prefilter
	HIPCHK(hipStreamWaitEvent(sw, ce[CE_PF_DONE], 0));
	HIPCHK(hipEventRecord(ce[CE_SWEEP_START], sw));
	if (n_pf) {
		if (masked) launch_prefix_task(h, L, sw, NWP, grid_task, L->tasks.as<uint2>(), &dc->n_tasks_cls[cls], qlist, L->wins.as<BhipWin>(), &dc->n_wins_cls[cls], dc, qmeta_cls);
		// (beside the lane tasks the clump-level pairs are the rare overflow of the prefilter, usually none at all: a small grid --
		// an empty launch of 2 048 workgroups waited ~0.24 ms for slots on a device busy with the next batch's seed lookups and staging)
		if (NWP) launch_prefix(h, L, sw, NWP, masked ? std::min<uint32_t>(grid_my, (uint32_t)h->n_cu) : grid_my, L->cand.as<uint2>(), &dc->n_cand_cls[cls], L->cand_cap, 0, qlist, &dc->n_wins_cls[cls], dc);
		else launch_myers(h, L, sw, NW, grid_my, L->cand.as<uint2>(), &dc->n_cand_cls[cls], L->cand_cap, 0, qlist, L->raw.as<BhipRawHit>(),
			&dc->n_raw, (uint32_t)L->raw_cap, h->best.as<uint32_t>(), nullptr, dc);
		HIPCHK(hipGetLastError());
		++L->launches;
	}
	HIPCHK(hipEventRecord(ce[CE_SWEEP_PF_DONE], sw));
	if (n_ex) {
		const uint64_t np = (uint64_t)n_ex * h->n_clumps;
		const uint32_t g = (uint32_t)std::min<uint64_t>((np + 15) / 16, grid_my);
		if (NWP) launch_prefix(h, L, sw, NWP, g, nullptr, nullptr, np, n_pf, qlist, &dc->n_wins_cls[cls], dc);
		else launch_myers(h, L, sw, NW, g, nullptr, nullptr, np, n_pf, qlist, L->raw.as<BhipRawHit>(), &dc->n_raw, (uint32_t)L->raw_cap,
			h->best.as<uint32_t>(), nullptr, dc);
		HIPCHK(hipGetLastError());
		++L->launches;
		L->n_pairs_ex += np;
	}
	HIPCHK(hipEventRecord(ce[CE_SWEEP_EX_DONE], sw));
	HIPCHK(hipStreamWaitEvent(po, ce[CE_SWEEP_EX_DONE], 0));
	if (NWP) { launch_window(h, L, po, cls, NWP, grid_my, L->wins.as<BhipWin>(), &dc->n_wins_cls[cls], dc); HIPCHK(hipGetLastError()); }
	L->pruned[cls] = masked && prune && n_pf;
	if (L->pruned[cls]) {
		// second sweep: the deferred lanes whose lower bound is not above the minimum found by the first sweep
		HIPCHK(hipEventRecord(L->ev_ph[cls][PH_WIN_DONE], po));
		HIPCHK(hipStreamWaitEvent(sw, L->ev_ph[cls][PH_WIN_DONE], 0));
		hipLaunchKernelGGL(k_task_filter, dim3((uint32_t)h->n_cu * 8), dim3(256), 0, sw, L->tasks2.as<uint2>(), &dc->n_tasks2_cls[cls], (uint32_t)L->task_cap, qlist,
			six_or_null(h), h->best.as<uint32_t>(), L->tasks2k.as<uint2>(), &dc->n_tasks2k_cls[cls]);
		launch_prefix_task(h, L, sw, NWP, grid_task, L->tasks2k.as<uint2>(), &dc->n_tasks2k_cls[cls], qlist, L->wins2.as<BhipWin>(), &dc->n_wins2_cls[cls], dc, qmeta_cls);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(L->ev_ph[cls][PH_SWEEP2_DONE], sw));
		HIPCHK(hipStreamWaitEvent(po, L->ev_ph[cls][PH_SWEEP2_DONE], 0));
		launch_window(h, L, po, cls, NWP, grid_my, L->wins2.as<BhipWin>(), &dc->n_wins2_cls[cls], dc);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipEventRecord(ce[CE_WIN_DONE], po));
	HIPCHK(hipEventRecord(L->ev_rs[RS_START], po));
	return 0;
}

// Enqueue the re-scoring of the kept reference lanes of a lane's shared slots on the post stream, behind its last class, and the read-back of
// the lane's counters.
static int enqueue_rescore(Handle *h, Lane *L, const BatchCall &b) {
	hipStream_t po = h->post_stream;
	Counters *dc = L->counters.as<Counters>();
	SharedCtr *sc = h->shared_ctr.as<SharedCtr>();
	const RefArgs R = ref_args(h);
	HIPCHK(hipEventRecord(L->ev_rs[RS_START], po));
	if (h->cur->st_has_junk) {       // back to the units of the original queries (see Handle::qcodes_s); this lane owns the shared slots [s0, s1)
		const uint32_t nl_ = h->cur->st_lanes, nsh_ = h->cur->st_nshared;
		uint32_t li_ = 0;
		for (uint32_t l = 0; l < nl_; ++l) if (h->lanes[l] == L) li_ = l;
		const uint32_t s0 = (uint32_t)(((uint64_t)li_ * nsh_ + nl_ - 1) / nl_), s1 = (uint32_t)(((uint64_t)(li_ + 1) * nsh_ + nl_ - 1) / nl_);
		hipLaunchKernelGGL(k_junk_adjust_raw, dim3((uint32_t)h->n_cu * 4), dim3(256), 0, po, L->raw.as<BhipRawHit>(), &dc->n_raw, (uint32_t)L->raw_cap, h->cur->nx.as<uint8_t>());
		if (s1 > s0) hipLaunchKernelGGL(k_junk_adjust_best, dim3(std::min<uint32_t>((s1 - s0 + 255) / 256, (uint32_t)h->n_cu * 4)), dim3(256), 0, po, h->best.as<uint32_t>(), h->cur->nx_six.as<uint8_t>(), s0, s1);
		HIPCHK(hipGetLastError());
	}
	// classify (exact matches leave here), register-band variants for the narrow bands, LDS band for the rest
	const uint32_t qw_g = (h->cur->st_maxlen + 7) / 8;
	hipLaunchKernelGGL(k_rescore_classify, dim3((uint32_t)h->n_cu * 8), dim3(256), 0, po, L->raw.as<BhipRawHit>(), &dc->n_raw, (uint32_t)L->raw_cap,
		h->best.as<uint32_t>(), b.all_hits, h->cur->qoff.as<uint64_t>(), six_or_null(h), rc_or_null(h),
		R.len, h->out.as<BhipHit>(), &sc->n_out, (uint32_t)h->out_cap, L->rs_lists.as<uint32_t>(), dc->n_rs, L->wide.as<uint32_t>(), &dc->n_wide,
		b.band_rows, h->opt_rescore_reg);
	HIPCHK(hipGetLastError());
	if (h->opt_rescore_reg) {
		for_each_int(SetList{}, [&](auto set) {
			constexpr int SET = decltype(set)::value;
			// where a hit's packed query comes from (option "fetch_once"): copied once into LDS where the set's registers and the rows' qw_g
			// dwords leave every resident wave in place, else 16 bytes per 32 rows, else a dword per 8 rows
			const BhipKernelRes res[BHIP_QF_COUNT] = {kernel_res<k_rescore_reg<SET, BHIP_QF_DWORD>>(), kernel_res<k_rescore_reg<SET, BHIP_QF_LDS>>(), kernel_res<k_rescore_reg<SET, BHIP_QF_CHUNK>>()};
			const BhipQueryFetch qf = bhip_plan_query_fetch(qw_g, h->opt_fetch_once && res[0].regs && res[1].regs && res[2].regs, res);
			L->qfetch[SET] = qf;
			const uint32_t grid = (uint32_t)h->n_cu * std::min<uint32_t>(32u, qf.blocks) * (uint32_t)h->opt_oversub;
			auto launch = [&](auto form) {
				hipLaunchKernelGGL((k_rescore_reg<SET, decltype(form)::value>), dim3(grid), dim3(64), qf.lds_bytes, po, L->raw.as<BhipRawHit>(), L->rs_lists.as<uint32_t>(), dc->n_rs, (uint32_t)L->raw_cap,
					h->cur->qoff.as<uint64_t>(), rc_or_null(h), h->cur->qpack.as<uint32_t>(), qw_g,
					R.bytes(), R.off, R.len, h->lut.as<uint8_t>(), h->out.as<BhipHit>(), &sc->n_out, (uint32_t)h->out_cap, &sc->err);
			};
			dispatch_int(IntList<BHIP_QF_DWORD, BHIP_QF_LDS, BHIP_QF_CHUNK>{}, qf.form, launch);
		});
		HIPCHK(hipGetLastError());
	}
	const uint32_t grid_rs = (uint32_t)h->n_cu * (h->opt_rescore_reg ? 4 : 16);
	const size_t lds_rs = (size_t)(b.band_rows + 1 + b.qw + b.rw) * 256;
	hipLaunchKernelGGL(k_rescore<false>, dim3(grid_rs), dim3(64), lds_rs, po, L->raw.as<BhipRawHit>(), &dc->n_raw, (uint32_t)L->raw_cap,
		L->rs_lists.as<uint32_t>() + (size_t)9 * L->raw_cap, &dc->n_rs[9], h->best.as<uint32_t>(), b.all_hits, h->cur->qcodes.as<uint8_t>(), h->cur->qoff.as<uint64_t>(),
		six_or_null(h), rc_or_null(h), R.bytes(), R.off, R.len, h->lut.as<uint8_t>(), h->out.as<BhipHit>(), &sc->n_out, (uint32_t)h->out_cap, L->wide.as<uint32_t>(),
		&dc->n_wide, (uint32_t *)nullptr, &dc->scratch_used, 0ull, &sc->err, b.qw ? h->cur->qpack.as<uint32_t>() : nullptr, b.band_rows, b.qw, b.rw);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(L->ev_rs[RS_DONE], po));
	HIPCHK(hipMemcpyAsync(L->hc_pinned, dc, sizeof(Counters), hipMemcpyDeviceToHost, po));
	return 0;
}

// enqueue one lane's whole chain (no host synchronisation): every class that has queries, then the re-scoring
static int enqueue_lane(Handle *h, Lane *L, const BatchCall &b) {
	int rc;
	if ((rc = lane_reserve_work(L))) return rc;
	HIPCHK(hipMemsetAsync(L->counters.p, 0, sizeof(Counters), h->pf_stream));
	L->launches = 0; L->prefix_words = 0; L->n_pairs_ex = 0; L->pf_launches = 0; L->fb_dirty = false;
	for (int c = 0; c < kNumClasses; ++c) { L->pf_masked[c] = false; L->pruned[c] = false; }
	for (int cls = 0; cls < kNumClasses; ++cls) if (L->npf[cls] + L->nex[cls]) if ((rc = enqueue_class(h, L, cls, b.all_hits))) return rc;
	return enqueue_rescore(h, L, b);
}

// Seed lookups of the NEXT staged batch, enqueued on the prefilter stream behind the current batch's prefilter: they run
// beside the current batch's sweeps and re-scoring (k_seed_ranges waits for HBM 70 % of its time and issues VALU work 6 % of
// it; the sweeps are VALU-bound).  Called with the current batch fully enqueued; waits (host) for the staging of the next batch
// or the end of the current one, whichever comes first.  Failures only mean the lookups run in place later.
static void seed_next_batch(Handle *h, StageSlot *cur, hipEvent_t cur_done) {
	if (!h->opt_seed_ahead || !h->has_acx || !h->has_masks || !h->opt_lane_masks || h->opt_host_routing) return;
	StageSlot *N = nullptr;
	for (StageSlot &S : h->slots) if (&S != cur && S.state == 1 && (!N || S.seq < N->seq)) N = &S;      // the batch that is aligned next
	if (!N || !N->st_nq) return;
	if (!N->resolved) {
		for (;;) {
			const hipError_t e = hipEventQuery(N->ev_done);
			if (e == hipSuccess) break;
			if (e != hipErrorNotReady) { (void)hipGetLastError(); return; }
			if (hipEventQuery(cur_done) != hipErrorNotReady) { (void)hipGetLastError(); return; }      // the current batch is through: nothing left to hide behind
			std::this_thread::yield();
		}
		(void)hipGetLastError();
		const BhipStageInfo &I = *N->info_pinned;
		if (I.err || I.junk) return;             // errors and the host routing pass are bhip_align_staged's business
		if (resolve_slot(h, N)) return;
	}
	if (N->st_has_junk || ensure_lanes(h, N->st_lanes)) return;
	for (uint32_t l = 0; l < N->st_lanes && l < h->lanes.size(); ++l) {
		Lane *L = h->lanes[l];
		for (int cls = 0; cls < kNumClasses; ++cls) {
			const uint32_t n_pf = N->npf[l][cls];
			if (!n_pf || !class_prefix_words(h, N->maxE[l][cls], class_words(cls, N->maxlen_lane[l]))) continue;      // (lane-resolved prefilter only)
			if (L->seeded_ok[cls] && L->seeded_seq[cls] == N->seq) continue;
			if (launch_seed(h, L, h->pf_stream, N, cls, N->idx_sorted.as<uint32_t>() + N->qlist_off[l][cls], n_pf, N->maxwords[l][cls], (double)N->seed_words[l][cls] / (double)n_pf, true)) { (void)hipGetLastError(); return; }
		}
		// the match profiles as well, when the lane has a single class (its two buffer pairs then simply alternate): built in place
		// they would run beside the prefilter -- which no longer has its seed lookups in front -- and slow it down
		int only = -1, n_cls = 0;
		for (int cls = 0; cls < kNumClasses; ++cls) if (N->npf[l][cls] + N->nex[l][cls]) { only = cls; ++n_cls; }
		if (n_cls == 1 && !(L->alt_ok && L->alt_seq == N->seq)) {
			const uint32_t n_list = N->npf[l][only] + N->nex[l][only];
			const int NW = class_words(only, N->maxlen_lane[l]), NWP = class_prefix_words(h, N->maxE[l][only], NW);
			L->alt_ok = false;
			if (hipEventRecord(L->ev_peq_alt[SPAN_START], h->pf_stream) != hipSuccess ||
			    launch_peq(h, h->pf_stream, N, N->idx_sorted.as<uint32_t>() + N->qlist_off[l][only], n_list, NW, NWP, L->peq_alt, L->peqp_alt, (uint32_t)h->opt_peq_ahead_blocks) ||
			    hipEventRecord(L->ev_peq_alt[SPAN_DONE], h->pf_stream) != hipSuccess) { (void)hipGetLastError(); return; }
			L->alt_ok = true; L->alt_seq = N->seq; L->alt_cls = only; L->alt_nwp = NWP; L->alt_n = n_list;
		}
	}
}

extern "C" int bhip_set_enqueued_hook(void *handle, void (*fn)(void *), void *ctx) {
	Handle *h = (Handle *)handle;
	if (!h) return fail(BHIP_E_ARG, "null handle");
	h->enqueued_hook = fn; h->enqueued_ctx = ctx;
	return BHIP_OK;
}

// A capacity that the `seen` items of a chain did not fit grows past them (an eighth on top where `eighth`, and 1 024); the chain is then
// redone.  lane < 0: a buffer of the whole batch.  One BHIP_DEBUG line per growth.
static bool grow_cap(uint64_t &cap, uint64_t seen, bool eighth, int lane, const char *what) {
	if (seen <= cap) return false;
	const uint64_t to = seen + (eighth ? seen / 8 : 0) + 1024;
	if (getenv("BHIP_DEBUG")) {
		if (lane >= 0) fprintf(stderr, "[bhip] redo: lane %d %s %llu -> %llu\n", lane, what, (unsigned long long)cap, (unsigned long long)to);
		else fprintf(stderr, "[bhip] redo: %s %llu -> %llu\n", what, (unsigned long long)cap, (unsigned long long)to);
	}
	cap = to;
	return true;
}

// the batch: the oldest one staged and not aligned yet, else the one aligned last (staged once, run any number of times)
static int pick_batch(Handle *h, BatchCall &b) {
	StageSlot *slot = nullptr;
	for (StageSlot &S : h->slots) if (S.state == 1 && (!slot || S.seq < slot->seq)) slot = &S;
	if (!slot) for (StageSlot &S : h->slots) if (S.state == 2 && (!slot || S.seq > slot->seq)) slot = &S;
	if (!slot) return fail(BHIP_E_ARG, "no staged queries (call bhip_stage_queries first)");
	{ int rcs = resolve_slot(h, slot); if (rcs) { slot->state = 0; return rcs; } }
	apply_slot(h, slot);
	b.slot = slot; b.n_q = h->cur->st_nq; b.n_shared = h->cur->st_nshared; b.nl = h->cur->st_lanes;
	return BHIP_OK;
}
// LDS plan of the re-scorer: band rows for the widest expected band (2*maxE+1 plus slack), query and reference staging; what BEST needs
static int plan_batch(Handle *h, BatchCall &b) {
	b.band_rows = std::min<uint32_t>(BHIP_RESCORE_WMAX, 2 * h->cur->st_maxE + 1 + 9);
	b.qw = (h->cur->st_maxlen + 7) / 8; b.rw = (h->cur->st_maxlen + b.band_rows + 24) / 8 + 2;
	if ((size_t)(b.band_rows + 1 + b.qw + b.rw) * 256 > 40 * 1024) { b.qw = 0; b.rw = 0; }      // long queries: per-row global reads instead
	if (!b.sel_best) return BHIP_OK;
	int rc;
	if ((rc = h->best_key.reserve((size_t)(b.n_q + 1) * 8)) || (rc = h->sort_idx.reserve(std::max<size_t>((size_t)h->out_cap, (size_t)b.n_q + 1) * 4))) return rc;      // (the rank array doubles as the per-entry flags)
	if (!h->nsel_pinned) HIPCHK(hipHostMalloc((void **)&h->nsel_pinned, 64, hipHostMallocDefault));
	return BHIP_OK;
}
// the records of this batch are still resident when the previous call only failed for the size of the caller's buffer
static bool records_resident(const Handle *h, const BatchCall &b) { return h->res_valid && h->res_seq == b.slot->seq && h->res_all_hits == b.mode; }
static void take_resident(Handle *h, BatchCall &b) {
	b.hsc.n_out = h->res_n_raw; b.hsc.err = 0; h->stats = h->res_stats; b.n_deliver = h->res_n; *b.n_hits = b.n_deliver; b.sorted_ahead = false;
}

// the scan over the n_q + 1 per-entry counters on `st`: its scratch
static int plan_scan(Handle *h, BatchCall &b, hipStream_t st) {
	b.tmp_bytes = 0;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, b.tmp_bytes, h->sort_keys.as<uint32_t>(), h->sort_keys2.as<uint32_t>(), (int)(b.n_q + 1), st));
	return h->sort_tmp.reserve(b.tmp_bytes);
}
// the grouping of the records on `st` into `sorted`: the counting sort by entry (scatter + a rank sort inside every group), or -- sel_best --
// the choice of one record per entry (two streaming passes).  sort_keys = records per entry (from the re-scoring kernels, or k_hit_count),
// sort_keys2 = their offsets, sort_idx = rank of a record inside its entry; n_dev: the record count where it still lives on the device
static int enqueue_grouping(Handle *h, const BatchCall &b, hipStream_t st, uint32_t n_host, const uint32_t *n_dev, DBuf &sorted) {
	uint32_t *cnt = h->sort_keys.as<uint32_t>(), *off = h->sort_keys2.as<uint32_t>(), *rank = h->sort_idx.as<uint32_t>();
	const uint32_t n_q = b.n_q, g = (uint32_t)h->n_cu * 8;
	const uint32_t *qmap = h->cur->has_qmap ? h->cur->qmap.as<uint32_t>() : (const uint32_t *)nullptr;
	size_t tmp_bytes = b.tmp_bytes;
	if (b.sel_best) {
		// (flags into the rank array: the ranks the re-scoring kernels took are not needed when nothing is sorted)
		hipLaunchKernelGGL(k_best_key, dim3(g), dim3(256), 0, st, h->out.as<BhipHit>(), n_host, n_dev, h->ref_order.as<uint32_t>(), cnt, h->best_key.as<unsigned long long>());
		hipLaunchKernelGGL(k_best_flag, dim3(std::min<uint32_t>((n_q + 256) / 256, g)), dim3(256), 0, st, cnt, n_q, rank);
		HIPCHK(hipcub::DeviceScan::ExclusiveSum(h->sort_tmp.p, tmp_bytes, rank, off, (int)(n_q + 1), st));
		hipLaunchKernelGGL(k_best_emit, dim3(g), dim3(256), 0, st, h->out.as<BhipHit>(), n_host, n_dev, h->ref_order.as<uint32_t>(), cnt, h->best_key.as<unsigned long long>(), off, sorted.as<BhipHit>(), qmap);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(h->nsel_pinned, off + n_q, 4, hipMemcpyDeviceToHost, st));      // (the scan runs over n_q + 1 counters, the last one zero: its offset is the total)
		return 0;
	}
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(h->sort_tmp.p, tmp_bytes, cnt, off, (int)(n_q + 1), st));
	hipLaunchKernelGGL(k_hit_scatter, dim3(g), dim3(256), 0, st, h->out.as<BhipHit>(), n_host, n_dev, off, rank, sorted.as<BhipHit>(), qmap);
	hipLaunchKernelGGL(k_hit_fix, dim3(std::min<uint32_t>((n_q + 255) / 256, (uint32_t)h->n_cu * 8)), dim3(256), 0, st, sorted.as<BhipHit>(), off, cnt, n_q, h->sort_scratch.as<BhipHit>(), (uint32_t)(h->sort_scratch.cap / sizeof(BhipHit)));
	HIPCHK(hipGetLastError());
	return 0;
}
// The records are grouped right behind the re-scorer, with the record count read on the device: no host round trip between the two
// (counts and ranks were taken by the re-scoring kernels as they wrote the records).  Void when a lane needs the wide-band re-scorer
// afterwards: more records are on their way then, and deliver() groups them all.
static int enqueue_grouping_ahead(Handle *h, BatchCall &b) {
	int rc;
	b.o_ahead = (h->opt_async_d2h && b.hits) ? (h->out_idx ^ 1) : 0;
	DBuf &sorted = b.o_ahead ? h->out_sorted2 : h->out_sorted;
	if ((rc = h->sort_idx.reserve((size_t)h->out_cap * 4)) || (rc = h->sort_keys.reserve((size_t)(b.n_q + 1) * 4)) || (rc = h->sort_keys2.reserve((size_t)(b.n_q + 1) * 4)) ||
	    (rc = sorted.reserve((size_t)h->out_cap * sizeof(BhipHit))) || (rc = h->sort_scratch.reserve((size_t)h->out_cap * sizeof(BhipHit)))) return rc;
	if ((rc = plan_scan(h, b, h->post_stream))) return rc;
	if (h->copy_pending[b.o_ahead]) HIPCHK(hipStreamWaitEvent(h->post_stream, h->ev_copied[b.o_ahead], 0));      // the copy that last read this buffer
	HIPCHK(hipEventRecord(h->ev[EV_GROUP_START], h->post_stream));
	if ((rc = enqueue_grouping(h, b, h->post_stream, (uint32_t)h->out_cap, &h->shared_ctr.as<SharedCtr>()->n_out, sorted))) return rc;
	HIPCHK(hipEventRecord(h->ev[EV_GROUP_DONE], h->post_stream));
	b.sorted_ahead = true;
	return BHIP_OK;
}

// Enqueue a whole chain, nothing waited for: the resets of the batch-wide buffers, every lane, the grouping ahead, the read-back of the shared
// counters; then the seed lookups of the next staged batch and -- first attempt only -- the caller's hook.
static int enqueue_chain(Handle *h, BatchCall &b, int attempt) {
	int rc;
	const uint32_t n_q = b.n_q;
	b.sorted_ahead = false;
	if ((rc = h->best.reserve((size_t)(b.n_shared + 1) * 4)) || (rc = h->out.reserve(h->out_cap * sizeof(BhipHit))) || (rc = h->shared_ctr.reserve(sizeof(SharedCtr)))) return rc;
	HIPCHK(hipEventRecord(h->ev[EV_BEGIN], h->stream));
	HIPCHK(hipMemsetAsync(h->best.p, 0xFF, (size_t)b.n_shared * 4, h->stream));
	HIPCHK(hipMemsetAsync(h->shared_ctr.p, 0, 2 * sizeof(uint32_t), h->stream));
	// the counting sort's counters (zeroed here, off the critical path) and ranks, for the re-scoring kernels
	if ((rc = h->sort_idx.reserve((size_t)h->out_cap * 4)) || (rc = h->sort_keys.reserve((size_t)(n_q + 1) * 4))) return rc;
	HIPCHK(hipMemsetAsync(h->sort_keys.p, 0, (size_t)(n_q + 1) * 4, h->stream));
	if (b.sel_best) HIPCHK(hipMemsetAsync(h->best_key.p, 0xFF, (size_t)(n_q + 1) * 8, h->stream));
	hipLaunchKernelGGL(k_set_rank_ptrs, dim3(1), dim3(1), 0, h->stream, h->shared_ctr.as<SharedCtr>(), h->sort_keys.as<uint32_t>(), h->sort_idx.as<uint32_t>());
	HIPCHK(hipEventRecord(h->ev[EV_RESET_DONE], h->stream));
	HIPCHK(hipStreamWaitEvent(h->sweep_stream, h->ev[EV_RESET_DONE], 0));
	// (the prefilter stream does not wait for these fills: nothing it runs touches `best` or the shared counters -- the sweeps and the
	// re-scorer do, on the stream the fills are on -- and the previous batch has been waited for by the host: the prefilter starts
	// ~75 us earlier)
	HIPCHK(hipStreamWaitEvent(h->post_stream, h->ev[EV_RESET_DONE], 0));
	for (uint32_t l = 0; l < b.nl; ++l) if (h->lanes[l]->n_entries) if ((rc = enqueue_lane(h, h->lanes[l], b))) return rc;
	HIPCHK(hipEventRecord(h->ev[EV_PF_DONE], h->pf_stream));          // this batch's share of the prefilter stream ends here
	if ((rc = enqueue_grouping_ahead(h, b))) return rc;
	if (!h->hsc_pinned) HIPCHK(hipHostMalloc((void **)&h->hsc_pinned, sizeof(SharedCtr), hipHostMallocDefault));
	HIPCHK(hipMemcpyAsync(h->hsc_pinned, h->shared_ctr.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->post_stream));
	HIPCHK(hipEventRecord(h->ev[EV_CHAIN_DONE], h->post_stream));
	seed_next_batch(h, b.slot, h->ev[EV_CHAIN_DONE]);
	if (h->enqueued_hook && attempt == 0) h->enqueued_hook(h->enqueued_ctx);      // the caller's host work for later batches, while the device is busy with this one
	return BHIP_OK;
}
static int wait_chain(Handle *h, const BatchCall &b) {
	HIPCHK(hipEventSynchronize(h->ev[EV_PF_DONE]));
	HIPCHK(hipStreamSynchronize(h->sweep_stream));
	HIPCHK(hipStreamSynchronize(h->post_stream));
	for (uint32_t l = 0; l < b.nl; ++l) if (h->lanes[l]->n_entries) h->lanes[l]->hc = *h->lanes[l]->hc_pinned;
	return BHIP_OK;
}
// a lane whose records mostly survive the counting filter does better with the exact table
static void adapt_prefilter_algo(Handle *h, const BatchCall &b) {
	for (uint32_t l = 0; l < b.nl; ++l) {
		Lane *L = h->lanes[l];
		// (with the minimum-only semantics the counting-filter kernel also splits off the lanes that cannot hold a minimum --
		// the second sweep -- which the exact-table kernel does not: it only takes over when most records survive)
		// Round 6: measured again with k_prefilter_cq on a database with strain-level redundancy (57 % of the records survive its filter: a read
		// of a 500-strain family meets the family's clumps in every one of its lists): the exact-table kernel took 61.5 ms per 2 M reads where
		// k_prefilter_cq takes 8.5 (gpurun_out/r06a, r06b) -- with the minimum-only semantics the switch is off while that kernel is in use
		const bool cq_min_only = !b.all_hits && h->opt_pf_cw == 2 && L->pf_algo_used == 3;
		// (survivors per prefiltered query of this chain: bhip_pf_group keeps a strain-rich lane at 16 lanes per query from its second batch on)
		uint32_t n_pf = 0;
		for (int cls = 0; cls < kNumClasses; ++cls) n_pf += L->npf[cls];
		if (L->n_entries && n_pf) L->pf_surv_per_query = (double)L->hc.surv_sum / (double)n_pf;
		if (L->n_entries && L->pf_algo == 0 && !cq_min_only && L->hc.ent_read > 100000 && (double)L->hc.surv_sum > (b.all_hits ? 0.20 : 0.50) * (double)L->hc.ent_read) L->pf_algo = 1;
	}
}
static void print_chain_counters(const Handle *h, const BatchCall &b) {      // BHIP_DEBUG
	for (uint32_t l = 0; l < b.nl; ++l) {
		const Lane *L = h->lanes[l];
		if (!L->n_entries) continue;
		fprintf(stderr, "[bhip] lane %u: %llu list records, %llu survived the counting filter, next prefilter algorithm %d\n", l, (unsigned long long)L->hc.ent_read, (unsigned long long)L->hc.surv_sum, L->pf_algo);
		for (int cls = 0; cls < kNumClasses; ++cls) if (L->npf[cls] + L->nex[cls])
			fprintf(stderr, "[bhip] lane %u class NW=%d: prefiltered %u exhaustive %u maxE %u maxwords %u | tasks %u + deferred %u (kept %u) clump pairs %u windows %u + %u | fallback queries(last class) %u raw %u\n",
				l, kClasses[cls], L->npf[cls], L->nex[cls], L->maxE[cls], L->maxwords[cls], L->hc.n_tasks_cls[cls], L->hc.n_tasks2_cls[cls], L->hc.n_tasks2k_cls[cls], L->hc.n_cand_cls[cls], L->hc.n_wins_cls[cls], L->hc.n_wins2_cls[cls], L->hc.n_fb, L->hc.n_raw);
		if (L->hc.n_fb) fprintf(stderr, "[bhip] lane %u: %u queries overflowed the first prefilter pass, %u the second (dense fallback)\n", l, L->hc.n_fb, L->hc.n_fb2);
		const uint32_t *rs = L->hc.n_rs;      // hits per re-scorer variant (k_rescore_classify's buckets; exact matches leave there and are not counted)
		fprintf(stderr, "[bhip] lane %u: re-scorer bands 4:%u 6:%u 8:%u 12:%u 16:%u 24:%u 32:%u 40:%u 48:%u lds:%u scratch:%u\n",
			l, rs[0], rs[1], rs[2], rs[3], rs[4], rs[5], rs[6], rs[7], rs[8], rs[9], L->hc.n_wide);
		// where the packed queries came from (option "fetch_once", bhip_fetch_plan.h): form / bytes of dynamic LDS per block
		if (h->opt_rescore_reg) {
			static const char *const qf_name[BHIP_QF_COUNT] = {"dword", "lds", "chunk"};
			const BhipQueryFetch *f = L->qfetch;      // (by register set: 0 = 4 .. 8 diagonals, 3 = 12, 1 = 16 / 24, 2 = 32 .. 48)
			fprintf(stderr, "[bhip] lane %u: re-scorer query fetch 4-8:%s/%u 12:%s/%u 16-24:%s/%u 32-48:%s/%u\n", l, qf_name[f[0].form], f[0].lds_bytes,
				qf_name[f[3].form], f[3].lds_bytes, qf_name[f[1].form], f[1].lds_bytes, qf_name[f[2].form], f[2].lds_bytes);
		}
	}
}
// capacity checks of the lanes' buffers (first call of a workload: grow and redo)
static int grow_lane_capacities(Handle *h, const BatchCall &b) {
	bool redo = false;
	for (uint32_t l = 0; l < b.nl; ++l) {
		Lane *L = h->lanes[l];
		if (!L->n_entries) continue;
		const Counters &c = L->hc;
		for (int cls = 0; cls < kNumClasses; ++cls) {
			redo |= grow_cap(L->cand_cap, c.n_cand_cls[cls], true, (int)l, "cand");
			redo |= grow_cap(L->task_cap, c.n_tasks_cls[cls], true, (int)l, "tasks");
			redo |= grow_cap(L->task_cap, c.n_tasks2_cls[cls], true, (int)l, "tasks");
			redo |= grow_cap(L->win_cap, c.n_wins2_cls[cls], true, (int)l, "wins");
			redo |= grow_cap(L->win_cap, c.n_wins_cls[cls], true, (int)l, "wins");
		}
		redo |= grow_cap(L->raw_cap, c.n_raw, true, (int)l, "raw");
	}
	return redo ? STEP_REDO : BHIP_OK;
}
// Rare: bands wider than the LDS plan (repeats inside one shear) go through the global-scratch variant of the re-scorer, lane by lane, each
// waited for.  Then the shared counters as they stand behind the last re-scorer.  Redo: the scratch was too small for a lane's bands.
static int rescore_wide_bands(Handle *h, BatchCall &b) {
	bool redo = false;
	const RefArgs R = ref_args(h);
	SharedCtr *sc = h->shared_ctr.as<SharedCtr>();
	for (uint32_t l = 0; l < b.nl; ++l) {
		Lane *L = h->lanes[l];
		if (!L->n_entries || !L->hc.n_wide) continue;
		b.sorted_ahead = false;                  // more records are on their way
		if (getenv("BHIP_DEBUG")) fprintf(stderr, "[bhip] lane %u: n_wide %u hits through the global-scratch re-scorer\n", l, L->hc.n_wide);
		Counters *dc = L->counters.as<Counters>();
		hipLaunchKernelGGL(k_rescore<true>, dim3(std::min<uint32_t>((L->hc.n_wide + 63) / 64, (uint32_t)h->n_cu * 16)), dim3(64), 256, h->post_stream,
			L->raw.as<BhipRawHit>(), &dc->n_raw, (uint32_t)L->raw_cap, L->wide.as<uint32_t>(), &dc->n_wide, h->best.as<uint32_t>(), b.all_hits,
			h->cur->qcodes.as<uint8_t>(), h->cur->qoff.as<uint64_t>(), six_or_null(h), rc_or_null(h),
			R.bytes(), R.off, R.len, h->lut.as<uint8_t>(), h->out.as<BhipHit>(),
			&sc->n_out, (uint32_t)h->out_cap, (uint32_t *)nullptr, (uint32_t *)nullptr, L->scratch.as<uint32_t>(), &dc->scratch_used,
			(unsigned long long)L->scratch_cap, &sc->err, (const uint32_t *)nullptr, 0u, 0u, 0u);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(&L->hc, dc, sizeof(Counters), hipMemcpyDeviceToHost, h->post_stream));
		HIPCHK(hipStreamSynchronize(h->post_stream));
		redo |= grow_cap(L->scratch_cap, L->hc.scratch_used, false, (int)l, "scratch");
	}
	if (b.sorted_ahead) b.hsc = *h->hsc_pinned;      // (nothing ran after the chain: the copy behind it is current)
	else HIPCHK(hipMemcpy(&b.hsc, h->shared_ctr.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return redo || (b.hsc.err & 2u) ? STEP_REDO : BHIP_OK;
}
// the shared error bits and the record buffer; then the number of records is known
static int check_shared_counters(Handle *h, BatchCall &b) {
	if (b.hsc.err & 1u) return fail(BHIP_E_RESCORE, "re-scoring could not reproduce a hit found by the edit-distance kernel (a query starting with a symbol outside the alphabet? the reference stops here as well: CRITICAL ERROR: Truncation within known good path, burst.c:812-816)");
	if (grow_cap(h->out_cap, b.hsc.n_out, true, -1, "out")) return STEP_REDO;
	b.n_deliver = b.sel_best ? (b.sorted_ahead ? *h->nsel_pinned : std::min<uint32_t>(b.hsc.n_out, b.n_q)) : b.hsc.n_out;      // (not grouped yet: an upper bound; deliver()'s grouping gives the number)
	*b.n_hits = b.n_deliver;
	h->last_n_out = 0;
	return BHIP_OK;
}
// statistics of a chain that went through, and the note that its records are resident
static void collect_stats(Handle *h, const BatchCall &b) {
	BhipStats &S = h->stats;
	S.n_queries = b.n_q; S.n_hits = b.n_deliver;
	uint64_t qlen_sum = 0;
	for (uint32_t l = 0; l < b.nl; ++l) {
		Lane *L = h->lanes[l];
		if (!L->n_entries) continue;
		const Counters &c = L->hc;
		S.n_pairs += L->n_pairs_ex + c.unit_sum; S.n_columns += c.col_sum; S.n_task_columns += c.tcol_sum; S.n_raw_hits += c.n_raw; S.acx_entries_read += c.ent_read;
		S.myers_launches += L->launches; S.prefilter_launches += L->pf_launches; if (L->pf_launches) S.prefilter_algo = (uint32_t)L->pf_algo_used; S.n_window_columns += c.wcol_sum; qlen_sum += c.qlen_sum;
		if (L->prefix_words) S.prefix_words = L->prefix_words;
		for (int cls = 0; cls < kNumClasses; ++cls) {
			S.n_pairs += c.n_cand_cls[cls]; S.n_windows += c.n_wins_cls[cls] + c.n_wins2_cls[cls]; S.n_lane_tasks += c.n_tasks_cls[cls] + c.n_tasks2k_cls[cls];
			if (!(L->npf[cls] + L->nex[cls])) continue;
			hipEvent_t *ce = L->ev_cls[cls];
			S.ms_peq += L->peq_ahead[cls] ? ev_ms(L->ev_peq_cur[SPAN_START], L->ev_peq_cur[SPAN_DONE]) : ev_ms(ce[CE_START], ce[CE_PEQ_DONE]);
			if (L->npf[cls]) S.ms_prefilter += ev_ms(ce[CE_PF_START], ce[CE_PF_DONE]);
			if (L->npf[cls] && L->pf_masked[cls]) {
				hipEvent_t *es = L->ev_seed[h->cur->seq & 1][cls];
				S.ms_seed += ev_ms(es[SPAN_START], es[SPAN_DONE]); S.ms_prefilter_hash += ev_ms(L->ev_pf[cls][PF_HASH_START], L->ev_pf[cls][PF_HASH_DONE]); S.n_seed_words += L->seed_words[cls];
			}
			float sweep = ev_ms(ce[CE_SWEEP_START], ce[CE_SWEEP_EX_DONE]), win = ev_ms(ce[CE_SWEEP_EX_DONE], ce[CE_WIN_DONE]);
			if (L->pruned[cls]) { const float second = ev_ms(L->ev_ph[cls][PH_WIN_DONE], L->ev_ph[cls][PH_SWEEP2_DONE]); sweep += second; win -= second; }   // filter + second task sweep sit between the two window launches
			S.ms_myers += sweep + win;
			if (L->prefix_words) { S.ms_myers_prefix += sweep; S.ms_myers_window += win; }
		}
		S.ms_rescore += ev_ms(L->ev_rs[RS_START], L->ev_rs[RS_DONE]);
	}
	S.bytes_algorithmic = 8ull * S.n_columns + qlen_sum / 2 + 192ull * S.n_pairs;
	h->res_valid = true; h->res_seq = b.slot->seq; h->res_all_hits = b.mode; h->res_n = b.n_deliver; h->res_n_raw = b.hsc.n_out; h->res_stats = h->stats;
}
// one attempt at the chain: enqueue, wait, check
static int run_chain(Handle *h, BatchCall &b, int attempt) {
	int rc;
	if ((rc = enqueue_chain(h, b, attempt)) || (rc = wait_chain(h, b))) return rc;
	adapt_prefilter_algo(h, b);
	if (getenv("BHIP_DEBUG")) print_chain_counters(h, b);
	if ((rc = grow_lane_capacities(h, b)) || (rc = rescore_wide_bands(h, b)) || (rc = check_shared_counters(h, b))) return rc;
	collect_stats(h, b);
	return BHIP_OK;
}

// The records were not grouped behind the re-scorer (or into the other buffer): count, scan, group on the main stream.  With sel_best the
// number of selected records is only known afterwards (rare path: records that stayed resident, wide bands).
static int group_late(Handle *h, BatchCall &b, int o, DBuf &sorted) {
	int rc;
	const uint32_t n = b.hsc.n_out, n_q = b.n_q;
	if (h->copy_pending[o]) { HIPCHK(hipEventSynchronize(h->ev_copied[o])); h->copy_pending[o] = false; }    // the copy that last read this buffer
	if ((rc = sorted.reserve((size_t)n * sizeof(BhipHit))) || (rc = h->sort_scratch.reserve((size_t)n * sizeof(BhipHit)))) return rc;
	uint32_t *cnt = h->sort_keys.as<uint32_t>(), *rank = h->sort_idx.as<uint32_t>();
	HIPCHK(hipMemsetAsync(cnt, 0, (size_t)(n_q + 1) * 4, h->stream));
	if (b.sel_best) HIPCHK(hipMemsetAsync(h->best_key.p, 0xFF, (size_t)(n_q + 1) * 8, h->stream));
	b.mark(0);
	hipLaunchKernelGGL(k_hit_count, dim3(std::min<uint32_t>((n + 255) / 256, (uint32_t)h->n_cu * 8)), dim3(256), 0, h->stream, h->out.as<BhipHit>(), n, (const uint32_t *)nullptr, cnt, rank);
	if ((rc = plan_scan(h, b, h->stream)) || (rc = enqueue_grouping(h, b, h->stream, n, (const uint32_t *)nullptr, sorted))) return rc;
	if (b.sel_best) {
		HIPCHK(hipStreamSynchronize(h->stream));
		b.n_deliver = *h->nsel_pinned; *b.n_hits = b.n_deliver; h->stats.n_hits = b.n_deliver; h->res_n = b.n_deliver;
		if (b.hits && b.n_deliver > b.cap) return fail(BHIP_E_CAPACITY, "hit buffer holds %llu records, %u needed", (unsigned long long)b.cap, b.n_deliver);
	}
	return BHIP_OK;
}
// Page-lock the caller's buffer for the asynchronous copy out of slot o (kept registered: callers alternate between two buffers).
// ok: the buffer is page-locked -- by this or an earlier call, or by the caller (bhip_alloc_host / bhip_host_register).
static int lock_caller_buffer(Handle *h, BhipHit *hits, size_t want, size_t bytes, int o, bool &ok) {
	if (!h->copy_stream) { HIPCHK(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking)); HIPCHK(hipEventCreateWithFlags(&h->ev_sorted, hipEventDisableTiming));
		for (auto &e : h->ev_copied) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
	ok = h->reg_ptr[o] == (void *)hits && h->reg_bytes[o] >= bytes;
	if (!ok) {
		hipPointerAttribute_t at;
		memset(&at, 0, sizeof at);
		if (hipPointerGetAttributes(&at, (const void *)hits) == hipSuccess && at.type == hipMemoryTypeHost) ok = true;
		else (void)hipGetLastError();
	}
	if (!ok) {
		if (h->reg_ptr[o]) { (void)hipHostUnregister(h->reg_ptr[o]); h->reg_ptr[o] = nullptr; }
		if (h->reg_ptr[o ^ 1] == (void *)hits) { if (h->copy_pending[o ^ 1]) { HIPCHK(hipEventSynchronize(h->ev_copied[o ^ 1])); h->copy_pending[o ^ 1] = false; }
			(void)hipHostUnregister(h->reg_ptr[o ^ 1]); h->reg_ptr[o ^ 1] = nullptr; }
		if (hipHostRegister((void *)hits, want, hipHostRegisterDefault) == hipSuccess) { h->reg_ptr[o] = (void *)hits; h->reg_bytes[o] = want; ok = true; }
		else (void)hipGetLastError();
	}
	return BHIP_OK;
}
// Hand the records over: grouped late where they were not grouped ahead, then copied into the caller's buffer -- on the copy stream behind
// the call (option async_d2h, page-locked buffer) or on the main stream, which is waited for.
static int deliver(Handle *h, BatchCall &b) {
	int rc;
	BhipStats &S = h->stats;
	if (b.hits && b.n_deliver > b.cap) return fail(BHIP_E_CAPACITY, "hit buffer holds %llu records, %u needed", (unsigned long long)b.cap, b.n_deliver);
	HIPCHK(hipEventRecord(h->ev[EV_DELIVER_START], h->stream));
	b.t0 = std::chrono::steady_clock::now();
	if (b.hsc.n_out) {
		if ((rc = h->sort_idx.reserve(std::max<size_t>((size_t)b.hsc.n_out, b.sel_best ? (size_t)b.n_q + 1 : 0) * 4)) || (rc = h->sort_keys.reserve((size_t)(b.n_q + 1) * 4)) ||
		    (rc = h->sort_keys2.reserve((size_t)(b.n_q + 1) * 4))) return rc;
		const bool async = h->opt_async_d2h && b.hits;
		const int o = async ? (h->out_idx ^= 1) : 0;
		DBuf &sorted = o ? h->out_sorted2 : h->out_sorted;
		if (b.sorted_ahead && o == b.o_ahead) b.mark(0);          // grouped already, behind the re-scorer
		else if ((rc = group_late(h, b, o, sorted))) return rc;
		b.mark(1);
		const size_t bytes = (size_t)b.n_deliver * sizeof(BhipHit);
		bool queued = false;
		if (async) {
			if ((rc = lock_caller_buffer(h, b.hits, (size_t)b.cap * sizeof(BhipHit), bytes, o, queued))) return rc;
			b.mark(2);
			if (queued) {
				HIPCHK(hipEventRecord(h->ev_sorted, h->stream));
				HIPCHK(hipStreamWaitEvent(h->copy_stream, h->ev_sorted, 0));
				HIPCHK(hipMemcpyAsync(b.hits, sorted.p, bytes, hipMemcpyDeviceToHost, h->copy_stream));
				HIPCHK(hipEventRecord(h->ev_copied[o], h->copy_stream));
				h->copy_pending[o] = true;
			}
		}
		if (b.hits && !queued) HIPCHK(hipMemcpyAsync(b.hits, sorted.p, bytes, hipMemcpyDeviceToHost, h->stream));
		h->last_n_out = b.n_deliver; h->last_out = o;
	}
	b.mark(3);
	HIPCHK(hipEventRecord(h->ev[EV_DELIVER_DONE], h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	if (getenv("BHIP_DEBUG_TIMES")) {
		const double *t = b.t_host, t_sync = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b.t0).count() - t[3];
		fprintf(stderr, "[bhip] delivery host ms: reserve+memset %.3f, sort launches %.3f, pointer check %.3f, copy enqueue %.3f, sync %.3f\n", t[0], t[1] - t[0], t[2] - t[1], t[3] - t[2], t_sync);
	}
	S.ms_h2d = h->cur->st_ms_h2d; S.ms_stage_copy = h->cur->st_ms_copy; S.ms_stage_route = h->cur->st_ms_route;
	S.ms_d2h = ev_ms(h->ev[EV_DELIVER_START], h->ev[EV_DELIVER_DONE]) + (b.sorted_ahead ? ev_ms(h->ev[EV_GROUP_START], h->ev[EV_GROUP_DONE]) : 0.0f); S.ms_total = ev_ms(h->ev[EV_BEGIN], h->ev[EV_DELIVER_DONE]);
	b.slot->state = 2;
	h->res_valid = false;
	return BHIP_OK;
}

extern "C" int bhip_align_staged(void *handle, int all_hits_arg, BhipHit *hits, uint64_t cap, uint64_t *n_hits) {
	Handle *h = (Handle *)handle;
	if (!h || !n_hits) return fail(BHIP_E_ARG, "null argument");
	*n_hits = 0;
	if (all_hits_arg < 0 || all_hits_arg > BHIP_HITS_BEST) return fail(BHIP_E_ARG, "all_hits must be 0, 1 or 2 (BHIP_HITS_BEST)");
	BatchCall b;
	b.mode = all_hits_arg; b.all_hits = all_hits_arg == BHIP_HITS_ALL ? 1 : 0; b.sel_best = all_hits_arg == BHIP_HITS_BEST;
	b.hits = hits; b.cap = cap; b.n_hits = n_hits;
	if (b.sel_best && !h->n_order) return fail(BHIP_E_ARG, "BHIP_HITS_BEST needs the reference order table (bhip_set_ref_order)");
	memset(&h->stats, 0, sizeof h->stats);
	HIPCHK(hipSetDevice(h->device));
	int rc;
	if ((rc = pick_batch(h, b))) return rc;
	if (!b.n_q) { b.slot->state = 2; return BHIP_OK; }
	if ((rc = plan_batch(h, b))) return rc;
	if (records_resident(h, b)) take_resident(h, b);
	else {
		h->res_valid = false;
		rc = STEP_REDO;
		for (int attempt = 0; attempt < 24 && rc == STEP_REDO; ++attempt) rc = run_chain(h, b, attempt);
		if (rc == STEP_REDO) return fail(BHIP_E_INTERNAL, "buffers kept overflowing");
		if (rc) return rc;
	}
	return deliver(h, b);
}

extern "C" int bhip_align_batch(void *handle, const uint8_t *q_codes, const uint64_t *q_off, const uint16_t *q_emac,
                                const uint32_t *q_six, const uint8_t *q_rc, const uint8_t *q_flags,
                                uint32_t n_q, uint32_t n_shared, int all_hits,
                                BhipHit *hits, uint64_t cap, uint64_t *n_hits) {
	if (!n_hits) return fail(BHIP_E_ARG, "null argument");
	*n_hits = 0;
	int rc = bhip_stage_queries(handle, q_codes, q_off, q_emac, q_six, q_rc, q_flags, n_q, n_shared);
	if (rc) return rc;
	return bhip_align_staged(handle, all_hits, hits, cap, n_hits);
}

extern "C" int bhip_align_pairs(void *handle, const uint8_t *q_codes, const uint64_t *q_off, const uint16_t *q_emac,
                                uint32_t n_q, const uint32_t *pair_q, const uint32_t *pair_clump, uint64_t n_pairs, uint8_t *mins) {
	Handle *h = (Handle *)handle;
	if (!h || !q_codes || !q_off || !q_emac || !pair_q || !pair_clump || !mins) return fail(BHIP_E_ARG, "null argument");
	memset(&h->stats, 0, sizeof h->stats);
	for (StageSlot &S : h->slots) { S.state = 0; S.st_valid = false; }
	h->cur = &h->slots[0];
	if (!n_pairs || !n_q) return BHIP_OK;
	HIPCHK(hipSetDevice(h->device));
	int rc;
	if ((rc = ensure_lanes(h, 1))) return rc;
	Lane *L = h->lanes[0];
	uint32_t maxlen = 0;
	for (uint32_t i = 0; i < n_q; ++i) maxlen = std::max<uint32_t>(maxlen, (uint32_t)(q_off[i + 1] - q_off[i]));
	if (maxlen > BHIP_MAX_QLEN) return fail(BHIP_E_QUERYLEN, "query longer than %d", BHIP_MAX_QLEN);
	const int cls = class_of_len(std::max<uint32_t>(maxlen, 1)), NW = class_words(cls, maxlen);
	std::vector<uint2> pr(n_pairs);
	for (uint64_t p = 0; p < n_pairs; ++p) {
		if (pair_q[p] >= n_q || pair_clump[p] >= h->n_clumps) return fail(BHIP_E_ARG, "pair %llu out of range", (unsigned long long)p);
		pr[p] = make_uint2(pair_q[p], pair_clump[p]);
	}
	h->cur->st_has_six = false; h->cur->st_has_rc = false;
	if ((rc = upload_queries(h, q_codes, q_off, q_emac, nullptr, nullptr, n_q))) return rc;
	if ((rc = L->peq.reserve((size_t)n_q * 16 * NW * 4))) return rc;
	if ((rc = h->pairs.reserve(n_pairs * sizeof(uint2)))) return rc;
	if ((rc = h->mins.reserve(n_pairs * 16))) return rc;
	hipStream_t st = h->stream;
	HIPCHK(hipMemcpyAsync(h->pairs.p, pr.data(), n_pairs * sizeof(uint2), hipMemcpyHostToDevice, st));
	HIPCHK(hipMemsetAsync(L->counters.p, 0, sizeof(Counters), st));
	Counters *dc = L->counters.as<Counters>();
	const uint32_t qb = 256u / (uint32_t)NW;
	hipLaunchKernelGGL(k_build_peq, dim3((uint32_t)std::min<uint64_t>(((uint64_t)n_q + qb - 1) / qb, (uint64_t)h->n_cu * 16)), dim3(256), 0, st,
		h->cur->qcodes.as<uint8_t>(), h->cur->qoff.as<uint64_t>(), (const uint32_t *)nullptr, n_q, NW, 0, h->mm, L->peq.as<uint32_t>(), (const uint32_t *)nullptr, 0u, h->peq_rows);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(h->ev[EV_BEGIN], st));
	launch_myers(h, L, st, NW, (uint32_t)std::min<uint64_t>((n_pairs + 15) / 16, (uint64_t)h->n_cu * 8), h->pairs.as<uint2>(), nullptr, n_pairs, 0, nullptr,
		nullptr, nullptr, 0, nullptr, h->mins.as<uint8_t>(), dc);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(h->ev[EV_KERNEL_DONE], st));
	HIPCHK(hipMemcpyAsync(mins, h->mins.p, n_pairs * 16, hipMemcpyDeviceToHost, st));
	Counters hc;
	HIPCHK(hipMemcpyAsync(&hc, dc, sizeof hc, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	h->stats.n_queries = n_q; h->stats.n_pairs = n_pairs; h->stats.n_columns = hc.col_sum; h->stats.myers_launches = 1;
	h->stats.bytes_algorithmic = 8ull * hc.col_sum + hc.qlen_sum / 2 + 192ull * n_pairs;
	h->stats.ms_myers = ev_ms(h->ev[EV_BEGIN], h->ev[EV_KERNEL_DONE]); h->stats.ms_total = h->stats.ms_myers;
	return BHIP_OK;
}

extern "C" int bhip_prefilter(void *handle, const uint8_t *q_codes, const uint64_t *q_off, const uint16_t *q_emac, uint32_t n_q,
                              uint32_t *out_q, uint32_t *out_clump, uint32_t *out_count, uint64_t cap, uint64_t *n_out) {
	Handle *h = (Handle *)handle;
	if (!h || !q_codes || !q_off || !q_emac || !n_out) return fail(BHIP_E_ARG, "null argument");
	if (!h->has_acx) return fail(BHIP_E_ARG, "handle has no accelerator");
	*n_out = 0;
	for (StageSlot &S : h->slots) { S.state = 0; S.st_valid = false; }
	h->cur = &h->slots[0];
	if (!n_q) return BHIP_OK;
	HIPCHK(hipSetDevice(h->device));
	int rc;
	if ((rc = ensure_lanes(h, 1))) return rc;
	Lane *L = h->lanes[0];
	for (int attempt = 0; attempt < 4; ++attempt) {
		if ((rc = upload_queries(h, q_codes, q_off, q_emac, nullptr, nullptr, n_q))) return rc;
		{
			std::vector<uint32_t> plan(n_q, 1u);
			for (uint32_t i = 0; i < n_q; ++i) plan[i] = make_seed_plan(q_codes + q_off[i], (uint32_t)(q_off[i + 1] - q_off[i]), q_emac[i], (uint32_t)h->K, h->opt_prefilter_stride, h->alt);
			if ((rc = upload_plan(h, n_q, plan))) return rc;
			// 4-bit packed copy of the queries at a fixed stride (layout used by the seed, profile and re-scoring kernels)
			const uint32_t qw_g = (h->cur->st_maxlen + 7) / 8;
			if ((rc = h->cur->qpack.reserve((size_t)n_q * qw_g * 4 + 16))) return rc;
			const uint64_t total = (uint64_t)n_q * qw_g;
			if (total) hipLaunchKernelGGL(k_pack_queries, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, (uint64_t)h->n_cu * 16)), dim3(256), 0, h->stream,
				h->cur->qcodes.as<uint8_t>(), h->cur->qoff.as<uint64_t>(), n_q, qw_g, h->cur->qpack.as<uint32_t>());
			HIPCHK(hipGetLastError());
		}
		if ((rc = L->cand.reserve(L->cand_cap * sizeof(uint2)))) return rc;
		if ((rc = L->candcnt.reserve(L->cand_cap * sizeof(uint32_t)))) return rc;
		HIPCHK(hipStreamSynchronize(h->stream));
		HIPCHK(hipMemsetAsync(L->counters.p, 0, sizeof(Counters), L->stream));
		Counters *dc = L->counters.as<Counters>();
		HIPCHK(hipEventRecord(h->ev[EV_BEGIN], L->stream));
		if ((rc = launch_prefilter(h, L, L->stream, nullptr, n_q, L->cand.as<uint2>(), L->candcnt.as<uint32_t>(), (uint32_t)L->cand_cap, false, &dc->n_cand, dc))) return rc;
		HIPCHK(hipEventRecord(h->ev[EV_KERNEL_DONE], L->stream));
		Counters hc;
		HIPCHK(hipMemcpyAsync(&hc, dc, sizeof hc, hipMemcpyDeviceToHost, L->stream));
		HIPCHK(hipStreamSynchronize(L->stream));
		if (hc.n_cand > L->cand_cap) { L->cand_cap = (uint64_t)hc.n_cand + 1024; continue; }
		*n_out = hc.n_cand;
		memset(&h->stats, 0, sizeof h->stats);
		h->stats.n_queries = n_q; h->stats.n_pairs = hc.n_cand; h->stats.acx_entries_read = hc.ent_read; h->stats.ms_prefilter = ev_ms(h->ev[EV_BEGIN], h->ev[EV_KERNEL_DONE]);
		if (hc.n_cand > cap) return fail(BHIP_E_CAPACITY, "candidate buffer holds %llu, %u needed", (unsigned long long)cap, hc.n_cand);
		std::vector<uint2> c(hc.n_cand); std::vector<uint32_t> cc(hc.n_cand);
		if (hc.n_cand) {
			HIPCHK(hipMemcpy(c.data(), L->cand.p, hc.n_cand * sizeof(uint2), hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(cc.data(), L->candcnt.p, hc.n_cand * sizeof(uint32_t), hipMemcpyDeviceToHost));
		}
		std::vector<uint32_t> ord(hc.n_cand);
		for (uint32_t i = 0; i < hc.n_cand; ++i) ord[i] = i;
		std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return c[a].x != c[b].x ? c[a].x < c[b].x : c[a].y < c[b].y; });
		for (uint32_t i = 0; i < hc.n_cand; ++i) {
			if (out_q) out_q[i] = c[ord[i]].x;
			if (out_clump) out_clump[i] = c[ord[i]].y;
			if (out_count) out_count[i] = cc[ord[i]];
		}
		return BHIP_OK;
	}
	return fail(BHIP_E_INTERNAL, "candidate buffer kept overflowing");
}

// Device-resident copy of the last call's records (same order as the host copy): for device-side collectives.
extern "C" int bhip_copy_hits_device(void *handle, void *dst_device, uint64_t cap_records, uint64_t *n_records) {
	Handle *h = (Handle *)handle;
	if (!h || !n_records) return fail(BHIP_E_ARG, "null argument");
	*n_records = h->last_n_out;
	if (!h->last_n_out) return BHIP_OK;
	// (a count query -- no destination, no room -- is answered like any buffer that is too small: BHIP_E_CAPACITY with *n_records set)
	if (!dst_device && cap_records) return fail(BHIP_E_ARG, "null destination");
	if (h->last_n_out > cap_records) return fail(BHIP_E_CAPACITY, "device buffer holds %llu records, %llu needed", (unsigned long long)cap_records, (unsigned long long)h->last_n_out);
	HIPCHK(hipSetDevice(h->device));
	HIPCHK(hipMemcpyAsync(dst_device, (h->last_out ? h->out_sorted2 : h->out_sorted).p, (size_t)h->last_n_out * sizeof(BhipHit), hipMemcpyDeviceToDevice, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	return BHIP_OK;
}

// With option "async_d2h" the records of bhip_align_staged / bhip_align_batch arrive in the caller's buffer behind the call
// (the count is final at return); this waits for every copy still in flight.
extern "C" int bhip_sync_hits(void *handle) {
	Handle *h = (Handle *)handle;
	if (!h) return fail(BHIP_E_ARG, "null handle");
	HIPCHK(hipSetDevice(h->device));
	for (int o = 0; o < 2; ++o) if (h->copy_pending[o]) { HIPCHK(hipEventSynchronize(h->ev_copied[o])); h->copy_pending[o] = false; }
	return BHIP_OK;
}

