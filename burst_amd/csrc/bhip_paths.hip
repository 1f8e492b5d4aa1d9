// burst_amd/csrc/bhip_paths.hip -- the alignment PATH of a placement (burst_hip --cigar; bhip_trace_paths, gfx950).  No reference
// counterpart: the reference reports how many mismatches and gaps a placement has (reScoreM_mat16, burst.c:713-886), never where.
//
// Definition ("Alignment paths").  For a record (query entry, refIx, finalPos, ed) the recurrence is the
// re-scorer's: planes D (score), H (left moves, gapQ), V (up moves, gapR), the tie-breaks of burst.c:771-798.  Every cell has a DECISION:
//   row 1      L if the cell's cost is 1 and the cell to its left scored 0 (burst.c:722-739), D otherwise
//   column 0   U
//   elsewhere  D if the diagonal is kept, U if it is not, L if the second comparison fails (burst.c:771-779, 789-795)
// The path starts at cell (m, finalPos), which must score ed, and follows the decisions back to row 0.  Forwards it reads
// D with cost 0 -> '=', D with cost 1 -> 'X', U -> 'I' (a query symbol without a reference column), L -> 'D' (a reference column
// without a query symbol); x0 + 1 = the first reference column the path consumes (x0 = the column at which row 0 is reached).
//
// The band.  Only the diagonals x - y in [finalPos - m - ed, finalPos - m + ed] are evaluated (2 ed + 1 cells per row), cells above ed
// collapsed to INVALID as in k_rescore.  Why that gives the decisions of the full matrix ON THE PATH:
//   - a cell off the band needs more than ed gap moves to reach (m, finalPos): it lies on no path of cost <= ed that ends there;
//   - call a cell GOOD when (its score) + (cheapest way from it to (m, finalPos)) = ed.  (m, finalPos) is good; a predecessor that ties
//     for the minimum of a good cell is good itself, hence on the band; a predecessor that does not tie has a score that is too high in
//     the full matrix, and the band can only raise a score (it removes predecessors), so it does not tie in the band either;
//   - by induction over the rows (and along a row, left to right) the score, H and V of every good cell are those of the full matrix:
//     its tied predecessors are good, so they are exact, and they are all the tie-breaks ever compare.
// The walk only visits good cells.  tests/test_gpu_paths.py holds the argument to a full-matrix restatement byte for byte.
//
// One work item per request.  A decision takes 2 bits (0 '=', 1 U, 2 L, 3 'X': the priority bits of the re-scorer's packed cell word,
// with the cost of a kept diagonal in the code that is otherwise unused).  Requests are grouped by band class on the host:
//   narrow  ed <= PATHS_NARROW_ED and m <= PATHS_NARROW_M: one decision word per row, band and decisions in LDS ([row][64 threads])
//   wide    everything else: decisions in the handle's grow-only scratch, [block][row][word][64 threads] -- the 64 stores of a wave for
//           one row word are one 256-byte line; the band in LDS up to 64 rows, in the scratch (same layout) beyond
// The wide requests are sorted by their scratch need, so that the 64 of a block are alike, and launched in groups that fit a fixed
// budget.  Ops are written backwards into a slot of 2 ed + 1 words per request (a path of cost ed has at most ed + 1 runs of '=' between
// its ed other ops), counted, scanned on the host, and gathered densely by a second kernel: what crosses PCIe is the ops themselves.
#include "bhip_handle.h"

#define PATHS_NARROW_ED 7u        // 15 diagonals: 30 bits of decisions per row
#define PATHS_NARROW_M  128u
#define PATHS_LDS_BAND  64u       // band rows (diagonals + 1 sentinel) kept in LDS by the wide kernel
#define PATHS_CHUNK_REQ (1u << 20)          // requests per upload
#define PATHS_CHUNK_SYM (1ull << 28)        // query symbols per upload (bytes)
#define PATHS_CHUNK_OPS (1ull << 26)        // op slots per upload (words)
#define PATHS_SCRATCH_WORDS (1ull << 27)    // decision + band scratch per launch (words: 512 MB)

struct PathReq { uint32_t qbase, m, refIx, finalPos, ed, opbase, pad0, pad1; };      // qbase: offset into the chunk's symbols; opbase: into its op slots
struct PathBlk { unsigned long long dec_off, band_off; uint32_t dw, pad; };          // wide class, per block: scratch offsets (words), decision words per row; band_off = ~0: LDS

__device__ __forceinline__ uint32_t paths_ref_dword(const uint32_t *__restrict__ refw, uint64_t clump_base, uint32_t z, int j8, uint32_t nchunks) {
	if (j8 < 0 || (uint32_t)j8 >= nchunks * 4) return 0u;
	return refw[(clump_base * 16 + (uint64_t)z * nchunks) * 4 + (uint32_t)j8];
}

// err[0] = lowest request (chunk-local index) whose cell (m, finalPos) does not score ed, err[1] = flags of what must not happen
// (1: the walk left the band, 2: more runs than the slot holds)
template <bool NARROW>
__global__ __launch_bounds__(64) void k_trace_paths(
		const PathReq *__restrict__ req, const uint32_t *__restrict__ list, uint32_t n, const PathBlk *__restrict__ blk,
		const uint8_t *__restrict__ qcodes, const uint32_t *__restrict__ refw, const uint64_t *__restrict__ ref_off, const uint32_t *__restrict__ clump_len,
		const uint8_t *__restrict__ lut, uint32_t *__restrict__ g_scratch,
		uint32_t *__restrict__ tmp_ops, uint32_t *__restrict__ n_ops, uint32_t *__restrict__ ref_first, uint32_t *__restrict__ gap_r, uint32_t *__restrict__ err) {
	extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
	__shared__ uint32_t s_mm[16];      // match masks as in k_rescore: bit r of s_mm[q] = (cost(q, r) == 0), bit 16 + r = (cost(q, r) != 255)
	const uint32_t tid = threadIdx.x;
	if (tid < 16) { uint32_t mk = 0; for (int r = 0; r < 16; ++r) mk |= (lut[16 * tid + r] == 0 ? 1u : 0u) << r | (lut[16 * tid + r] != 255 ? 1u : 0u) << (16 + r); s_mm[tid] = mk; }
	__syncthreads();
	const uint32_t li = blockIdx.x * 64 + tid;
	if (li >= n) return;
	const uint32_t ri = list[li];
	const PathReq rq = req[ri];
	const uint32_t B = rq.ed, c = rq.refIx >> 4, z = rq.refIx & 15, L = clump_len[c], nchunks = (L + 31) >> 5;
	const uint64_t cbase = ref_off[c];
	const int m = (int)rq.m, dlo = (int)rq.finalPos - m - (int)B, Wd = 2 * (int)B + 1;
	uint32_t *band, *dec; uint32_t DW;
	if (NARROW) { band = smem + tid; dec = smem + (2 * PATHS_NARROW_ED + 2) * 64 + tid; DW = 1; }
	else {
		const PathBlk b = blk[blockIdx.x];
		band = b.band_off == ~0ull ? smem + tid : g_scratch + b.band_off + tid;
		dec = g_scratch + b.dec_off + tid; DW = b.dw;
	}
	// the re-scorer's packed cell word (k_rescore): score | 255 - H | priority diag < up < left | V; the three-way choice is one minimum
	constexpr uint32_t SS = 18, GS = 10;
	const uint32_t INVALID = (512u << SS) | (255u << GS);
	const uint32_t STEP_U = (1u << SS) + 1u + (1u << 8), STEP_L = (1u << SS) - (1u << GS) + (2u << 8);
	for (int k = 0; k <= Wd; ++k) {      // row 0: D = 0 wherever the column exists (burst.c:4052)
		const int x = dlo + k;
		band[(uint32_t)k * 64] = (k < Wd && x >= 0 && x <= (int)L) ? (255u << GS) : INVALID;
	}
	for (int y = 1; y <= m; ++y) {
		const uint32_t qc = qcodes[rq.qbase + (uint32_t)(y - 1)] & 15u;
		const uint32_t mrow = s_mm[qc], m1 = mrow >> 16;
		const uint32_t col0 = (uint32_t)y <= B ? (((uint32_t)y << SS) | (255u << GS) | (uint32_t)y) : INVALID;   // D = y, H = 0, V = y (burst.c:747-750)
		const int x0 = y + dlo;
		uint32_t left = (x0 - 1 == 0) ? col0 : INVALID;
		int pos = x0 - 1;      // 0-based reference position of column x0
		uint32_t dw = paths_ref_dword(refw, cbase, z, pos >> 3, nchunks);
		uint32_t prev_sym = (y == 1) ? ((paths_ref_dword(refw, cbase, z, (pos - 1) >> 3, nchunks) >> (4 * ((pos - 1) & 7))) & 15u) : 0u;
		uint32_t dg = band[0], dacc = 0;
		uint32_t *drow = dec + (size_t)(y - 1) * DW * 64;
		for (int k = 0; k < Wd; ++k, ++pos) {
			const int x = x0 + k;
			if ((pos & 7) == 0 && k) dw = paths_ref_dword(refw, cbase, z, pos >> 3, nchunks);
			const uint32_t r = (dw >> (4 * (pos & 7))) & 15u;
			const uint32_t up = band[(uint32_t)(k + 1) * 64];
			uint32_t cell, d = 1u;      // column 0: U
			if (x < 1) cell = (x == 0) ? col0 : INVALID;
			else if (x > (int)L) cell = INVALID;
			else {
				const uint32_t cst = ((mrow >> r) & 1u) ? 0u : (((m1 >> r) & 1u) ? 1u : 255u);
				if (y == 1) {   // burst.c:722-739
					uint32_t hh = 0;
					if (cst == 1 && x >= 2) hh = (mrow >> prev_sym) & 1u;      // the left cell of row 1 scored 0 iff its symbol matches
					cell = cst == 255u ? INVALID : ((cst << SS) | ((255u - hh) << GS));
					d = hh ? 2u : (cst ? 3u : 0u);
				} else {
					const uint32_t cD = dg + (cst << SS), cU = up + STEP_U, cL = left + STEP_L;
					uint32_t cm = cD < cU ? cD : cU;
					cm = cm < cL ? cm : cL;
					d = (cm >> 8) & 3u;
					if (d == 0u && cst) d = 3u;
					cm &= ~0x300u;
					cell = (cm >> SS) > B ? INVALID : cm;                                // burst.c:802-803
				}
			}
			prev_sym = r;
			band[(uint32_t)k * 64] = cell;
			left = cell;
			dg = up;
			dacc |= d << (2 * (k & 15));
			if ((k & 15) == 15 || k == Wd - 1) { drow[(uint32_t)(k >> 4) * 64] = dacc; dacc = 0; }
		}
	}
	// cell (m, finalPos) sits on diagonal ed of the band
	const uint32_t fin = band[B * 64];
	if ((fin >> SS) != B) { atomicMin(&err[0], ri); n_ops[ri] = 0; ref_first[ri] = 0; gap_r[ri] = 0; return; }
	// the walk back; runs are written from the end of the slot towards its start, so that they read forwards
	const uint32_t slot = 2 * B + 1;
	uint32_t *p = tmp_ops + rq.opbase + slot;
	uint32_t cnt = 0, cur_code = 0, cur_len = 0, nI = 0, bad = 0;
	int y = m, x = (int)rq.finalPos;
	while (y > 0) {
		uint32_t d = 1u;
		if (x > 0) {
			const int k = x - y - dlo;
			if (k < 0 || k >= Wd) { bad = 1u; break; }
			d = (dec[((size_t)(y - 1) * DW + (uint32_t)(k >> 4)) * 64] >> (2 * (k & 15))) & 3u;
		}
		const uint32_t code = d == 0u ? 7u : d == 3u ? 8u : d == 1u ? 1u : 2u;      // BAM: I = 1, D = 2, '=' = 7, X = 8
		if (code == cur_code) ++cur_len;
		else {
			if (cur_len) { if (cnt == slot) { bad = 2u; break; } *--p = cur_len << 4 | cur_code; ++cnt; }
			cur_code = code; cur_len = 1;
		}
		if (d == 0u || d == 3u) { --y; --x; } else if (d == 1u) { --y; ++nI; } else --x;
	}
	if (!bad && cur_len) { if (cnt == slot) bad = 2u; else { *--p = cur_len << 4 | cur_code; ++cnt; } }
	if (bad) { atomicOr(&err[1], bad); cnt = 0; }
	n_ops[ri] = cnt; ref_first[ri] = (uint32_t)x + 1u; gap_r[ri] = nI;
}

// one thread per request: its runs from the end of its slot to their place in the dense array
__global__ __launch_bounds__(256) void k_paths_gather(const PathReq *__restrict__ req, const uint32_t *__restrict__ n_ops, const unsigned long long *__restrict__ off, uint32_t n,
		const uint32_t *__restrict__ tmp_ops, uint32_t *__restrict__ dense) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const uint32_t k = n_ops[i], slot = 2 * req[i].ed + 1;
		if (k > slot) continue;
		const uint32_t *src = tmp_ops + req[i].opbase + (slot - k);
		uint32_t *dst = dense + off[i];
		for (uint32_t j = 0; j < k; ++j) dst[j] = src[j];
	}
}

struct PathState {
	DBuf req, list, blk, codes, tmp_ops, n_ops, ref_first, gap_r, err, scratch, off, dense;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	uint64_t us_last = 0, us_total = 0, n_req = 0, n_ops_total = 0;
};

// (bhip_handle.h: Handle::paths)
void bhip_paths_release(Handle *h) {
	PathState *st = (PathState *)h->paths;
	if (!st) return;
	DBuf *all[] = {&st->req, &st->list, &st->blk, &st->codes, &st->tmp_ops, &st->n_ops, &st->ref_first, &st->gap_r, &st->err, &st->scratch, &st->off, &st->dense};
	for (DBuf *b : all) b->release();
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->paths = nullptr;
}

static inline uint32_t wide_dw(uint32_t ed) { return (2 * (2 * ed + 1) + 31) / 32; }
static inline bool is_narrow(const PathReq &r) { return r.ed <= PATHS_NARROW_ED && r.m <= PATHS_NARROW_M; }

// requests [r0, r1) of the call: one upload, the kernels, the counts back; the ops themselves when they still fit the caller's array
static int trace_chunk(Handle *h, PathState *st, const uint8_t *q_codes, const uint64_t *q_off, const BhipPathReq *requests, uint64_t r0, uint64_t r1,
		std::vector<uint32_t> &qpos, uint32_t *ops, uint64_t ops_cap, uint64_t *op_off, uint32_t *ref_first, uint32_t *gap_r, bool *ops_fit, uint64_t *first_bad) {
	const uint32_t n = (uint32_t)(r1 - r0);
	std::vector<PathReq> req(n);
	std::vector<uint8_t> codes;
	std::vector<uint32_t> touched;
	uint64_t n_slots = 0;
	for (uint32_t i = 0; i < n; ++i) {
		const BhipPathReq &u = requests[r0 + i];
		const uint32_t m = (uint32_t)(q_off[u.q + 1] - q_off[u.q]);
		if (qpos[u.q] == 0xFFFFFFFFu) {
			qpos[u.q] = (uint32_t)codes.size(); touched.push_back(u.q);
			codes.insert(codes.end(), q_codes + q_off[u.q], q_codes + q_off[u.q] + m);
		}
		PathReq &r = req[i];
		r.qbase = qpos[u.q]; r.m = m; r.refIx = u.refIx; r.finalPos = u.finalPos; r.ed = u.ed; r.opbase = (uint32_t)n_slots; r.pad0 = r.pad1 = 0;
		n_slots += 2ull * u.ed + 1;
	}
	for (uint32_t q : touched) qpos[q] = 0xFFFFFFFFu;
	// class lists: the narrow requests in input order, then the wide ones by falling scratch need
	std::vector<uint32_t> list; list.reserve(n);
	for (uint32_t i = 0; i < n; ++i) if (is_narrow(req[i])) list.push_back(i);
	const uint32_t n_narrow = (uint32_t)list.size();
	for (uint32_t i = 0; i < n; ++i) if (!is_narrow(req[i])) list.push_back(i);
	std::sort(list.begin() + n_narrow, list.end(), [&](uint32_t a, uint32_t b) {
		const uint64_t ka = (uint64_t)req[a].m * wide_dw(req[a].ed), kb = (uint64_t)req[b].m * wide_dw(req[b].ed);
		return ka != kb ? ka > kb : a < b; });
	const uint32_t n_wide = n - n_narrow, n_wblk = (n_wide + 63) / 64;
	// wide blocks: what each needs of the scratch, and the groups of blocks that share one launch
	std::vector<PathBlk> blk(n_wblk);
	std::vector<uint32_t> group_end;
	uint64_t used = 0, scratch_words = 0;
	for (uint32_t b = 0; b < n_wblk; ++b) {
		uint32_t mm = 0, dw = 0, rows = 0;
		for (uint32_t j = b * 64; j < std::min(n_wide, b * 64 + 64); ++j) {
			const PathReq &r = req[list[n_narrow + j]];
			mm = std::max(mm, r.m); dw = std::max(dw, wide_dw(r.ed)); rows = std::max(rows, 2 * r.ed + 2);
		}
		const uint64_t need_dec = (uint64_t)mm * dw * 64, need_band = rows > PATHS_LDS_BAND ? (uint64_t)rows * 64 : 0;
		if (used && used + need_dec + need_band > PATHS_SCRATCH_WORDS) { group_end.push_back(b); used = 0; }
		blk[b].dec_off = used; blk[b].band_off = need_band ? used + need_dec : ~0ull; blk[b].dw = dw; blk[b].pad = 0;
		used += need_dec + need_band;
		scratch_words = std::max(scratch_words, used);
	}
	if (n_wblk) group_end.push_back(n_wblk);

	int rc = st->req.reserve((size_t)n * sizeof(PathReq)); if (rc) return rc;
	rc = st->list.reserve((size_t)n * 4); if (rc) return rc;
	rc = st->blk.reserve((size_t)n_wblk * sizeof(PathBlk) + 16); if (rc) return rc;
	rc = st->codes.reserve(codes.size() + 16); if (rc) return rc;
	rc = st->tmp_ops.reserve(n_slots * 4); if (rc) return rc;
	rc = st->n_ops.reserve((size_t)n * 4); if (rc) return rc;
	rc = st->ref_first.reserve((size_t)n * 4); if (rc) return rc;
	rc = st->gap_r.reserve((size_t)n * 4); if (rc) return rc;
	rc = st->err.reserve(16); if (rc) return rc;
	rc = st->scratch.reserve(scratch_words * 4 + 16); if (rc) return rc;
	HIPCHK(hipMemcpyAsync(st->req.p, req.data(), (size_t)n * sizeof(PathReq), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(st->list.p, list.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
	if (n_wblk) HIPCHK(hipMemcpyAsync(st->blk.p, blk.data(), (size_t)n_wblk * sizeof(PathBlk), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(st->codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice, h->stream));
	const uint32_t err0[2] = {0xFFFFFFFFu, 0u};
	HIPCHK(hipMemcpyAsync(st->err.p, err0, 8, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipEventRecord(st->ev0, h->stream));
	if (n_narrow) {
		const size_t lds = ((size_t)(2 * PATHS_NARROW_ED + 2) + PATHS_NARROW_M) * 64 * 4;
		hipLaunchKernelGGL(k_trace_paths<true>, dim3((n_narrow + 63) / 64), dim3(64), lds, h->stream, st->req.as<PathReq>(), st->list.as<uint32_t>(), n_narrow, (const PathBlk *)nullptr,
			st->codes.as<uint8_t>(), h->ref_lane.as<uint32_t>(), h->ref_off.as<uint64_t>(), h->clump_len.as<uint32_t>(), h->lut.as<uint8_t>(), st->scratch.as<uint32_t>(),
			st->tmp_ops.as<uint32_t>(), st->n_ops.as<uint32_t>(), st->ref_first.as<uint32_t>(), st->gap_r.as<uint32_t>(), st->err.as<uint32_t>());
		HIPCHK(hipGetLastError());
	}
	uint32_t b0 = 0;
	for (uint32_t b1 : group_end) {      // (launches on one stream: a group's scratch is free again when the next one starts)
		const uint32_t first = b0 * 64, cnt = std::min(n_wide, b1 * 64) - first;
		hipLaunchKernelGGL(k_trace_paths<false>, dim3(b1 - b0), dim3(64), (size_t)PATHS_LDS_BAND * 64 * 4, h->stream, st->req.as<PathReq>(), st->list.as<uint32_t>() + n_narrow + first, cnt,
			st->blk.as<PathBlk>() + b0, st->codes.as<uint8_t>(), h->ref_lane.as<uint32_t>(), h->ref_off.as<uint64_t>(), h->clump_len.as<uint32_t>(), h->lut.as<uint8_t>(),
			st->scratch.as<uint32_t>(), st->tmp_ops.as<uint32_t>(), st->n_ops.as<uint32_t>(), st->ref_first.as<uint32_t>(), st->gap_r.as<uint32_t>(), st->err.as<uint32_t>());
		HIPCHK(hipGetLastError());
		b0 = b1;
	}
	HIPCHK(hipEventRecord(st->ev1, h->stream));
	std::vector<uint32_t> cnts(n);
	uint32_t err[2] = {0, 0};
	HIPCHK(hipMemcpyAsync(cnts.data(), st->n_ops.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(ref_first + r0, st->ref_first.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(gap_r + r0, st->gap_r.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(err, st->err.p, 8, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	st->us_last += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	if (err[1]) return fail(BHIP_E_INTERNAL, "bhip_trace_paths: a walk left its band or its slot (flags %u)", err[1]);
	if (err[0] != 0xFFFFFFFFu) { *first_bad = r0 + err[0]; return BHIP_E_RESCORE; }
	std::vector<unsigned long long> off(n);
	uint64_t tot = op_off[r0];
	for (uint32_t i = 0; i < n; ++i) { off[i] = tot - op_off[r0]; tot += cnts[i]; op_off[r0 + i + 1] = tot; }
	const uint64_t n_chunk = tot - op_off[r0];
	if (tot > ops_cap) *ops_fit = false;
	if (!*ops_fit || !n_chunk) return BHIP_OK;
	rc = st->off.reserve((size_t)n * 8); if (rc) return rc;
	rc = st->dense.reserve(n_chunk * 4); if (rc) return rc;
	HIPCHK(hipMemcpyAsync(st->off.p, off.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipEventRecord(st->ev0, h->stream));
	hipLaunchKernelGGL(k_paths_gather, dim3(std::min<uint32_t>((n + 255) / 256, 4096)), dim3(256), 0, h->stream, st->req.as<PathReq>(), st->n_ops.as<uint32_t>(),
		st->off.as<unsigned long long>(), n, st->tmp_ops.as<uint32_t>(), st->dense.as<uint32_t>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(st->ev1, h->stream));
	HIPCHK(hipMemcpyAsync(ops + op_off[r0], st->dense.p, n_chunk * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	st->us_last += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
	return BHIP_OK;
}

extern "C" int bhip_trace_paths(void *handle, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPathReq *requests, uint64_t n_requests,
		uint32_t *ops, uint64_t ops_cap, uint64_t *op_off, uint32_t *ref_first, uint32_t *gap_r) {
	Handle *h = (Handle *)handle;
	if (!h || !q_codes || !q_off || !op_off || (n_requests && (!requests || !ref_first || !gap_r)) || (ops_cap && !ops))
		return fail(BHIP_E_ARG, "bhip_trace_paths: null argument");
	// every request is checked on the host before the device is touched: the kernels index by these values alone
	for (uint64_t i = 0; i < n_requests; ++i) {
		const BhipPathReq &u = requests[i];
		if (u.q >= n_queries) return fail(BHIP_E_ARG, "bhip_trace_paths: request %llu names query %u of %u", (unsigned long long)i, u.q, n_queries);
		if (q_off[u.q + 1] < q_off[u.q] || q_off[u.q + 1] - q_off[u.q] > BHIP_MAX_QLEN || q_off[u.q + 1] == q_off[u.q])
			return fail(BHIP_E_ARG, "bhip_trace_paths: request %llu: query %u has %llu symbols (1 .. %d)", (unsigned long long)i, u.q, (unsigned long long)(q_off[u.q + 1] - q_off[u.q]), BHIP_MAX_QLEN);
		if (u.refIx >= 16ull * h->n_clumps || u.refIx >= h->tot_refs)
			return fail(BHIP_E_ARG, "bhip_trace_paths: request %llu names reference %u of %u", (unsigned long long)i, u.refIx, h->tot_refs);
		if (u.finalPos < 1 || u.finalPos > h->h_clump_len[u.refIx >> 4])
			return fail(BHIP_E_ARG, "bhip_trace_paths: request %llu ends at column %u of a clump of %u", (unsigned long long)i, u.finalPos, h->h_clump_len[u.refIx >> 4]);
		if (u.ed > 254u) return fail(BHIP_E_ARG, "bhip_trace_paths: request %llu has edit distance %u (0 .. 254)", (unsigned long long)i, u.ed);
	}
	op_off[0] = 0;
	if (!n_requests) return BHIP_OK;
	HIPCHK(hipSetDevice(h->device));
	PathState *st = (PathState *)h->paths;
	if (!st) {
		st = new PathState();
		h->paths = st;
		if (hipEventCreate(&st->ev0) != hipSuccess || hipEventCreate(&st->ev1) != hipSuccess) { bhip_paths_release(h); return fail(BHIP_E_DEVICE, "hipEventCreate failed"); }
	}
	st->us_last = 0;
	std::vector<uint32_t> qpos(n_queries, 0xFFFFFFFFu);
	bool ops_fit = true;
	uint64_t first_bad = 0;
	for (uint64_t r0 = 0; r0 < n_requests;) {
		uint64_t r1 = r0, sym = 0, slots = 0;
		while (r1 < n_requests && r1 - r0 < PATHS_CHUNK_REQ) {
			const uint64_t m = q_off[requests[r1].q + 1] - q_off[requests[r1].q], s = 2ull * requests[r1].ed + 1;
			if (r1 > r0 && (sym + m > PATHS_CHUNK_SYM || slots + s > PATHS_CHUNK_OPS)) break;
			sym += m; slots += s; ++r1;
		}
		const int rc = trace_chunk(h, st, q_codes, q_off, requests, r0, r1, qpos, ops, ops_cap, op_off, ref_first, gap_r, &ops_fit, &first_bad);
		if (rc == BHIP_E_RESCORE) {
			const BhipPathReq &u = requests[first_bad];
			return fail(BHIP_E_RESCORE, "bhip_trace_paths: request %llu (query %u, reference %u, end column %u): cell (m, finalPos) does not score %u",
			            (unsigned long long)first_bad, u.q, u.refIx, u.finalPos, u.ed);
		}
		if (rc) return rc;
		r0 = r1;
	}
	st->us_total += st->us_last; st->n_req += n_requests; st->n_ops_total += op_off[n_requests];
	if (!ops_fit) return fail(BHIP_E_CAPACITY, "bhip_trace_paths: %llu ops, room for %llu", (unsigned long long)op_off[n_requests], (unsigned long long)ops_cap);
	return BHIP_OK;
}

extern "C" int bhip_paths_info(void *handle, uint64_t info[4]) {
	Handle *h = (Handle *)handle;
	if (!h || !info) return fail(BHIP_E_ARG, "bhip_paths_info: null argument");
	const PathState *st = (const PathState *)h->paths;
	info[0] = st ? st->us_last : 0; info[1] = st ? st->us_total : 0; info[2] = st ? st->n_req : 0; info[3] = st ? st->n_ops_total : 0;
	return BHIP_OK;
}
