// burst_amd/csrc/bhip_conspairs.hip -- sample-to-sample identity of the consensus rows of every reference (burst_hip --consensus-pairs;
// bhip_consensus_pairs, gfx950).  No reference counterpart: the definition is this project's own (include/burst_hip.h "Consensus pairs",
// DESIGN.md section 7l), a pure function of the samples' consensus segments in integer arithmetic.
//
// A ROW is a (sample, header) with its segments; a position of a row is COMPARABLE when its letter is one of A C G T -.  For two rows of
// one header, Compared = the positions comparable in both, Same = those of them with equal letters.
//
// The work follows segments + covered positions + participating pairs x union words, never a reference's length:
//   host                every argument checked; the rows, and the headers with their rows in sample order (a sort of the rows by header <<
//                       16 | sample); headers with fewer than two rows are dropped; the groups and slabs that fit the budget
//   k_cp_keys, sort     the segments by start key header << 32 | pos
//   k_cp_reach, scan    inclusive MAX-scan of the one-past-end keys in that order (pos + len <= 2^32 - 1 keeps every end key of header h
//                       below every start key of header h + 1: the scan starts anew at a header change by itself)
//   k_cp_heads, scan    a segment opens a UNION INTERVAL when its start key is greater than the reach before it (equal = abutting = the
//                       same interval); the exclusive sum of the interval lengths is the COMPRESSED AXIS: a header's positions that any
//                       sample covers, side by side
//   k_cp_cstart         per segment its first compressed position within its header (a segment lies inside one interval)
//   k_cp_planes         one wave per segment, a lane per 64-bit word it touches: three CODE PLANES per row (bit k of the code 1..5 of A C G T
//                       -, 0 = not comparable) are OR-ed into the row's words.  A header's planes start on a word boundary
//   k_cp_pairs          one workgroup per tile of CP_TILE x CP_TILE row pairs of one header and CP_SPLIT words: the rows of both tile edges
//                       go through LDS CP_CHUNK words at a time, a thread owns one pair: compared += popc(called_a & called_b), same +=
//                       popc(called_a & called_b & ~(a0 ^ b0 | a1 ^ b1 | a2 ^ b2)), added to the pair's cell with integer atomics
//   k_cp_flags, scan, k_cp_emit   the cells with compared >= min_compared, in the order of the cells = (header, a, b)
// All sums are integers, OR and + commute, every selection is by key: no order of threads, waves or workgroups changes a byte, and
// neither does the budget: groups and slabs only change WHEN a word is added to its cell.
// CP_TILE, CP_CHUNK and CP_SPLIT are unmeasured choices.
#include "bhip_pile.h"
#include <algorithm>
#include <vector>

#define CP_TILE 16u
#define CP_CHUNK 32u                         // words of a row staged at a time
#define CP_ROWW (3u * CP_CHUNK)              // u64 per staged row
#define CP_STRIDE (CP_ROWW + 1u)             // 97 u64: 16 rows read by one half-wave fall on 32 different banks
#define CP_SPLIT 256u                        // words of a header one workgroup walks
#define CP_NOROW 0xFFFFFFFFu
#define CP_MAX_GROUP_CELLS (1ull << 24)

struct CpHdr { uint32_t header, m, nw, pad; pile_u64 row0, plane_base, cell_base, unit_off; };      // a header of one launch
struct CpCell { uint32_t compared, same; };

struct CpState {
	DBuf segs, letters, seg_row, row_hdr, row_sample, key, end, key_s, ord_in, ord, reach_in, reach, head, ix, iv_key, iv_end, iv_len, iv_off, c_start,
	     hdrs, planes, cells, flags, fidx, out, tmp;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	uint64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	void each(void (*f)(DBuf *, void *), void *u) {
		DBuf *all[] = {&segs, &letters, &seg_row, &row_hdr, &row_sample, &key, &end, &key_s, &ord_in, &ord, &reach_in, &reach, &head, &ix, &iv_key, &iv_end, &iv_len,
			&iv_off, &c_start, &hdrs, &planes, &cells, &flags, &fidx, &out, &tmp};
		for (DBuf *x : all) f(x, u);
	}
	uint64_t bytes() { uint64_t b = 0; each([](DBuf *x, void *u) { *(uint64_t *)u += x->cap; }, &b); return b; }
};

__host__ __device__ __forceinline__ unsigned long long cp_key(uint32_t header, uint32_t pos) { return (unsigned long long)header << 32 | pos; }
// first cell of row ra among the pairs (ra < rb) of m rows; first tile of tile row bi among the tiles (bi <= bj) of nb tile rows
__host__ __device__ __forceinline__ unsigned long long cp_row_start(unsigned long long ra, unsigned long long m) { return ra * (2ull * m - ra - 1ull) / 2ull; }
__host__ __device__ __forceinline__ unsigned long long cp_tile_start(unsigned long long bi, unsigned long long nb) { return bi * nb - bi * (bi - 1ull) / 2ull; }

__global__ __launch_bounds__(PILE_BLOCK) void k_cp_keys(const BhipPairSeg *__restrict__ segs, uint64_t n, pile_u64 *__restrict__ key, pile_u64 *__restrict__ end,
		pile_u64 *__restrict__ ord_in) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const BhipPairSeg g = segs[i];
		key[i] = cp_key(g.header, g.pos);
		end[i] = cp_key(g.header, g.pos + g.len);      // (pos + len <= 2^32 - 1: checked on the host)
		ord_in[i] = i;
	}
}

__global__ __launch_bounds__(PILE_BLOCK) void k_cp_reach(const pile_u64 *__restrict__ ord, const pile_u64 *__restrict__ end, uint64_t n, pile_u64 *__restrict__ reach_in) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const pile_u64 s = ord[i];
		reach_in[i] = s < n ? end[s] : 0ull;
	}
}

// (head[n] = 0: the scan's extra element holds the number of intervals)
__global__ __launch_bounds__(PILE_BLOCK) void k_cp_heads(const pile_u64 *__restrict__ key_s, const pile_u64 *__restrict__ reach, uint64_t n, pile_u64 *__restrict__ head) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x)
		head[i] = (i < n && (i == 0 || key_s[i] > reach[i - 1])) ? 1ull : 0ull;
}

__global__ __launch_bounds__(PILE_BLOCK) void k_cp_ivs(const pile_u64 *__restrict__ key_s, const pile_u64 *__restrict__ reach, const pile_u64 *__restrict__ head,
		const pile_u64 *__restrict__ ix, uint64_t n, uint64_t n_iv, pile_u64 *__restrict__ iv_key, pile_u64 *__restrict__ iv_end) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const pile_u64 s = ix[i] - (head[i] ? 0ull : 1ull);      // the interval segment i belongs to
		if (s >= n_iv) continue;
		if (head[i]) iv_key[s] = key_s[i];
		if (i + 1 == n || head[i + 1]) iv_end[s] = reach[i];      // the last segment of its interval
	}
}

__global__ __launch_bounds__(PILE_BLOCK) void k_cp_lens(const pile_u64 *__restrict__ iv_key, const pile_u64 *__restrict__ iv_end, uint64_t n_iv, pile_u64 *__restrict__ iv_len) {
	for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s <= n_iv; s += (uint64_t)gridDim.x * blockDim.x)
		iv_len[s] = s < n_iv ? iv_end[s] - iv_key[s] : 0ull;
}

// iv_off = the exclusive sum of the interval lengths.  c_start[i] = the first compressed position, within its header, of sorted segment i
__global__ __launch_bounds__(PILE_BLOCK) void k_cp_cstart(const pile_u64 *__restrict__ key_s, const pile_u64 *__restrict__ head, const pile_u64 *__restrict__ ix, uint64_t n,
		const pile_u64 *__restrict__ iv_key, const pile_u64 *__restrict__ iv_off, uint64_t n_iv, pile_u64 *__restrict__ c_start) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const pile_u64 s = ix[i] - (head[i] ? 0ull : 1ull);
		if (s >= n_iv) { c_start[i] = 0ull; continue; }
		const pile_u64 hkey = key_s[i] & 0xFFFFFFFF00000000ull;      // (no start key has position 0: the keys <= hkey are those of the headers before)
		const uint64_t s0 = pile_upper_bound(iv_key, n_iv, hkey);
		c_start[i] = iv_off[s] - iv_off[s0 < n_iv ? s0 : s] + (key_s[i] - iv_key[s]);
	}
}

__device__ __forceinline__ uint32_t cp_code(char c) { return c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 3u : c == 'T' ? 4u : c == '-' ? 5u : 0u; }

// one wave per sorted segment s_lo + wave, a lane per word.  L: the headers of the launch, the first of them kept header gk0; w0: the first
// word of the slab (0 when the launch holds whole headers); planes: [row][word of the launch][3], zeroed before
__global__ __launch_bounds__(PILE_BLOCK) void k_cp_planes(const pile_u64 *__restrict__ ord, const BhipPairSeg *__restrict__ segs, uint64_t n_segs, const char *__restrict__ letters,
		const pile_u64 *__restrict__ c_start, const uint32_t *__restrict__ seg_row, const uint32_t *__restrict__ row_hdr, const CpHdr *__restrict__ L, uint32_t n_l,
		uint32_t gk0, uint32_t w0, uint64_t s_lo, uint64_t s_hi, pile_u64 *__restrict__ planes) {
	const uint64_t i = s_lo + (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / 64u;
	const uint32_t lane = threadIdx.x & 63u;
	if (i >= s_hi) return;
	const pile_u64 s = ord[i];
	if (s >= n_segs) return;
	const uint32_t grow = seg_row[s];
	if (grow == CP_NOROW) return;      // a header with one sample
	const uint32_t g = row_hdr[grow] - gk0;
	if (g >= n_l) return;
	const CpHdr H = L[g];
	const BhipPairSeg sg = segs[s];
	const pile_u64 lr = grow - H.row0, c = c_start[i], ce = c + sg.len;
	const char *let = letters + sg.off;
	for (pile_u64 wd = (c >> 6) + lane; wd <= ((ce - 1ull) >> 6); wd += 64ull) {
		if (wd < w0 || wd - w0 >= H.nw) continue;
		const pile_u64 lo = c > (wd << 6) ? c : (wd << 6), hi = ce < ((wd + 1ull) << 6) ? ce : ((wd + 1ull) << 6);
		pile_u64 p0 = 0, p1 = 0, p2 = 0;
		for (pile_u64 x = lo; x < hi; ++x) {
			const pile_u64 code = cp_code(let[x - c]);
			const uint32_t bit = (uint32_t)(x & 63ull);
			p0 |= (code & 1ull) << bit; p1 |= ((code >> 1) & 1ull) << bit; p2 |= ((code >> 2) & 1ull) << bit;
		}
		pile_u64 *dst = planes + H.plane_base + (lr * H.nw + (wd - w0)) * 3ull;
		if (p0) atomicOr(&dst[0], p0);      // (two segments of a row can share a word)
		if (p1) atomicOr(&dst[1], p1);
		if (p2) atomicOr(&dst[2], p2);
	}
}

// the header of launch unit / cell `v`: the last entry whose unit_off (by_cell: cell_base) is <= v
__device__ __forceinline__ uint32_t cp_find(const CpHdr *__restrict__ L, uint32_t n_l, pile_u64 v, bool by_cell) {
	uint32_t lo = 0, hi = n_l;      // (entry 0 starts at 0)
	while (lo + 1u < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((by_cell ? L[mid].cell_base : L[mid].unit_off) <= v) lo = mid; else hi = mid; }
	return lo;
}

__global__ __launch_bounds__(256) void k_cp_pairs(const CpHdr *__restrict__ L, uint32_t n_l, const pile_u64 *__restrict__ planes, CpCell *__restrict__ cells) {
	__shared__ pile_u64 lds[2u * CP_TILE * CP_STRIDE];
	const uint32_t tid = threadIdx.x;
	const CpHdr H = L[cp_find(L, n_l, blockIdx.x, false)];
	const pile_u64 lu = blockIdx.x - H.unit_off;
	const uint32_t splits = (H.nw + CP_SPLIT - 1u) / CP_SPLIT, nb = (H.m + CP_TILE - 1u) / CP_TILE;
	const pile_u64 tile = lu / splits;
	const uint32_t sp = (uint32_t)(lu % splits);
	uint32_t blo = 0, bhi = nb;      // the last tile row whose first tile is <= tile
	while (blo + 1u < bhi) { const uint32_t mid = blo + ((bhi - blo) >> 1); if (cp_tile_start(mid, nb) <= tile) blo = mid; else bhi = mid; }
	const uint32_t bi = blo, bj = bi + (uint32_t)(tile - cp_tile_start(bi, nb));
	if (bj >= nb) return;      // (uniform: cannot happen with a table the host made)
	const uint32_t ti = tid >> 4, tj = tid & 15u, ra = bi * CP_TILE + ti, rb = bj * CP_TILE + tj;
	const bool valid = ra < rb && rb < H.m;
	const uint32_t w_lo = sp * CP_SPLIT, w_hi = w_lo + CP_SPLIT < H.nw ? w_lo + CP_SPLIT : H.nw;
	uint32_t compared = 0, same = 0;
	for (uint32_t wb = w_lo; wb < w_hi; wb += CP_CHUNK) {
		for (uint32_t x = tid; x < 2u * CP_TILE * CP_ROWW; x += 256u) {
			const uint32_t row = x / CP_ROWW, off = x % CP_ROWW, w = wb + off / 3u;
			const uint32_t r = row < CP_TILE ? bi * CP_TILE + row : bj * CP_TILE + (row - CP_TILE);
			lds[row * CP_STRIDE + off] = (r < H.m && w < w_hi) ? planes[H.plane_base + ((pile_u64)r * H.nw + wb) * 3ull + off] : 0ull;
		}
		__syncthreads();
		if (valid) {
			const pile_u64 *a = lds + ti * CP_STRIDE, *b = lds + (CP_TILE + tj) * CP_STRIDE;
#pragma unroll 4
			for (uint32_t w = 0; w < CP_CHUNK; ++w) {
				const pile_u64 a0 = a[3u * w], a1 = a[3u * w + 1u], a2 = a[3u * w + 2u], b0 = b[3u * w], b1 = b[3u * w + 1u], b2 = b[3u * w + 2u];
				const pile_u64 both = (a0 | a1 | a2) & (b0 | b1 | b2);
				compared += (uint32_t)__popcll(both);
				same += (uint32_t)__popcll(both & ~((a0 ^ b0) | (a1 ^ b1) | (a2 ^ b2)));
			}
		}
		__syncthreads();
	}
	if (valid && compared) {
		CpCell *c = cells + H.cell_base + cp_row_start(ra, H.m) + (rb - ra - 1u);
		atomicAdd(&c->compared, compared);
		if (same) atomicAdd(&c->same, same);
	}
}

__global__ __launch_bounds__(PILE_BLOCK) void k_cp_flags(const CpCell *__restrict__ cells, uint64_t n, uint32_t min_compared, uint32_t *__restrict__ flags) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x)
		flags[i] = (i < n && cells[i].compared >= min_compared) ? 1u : 0u;
}

__global__ __launch_bounds__(PILE_BLOCK) void k_cp_emit(const CpCell *__restrict__ cells, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ fidx, uint64_t n,
		uint64_t n_sel, const CpHdr *__restrict__ L, uint32_t n_l, const uint32_t *__restrict__ row_sample, BhipPair *__restrict__ out) {
	for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		if (!flags[i] || fidx[i] >= n_sel) continue;
		const CpHdr H = L[cp_find(L, n_l, i, true)];
		const pile_u64 lp = i - H.cell_base;
		uint32_t lo = 0, hi = H.m - 1u;      // the last row whose first cell is <= lp (rows 0 .. m - 2 have cells)
		while (lo + 1u < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (cp_row_start(mid, H.m) <= lp) lo = mid; else hi = mid; }
		const uint32_t ra = lo, rb = ra + 1u + (uint32_t)(lp - cp_row_start(ra, H.m));
		if (rb >= H.m) continue;
		BhipPair p;
		p.header = H.header; p.a = row_sample[H.row0 + ra]; p.b = row_sample[H.row0 + rb]; p.pad = 0u; p.compared = cells[i].compared; p.same = cells[i].same;
		out[fidx[i]] = p;
	}
}

// (bhip_handle.h: Handle::conspairs)
void bhip_conspairs_release(Handle *h) {
	CpState *st = (CpState *)h->conspairs;
	if (!st) return;
	st->each([](DBuf *x, void *) { x->release(); }, nullptr);
	if (st->ev0) (void)hipEventDestroy(st->ev0);
	if (st->ev1) (void)hipEventDestroy(st->ev1);
	delete st;
	h->conspairs = nullptr;
}

extern "C" int bhip_consensus_pairs_info(void *handle, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	if (!h || !info) return fail(BHIP_E_ARG, "bhip_consensus_pairs_info: null argument");
	if (h->conspairs) memcpy(info, ((CpState *)h->conspairs)->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t));
	return BHIP_OK;
}

namespace {
struct CpRow { uint64_t key; uint64_t seg0; uint32_t n_seg; };      // key = header << 16 | sample
struct CpHost { uint32_t header, m; uint64_t row0, seg_lo, seg_hi, U; };      // a kept header: its rows, its segments in the sorted order, its union length
struct CpTimer {
	CpState *st; hipStream_t S; uint64_t us = 0;
	int begin() { return hipEventRecord(st->ev0, S) == hipSuccess ? 0 : 1; }
	int end() {      // (ends with the stream idle)
		if (hipEventRecord(st->ev1, S) != hipSuccess || hipStreamSynchronize(S) != hipSuccess) return 1;
		us += (uint64_t)(ev_ms(st->ev0, st->ev1) * 1000.0f);
		return 0;
	}
};
}

// one launch: the planes of the launch's headers (whole, or the slab [w0, w0 + nw) of one header), then their pairs added to the cells
static int cp_launch(Handle *h, CpState *st, std::vector<CpHdr> &L, uint32_t gk0, uint32_t w0, uint64_t s_lo, uint64_t s_hi, uint64_t n_segs) {
	hipStream_t S = h->stream;
	pile_u64 words = 0, units = 0;
	for (CpHdr &H : L) {
		H.plane_base = words; H.unit_off = units;
		words += (pile_u64)H.m * H.nw * 3ull;
		const pile_u64 nb = (H.m + CP_TILE - 1u) / CP_TILE;
		units += nb * (nb + 1ull) / 2ull * ((H.nw + CP_SPLIT - 1u) / CP_SPLIT);
	}
	if (units > 0x7FFFFFFFull) return fail(BHIP_E_ARG, "bhip_consensus_pairs: %llu workgroups in one launch: lower the option conspairs_bytes", units);
	int rc = st->planes.reserve(words * 8 + 16); if (rc) return rc;
	rc = st->hdrs.reserve(L.size() * sizeof(CpHdr)); if (rc) return rc;
	HIPCHK(hipMemcpyAsync(st->hdrs.p, L.data(), L.size() * sizeof(CpHdr), hipMemcpyHostToDevice, S));
	HIPCHK(hipMemsetAsync(st->planes.p, 0, words * 8, S));
	const uint64_t waves = s_hi - s_lo;
	hipLaunchKernelGGL(k_cp_planes, dim3((uint32_t)((waves + 3) / 4)), dim3(PILE_BLOCK), 0, S, st->ord.as<pile_u64>(), st->segs.as<BhipPairSeg>(), n_segs, st->letters.as<char>(),
		st->c_start.as<pile_u64>(), st->seg_row.as<uint32_t>(), st->row_hdr.as<uint32_t>(), st->hdrs.as<CpHdr>(), (uint32_t)L.size(), gk0, w0, s_lo, s_hi, st->planes.as<pile_u64>());
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_cp_pairs, dim3((uint32_t)units), dim3(256), 0, S, st->hdrs.as<CpHdr>(), (uint32_t)L.size(), st->planes.as<pile_u64>(), st->cells.as<CpCell>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(S));      // (L and the table on the device are written again by the next launch)
	return BHIP_OK;
}

extern "C" int bhip_consensus_pairs(void *handle, uint32_t n_samples, const BhipPairSeg *segs, uint64_t n_segs, const char *letters, uint64_t n_letters,
		uint32_t min_compared, BhipPair *pairs, uint64_t pair_cap, uint64_t *n_pairs, uint64_t info[8]) {
	Handle *h = (Handle *)handle;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!h || !n_pairs || (n_segs && (!segs || !letters)) || (pair_cap && !pairs)) return fail(BHIP_E_ARG, "bhip_consensus_pairs: null argument");
	*n_pairs = 0;
	CpState *st = (CpState *)h->conspairs;
	if (!st) { st = new CpState(); h->conspairs = st; }      // (host memory alone: the events and buffers are made by the first call that launches)
	memset(st->info, 0, sizeof st->info);
	// every value the kernels index by is checked here, before the device is touched
	if (n_samples > 65535u) return fail(BHIP_E_ARG, "bhip_consensus_pairs: %u samples (at most 65535)", n_samples);
	if (!min_compared || min_compared > 0x7FFFFFFFu) return fail(BHIP_E_ARG, "bhip_consensus_pairs: min_compared %u (1 .. 2^31 - 1)", min_compared);
	if (n_segs >> 32) return fail(BHIP_E_ARG, "bhip_consensus_pairs: %llu segments (fewer than 2^32)", (pile_u64)n_segs);
	std::vector<CpRow> rows;
	uint32_t max_header = 0;
	for (uint64_t i = 0; i < n_segs; ++i) {
		const BhipPairSeg &g = segs[i];
		if (g.sample >= n_samples) return fail(BHIP_E_ARG, "bhip_consensus_pairs: segment %llu names sample %u of %u", (pile_u64)i, g.sample, n_samples);
		if (!g.pos || !g.len) return fail(BHIP_E_ARG, "bhip_consensus_pairs: segment %llu has position %u and length %u (both >= 1)", (pile_u64)i, g.pos, g.len);
		if ((uint64_t)g.pos + g.len > 0xFFFFFFFFull) return fail(BHIP_E_ARG, "bhip_consensus_pairs: segment %llu: position %u + length %u (at most 2^32 - 1)", (pile_u64)i, g.pos, g.len);
		if (g.off > n_letters || g.len > n_letters - g.off) return fail(BHIP_E_ARG, "bhip_consensus_pairs: segment %llu owns letters %llu + %u of %llu", (pile_u64)i, (pile_u64)g.off, g.len, (pile_u64)n_letters);
		bool new_row = true;
		if (i) {
			const BhipPairSeg &p = segs[i - 1];
			if (p.sample > g.sample || (p.sample == g.sample && p.header > g.header))
				return fail(BHIP_E_ARG, "bhip_consensus_pairs: segments not ascending by (sample, header, pos) at segment %llu", (pile_u64)i);
			if (p.sample == g.sample && p.header == g.header) {
				if ((uint64_t)g.pos < (uint64_t)p.pos + p.len)
					return fail(BHIP_E_ARG, "bhip_consensus_pairs: segment %llu at position %u starts before the end of the one before it (%u + %u): out of order or overlapping", (pile_u64)i, g.pos, p.pos, p.len);
				new_row = false;
			}
		}
		if (new_row) { CpRow r; r.key = (uint64_t)g.header << 16 | g.sample; r.seg0 = i; r.n_seg = 0; rows.push_back(r); }
		++rows.back().n_seg;
		max_header = std::max(max_header, g.header);
	}
	info[0] = n_segs;
	memcpy(st->info, info, sizeof st->info);
	if (n_samples < 2 || !n_segs) return BHIP_OK;      // (no pair anywhere, no launch)
	// the headers with their rows in sample order; those with fewer than two rows are dropped
	std::sort(rows.begin(), rows.end(), [](const CpRow &a, const CpRow &b) { return a.key < b.key; });
	std::vector<CpHost> kept;
	std::vector<uint32_t> seg_row(n_segs, CP_NOROW), row_hdr, row_sample;
	uint64_t seg_at = 0, examined = 0;
	for (size_t a = 0; a < rows.size();) {
		size_t b = a; uint64_t ns = 0;
		for (; b < rows.size() && (rows[b].key >> 16) == (rows[a].key >> 16); ++b) ns += rows[b].n_seg;
		if (b - a >= 2) {
			CpHost k; k.header = (uint32_t)(rows[a].key >> 16); k.m = (uint32_t)(b - a); k.row0 = row_sample.size(); k.seg_lo = seg_at; k.seg_hi = seg_at + ns; k.U = 0;
			for (size_t r = a; r < b; ++r) {
				for (uint32_t t = 0; t < rows[r].n_seg; ++t) seg_row[rows[r].seg0 + t] = (uint32_t)row_sample.size();
				row_hdr.push_back((uint32_t)kept.size()); row_sample.push_back((uint32_t)(rows[r].key & 0xFFFFu));
			}
			examined += (uint64_t)k.m * (k.m - 1) / 2;
			kept.push_back(k);
		}
		seg_at += ns;
		a = b;
	}
	info[1] = kept.size(); info[3] = examined;
	memcpy(st->info, info, sizeof st->info);
	if (kept.empty()) return BHIP_OK;      // (no header with two samples, no launch)

	HIPCHK(hipSetDevice(h->device));
	if (!st->ev0 && hipEventCreate(&st->ev0) != hipSuccess) { st->ev0 = nullptr; return fail(BHIP_E_DEVICE, "hipEventCreate failed"); }
	if (!st->ev1 && hipEventCreate(&st->ev1) != hipSuccess) { st->ev1 = nullptr; return fail(BHIP_E_DEVICE, "hipEventCreate failed"); }
	hipStream_t S = h->stream;
	CpTimer T{st, S};
	const uint64_t n = n_segs, n_rows = row_sample.size();
	const int end_bit = 32 + std::max(1, pile_bits(max_header));
	int rc = st->segs.reserve(n * sizeof(BhipPairSeg)); if (rc) return rc;
	rc = st->letters.reserve(n_letters + 16); if (rc) return rc;
	rc = st->seg_row.reserve(n * 4); if (rc) return rc;
	rc = st->row_hdr.reserve(n_rows * 4); if (rc) return rc;
	rc = st->row_sample.reserve(n_rows * 4); if (rc) return rc;
	DBuf *per_seg[] = {&st->key, &st->end, &st->key_s, &st->ord_in, &st->ord, &st->reach_in, &st->reach, &st->c_start};
	for (DBuf *x : per_seg) { rc = x->reserve(n * 8); if (rc) return rc; }
	rc = st->head.reserve((n + 1) * 8); if (rc) return rc;
	rc = st->ix.reserve((n + 1) * 8); if (rc) return rc;
	size_t tb_sort = 0, tb_max = 0, tb_sum = 0;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, st->key.as<pile_u64>(), st->key_s.as<pile_u64>(), st->ord_in.as<pile_u64>(), st->ord.as<pile_u64>(), (size_t)n, 0, end_bit, S));
	HIPCHK(hipcub::DeviceScan::InclusiveScan(nullptr, tb_max, st->reach_in.as<pile_u64>(), st->reach.as<pile_u64>(), hipcub::Max(), (size_t)n, S));
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_sum, st->head.as<pile_u64>(), st->ix.as<pile_u64>(), (size_t)(n + 1), S));
	rc = st->tmp.reserve(std::max(tb_sort, std::max(tb_max, tb_sum)) + 16); if (rc) return rc;
	HIPCHK(hipMemcpyAsync(st->segs.p, segs, n * sizeof(BhipPairSeg), hipMemcpyHostToDevice, S));
	HIPCHK(hipMemcpyAsync(st->letters.p, letters, n_letters, hipMemcpyHostToDevice, S));
	HIPCHK(hipMemcpyAsync(st->seg_row.p, seg_row.data(), n * 4, hipMemcpyHostToDevice, S));
	HIPCHK(hipMemcpyAsync(st->row_hdr.p, row_hdr.data(), n_rows * 4, hipMemcpyHostToDevice, S));
	HIPCHK(hipMemcpyAsync(st->row_sample.p, row_sample.data(), n_rows * 4, hipMemcpyHostToDevice, S));
	// 1. the union intervals of every header
	if (T.begin()) return fail(BHIP_E_DEVICE, "bhip_consensus_pairs: hipEventRecord failed");
	hipLaunchKernelGGL(k_cp_keys, dim3(pile_grid(n)), dim3(PILE_BLOCK), 0, S, st->segs.as<BhipPairSeg>(), n, st->key.as<pile_u64>(), st->end.as<pile_u64>(), st->ord_in.as<pile_u64>());
	HIPCHK(hipGetLastError());
	size_t tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceRadixSort::SortPairs(st->tmp.p, tb, st->key.as<pile_u64>(), st->key_s.as<pile_u64>(), st->ord_in.as<pile_u64>(), st->ord.as<pile_u64>(), (size_t)n, 0, end_bit, S));
	hipLaunchKernelGGL(k_cp_reach, dim3(pile_grid(n)), dim3(PILE_BLOCK), 0, S, st->ord.as<pile_u64>(), st->end.as<pile_u64>(), n, st->reach_in.as<pile_u64>());
	HIPCHK(hipGetLastError());
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::InclusiveScan(st->tmp.p, tb, st->reach_in.as<pile_u64>(), st->reach.as<pile_u64>(), hipcub::Max(), (size_t)n, S));
	hipLaunchKernelGGL(k_cp_heads, dim3(pile_grid(n + 1)), dim3(PILE_BLOCK), 0, S, st->key_s.as<pile_u64>(), st->reach.as<pile_u64>(), n, st->head.as<pile_u64>());
	HIPCHK(hipGetLastError());
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(st->tmp.p, tb, st->head.as<pile_u64>(), st->ix.as<pile_u64>(), (size_t)(n + 1), S));
	pile_u64 n_iv = 0;
	HIPCHK(hipMemcpyAsync(&n_iv, (char *)st->ix.p + n * 8, 8, hipMemcpyDeviceToHost, S));
	if (T.end()) return fail(BHIP_E_DEVICE, "bhip_consensus_pairs: the union intervals: %s", hipGetErrorString(hipGetLastError()));
	if (!n_iv || n_iv > n) return fail(BHIP_E_INTERNAL, "bhip_consensus_pairs: %llu union intervals of %llu segments", n_iv, (pile_u64)n);
	DBuf *per_iv[] = {&st->iv_key, &st->iv_end, &st->iv_len, &st->iv_off};
	for (DBuf *x : per_iv) { rc = x->reserve((n_iv + 1) * 8); if (rc) return rc; }
	tb_sum = 0;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_sum, st->iv_len.as<pile_u64>(), st->iv_off.as<pile_u64>(), (size_t)(n_iv + 1), S));
	rc = st->tmp.reserve(tb_sum + 16); if (rc) return rc;
	if (T.begin()) return fail(BHIP_E_DEVICE, "bhip_consensus_pairs: hipEventRecord failed");
	hipLaunchKernelGGL(k_cp_ivs, dim3(pile_grid(n)), dim3(PILE_BLOCK), 0, S, st->key_s.as<pile_u64>(), st->reach.as<pile_u64>(), st->head.as<pile_u64>(), st->ix.as<pile_u64>(), n,
		(uint64_t)n_iv, st->iv_key.as<pile_u64>(), st->iv_end.as<pile_u64>());
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_cp_lens, dim3(pile_grid(n_iv + 1)), dim3(PILE_BLOCK), 0, S, st->iv_key.as<pile_u64>(), st->iv_end.as<pile_u64>(), (uint64_t)n_iv, st->iv_len.as<pile_u64>());
	HIPCHK(hipGetLastError());
	tb = st->tmp.cap;
	HIPCHK(hipcub::DeviceScan::ExclusiveSum(st->tmp.p, tb, st->iv_len.as<pile_u64>(), st->iv_off.as<pile_u64>(), (size_t)(n_iv + 1), S));
	hipLaunchKernelGGL(k_cp_cstart, dim3(pile_grid(n)), dim3(PILE_BLOCK), 0, S, st->key_s.as<pile_u64>(), st->head.as<pile_u64>(), st->ix.as<pile_u64>(), n, st->iv_key.as<pile_u64>(),
		st->iv_off.as<pile_u64>(), (uint64_t)n_iv, st->c_start.as<pile_u64>());
	HIPCHK(hipGetLastError());
	std::vector<pile_u64> iv_key(n_iv), iv_len(n_iv);
	HIPCHK(hipMemcpyAsync(iv_key.data(), st->iv_key.p, n_iv * 8, hipMemcpyDeviceToHost, S));
	HIPCHK(hipMemcpyAsync(iv_len.data(), st->iv_len.p, n_iv * 8, hipMemcpyDeviceToHost, S));
	if (T.end()) return fail(BHIP_E_DEVICE, "bhip_consensus_pairs: the compressed axis: %s", hipGetErrorString(hipGetLastError()));
	// the union length of every kept header (both lists ascend by header)
	uint64_t total_U = 0;
	{
		size_t k = 0;
		for (pile_u64 s = 0; s < n_iv; ++s) {
			const uint32_t hd = (uint32_t)(iv_key[s] >> 32);
			while (k < kept.size() && kept[k].header < hd) ++k;
			if (k < kept.size() && kept[k].header == hd) kept[k].U += iv_len[s];
		}
		for (const CpHost &k2 : kept) {
			if (!k2.U || k2.U > 0xFFFFFFFFull) return fail(BHIP_E_INTERNAL, "bhip_consensus_pairs: header %u has a union of %llu positions", k2.header, (pile_u64)k2.U);
			total_U += k2.U;
		}
	}
	info[2] = total_U;

	// 2. + 3. + 4. the groups of headers whose planes fit the budget; a header too large for it alone, in slabs of words
	const uint64_t budget_words = (uint64_t)std::max<long long>(h->opt_conspairs_bytes, 8) / 8;
	std::vector<BhipPair> result;
	std::vector<CpHdr> L;
	for (size_t g0 = 0; g0 < kept.size();) {
		size_t g1 = g0; uint64_t words = 0, cells = 0;
		bool slabs = false;
		for (; g1 < kept.size(); ++g1) {
			const uint64_t W = (kept[g1].U + 63) / 64, need = (uint64_t)kept[g1].m * W * 3, pc = (uint64_t)kept[g1].m * (kept[g1].m - 1) / 2;
			if (need > budget_words) { if (g1 == g0) { slabs = true; ++g1; cells = pc; } break; }
			if (g1 > g0 && (words + need > budget_words || cells + pc > CP_MAX_GROUP_CELLS)) break;
			words += need; cells += pc;
		}
		if (cells >> 32) return fail(BHIP_E_ARG, "bhip_consensus_pairs: %llu pairs of one header (fewer than 2^32)", (pile_u64)cells);
		rc = st->cells.reserve(cells * sizeof(CpCell)); if (rc) return rc;
		rc = st->flags.reserve((cells + 1) * 4); if (rc) return rc;
		rc = st->fidx.reserve((cells + 1) * 4); if (rc) return rc;
		tb_sum = 0;
		HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_sum, st->flags.as<uint32_t>(), st->fidx.as<uint32_t>(), (size_t)(cells + 1), S));
		rc = st->tmp.reserve(tb_sum + 16); if (rc) return rc;
		L.clear();
		uint64_t cell_at = 0;
		for (size_t g = g0; g < g1; ++g) {
			CpHdr H; memset(&H, 0, sizeof H);
			H.header = kept[g].header; H.m = kept[g].m; H.nw = (uint32_t)((kept[g].U + 63) / 64); H.row0 = kept[g].row0; H.cell_base = cell_at;
			cell_at += (uint64_t)H.m * (H.m - 1) / 2;
			L.push_back(H);
		}
		if (T.begin()) return fail(BHIP_E_DEVICE, "bhip_consensus_pairs: hipEventRecord failed");
		HIPCHK(hipMemsetAsync(st->cells.p, 0, cells * sizeof(CpCell), S));
		if (!slabs) { rc = cp_launch(h, st, L, (uint32_t)g0, 0u, kept[g0].seg_lo, kept[g1 - 1].seg_hi, n); if (rc) return rc; }
		else {
			const uint32_t W = L[0].nw;
			const uint64_t sw = std::max<uint64_t>(1, budget_words / (3ull * L[0].m));      // (one word of every row is the least a launch holds)
			for (uint64_t w0 = 0; w0 < W; w0 += sw) {
				L[0].nw = (uint32_t)std::min<uint64_t>(sw, W - w0);
				rc = cp_launch(h, st, L, (uint32_t)g0, (uint32_t)w0, kept[g0].seg_lo, kept[g0].seg_hi, n); if (rc) return rc;
			}
			L[0].nw = W; L[0].plane_base = 0; L[0].unit_off = 0;
			HIPCHK(hipMemcpyAsync(st->hdrs.p, L.data(), sizeof(CpHdr), hipMemcpyHostToDevice, S));
		}
		hipLaunchKernelGGL(k_cp_flags, dim3(pile_grid(cells + 1)), dim3(PILE_BLOCK), 0, S, st->cells.as<CpCell>(), cells, min_compared, st->flags.as<uint32_t>());
		HIPCHK(hipGetLastError());
		tb = st->tmp.cap;
		HIPCHK(hipcub::DeviceScan::ExclusiveSum(st->tmp.p, tb, st->flags.as<uint32_t>(), st->fidx.as<uint32_t>(), (size_t)(cells + 1), S));
		uint32_t n_sel = 0;
		HIPCHK(hipMemcpyAsync(&n_sel, (char *)st->fidx.p + cells * 4, 4, hipMemcpyDeviceToHost, S));
		if (T.end()) return fail(BHIP_E_DEVICE, "bhip_consensus_pairs: the pairs: %s", hipGetErrorString(hipGetLastError()));
		if (n_sel > cells) return fail(BHIP_E_INTERNAL, "bhip_consensus_pairs: %u of %llu pairs selected", n_sel, (pile_u64)cells);
		if (n_sel) {
			rc = st->out.reserve((uint64_t)n_sel * sizeof(BhipPair)); if (rc) return rc;
			const size_t at = result.size();
			result.resize(at + n_sel);
			if (T.begin()) return fail(BHIP_E_DEVICE, "bhip_consensus_pairs: hipEventRecord failed");
			hipLaunchKernelGGL(k_cp_emit, dim3(pile_grid(cells)), dim3(PILE_BLOCK), 0, S, st->cells.as<CpCell>(), st->flags.as<uint32_t>(), st->fidx.as<uint32_t>(), cells, (uint64_t)n_sel,
				st->hdrs.as<CpHdr>(), (uint32_t)L.size(), st->row_sample.as<uint32_t>(), st->out.as<BhipPair>());
			HIPCHK(hipGetLastError());
			HIPCHK(hipMemcpyAsync(result.data() + at, st->out.p, (uint64_t)n_sel * sizeof(BhipPair), hipMemcpyDeviceToHost, S));
			if (T.end()) return fail(BHIP_E_DEVICE, "bhip_consensus_pairs: the selection: %s", hipGetErrorString(hipGetLastError()));
		}
		g0 = g1;
	}
	info[4] = result.size(); info[5] = T.us; info[6] = st->bytes();
	*n_pairs = result.size();
	if (result.size() > pair_cap) {
		info[4] = 0;
		memcpy(st->info, info, sizeof st->info);
		return fail(BHIP_E_CAPACITY, "bhip_consensus_pairs: %llu pairs, room for %llu", (pile_u64)result.size(), (pile_u64)pair_cap);
	}
	if (!result.empty()) memcpy(pairs, result.data(), result.size() * sizeof(BhipPair));
	memcpy(st->info, info, sizeof st->info);
	return BHIP_OK;
}
