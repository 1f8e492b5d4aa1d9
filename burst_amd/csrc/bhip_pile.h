// burst_amd/csrc/bhip_pile.h -- what bhip_pile_run (bhip_pile.hip) and bhip_consensus_run (bhip_consensus.hip) share: the lines as the
// device holds them, the candidate sites, the scratch buffers on the handle, and the stages both entry points run -- the host checks of
// the lines, the event count with the sorted starts and one-past-ends, and the candidate sites (walk, sort, heads, reduce).
#ifndef BHIP_PILE_H
#define BHIP_PILE_H
#include "bhip_handle.h"

#define PILE_BLOCK 256
#define PILE_MAX_GRID 65536u
#define PILE_CLS_DEL 4u
#define PILE_CLS_OTHER 5u
#define PILE_CLS_INS 6u

struct PileLine { unsigned long long qbase, op_off; uint32_t refIx, ref_first, header, pos, w, n_ops; };      // qbase: offset of the query entry in the uploaded symbols
struct PileCand { unsigned long long key; uint32_t n[6], ins, ref; };
typedef unsigned long long pile_u64;

// code of 0-based column `col` of a lane whose first dword is refw[base]
__device__ __forceinline__ uint32_t pile_ref(const uint32_t *__restrict__ refw, uint64_t base, uint32_t col) { return (refw[base + (col >> 3)] >> (4u * (col & 7u))) & 15u; }
// number of sorted keys that are <= key
__device__ __forceinline__ uint64_t pile_upper_bound(const unsigned long long *__restrict__ keys, uint64_t n, unsigned long long key) {
	uint64_t lo = 0, hi = n;
	while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (keys[mid] <= key) lo = mid + 1; else hi = mid; }
	return lo;
}

struct PileState {
	DBuf lines, span, ops, codes, cnt, off, ev_key, ev_val, ev_key_s, ev_val_s, head, idx, cand, k_start, k_end, w_start, w_end, k_start_s, k_end_s, w_start_s, w_end_s,
	     cs, ce, site, keep, out, n_sel, tmp;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	uint64_t bytes() const {
		const DBuf *all[] = {&lines, &span, &ops, &codes, &cnt, &off, &ev_key, &ev_val, &ev_key_s, &ev_val_s, &head, &idx, &cand, &k_start, &k_end, &w_start, &w_end,
			&k_start_s, &k_end_s, &w_start_s, &w_end_s, &cs, &ce, &site, &keep, &out, &n_sel, &tmp};
		uint64_t b = 0;
		for (const DBuf *x : all) b += x->cap;
		return b;
	}
};

static inline uint32_t pile_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + PILE_BLOCK - 1) / PILE_BLOCK, PILE_MAX_GRID); }
static inline int pile_bits(uint32_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

// the lines of a call as the kernels take them, every one checked on the host (`who` opens the error texts)
struct PileInput {
	std::vector<PileLine> dl; std::vector<uint32_t> span; std::vector<uint8_t> codes;
	uint32_t max_header = 0;
	int end_bit() const { return 32 + std::max(1, pile_bits(max_header)); }      // the bits of a key header << 32 | position
};
int pile_check_lines(const char *who, Handle *h, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
		const uint32_t *ops, uint64_t n_ops, PileInput &in);
// the handle's scratch state, made by the first call that launches
int pile_state(Handle *h, PileState **out);
// upload; the events of every line counted and scanned (st->off); the starts and one-past-ends sorted (st->k_start_s, st->k_end_s; st->k_start
// and st->k_end keep the order of the lines) with the running sums of their weights (st->cs, st->ce).  Ends with the stream idle
int pile_stage_lines(Handle *h, PileState *st, const PileInput &in, const uint32_t *ops, uint64_t n_ops, pile_u64 *n_events, uint64_t *us);
// n_events >= 1: the events written and sorted, a candidate opened at every new key (st->head, st->idx), st->cand sized.  Ends with the stream idle
int pile_stage_cands(Handle *h, PileState *st, const PileInput &in, uint64_t n_events, const char *who, pile_u64 *n_cand, uint64_t *us);
// enqueues the reduction of the sorted events into st->cand
int pile_launch_reduce(Handle *h, PileState *st, uint64_t n_events, uint64_t n_cand);
#endif
