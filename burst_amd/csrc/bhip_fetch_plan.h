// burst_amd/csrc/bhip_fetch_plan.h -- where the packed query of a re-scored hit is fetched from (option "fetch_once"), as a function of its
// inputs alone: the kernels' registers and LDS, the word count of the length class and the option.  The rule: a form that keeps operands in
// dynamic LDS, or needs more registers, is taken only where it costs no resident wave against the kernel it replaces.  No HIP in here:
// tests/csrc/fetch_plan_host.cpp compiles it with the host compiler and tests/test_fetch_plan_cpu.py pins its rows.
#ifndef BHIP_FETCH_PLAN_H
#define BHIP_FETCH_PLAN_H
#include <stdint.h>
#include <stddef.h>
#include <algorithm>

// what the runtime says about a kernel (hipFuncAttributes::numRegs, sharedSizeBytes)
struct BhipKernelRes { int regs; size_t lds; };

// Resident blocks per CU of a kernel from its register / LDS use (512 VGPRs per SIMD lane granted in steps of 8, at most 8 waves per SIMD;
// about 148 KB of the 160 KB of LDS in steps of 512 B -- measured on gfx950: 11 single-wave blocks of 13 144 B fit a CU and 12 do not, 10 of
// 14 168 B fit and 11 do not)
static inline uint32_t bhip_resident_blocks(uint32_t threads, BhipKernelRes k, size_t dyn_lds) {
	const uint32_t waves_per_block = (threads + 63) / 64;
	const uint32_t by_reg = 4u * std::min(8u, 512u / (uint32_t)std::max(8, (k.regs + 7) & ~7)) / waves_per_block;
	const size_t lds = k.lds + dyn_lds;
	const uint32_t by_lds = lds ? (uint32_t)((148u * 1024u) / std::max<size_t>(512, (lds + 511) & ~(size_t)511)) : 64u;
	return std::max(1u, std::min(by_reg, by_lds));
}
#define BHIP_LDS_BLOCK_MAX 65536u            // dynamic LDS one block may ask for

// ---- the packed query of a hit in k_rescore_reg<SET, FORM> (64-thread blocks) ----
//   BHIP_QF_DWORD  one dword of `qpack` every 8 rows (the form before this option)
//   BHIP_QF_LDS    the whole row copied once into a private LDS column of qw dwords, [dword][thread]
//   BHIP_QF_CHUNK  one aligned 16-byte chunk every 32 rows: the class is too long for the LDS form
enum { BHIP_QF_DWORD = 0, BHIP_QF_LDS = 1, BHIP_QF_CHUNK = 2, BHIP_QF_COUNT = 3 };
struct BhipQueryFetch {
	int form;
	uint32_t lds_bytes;      // dynamic LDS of the launch (BHIP_QF_LDS: qw * 256)
	uint32_t blocks;         // resident 64-thread blocks per CU of the chosen kernel
	bool tail;               // BHIP_QF_CHUNK: a row is no multiple of four dwords, so the rows start at any dword of a chunk and the last
	                         // chunk of a row reaches into the next row (into the slack behind the array for the last row)
};
// qw: dwords per row of `qpack` (the lane's longest class); res[form]: the three kernels of one register set
static inline BhipQueryFetch bhip_plan_query_fetch(uint32_t qw, int fetch_once, const BhipKernelRes res[BHIP_QF_COUNT]) {
	const uint32_t base = bhip_resident_blocks(64u, res[BHIP_QF_DWORD], 0);
	if (!fetch_once || !qw) return {BHIP_QF_DWORD, 0u, base, false};
	const uint64_t lds = (uint64_t)qw * 256u;
	if (lds <= BHIP_LDS_BLOCK_MAX) {
		const uint32_t b = bhip_resident_blocks(64u, res[BHIP_QF_LDS], (size_t)lds);
		if (b >= base) return {BHIP_QF_LDS, (uint32_t)lds, b, false};
	}
	const uint32_t b = bhip_resident_blocks(64u, res[BHIP_QF_CHUNK], 0);
	if (b >= base) return {BHIP_QF_CHUNK, 0u, b, (qw & 3u) != 0};
	return {BHIP_QF_DWORD, 0u, base, false};
}
#endif
