/* bh_dna.c -- the compressive (-d DNA / RNA) database build: duplicate marks and the shear they guide (process_references, DNA_16
 * branch, burst.c:1859-2108).
 *
 * bh_dna_marks_host is a plain restatement of the reference's marks: a counting sort of the eligible positions by their 13-mer, a
 * sort of each bin by the symbols [13, W), then the tally and the marking loop exactly as burst.c:1961-2023 write them (the tally
 * never resets `sh` inside a bin, the marking loop does; a bin's final run is never evaluated).  It is the path of a machine
 * without a device, the path the CPU tests take, and what the device pass (bhip_dna_marks, bhip_dnadb.hip) is compared with.
 * bh_dna_shear is the serial flag-guided shear of burst.c:2031-2103. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <omp.h>

#define NL 13
#define NIB_BITS (2 * NL)

/* conv of a full class of c + 1 equal windows (burst.c:2013-2015).  t == 0 (maxChain > 2048 c) reaches __builtin_clz(0): the compiled
 * reference evaluates 35 - lzcnt(0) = 3 there (pinned by the golden case `chain_t0`, tests/golden/make_golden_dna.py) */
static inline uint8_t full_conv(uint64_t c, uint64_t maxChain) {
	uint64_t t = c * 2048 / maxChain;
	if (t > 2048) t = 2048;
	if (!t) return 3;
	return (uint8_t)(31 - __builtin_clz((uint32_t)t) + 4);
}

/* the window comparison of the two loops: first differing symbol of [NL, W), or W - NL when there is none (whereDiff, 1791-1804) */
static inline uint32_t where_diff(const uint8_t *a, const uint8_t *b, uint32_t eqlen) {
	uint32_t k = 0;
	while (k < eqlen && a[k] == b[k]) ++k;
	return k;
}

static const uint8_t *g_sym;
static uint32_t g_cmp_len;
static int pos_cmp(const void *x, const void *y) {
	const uint64_t a = *(const uint64_t *)x, b = *(const uint64_t *)y;
	const int c = memcmp(g_sym + a + NL, g_sym + b + NL, g_cmp_len);
	return c ? c : (a < b ? -1 : a > b);
}

int bh_dna_marks_host(const uint8_t *sym, const uint64_t *ref_start, const uint32_t *ref_len, uint64_t n_refs, uint32_t W,
                      uint64_t *max_chain, uint64_t *max_sh, uint8_t *flags) {
	if (W < 24) return bh_set_error(BH_E_USAGE, "ERROR: window %u (shear + overlap) below 24 symbols", W);
	if (!n_refs) return BH_OK;
	const uint64_t span = ref_start[n_refs - 1] + ref_len[n_refs - 1];
	memset(flags, 0, span);
	/* 1. eligible positions (1899-1915) */
	uint64_t cand = 0;
	for (uint64_t i = 0; i < n_refs; ++i) if (ref_len[i] > W) cand += ref_len[i] - W;
	uint32_t *bin = malloc((cand + 1) * 4), *bin2 = malloc((cand + 1) * 4);
	uint64_t *pos = malloc((cand + 1) * 8), *pos2 = malloc((cand + 1) * 8);
	const uint64_t NLB = 1ull << NIB_BITS;
	uint64_t *bstart = calloc(NLB + 1, 8);
	if (!bin || !bin2 || !pos || !pos2 || !bstart) { free(bin); free(bin2); free(pos); free(pos2); free(bstart); return bh_set_error(BH_E_OOM, "OOM:dna_marks"); }
	uint64_t n = 0;
	for (uint64_t i = 0; i < n_refs; ++i) {
		if (ref_len[i] <= W) continue;
		const uint8_t *so = sym + ref_start[i];
		for (uint32_t j = 0; j < ref_len[i] - W; ++j) {
			const uint8_t *s = so + j;
			uint32_t nib = 0; int k = 0;
			for (; k < NL; ++k) { if (!s[k] || s[k] > 4) break; nib = nib << 2 | (uint32_t)(s[k] - 1); }
			if (k < NL) continue;
			bin[n] = nib; pos[n++] = ref_start[i] + j;
		}
	}
	/* 2. counting sort by bin (two stable 13-bit passes), then each bin by its symbols [13, W) */
	{
		const uint32_t R = 1u << 13;
		uint64_t *cnt = malloc((R + 1) * 8);
		for (int pass = 0; pass < 2; ++pass) {
			const int sh = 13 * pass;
			memset(cnt, 0, (R + 1) * 8);
			for (uint64_t i = 0; i < n; ++i) ++cnt[((bin[i] >> sh) & (R - 1)) + 1];
			for (uint32_t b = 0; b < R; ++b) cnt[b + 1] += cnt[b];
			for (uint64_t i = 0; i < n; ++i) { const uint64_t d = cnt[(bin[i] >> sh) & (R - 1)]++; bin2[d] = bin[i]; pos2[d] = pos[i]; }
			uint32_t *tb = bin; bin = bin2; bin2 = tb;
			uint64_t *tp = pos; pos = pos2; pos2 = tp;
		}
		free(cnt);
	}
	free(bin2); free(pos2);
	for (uint64_t i = 0; i < n; ++i) ++bstart[bin[i] + 1];
	for (uint64_t b = 0; b < NLB; ++b) bstart[b + 1] += bstart[b];
	free(bin);
	g_sym = sym; g_cmp_len = W - NL;
	#pragma omp parallel for schedule(dynamic, 4096)
	for (uint64_t b = 0; b < NLB; ++b)
		if (bstart[b + 1] - bstart[b] > 1) qsort(pos + bstart[b], bstart[b + 1] - bstart[b], 8, pos_cmp);
	const uint32_t eqlen = W - NL, nibLen = 24 - NL;
	/* 3. tally (1961-1986): only while neither value has been set */
	if (*max_chain == 0 && *max_sh == 0) {
		uint64_t mc = 0, ms = 0;
		#pragma omp parallel for schedule(dynamic, 4096) reduction(max:mc, ms)
		for (uint64_t b = 0; b < NLB; ++b) {
			uint64_t chain = 0, sh = 0;
			for (uint64_t j = bstart[b] + 1; j < bstart[b + 1]; ++j) {
				const uint32_t where = where_diff(sym + pos[j - 1] + NL, sym + pos[j] + NL, eqlen);
				if (where >= nibLen) ++sh;
				else if (sh > ms) ms = sh;
				if (where >= eqlen) ++chain;
				else { if (chain > mc) mc = chain; chain = 0; }
			}
		}
		*max_chain = mc; *max_sh = ms;
	}
	/* 4. thresholds (1989), 5. marks (1993-2023) */
	const uint64_t maxChain = *max_chain, sh1 = (uint64_t)(sqrt((double)*max_sh) / 2), sh2 = sh1 * 4 / 3, sh3 = sh1 * 3;
	int div0 = 0;
	#pragma omp parallel for schedule(dynamic, 4096) reduction(|:div0)
	for (uint64_t b = 0; b < NLB; ++b) {
		uint64_t chain = 0, sh = 0;
		for (uint64_t j = bstart[b] + 1; j < bstart[b + 1]; ++j) {
			const uint32_t where = where_diff(sym + pos[j - 1] + NL, sym + pos[j] + NL, eqlen);
			if (where >= nibLen) ++sh;
			else {
				if (sh > sh1) {
					const uint8_t conv = sh >= sh3 ? 3 : sh >= sh2 ? 2 : 1;
					for (uint64_t k = j - sh; k <= j; ++k) flags[pos[k - 1]] |= conv;
				}
				sh = 0;
			}
			if (where >= eqlen) ++chain;
			else {
				if (chain) {
					if (!maxChain) div0 = 1;
					else {
						const uint8_t conv = full_conv(chain, maxChain);
						for (uint64_t k = j - chain; k <= j; ++k) flags[pos[k - 1]] |= conv;
					}
				}
				chain = 0;
			}
		}
	}
	free(pos); free(bstart);
	if (div0) return bh_set_error(BH_E_USAGE, "ERROR: a later partition holds duplicate windows but the first tallied partition had none "
	                              "(the reference divides by zero here); use fewer partitions (-dp)");
	return BH_OK;
}

int bh_dna_shear(const uint8_t *flags, const uint64_t *ref_start, const uint32_t *ref_len, uint32_t n_refs, uint32_t shear, uint32_t ov,
                 uint32_t *frag_ref, uint32_t *frag_start, uint32_t *frag_len, uint64_t cap, uint64_t *n_frag) {
	uint64_t x = 0;
	for (uint32_t i = 0; i < n_refs; ++i) {
		const uint8_t *f = flags + ref_start[i];
		const uint32_t L = ref_len[i];
		uint32_t bstFlgPos = 0, end = 0, bstFlg = f[0];
		while (end < L) {
			const uint64_t ix = x++;
			if (ix >= cap) return bh_set_error(BH_E_INTERNAL, "ERROR: Rebase overflow.");
			frag_ref[ix] = i; frag_start[ix] = bstFlgPos;
			uint32_t bf = 0, bi = 0;
			const uint32_t maxIX = L < bstFlgPos + shear ? L : bstFlgPos + shear;
			for (uint32_t j = bstFlgPos + 1; j < maxIX; ++j) if (f[j] >= bf) bf = f[j], bi = j;
			if (bf > bstFlg) bstFlgPos = bi;
			else bstFlgPos += shear;
			if (bstFlg > 3) end = maxIX + ov < L ? maxIX + ov : L;
			else end = bstFlgPos + ov < L ? bstFlgPos + ov : L;
			if (bstFlgPos < L) bstFlg = f[bstFlgPos];
			frag_len[ix] = end - frag_start[ix];
		}
	}
	*n_frag = x;
	return BH_OK;
}
