/* tests/cigar_restate.c -- TEST INFRASTRUCTURE ONLY: the canonical alignment path of DESIGN.md section 3 ("Alignment paths") on the
 * FULL matrix, no band, no packed words.  The recurrence is oracle/burst_oracle.c:orc_rescore_lane line for line, with the decision of
 * every cell recorded, then the walk back from (m, finalPos).  tests/test_cigar_cpu.py pins it to orc_rescore_lane; the GPU tests hold
 * bhip_trace_paths to it byte for byte.  Compiled by the tests into a temporary directory. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static inline uint8_t sat8(unsigned v) { return v > 255u ? 255u : (uint8_t)v; }

enum { DEC_D = 0, DEC_U = 1, DEC_L = 2 };

typedef struct CgOut {
	uint32_t ed, gapQ, gapR, finalPos;   /* what orc_rescore_lane reports: gapR from the FIRST best end column, finalPos the LAST */
	uint32_t v_final;                    /* V of cell (m, finalPos) */
	uint32_t n_best_cols;                /* end columns that attain the best (score, H) */
	uint32_t n_ops, ref_first, n_I, n_D, n_X, n_EQ;
	uint32_t n_same_cols;                /* end columns with the (score, H) of cell (m, finalPos of the path): n_best_cols when the path ends in the best column */
} CgOut;

/* q[m] against r[n] with bound B.  final_pos = 0: the end column is chosen as the re-scorer chooses it (returns 0 when no column scores
 * <= B); final_pos >= 1: the path ends there and the cell must score exactly B (returns 0 otherwise).  ops: words length << 4 | code
 * (I = 1, D = 2, '=' = 7, X = 8), forward order, runs merged; returns -1 when ops_cap is too small. */
int cg_trace(const uint8_t *q, uint32_t m, const uint8_t *r, uint32_t n, uint32_t B, const uint8_t lut[256], uint32_t final_pos,
             uint32_t *ops, uint32_t ops_cap, CgOut *out) {
	const size_t W = (size_t)n + 1;
	uint8_t *D = calloc((size_t)(m + 1) * W * 5, 1);
	uint8_t *H = D + (size_t)(m + 1) * W, *V = H + (size_t)(m + 1) * W, *dec = V + (size_t)(m + 1) * W, *cost = dec + (size_t)(m + 1) * W;
	#define AT(P, y, x) P[(size_t)(y) * W + (x)]
	memset(out, 0, sizeof *out);
	/* row 0 is all zero (burst.c:4052); row 1: burst.c:722-739 */
	AT(D, 1, 0) = 1; AT(H, 1, 0) = 0; AT(V, 1, 0) = 1; AT(dec, 1, 0) = DEC_U;
	for (uint32_t x = 1; x <= n; ++x) {
		const uint8_t s = lut[16 * q[0] + r[x - 1]];
		const int l = (s == 1 && AT(D, 1, x - 1) == 0);
		AT(D, 1, x) = s; AT(H, 1, x) = l ? 1 : 0; AT(V, 1, x) = 0;
		AT(dec, 1, x) = l ? DEC_L : DEC_D; AT(cost, 1, x) = s;
	}
	for (uint32_t y = 2; y <= m; ++y) {
		AT(D, y, 0) = sat8(y); AT(H, y, 0) = 0; AT(V, y, 0) = sat8(y); AT(dec, y, 0) = DEC_U;
		const uint8_t *L = lut + 16 * q[y - 1];
		for (uint32_t x = 1; x <= n; ++x) {
			const unsigned c = L[r[x - 1]];
			unsigned sD = sat8(AT(D, y - 1, x - 1) + c), hD = AT(H, y - 1, x - 1), vD = AT(V, y - 1, x - 1);
			unsigned sU = sat8(AT(D, y - 1, x) + 1u), hU = AT(H, y - 1, x), vU = sat8(AT(V, y - 1, x) + 1u);
			unsigned s = sD < sU ? sD : sU, h, v, d;
			const int keepD = (sD == s) && !((sU == sD) && (hU > hD));
			if (keepD) h = hD, v = vD, d = DEC_D; else h = hU, v = vU, d = DEC_U;
			unsigned sL = sat8(AT(D, y, x - 1) + 1u), hL = sat8(AT(H, y, x - 1) + 1u), vL = AT(V, y, x - 1);
			unsigned s2 = s < sL ? s : sL;
			const int keep = (s == s2) && !((sL == s) && (hL > h));
			if (!keep) h = hL, v = vL, d = DEC_L;
			s = s2;
			if (s >= B + 1) s = 255;
			AT(D, y, x) = (uint8_t)s; AT(H, y, x) = (uint8_t)h; AT(V, y, x) = (uint8_t)v; AT(dec, y, x) = (uint8_t)d; AT(cost, y, x) = (uint8_t)c;
		}
	}
	/* final selection and finalPos as orc_rescore_lane (burst.c:824-842, 862-879) */
	unsigned bs = 255, bh = 0, bv = 0;
	for (uint32_t x = 1; x <= n; ++x) {
		const unsigned s = AT(D, m, x), h = AT(H, m, x);
		if (s < bs || (s == bs && h > bh)) bs = s, bh = h, bv = AT(V, m, x);
	}
	uint32_t fin = 0, ncols = 0;
	for (uint32_t x = 1; x <= n; ++x) if (AT(D, m, x) == bs && AT(H, m, x) == bh) { fin = x; ++ncols; }
	out->ed = bs; out->gapQ = bh; out->gapR = bv; out->finalPos = fin; out->n_best_cols = ncols;
	int ok = 1;
	if (!final_pos) { if (bs > B) ok = 0; final_pos = fin; }
	else if (final_pos > n || AT(D, m, final_pos) != B) ok = 0;
	if (!ok) { free(D); return 0; }
	out->v_final = AT(V, m, final_pos);
	for (uint32_t x = 1; x <= n; ++x) if (AT(D, m, x) == AT(D, m, final_pos) && AT(H, m, x) == AT(H, m, final_pos)) ++out->n_same_cols;
	/* the walk back: runs collected backwards, reversed at the end */
	uint32_t y = m, x = final_pos, cnt = 0, cur = 0, len = 0;
	int over = 0;
	while (y > 0) {
		const unsigned d = AT(dec, y, x);
		uint32_t code;
		if (d == DEC_D) { code = AT(cost, y, x) ? 8u : 7u; if (code == 8u) ++out->n_X; else ++out->n_EQ; }
		else if (d == DEC_U) { code = 1u; ++out->n_I; }
		else { code = 2u; ++out->n_D; }
		if (code == cur) ++len;
		else {
			if (len) { if (cnt < ops_cap) ops[cnt] = len << 4 | cur; else over = 1; ++cnt; }
			cur = code; len = 1;
		}
		if (d == DEC_D) { --y; --x; } else if (d == DEC_U) --y; else --x;
	}
	if (len) { if (cnt < ops_cap) ops[cnt] = len << 4 | cur; else over = 1; ++cnt; }
	free(D);
	if (over) return -1;
	for (uint32_t i = 0; i < cnt / 2; ++i) { const uint32_t t = ops[i]; ops[i] = ops[cnt - 1 - i]; ops[cnt - 1 - i] = t; }
	out->n_ops = cnt; out->ref_first = x + 1;
	return 1;
	#undef AT
}
