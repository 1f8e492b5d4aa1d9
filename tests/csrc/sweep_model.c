/* tests/csrc/sweep_model.c -- TEST INFRASTRUCTURE ONLY: the prefix stage of the two-stage sweep as a plain full matrix.
 *
 * D[0][x] = 0 (an alignment may start in any column), D[y][0] = y, and
 * D[y][x] = min(D[y-1][x-1] + cost(q[y-1], r[x-1]), D[y-1][x] + 1, D[y][x-1] + 1),
 * cost = 0 where the 16 x 16 score table holds 0 for (query symbol, reference symbol) and 1 otherwise; a reference symbol of code 0
 * (the pads behind a lane and the filler of its last 32-column chunk) matches nothing.  No bit vectors, no bands, no carries: one
 * column of P + 1 integers at a time.  tests/sweeplib.py compiles this file and groups the rows it returns. */
#include <stdint.h>
#include <stdlib.h>

/* row P of the matrix of q[0 .. P) against each of n_lanes lanes of Lp symbols (lane-major: lanes[z * Lp + x]) into out[z * Lp + x],
 * x = 0 .. Lp - 1 standing for the 1-based columns 1 .. Lp.  Returns 0, or -1 when memory ran out. */
int sw_prefix_rows(const uint8_t *q, uint32_t P, const uint8_t *lanes, uint32_t n_lanes, uint32_t Lp, const uint8_t *lut, int32_t *out) {
	int32_t *col = (int32_t *)malloc(((size_t)P + 1) * sizeof(int32_t));
	int32_t *cost = (int32_t *)malloc(16 * ((size_t)P + 1) * sizeof(int32_t));      /* cost[r * P + y - 1]: query symbol y against reference code r */
	if (!col || !cost) { free(col); free(cost); return -1; }
	for (uint32_t rs = 0; rs < 16; ++rs)
		for (uint32_t y = 0; y < P; ++y) cost[(size_t)rs * P + y] = (rs != 0u && lut[(q[y] & 15u) * 16u + rs] == 0) ? 0 : 1;
	for (uint32_t z = 0; z < n_lanes; ++z) {
		const uint8_t *r = lanes + (size_t)z * Lp;
		for (uint32_t y = 0; y <= P; ++y) col[y] = (int32_t)y;                  /* column 0 */
		for (uint32_t x = 1; x <= Lp; ++x) {
			const int32_t *cr = cost + (size_t)(r[x - 1] & 15u) * P;
			int32_t diag = col[0];                                             /* D[y-1][x-1] */
			col[0] = 0;
			for (uint32_t y = 1; y <= P; ++y) {
				int32_t v = diag + cr[y - 1];
				if (col[y] + 1 < v) v = col[y] + 1;                            /* from the left: D[y][x-1] + 1 */
				if (col[y - 1] + 1 < v) v = col[y - 1] + 1;                    /* from above: D[y-1][x] + 1 */
				diag = col[y];
				col[y] = v;
			}
			out[(size_t)z * Lp + (x - 1)] = col[P];
		}
	}
	free(col); free(cost);
	return 0;
}
