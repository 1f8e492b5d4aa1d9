/* tests/cigar_host_main.c -- TEST INFRASTRUCTURE ONLY: the host side of --cigar (csrc/host/bh_paths.c: collector, trace call with its
 * capacity retry, renderer) as a stand-alone program on hand-made inputs, for a build with -fsanitize=address,undefined
 * (tests/test_cigar_cpu.py builds and runs it; no device, no Python in the process).  The tracer is a fake with a known answer. */
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>

/* the device entry points bh_paths.c names; never called here (the tracer is replaced) */
int bhip_trace_paths(void *h, const uint8_t *c, const uint64_t *o, uint32_t nq, const BhipPathReq *r, uint64_t n, uint32_t *ops, uint64_t cap, uint64_t *off, uint32_t *f, uint32_t *g) {
	(void)h; (void)c; (void)o; (void)nq; (void)r; (void)n; (void)ops; (void)cap; (void)off; (void)f; (void)g; return BHIP_E_DEVICE;
}
int bhip_paths_info(void *h, uint64_t info[4]) { (void)h; memset(info, 0, 32); return 0; }
const char *bhip_last_error(void) { return "no device in this program"; }

static int n_calls, n_capacity;
/* request i (finalPos = 100 + its record number, ed = record number % 4): ed + 1 runs of '=' with ed X between them, starting at column q + 1 */
static int fake_trace(void *ctx, const BhQueries *Q, const BhipPathReq *req, uint64_t n, uint32_t *ops, uint64_t cap, uint64_t *off, uint32_t *first, uint32_t *gap_r) {
	(void)ctx; (void)Q;
	++n_calls;
	off[0] = 0;
	for (uint64_t i = 0; i < n; ++i) off[i + 1] = off[i] + 2 * req[i].ed + 1;
	for (uint64_t i = 0; i < n; ++i) { first[i] = req[i].q + 1; gap_r[i] = 0; }
	if (off[n] > cap) { ++n_capacity; return BH_E_CAPACITY; }
	for (uint64_t i = 0; i < n; ++i) {
		uint32_t *o = ops + off[i];
		for (uint32_t k = 0; k <= req[i].ed; ++k) { *o++ = (req[i].finalPos + k) << 4 | BHIP_OP_EQ; if (k < req[i].ed) *o++ = 1u << 4 | BHIP_OP_X; }
	}
	return BH_OK;
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main(int argc, char **argv) {
	if (argc < 2) { fputs("usage: cigar_host_main OUT\n", stderr); return 2; }
	/* the renderer */
	char t[64];
	const uint32_t ops1[] = {5u << 4 | BHIP_OP_EQ, 1u << 4 | BHIP_OP_X, 2u << 4 | BHIP_OP_I, 94u << 4 | BHIP_OP_EQ, 3u << 4 | BHIP_OP_D, 1u << 4 | BHIP_OP_EQ};
	CHECK(bh_cigar_text(ops1, 6, t, sizeof t) == 13 && !strcmp(t, "5=1X2I94=3D1="));
	CHECK(bh_cigar_text(ops1, 6, t, 13) == 0);                       /* no room for the NUL */
	CHECK(bh_cigar_text(ops1, 6, t, 14) == 13);
	const uint32_t big[] = {0xFFFFFFFu << 4 | BHIP_OP_EQ};
	CHECK(bh_cigar_text(big, 1, t, sizeof t) == 10 && !strcmp(t, "268435455="));
	const uint32_t bad_code[] = {4u << 4 | 3u}, zero_len[] = {BHIP_OP_EQ};
	CHECK(bh_cigar_text(bad_code, 1, t, sizeof t) == 0 && bh_cigar_text(zero_len, 1, t, sizeof t) == 0);
	CHECK(bh_cigar_text(ops1, 0, t, sizeof t) == 0);
	/* the collector and the writer: 3 chunks (the middle one empty), 300 records of which every one has two lines in different chunks
	 * and some a third, so that the records are fewer than the lines; their ops fit the room of the first call */
	enum { NREC = 300 };
	BhipHit *hits = calloc(NREC + 1, sizeof(*hits));
	CHECK(hits);
	for (uint32_t i = 0; i < NREC; ++i) { hits[i].q = i; hits[i].refIx = 7 * i; hits[i].finalPos = 100 + i; hits[i].ed = (uint8_t)(i % 4); }
	hits[NREC].q = NREC; hits[NREC].refIx = 1; hits[NREC].finalPos = 9; hits[NREC].ed = 200;
	BhPathBuf bufs[3]; memset(bufs, 0, sizeof bufs);
	char *text[3] = {NULL, NULL, NULL}; size_t len[3] = {0, 0, 0};
	FILE *m0 = open_memstream(&text[0], &len[0]), *m2 = open_memstream(&text[2], &len[2]);
	CHECK(m0 && m2);
	for (uint32_t i = 0; i < NREC; ++i) {
		fprintf(m0, "read%u\tref\t%u\n", i, i); CHECK(bh_paths_push(&bufs[0], i, 1000));
		fprintf(m2, "dup%u\tref\tx\ty\n", NREC - 1 - i); CHECK(bh_paths_push(&bufs[2], NREC - 1 - i, 0));
		if (i % 5 == 0) { fprintf(m2, "third%u\n", i); CHECK(bh_paths_push(&bufs[2], i, 5)); }
	}
	fclose(m0); fclose(m2);
	text[1] = NULL; len[1] = 0;
	BhPaths *p = NULL;
	CHECK(bh_paths_open(NULL, &p) == BH_OK);
	bh_paths_set_trace(p, fake_trace, NULL);
	FILE *out = fopen(argv[1], "wb");
	CHECK(out);
	BhQueries Q; memset(&Q, 0, sizeof Q);
	CHECK(bh_paths_emit(p, out, &Q, hits, text, len, bufs, 3) == BH_OK);
	uint64_t nr = 0, no = 0, nl = 0;
	bh_paths_totals(p, &nr, &no, &nl);
	CHECK(nr == NREC && nl == 2 * NREC + NREC / 5 && n_calls == 1 && n_capacity == 0);
	uint64_t want = 0; for (uint32_t i = 0; i < NREC; ++i) want += 2 * (i % 4) + 1;
	CHECK(no == want);
	/* 60 records of 401 ops each do not fit the room of the first call: the capacity answer, then the second call */
	BhipHit *bigs = calloc(64, sizeof(*bigs)); CHECK(bigs);
	BhPathBuf bb; memset(&bb, 0, sizeof bb);
	char *bt = NULL; size_t bl = 0; FILE *mb = open_memstream(&bt, &bl); CHECK(mb);
	for (uint32_t i = 0; i < 60; ++i) { bigs[i].q = i; bigs[i].finalPos = 1; bigs[i].ed = 200; fprintf(mb, "big%u\n", i); CHECK(bh_paths_push(&bb, i, 0)); }
	fclose(mb);
	char *bts[1] = {bt};
	CHECK(bh_paths_emit(p, out, &Q, bigs, bts, &bl, &bb, 1) == BH_OK);
	CHECK(n_calls == 3 && n_capacity == 1);
	/* text and notes that do not belong together are refused, not read past */
	BhPathBuf one; memset(&one, 0, sizeof one); CHECK(bh_paths_push(&one, 0, 0)); CHECK(bh_paths_push(&one, 1, 0));
	char *ot[1] = {"only one line\n"}; size_t ol = strlen(ot[0]);
	CHECK(bh_paths_emit(p, out, &Q, hits, ot, &ol, &one, 1) == BH_E_INTERNAL);
	one.n = 1;
	char *ot2[1] = {"two\nlines\n"}; ol = strlen(ot2[0]);
	CHECK(bh_paths_emit(p, out, &Q, hits, ot2, &ol, &one, 1) == BH_E_INTERNAL);
	BhPathBuf none; memset(&none, 0, sizeof none);
	CHECK(bh_paths_emit(p, out, &Q, hits, ot2, &ol, &none, 1) == BH_E_INTERNAL);
	ol = 0;
	CHECK(bh_paths_emit(p, out, &Q, hits, ot2, &ol, &none, 1) == BH_OK);
	CHECK(fclose(out) == 0);
	bh_paths_close(p);
	free(bufs[0].l); free(bufs[2].l); free(bb.l); free(one.l); free(text[0]); free(text[2]); free(bt); free(hits); free(bigs);
	puts("cigar_host_main ok");
	return 0;
}
