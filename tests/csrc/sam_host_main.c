/* bh_sam.c as a stand-alone program (built by tests/test_sam_cpu.py with the address and undefined-behaviour sanitizers, with bh_paths.c
 * and bh_tables.c): bh_md_host on hand-made paths, the writer behind a fake tracer and bh_md_host as its MD function -- the capacity retry
 * of the MD call, flags, secondary lines, a duplicate read, name truncation, unmapped reads in file order --, the SN collision, and a
 * failing MD function that leaves no file.  The device entry points and the coverage's length sources are stubs: nothing here reaches them. */
#include "burst_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

int bhip_trace_paths(void *h, const uint8_t *c, const uint64_t *o, uint32_t nq, const BhipPathReq *r, uint64_t n, uint32_t *ops, uint64_t cap, uint64_t *off, uint32_t *f, uint32_t *g) {
	(void)h; (void)c; (void)o; (void)nq; (void)r; (void)n; (void)ops; (void)cap; (void)off; (void)f; (void)g; return BHIP_E_DEVICE;
}
int bhip_paths_info(void *h, uint64_t info[4]) { (void)h; memset(info, 0, 32); return 0; }
int bhip_md_tags(void *h, const BhipPathReq *r, const uint32_t *f, const uint64_t *off, const uint32_t *ops, uint64_t n, char *md, uint64_t cap, uint64_t *md_off, uint32_t *nm, uint64_t info[8]) {
	(void)h; (void)r; (void)f; (void)off; (void)ops; (void)n; (void)md; (void)cap; (void)md_off; (void)nm; (void)info; return BHIP_E_DEVICE;
}
const char *bhip_last_error(void) { return "no device in this program"; }
int bh_cov_read_lengths(const char *file, const char *flag, uint32_t n, const char *const *heads, uint32_t *len) { (void)file; (void)flag; (void)n; (void)heads; (void)len; return BH_E_IO; }
int bh_cov_default_lengths(const BhDb *db, void *hh, uint32_t *len) { (void)db; (void)hh; (void)len; return BH_E_DEVICE; }

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
#define W(n, op) ((uint32_t)(n) << 4 | (op))

/* one lane of 64 columns: A C G T repeated, but K at column 9 (0-based 8) and the pad code at column 33 (0-based 32) */
static uint8_t lane[64];
static int n_md_calls, n_md_capacity, md_fails;
/* request i: the ops of its record, from the lane column its finalPos names */
static const uint32_t path_ops[4][4] = {{W(8, BHIP_OP_EQ)}, {W(3, BHIP_OP_EQ), W(2, BHIP_OP_D), W(1, BHIP_OP_X), W(4, BHIP_OP_EQ)}, {W(1, BHIP_OP_I), W(7, BHIP_OP_EQ)}, {W(2, BHIP_OP_X)}};
static const uint32_t path_n[4] = {1, 4, 2, 1};
static int fake_trace(void *ctx, const BhQueries *Q, const BhipPathReq *req, uint64_t n, uint32_t *ops, uint64_t cap, uint64_t *off, uint32_t *first, uint32_t *gap_r) {
	(void)ctx; (void)Q;
	off[0] = 0;
	for (uint64_t i = 0; i < n; ++i) { off[i + 1] = off[i] + path_n[req[i].ed]; first[i] = req[i].finalPos; gap_r[i] = 0; }
	if (off[n] > cap) return BH_E_CAPACITY;
	for (uint64_t i = 0; i < n; ++i) memcpy(ops + off[i], path_ops[req[i].ed], path_n[req[i].ed] * 4);
	return BH_OK;
}
static int md_by_host(void *ctx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t n, char *md, uint64_t cap, uint64_t *md_off,
                      uint32_t *nm, uint64_t info[8]) {
	(void)ctx; (void)req;
	++n_md_calls;
	if (md_fails) return bh_set_error(BH_E_DEVICE, "the MD function fails on purpose");
	memset(info, 0, 64);
	md_off[0] = 0;
	for (uint64_t i = 0; i < n; ++i) {
		uint64_t len = 0;
		const uint64_t room = md_off[i] < cap ? cap - md_off[i] : 0;
		const int rc = bh_md_host(lane, 64, first[i], ops + off[i], off[i + 1] - off[i], room ? md + md_off[i] : NULL, room, &len, &nm[i]);
		if (rc && rc != BH_E_CAPACITY) return rc;
		md_off[i + 1] = md_off[i] + len;
	}
	if (md_off[n] > cap) { ++n_md_capacity; return BH_E_CAPACITY; }
	return BH_OK;
}

static char *slurp(const char *path) {
	FILE *f = fopen(path, "rb");
	if (!f) return NULL;
	char *s = calloc(1, 1 << 16);
	if (s && fread(s, 1, (1 << 16) - 1, f) == 0) s[0] = 0;
	fclose(f);
	return s;
}

int main(int argc, char **argv) {
	if (argc < 2) { fputs("usage: sam_host_main OUT.b6\n", stderr); return 2; }
	for (int i = 0; i < 64; ++i) lane[i] = (uint8_t)(1 + i % 4);
	lane[8] = 6; lane[32] = 0;
	/* ---- bh_md_host ---- */
	char md[64]; uint64_t len = 0; uint32_t nm = 0;
	const uint32_t p1[] = {W(3, BHIP_OP_EQ), W(2, BHIP_OP_D), W(1, BHIP_OP_X), W(4, BHIP_OP_EQ)};
	CHECK(bh_md_host(lane, 64, 1, p1, 4, md, sizeof md, &len, &nm) == BH_OK && len == 7 && !memcmp(md, "3^TA0C4", 7) && nm == 3);
	CHECK(bh_md_host(lane, 64, 1, p1, 4, md, 6, &len, &nm) == BH_E_CAPACITY && len == 7);
	CHECK(bh_md_host(lane, 64, 1, p1, 4, NULL, 0, &len, &nm) == BH_E_CAPACITY && len == 7);
	const uint32_t p2[] = {W(1, BHIP_OP_X), W(1, BHIP_OP_D)};
	CHECK(bh_md_host(lane, 64, 8, p2, 2, md, sizeof md, &len, &nm) == BH_OK && len == 6 && !memcmp(md, "0T0^K0", 6) && nm == 2);
	const uint32_t p3[] = {W(1, BHIP_OP_X)};
	CHECK(bh_md_host(lane, 64, 33, p3, 1, md, sizeof md, &len, &nm) == BH_OK && len == 3 && !memcmp(md, "0N0", 3));      /* the pad code */
	CHECK(bh_md_host(lane, 64, 64, p3, 1, md, sizeof md, &len, &nm) == BH_OK);                                                /* the lane's last column */
	CHECK(bh_md_host(lane, 64, 65, p3, 1, md, sizeof md, &len, &nm) == BH_E_USAGE);
	CHECK(bh_md_host(lane, 64, 0, p3, 1, md, sizeof md, &len, &nm) == BH_E_USAGE);
	const uint32_t bad[] = {W(4, 3u)}, zero[] = {BHIP_OP_EQ};
	CHECK(bh_md_host(lane, 64, 1, bad, 1, md, sizeof md, &len, &nm) == BH_E_USAGE && bh_md_host(lane, 64, 1, zero, 1, md, sizeof md, &len, &nm) == BH_E_USAGE);
	CHECK(bh_md_host(lane, 64, 5, NULL, 0, md, sizeof md, &len, &nm) == BH_OK && len == 1 && md[0] == '0' && nm == 0);
	/* ---- the SN collision ---- */
	BhSam *sm = NULL;
	const char *clash[] = {"chr1 first", "chr2", "chr1\tsecond"};
	const uint32_t lens3[] = {64, 64, 64};
	CHECK(bh_sam_open_heads(3, clash, lens3, 0, &sm) == BH_E_USAGE && !sm);
	CHECK(strstr(bh_last_error(), "'chr1 first'") && strstr(bh_last_error(), "'chr1\tsecond'"));
	puts(bh_last_error());
	const char *same[] = {"chr1 x", "chr1 x"};      /* (the same header twice is no collision of two different ones) */
	CHECK(bh_sam_open_heads(2, same, lens3, 0, &sm) == BH_OK);
	bh_sam_close(sm); sm = NULL;
	/* ---- the writer ----
	 * four unique queries: u0 = reads {r0 extra, dup}, forward, 2 placements each (records 0, 1); u1 = read r1, on the reverse entry (record 2);
	 * u2 = read `lost` without a line; u3 = read r3 (record 3).  Entries 0 .. 3 forward, 4 .. 7 their reverse complements */
	char dump[] = "r3\0lost one\0r0 extra\0r1\0dup";      /* (file order: r3, lost, r0, r1, dup) */
	char *heads[5] = {dump + 12, dump + 24, dump + 21, dump + 3, dump + 0};      /* sorted-sequence order: u0: r0 extra, dup; u1: r1; u2: lost one; u3: r3 */
	uint64_t offset[5] = {0, 2, 3, 4, 5};
	uint8_t codes[8 * 8];
	uint64_t qoff[9];
	uint32_t six[8]; uint8_t rcs[8];
	for (int e = 0; e < 8; ++e) { qoff[e] = 8u * (unsigned)e; six[e] = (uint32_t)(e % 4); rcs[e] = e >= 4; for (int k = 0; k < 8; ++k) codes[8 * e + k] = (uint8_t)(e < 4 ? 1 + (e + k) % 4 : 4 - (e + k) % 4); }
	qoff[8] = 64;
	codes[0] = 0; codes[1] = 15;      /* a pad code and an IUPAC letter in SEQ */
	BhQueries Q; memset(&Q, 0, sizeof Q);
	Q.totQ = 5; Q.numUniq = 4; Q.numEntries = 8; Q.dump = dump; Q.heads = heads; Q.offset = offset; Q.codes = codes; Q.qoff = qoff; Q.six = six; Q.rc = rcs;
	BhipHit hits[4]; memset(hits, 0, sizeof hits);
	hits[0].q = 0; hits[0].refIx = 0; hits[0].finalPos = 1; hits[0].ed = 0;       /* 8= from column 1 */
	hits[1].q = 0; hits[1].refIx = 0; hits[1].finalPos = 5; hits[1].ed = 1;       /* 3=2D1X4= from column 5 */
	hits[2].q = 5; hits[2].refIx = 0; hits[2].finalPos = 30; hits[2].ed = 2;      /* 1I7= from column 30: crosses the pad column as a match */
	hits[3].q = 3; hits[3].refIx = 0; hits[3].finalPos = 8; hits[3].ed = 3;       /* 2X on columns 8 and 9 */
	BhPathBuf bufs[2]; memset(bufs, 0, sizeof bufs);
	char *text[2] = {NULL, NULL}; size_t tl[2] = {0, 0};
	FILE *m0 = open_memstream(&text[0], &tl[0]), *m1 = open_memstream(&text[1], &tl[1]);
	CHECK(m0 && m1);
	/* u0: per read its two lines (header 1, then header 0), read after read; then u1's reverse line */
	const char *u0[2] = {"r0 extra", "dup"};
	for (int j = 0; j < 2; ++j) {
		fprintf(m0, "%s\tchrB x\t100.0\t8\t0\t0\t1\t8\t1001\t1008\t0\t%d\n", u0[j], j); CHECK(bh_paths_push_line(&bufs[0], 0, 1000, 1, 0));
		fprintf(m0, "%s\tchrA\t62.5\t10\t1\t2\t1\t8\t5\t14\t3\t%d\n", u0[j], j); CHECK(bh_paths_push_line(&bufs[0], 1, 0, 0, 0));
	}
	fprintf(m0, "r1\tchrA\t87.5\t8\t0\t1\t1\t8\t36\t30\t1\t0\n"); CHECK(bh_paths_push_line(&bufs[0], 2, 0, 0, 1));
	fprintf(m1, "r3\tchrA\t75.0\t2\t2\t0\t1\t2\t8\t9\t2\t0\n"); CHECK(bh_paths_push_line(&bufs[1], 3, 0, 0, 1));
	fclose(m0); fclose(m1);
	const char *names[] = {"chrA", "chrB x"};
	const uint32_t lens[] = {64, 5000};
	char sam_path[4096], tmp_glob[4096];
	snprintf(sam_path, sizeof sam_path, "%s.sam", argv[1]);
	snprintf(tmp_glob, sizeof tmp_glob, "%s.sam.tmp%ld", argv[1], (long)getpid());
	for (int pass = 0; pass < 3; ++pass) {      /* 0: mapped only; 1: with the unmapped reads; 2: the MD function fails */
		CHECK(bh_sam_open_heads(2, names, lens, pass >= 1, &sm) == BH_OK);
		bh_sam_set_md(sm, md_by_host, NULL);
		md_fails = pass == 2;
		BhPaths *p = NULL;
		CHECK(bh_paths_open(NULL, &p) == BH_OK);
		bh_paths_set_trace(p, fake_trace, NULL);
		CHECK(bh_sam_begin(sm, NULL, &Q, argv[1]) == BH_OK);
		bh_paths_set_sam(p, sm, pass == 1);
		CHECK(access(tmp_glob, F_OK) == 0 && access(sam_path, F_OK) != 0);
		FILE *out = fopen(argv[1], "wb");
		CHECK(out);
		const int rc = bh_paths_emit(p, out, &Q, hits, text, tl, bufs, 2);
		CHECK(fclose(out) == 0);
		if (pass == 2) {
			CHECK(rc == BH_E_DEVICE && bh_sam_end(sm) == BH_E_DEVICE);
			CHECK(access(tmp_glob, F_OK) != 0 && access(sam_path, F_OK) != 0);      /* (neither the file nor its temporary name) */
			bh_sam_close(sm); bh_paths_close(p);
			break;
		}
		CHECK(rc == BH_OK && bh_sam_end(sm) == BH_OK);
		CHECK(access(tmp_glob, F_OK) != 0 && access(sam_path, F_OK) == 0);
		uint64_t info[4];
		bh_sam_last_info(sm, info);
		CHECK(info[0] == 6 && info[1] == (pass ? 1u : 0u) && info[2] == 1 + 7 + 1 + 5);
		bh_sam_print_info(sm);
		char *got = slurp(sam_path), *b6 = slurp(argv[1]);
		CHECK(got && b6);
		const char *want_head = "@HD\tVN:1.6\tSO:unknown\tGO:query\n@SQ\tSN:chrA\tLN:64\n@SQ\tSN:chrB\tLN:5000\n@PG\tID:burst_hip\tPN:burst_hip\n";
		const char *want_rec =
			"r0\t0\tchrB\t1001\t255\t8=\t*\t0\t0\t.DGTACGT\t*\tNM:i:0\tMD:Z:8\n"
			"r0\t256\tchrA\t5\t255\t3=2D1X4=\t*\t0\t0\t.DGTACGT\t*\tNM:i:3\tMD:Z:3^TK0C4\n"
			"dup\t0\tchrB\t1001\t255\t8=\t*\t0\t0\t.DGTACGT\t*\tNM:i:0\tMD:Z:8\n"
			"dup\t256\tchrA\t5\t255\t3=2D1X4=\t*\t0\t0\t.DGTACGT\t*\tNM:i:3\tMD:Z:3^TK0C4\n"
			"r1\t16\tchrA\t30\t255\t1I7=\t*\t0\t0\tGCATGCAT\t*\tNM:i:1\tMD:Z:7\n"
			"r3\t0\tchrA\t8\t255\t2X\t*\t0\t0\tTACGTACG\t*\tNM:i:2\tMD:Z:0T0K0\n";
		const char *want_unm = "lost\t4\t*\t0\t0\t*\t*\t0\t0\tGTACGTAC\t*\n";
		CHECK(!strncmp(got, want_head, strlen(want_head)));
		if (strncmp(got + strlen(want_head), want_rec, strlen(want_rec))) { fputs(got, stderr); CHECK(!"records"); }
		CHECK(!strcmp(got + strlen(want_head) + strlen(want_rec), pass ? want_unm : ""));
		const char *first_line = "r0 extra\tchrB x\t100.0\t8\t0\t0\t1\t8\t1001\t1008\t0\t0";
		/* the .b6: as rendered without the columns, with them when asked */
		CHECK((strstr(b6, "\t1001\t8=\n") != NULL) == (pass == 1) && !strncmp(b6, first_line, strlen(first_line)));
		free(got); free(b6);
		bh_sam_close(sm); bh_paths_close(p);
		CHECK(unlink(sam_path) == 0);
	}
	CHECK(n_md_calls == 3 && n_md_capacity == 0);
	free(bufs[0].l); free(bufs[1].l); free(text[0]); free(text[1]);
	puts("sam_host_main ok");
	return 0;
}
