/* bh_sam.c -- SAM output beside the .b6, with NM and MD tags (burst_hip --sam, host.Session(sam=True)).
 *
 * No reference counterpart: the reference writes the 12 or 13 columns of its .b6 and leaves "parse the alignments downstream" to its
 * user.  A converter from that text cannot write an MD tag -- the reference bases sit packed on the device -- so the records are written
 * here, from what the run has in hand:
 *   the paths        the tracer of the --cigar columns hands every traced group to this file's collector (bh_paths_add_collector: the
 *                    group's records, first columns and ops, the notes of the printed lines, and the rendered text of those lines),
 *                    so nothing is traced twice, with or without --cigar, beside --variants or --chimeras
 *   NM and MD        ONE bhip_md_tags call per group on the handle that traced it (bh_sam_set_md: another function, for the tests)
 *   the rest         columns 1, 9, 10 of the rendered line, the header number of its note, the codes of the path's query entry
 * The file OUT.sam is written under a temporary name and renamed when the sample has succeeded (bh_sam_end); a sample that fails alone
 * (bh_sam_discard) and a run that ends on an error (bh_sam_close) leave none.
 *
 * bh_md_host is the definition of the MD string once more in plain sequential C over a lane given as an array of codes: the yardstick of
 * the tests.  The definition: include/burst_hip.h "MD tags", DESIGN.md section 7g. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static const char SAM_LETTERS[] = ".ACGTNKMRYSWBVHD";      /* SEQ: the codes as the loader read them (U is T, lower case is upper case) */
static const char MD_LETTERS[] = "NACGTNKMRYSWBVHD";       /* MD: the pad code prints N */

struct BhSam {
	const BhDb *db;
	uint32_t nH; char **sn; uint32_t *len; int have_len;      /* per unique-header number: SN, LN */
	int unmapped, dead;
	bh_md_fn fn; void *ctx; void *hh;
	/* the sample being written */
	const BhQueries *Q; FILE *tmp; char *tmpn, *finn;
	uint8_t *mapped;                                           /* [totQ] the read (index into Q->heads) has a line */
	uint64_t nRec, nUnm, mdBytes, us;
	/* buffers kept between groups */
	char *md; uint64_t mdCap; uint64_t *mdOff; uint32_t *nm; uint64_t reqCap;
	char *rec; size_t recLen, recCap;
	uint64_t info[4]; int have_info;                           /* of the last sample that was ended */
};

/* ---- the definition in plain C ---- */
int bh_md_host(const uint8_t *lane, uint32_t lane_len, uint32_t ref_first, const uint32_t *ops, uint64_t n_ops, char *md, uint64_t md_cap, uint64_t *md_len, uint32_t *nm) {
	if ((lane_len && !lane) || (n_ops && !ops) || (md_cap && !md) || !md_len || !nm) return bh_set_error(BH_E_USAGE, "bh_md_host: null argument");
	*md_len = 0; *nm = 0;
	if (ref_first < 1) return bh_set_error(BH_E_USAGE, "bh_md_host: first column 0 (columns are 1-based)");
	uint64_t o = 0, col = (uint64_t)ref_first - 1, u = 0; uint32_t edits = 0;
	char t[24];
	#define PUT(c) do { const char c_ = (char)(c); if (o < md_cap) md[o] = c_; ++o; } while (0)      /* (the argument is evaluated whether or not there is room) */
	#define NUM(v) do { uint64_t v_ = (v); int d_ = 0; do { t[d_++] = (char)('0' + v_ % 10); v_ /= 10; } while (v_); while (d_) PUT(t[--d_]); } while (0)
	for (uint64_t k = 0; k < n_ops; ++k) {
		const uint32_t len = ops[k] >> 4, code = ops[k] & 15u;
		if (!len || (code != BHIP_OP_I && code != BHIP_OP_D && code != BHIP_OP_EQ && code != BHIP_OP_X))
			return bh_set_error(BH_E_USAGE, "bh_md_host: op %llu: word 0x%x is not a run of I, D, = or X", (unsigned long long)k, ops[k]);
		if (code == BHIP_OP_I) { edits += len; continue; }
		if (col + len > lane_len) return bh_set_error(BH_E_USAGE, "bh_md_host: op %llu: the columns from %u on leave a lane of %u", (unsigned long long)k, ref_first, lane_len);
		if (code == BHIP_OP_EQ) { u += len; col += len; continue; }
		edits += len;
		if (code == BHIP_OP_D) { NUM(u); PUT('^'); u = 0; }
		for (uint32_t i = 0; i < len; ++i, ++col) {
			if (code == BHIP_OP_X) { NUM(u); u = 0; }
			PUT(MD_LETTERS[lane[col] & 15u]);
		}
	}
	NUM(u);
	#undef PUT
	#undef NUM
	*md_len = o; *nm = edits;
	return o > md_cap ? BH_E_CAPACITY : BH_OK;
}

/* the device: ctx = the handle */
static int md_device(void *ctx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t n, char *md, uint64_t md_cap, uint64_t *md_off,
                     uint32_t *nm, uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "sam: the MD tags are written on the device and rank 0 has no device handle");
	const int rc = bhip_md_tags(ctx, req, first, off, ops, n, md, md_cap, md_off, nm, info);
	if (rc == BHIP_E_CAPACITY) return BH_E_CAPACITY;
	if (rc) return bh_set_error(rc == BHIP_E_ARG || rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "sam: %s", bhip_last_error());
	return BH_OK;
}

static size_t name_len(const char *s) { size_t n = 0; while (s[n] && s[n] != ' ' && s[n] != '\t' && s[n] != '\r' && s[n] != '\n' && s[n] != '\v' && s[n] != '\f') ++n; return n; }

typedef struct { const char *sn, *head; } SnRow;
static int sn_cmp(const void *a, const void *b) { return strcmp(((const SnRow *)a)->sn, ((const SnRow *)b)->sn); }

/* SN of every header: the header up to its first white space.  Two different headers must not share one (`flag` opens the error text) */
int bh_sam_names(const char *flag, uint32_t n_headers, const char *const *heads, char ***out) {
	if (!out || !flag) return bh_set_error(BH_E_USAGE, "bh_sam_names: no place for the names");
	*out = NULL;
	if (!n_headers || !heads) return bh_set_error(BH_E_USAGE, "bh_sam_names: no headers");
	char **sn = calloc(n_headers, sizeof(*sn));
	SnRow *rows = malloc((size_t)n_headers * sizeof(*rows));
	int ok = sn && rows;
	for (uint32_t h = 0; ok && h < n_headers; ++h) {
		const char *s = heads[h] ? heads[h] : "";
		ok = (sn[h] = strndup(s, name_len(s))) != NULL;
		if (ok) { rows[h].sn = sn[h]; rows[h].head = s; }
	}
	int rc = ok ? BH_OK : bh_set_error(BH_E_OOM, "OOM:sam");
	if (ok) {
		qsort(rows, n_headers, sizeof(*rows), sn_cmp);
		for (uint32_t r = 1; r < n_headers && !rc; ++r) if (!strcmp(rows[r].sn, rows[r - 1].sn) && strcmp(rows[r].head, rows[r - 1].head))
			rc = bh_set_error(BH_E_USAGE, "ERROR: %s: the reference headers '%s' and '%s' share the name '%s' (a header up to its first white space)", flag, rows[r - 1].head, rows[r].head, rows[r].sn);
	}
	free(rows);
	if (rc) { bh_sam_names_free(sn, n_headers); return rc; }
	*out = sn;
	return BH_OK;
}
void bh_sam_names_free(char **sn, uint32_t n_headers) {
	if (sn) for (uint32_t h = 0; h < n_headers; ++h) free(sn[h]);
	free(sn);
}

int bh_sam_open_heads(uint32_t n_headers, const char *const *heads, const uint32_t *lengths, int unmapped, BhSam **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_sam_open: no place for the object");
	*out = NULL;
	if (!n_headers || !heads) return bh_set_error(BH_E_USAGE, "bh_sam_open: no headers");
	BhSam *sm = calloc(1, sizeof(*sm));
	if (!sm) return bh_set_error(BH_E_OOM, "OOM:sam");
	sm->nH = n_headers; sm->unmapped = unmapped != 0;
	sm->len = calloc(n_headers, 4);
	if (!sm->len) { bh_sam_close(sm); return bh_set_error(BH_E_OOM, "OOM:sam"); }
	const int rc = bh_sam_names("--sam", n_headers, heads, &sm->sn);
	if (rc) { bh_sam_close(sm); return rc; }
	if (lengths) { memcpy(sm->len, lengths, (size_t)n_headers * 4); sm->have_len = 1; }
	*out = sm;
	return BH_OK;
}

int bh_sam_open(const BhDb *db, const char *lengths_file, int unmapped, BhSam **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_sam_open: no place for the object");
	*out = NULL;
	if (!db || !db->numRefHeads || !db->refMap || !db->refHead) return bh_set_error(BH_E_USAGE, "bh_sam_open: no database / no reference headers");
	const char **head = calloc(db->numRefHeads, sizeof(*head));
	if (!head) return bh_set_error(BH_E_OOM, "OOM:sam");
	for (uint32_t i = 0; i < db->origTotR; ++i) if (db->refMap[i] < db->numRefHeads) head[db->refMap[i]] = db->refHead[i];      /* (the numbers the report's notes use) */
	for (uint32_t h = 0; h < db->numRefHeads; ++h) if (!head[h]) head[h] = "";
	int rc = bh_sam_open_heads(db->numRefHeads, head, NULL, unmapped, out);
	if (!rc) {
		(*out)->db = db;
		if (lengths_file && !(rc = bh_cov_read_lengths(lengths_file, "--sam-lengths", db->numRefHeads, head, (*out)->len))) (*out)->have_len = 1;
		if (rc) { bh_sam_close(*out); *out = NULL; }
	}
	free(head);
	return rc;
}

void bh_sam_set_md(BhSam *sm, bh_md_fn fn, void *ctx) { if (sm) { sm->fn = fn; sm->ctx = ctx; } }

static int die(BhSam *sm, int rc) { sm->dead = rc; return rc; }
static void drop_file(BhSam *sm) {
	if (sm->tmp) { fclose(sm->tmp); sm->tmp = NULL; }
	if (sm->tmpn) { (void)unlink(sm->tmpn); free(sm->tmpn); sm->tmpn = NULL; }
	free(sm->finn); sm->finn = NULL;
	free(sm->mapped); sm->mapped = NULL;
	sm->Q = NULL;
}

/* a new sample: OUT.sam under a temporary name, the header */
int bh_sam_begin(BhSam *sm, void *hh, const BhQueries *Q, const char *out_path) {
	if (!sm || !Q || !out_path) return bh_set_error(BH_E_USAGE, "bh_sam_begin: no sam object / queries / output");
	if (sm->dead) return bh_set_error(sm->dead, "the SAM output was ended by an earlier error");
	drop_file(sm);      /* (a sample that was begun and never ended) */
	if (!sm->have_len) {      /* the database's own extents, as the coverage takes them */
		if (!sm->db) return die(sm, bh_set_error(BH_E_USAGE, "bh_sam_begin: no reference lengths"));
		const int rc = bh_cov_default_lengths(sm->db, hh, sm->len);
		if (rc) return die(sm, rc);
		sm->have_len = 1;
	}
	sm->hh = hh; sm->nRec = sm->nUnm = sm->mdBytes = sm->us = 0;
	sm->mapped = calloc(Q->totQ + 1, 1);
	if (!sm->mapped || asprintf(&sm->finn, "%s.sam", out_path) < 0) { sm->finn = NULL; drop_file(sm); return die(sm, bh_set_error(BH_E_OOM, "OOM:sam")); }
	if (asprintf(&sm->tmpn, "%s.sam.tmp%ld", out_path, (long)getpid()) < 0) { sm->tmpn = NULL; drop_file(sm); return die(sm, bh_set_error(BH_E_OOM, "OOM:sam")); }
	if (!(sm->tmp = fopen(sm->tmpn, "wb"))) {
		const int rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", sm->tmpn);
		free(sm->tmpn); sm->tmpn = NULL;      /* (not ours to remove) */
		drop_file(sm);
		return rc;      /* (the sample's own error: the object stays usable) */
	}
	setvbuf(sm->tmp, NULL, _IOFBF, 1 << 22);
	sm->Q = Q;
	fputs("@HD\tVN:1.6\tSO:unknown\tGO:query\n", sm->tmp);
	for (uint32_t h = 0; h < sm->nH; ++h) fprintf(sm->tmp, "@SQ\tSN:%s\tLN:%u\n", sm->sn[h], sm->len[h]);
	fputs("@PG\tID:burst_hip\tPN:burst_hip\n", sm->tmp);      /* (no command line: a --samples sample's file equals a separate invocation's) */
	return BH_OK;
}

static int rec_room(BhSam *sm, size_t n) {
	if (sm->recLen + n <= sm->recCap) return 1;
	size_t nc = sm->recCap ? sm->recCap * 2 : (1u << 20);
	while (nc < sm->recLen + n) nc *= 2;
	char *np = realloc(sm->rec, nc);
	if (!np) return 0;
	sm->rec = np; sm->recCap = nc;
	return 1;
}
static void rec_mem(BhSam *sm, const char *s, size_t n) { memcpy(sm->rec + sm->recLen, s, n); sm->recLen += n; }      /* (room was made by the caller) */
#define REC_LIT(sm, lit) rec_mem(sm, lit, sizeof(lit) - 1)
static void rec_u64(BhSam *sm, uint64_t v) { char t[24]; int d = 0; do { t[d++] = (char)('0' + v % 10); v /= 10; } while (v); while (d) sm->rec[sm->recLen++] = t[--d]; }
static void rec_seq(BhSam *sm, const BhQueries *Q, uint64_t entry) {
	const uint8_t *c = Q->codes + Q->qoff[entry]; const uint64_t n = Q->qoff[entry + 1] - Q->qoff[entry];
	if (!n) { sm->rec[sm->recLen++] = '*'; return; }
	for (uint64_t i = 0; i < n; ++i) sm->rec[sm->recLen++] = SAM_LETTERS[c[i] & 15u];
}

/* a traced group of the report (bh_paths_emit): the distinct records idx[0 .. nr) (ascending) with their requests, first columns and ops,
 * the notes of the lines printed from them in file order, and the rendered text of those lines.  Every mode prints, per unique query, the
 * lines of its reads one read after the other, the same number for each: the notes of a unique query are one run, which its reads share
 * in equal parts -- the first line of a part is the read's primary record, the others carry 0x100 */
static int collect(void *ctx, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t nr,
                   const BhPathBuf *bufs, char *const *text, const size_t *text_len, uint64_t n_chunks) {
	BhSam *sm = ctx;
	if (!sm) return BH_OK;
	if (sm->dead) return bh_set_error(sm->dead, "the SAM output was ended by an earlier error");
	const BhQueries *Q = sm->Q;
	if (!Q || !sm->tmp) return die(sm, bh_set_error(BH_E_INTERNAL, "sam: lines before bh_sam_begin"));
	if (!nr) return BH_OK;
	if (nr + 1 > sm->reqCap) {
		uint64_t nc = sm->reqCap ? sm->reqCap : 1024;
		while (nc < nr + 1) nc *= 2;
		uint64_t *o = realloc(sm->mdOff, nc * sizeof(*o)); if (o) sm->mdOff = o;
		uint32_t *m = realloc(sm->nm, nc * sizeof(*m)); if (m) sm->nm = m;
		if (!o || !m) return die(sm, bh_set_error(BH_E_OOM, "OOM:sam"));
		sm->reqCap = nc;
	}
	uint64_t info[8] = {0};
	int rc = BH_OK;
	for (int attempt = 0; attempt < 2; ++attempt) {      /* (the room grows once: the call says how many bytes it has) */
		const uint64_t want = attempt ? sm->mdOff[nr] : 4 * (nr + off[nr]) + 16;
		if (want > sm->mdCap) {
			char *np = realloc(sm->md, want);
			if (!np) return die(sm, bh_set_error(BH_E_OOM, "OOM:sam"));
			sm->md = np; sm->mdCap = want;
		}
		rc = sm->fn ? sm->fn(sm->ctx, req, first, off, ops, nr, sm->md, sm->mdCap, sm->mdOff, sm->nm, info) : md_device(sm->hh, req, first, off, ops, nr, sm->md, sm->mdCap, sm->mdOff, sm->nm, info);
		if (rc != BH_E_CAPACITY) break;
		if (attempt || sm->mdOff[nr] <= sm->mdCap) { rc = bh_set_error(BH_E_INTERNAL, "sam: %lu MD bytes do not fit the room the first call asked for", (unsigned long)sm->mdOff[nr]); break; }
	}
	if (rc) return die(sm, rc);
	for (uint64_t i = 0; i < nr; ++i) if (sm->mdOff[i + 1] < sm->mdOff[i] || sm->mdOff[i + 1] > sm->mdCap) return die(sm, bh_set_error(BH_E_INTERNAL, "sam: the MD strings of a group do not lie in its buffer"));
	sm->mdBytes += sm->mdOff[nr]; sm->us += info[0];
	#define RECORD_OF(ln, lo) do { uint64_t lo_ = 0, hi_ = nr; while (lo_ + 1 < hi_) { const uint64_t mid_ = (lo_ + hi_) / 2; if (idx[mid_] <= (ln)->hit) lo_ = mid_; else hi_ = mid_; } \
		if (idx[lo_] != (ln)->hit) return die(sm, bh_set_error(BH_E_INTERNAL, "sam: a printed line shows record %lu, which was not traced", (unsigned long)(ln)->hit)); \
		if (req[lo_].q >= Q->numEntries) return die(sm, bh_set_error(BH_E_INTERNAL, "sam: a record of query entry %u of %lu", req[lo_].q, (unsigned long)Q->numEntries)); \
		lo = lo_; } while (0)
	for (uint64_t c = 0; c < n_chunks; ++c) {
		const char *s = text[c], *end = s + text_len[c];
		sm->recLen = 0;
		for (uint64_t i = 0, e; i < bufs[c].n; i = e) {
			uint64_t lo;
			RECORD_OF(&bufs[c].l[i], lo);
			const uint32_t uq = Q->six[req[lo].q];
			for (e = i + 1; e < bufs[c].n; ++e) { uint64_t l2; RECORD_OF(&bufs[c].l[e], l2); if (Q->six[req[l2].q] != uq) break; }
			if (uq >= Q->numUniq) return die(sm, bh_set_error(BH_E_INTERNAL, "sam: unique query %u of %lu", uq, (unsigned long)Q->numUniq));
			const uint64_t reads = Q->offset[uq + 1] - Q->offset[uq];
			if (!reads || (e - i) % reads) return die(sm, bh_set_error(BH_E_INTERNAL, "sam: %lu lines for the %lu reads of unique query %u", (unsigned long)(e - i), (unsigned long)reads, uq));
			const uint64_t per = (e - i) / reads;
			for (uint64_t k = i; k < e; ++k) {
				const BhPathLine *ln = &bufs[c].l[k];
				RECORD_OF(ln, lo);
				const char *nlp = s < end ? memchr(s, '\n', (size_t)(end - s)) : NULL;
				if (!nlp) return die(sm, bh_set_error(BH_E_INTERNAL, "sam: %lu line records, fewer lines of text", (unsigned long)bufs[c].n));
				/* columns 9 and 10 of the line */
				const char *p = s; int tabs = 0;
				while (p < nlp && tabs < 8) if (*p++ == '\t') ++tabs;
				char *q9 = NULL;
				const long long st = tabs == 8 ? strtoll(p, &q9, 10) : 0;
				if (tabs != 8 || !q9 || q9 >= nlp || *q9 != '\t') return die(sm, bh_set_error(BH_E_INTERNAL, "sam: a printed line has fewer than 10 columns"));
				const long long ed = strtoll(q9 + 1, NULL, 10);
				if (ln->header >= sm->nH) return die(sm, bh_set_error(BH_E_INTERNAL, "sam: a printed line names header %u of %u", ln->header, sm->nH));
				const size_t ql = name_len(s), snl = strlen(sm->sn[ln->header]);
				const uint64_t n_ops = off[lo + 1] - off[lo], mdl = sm->mdOff[lo + 1] - sm->mdOff[lo], qn = Q->qoff[req[lo].q + 1] - Q->qoff[req[lo].q];
				if (!rec_room(sm, ql + snl + 12 * n_ops + qn + mdl + 128)) return die(sm, bh_set_error(BH_E_OOM, "OOM:sam"));
				rec_mem(sm, s, ql); sm->rec[sm->recLen++] = '\t';
				rec_u64(sm, (st > ed ? 0x10u : 0u) | ((k - i) % per ? 0x100u : 0u)); sm->rec[sm->recLen++] = '\t';
				rec_mem(sm, sm->sn[ln->header], snl); sm->rec[sm->recLen++] = '\t';
				rec_u64(sm, (uint64_t)ln->refOff + first[lo]);
				REC_LIT(sm, "\t255\t");
				const size_t cl = bh_cigar_text(ops + off[lo], n_ops, sm->rec + sm->recLen, 12 * n_ops + 2);
				if (!cl) return die(sm, bh_set_error(BH_E_INTERNAL, "sam: record %lu has a path of %lu ops that does not render", (unsigned long)ln->hit, (unsigned long)n_ops));
				sm->recLen += cl;
				REC_LIT(sm, "\t*\t0\t0\t");
				rec_seq(sm, Q, req[lo].q);
				REC_LIT(sm, "\t*\tNM:i:");
				rec_u64(sm, sm->nm[lo]);
				REC_LIT(sm, "\tMD:Z:");
				rec_mem(sm, sm->md + sm->mdOff[lo], mdl);
				sm->rec[sm->recLen++] = '\n';
				sm->mapped[Q->offset[uq] + (k - i) / per] = 1;
				++sm->nRec;
				s = nlp + 1;
			}
		}
		if (s != end) return die(sm, bh_set_error(BH_E_INTERNAL, "sam: more lines of text than line records"));
		if (sm->recLen && fwrite(sm->rec, 1, sm->recLen, sm->tmp) != sm->recLen) return die(sm, bh_set_error(BH_E_IO, "ERROR: write failed: %s", sm->tmpn));
	}
	#undef RECORD_OF
	return BH_OK;
}
int bh_paths_set_sam(BhPaths *paths, BhSam *sm, int columns) { return bh_paths_add_collector(paths, collect, sm, columns); }

typedef struct { const char *p; uint64_t j; } ReadAt;
static int readat_cmp(const void *a, const void *b) { const char *x = ((const ReadAt *)a)->p, *y = ((const ReadAt *)b)->p; return (x > y) - (x < y); }

/* the reads without a line, in the order of the query file (their names lie in the file's text in that order) */
static int write_unmapped(BhSam *sm) {
	const BhQueries *Q = sm->Q;
	const uint64_t n = Q->totQ;
	ReadAt *at = malloc((n + 1) * sizeof(*at));
	uint64_t *uq_of = malloc((n + 1) * sizeof(*uq_of));
	if (!at || !uq_of) { free(at); free(uq_of); return bh_set_error(BH_E_OOM, "OOM:sam"); }
	for (uint64_t i = 0; i < Q->numUniq; ++i) for (uint64_t j = Q->offset[i]; j < Q->offset[i + 1] && j < n; ++j) uq_of[j] = i;
	for (uint64_t j = 0; j < n; ++j) { at[j].p = Q->heads[j]; at[j].j = j; }
	qsort(at, n, sizeof(*at), readat_cmp);
	int rc = BH_OK;
	for (uint64_t k = 0; k < n && !rc; ++k) {
		const uint64_t j = at[k].j;
		if (sm->mapped[j]) continue;
		const size_t ql = name_len(at[k].p);
		const uint64_t qn = Q->qoff[uq_of[j] + 1] - Q->qoff[uq_of[j]];
		sm->recLen = 0;
		if (!rec_room(sm, ql + qn + 64)) { rc = bh_set_error(BH_E_OOM, "OOM:sam"); break; }
		rec_mem(sm, at[k].p, ql);
		REC_LIT(sm, "\t4\t*\t0\t0\t*\t*\t0\t0\t");
		rec_seq(sm, Q, uq_of[j]);      /* (the forward entry of the read's unique query) */
		REC_LIT(sm, "\t*\n");
		if (fwrite(sm->rec, 1, sm->recLen, sm->tmp) != sm->recLen) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", sm->tmpn);
		++sm->nUnm;
	}
	free(at); free(uq_of);
	return rc;
}

/* the sample has succeeded: the unmapped records, the file under its name */
int bh_sam_end(BhSam *sm) {
	if (!sm) return bh_set_error(BH_E_USAGE, "bh_sam_end: no sam object");
	if (sm->dead) { drop_file(sm); return bh_set_error(sm->dead, "the SAM output was ended by an earlier error: no file is written"); }
	if (!sm->tmp) return bh_set_error(BH_E_USAGE, "bh_sam_end: no sample was begun");
	int rc = sm->unmapped ? write_unmapped(sm) : BH_OK;
	FILE *f = sm->tmp; sm->tmp = NULL;
	if ((ferror(f) | fclose(f)) && !rc) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", sm->tmpn);
	if (!rc && rename(sm->tmpn, sm->finn)) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", sm->tmpn, sm->finn);
	if (!rc) { free(sm->tmpn); sm->tmpn = NULL; }      /* (renamed: nothing to remove) */
	sm->info[0] = sm->nRec; sm->info[1] = sm->nUnm; sm->info[2] = sm->mdBytes; sm->info[3] = sm->us; sm->have_info = !rc;
	drop_file(sm);
	if (rc && rc != BH_E_IO) sm->dead = rc;
	return rc;
}

/* the sample failed alone: no file */
void bh_sam_discard(BhSam *sm) { if (sm) drop_file(sm); }
void bh_sam_abort(BhSam *sm) { if (sm) { drop_file(sm); if (!sm->dead) sm->dead = BH_E_DEVICE; } }

/* one line on standard output: the last sample's figures */
void bh_sam_print_info(BhSam *sm) {
	if (!sm || !sm->have_info || sm->dead) return;
	printf("Sam: %lu records, %lu unmapped records, %lu MD bytes, device %.3f ms\n", (unsigned long)sm->info[0], (unsigned long)sm->info[1], (unsigned long)sm->info[2], sm->info[3] / 1e3);
}
void bh_sam_last_info(const BhSam *sm, uint64_t info[4]) {
	if (!info) return;
	if (sm && sm->have_info) memcpy(info, sm->info, 4 * sizeof(uint64_t)); else memset(info, 0, 4 * sizeof(uint64_t));
}

void bh_sam_close(BhSam *sm) {
	if (!sm) return;
	drop_file(sm);      /* (a sample that was not ended: an abort, an error, or a caller that gave up) */
	if (sm->sn) for (uint32_t h = 0; h < sm->nH; ++h) free(sm->sn[h]);
	free(sm->sn); free(sm->len); free(sm->md); free(sm->mdOff); free(sm->nm); free(sm->rec);
	free(sm);
}
