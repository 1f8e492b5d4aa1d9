/* bh_em.c -- abundance tables: the reads of multi-mapped lines split over their references by expectation-maximisation
 * (burst_hip --abundance, host.Session(abundance=...)).
 *
 * No reference counterpart: the reference's README hands "EM interpolation" of ALLPATHS output to its users and its COMMUNIST mode is a
 * stub.  The definition is bhip_em_run's (include/burst_hip.h); the groups come from the report itself
 * (bh_report_view_sink: one entry per (unique query, placement) with the query's number beside it), the iterations run on the device,
 * and this file holds what is left: the groups of a sample, the columns' names, the table -- and bh_em_host, the definition once more in
 * plain C, which the tests without a device and the yardstick use. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define EM_ONE ((uint64_t)1 << 30)

struct BhEm {
	char *prefix;
	uint32_t nH, nCols, maxIters; uint64_t tol;
	char **head;                         /* [nH] header of every unique-header number (copies) */
	char **names; uint64_t **cols;       /* per sample: column name, counts [nH] or NULL = the sample failed alone */
	int dead;
	bh_em_solver_fn fn; void *ctx;
	uint64_t info[8], reads; int have_info;      /* of the last sample that was solved */
};

/* ---- the definition in plain C ---- */
typedef struct { uint32_t start, size, w; } EmSeg;
static int u64_cmp(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return (x > y) - (x < y); }
static int seg_cmp(const void *a, const void *b, void *refs) {
	const EmSeg *x = a, *y = b; const uint32_t *r = refs;
	if (x->size != y->size) return x->size < y->size ? -1 : 1;
	for (uint32_t i = 0; i < x->size; ++i) if (r[x->start + i] != r[y->start + i]) return r[x->start + i] < r[y->start + i] ? -1 : 1;
	return 0;
}

int bh_em_host(void *unused, uint32_t n_headers, uint32_t n_groups, const uint32_t *group_w, const BhipEmLine *lines, uint64_t n_lines, uint32_t max_iters,
               uint64_t tol, uint64_t *counts, uint64_t info[8]) {
	(void)unused;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!counts || !n_headers) return bh_set_error(BH_E_USAGE, "bh_em_host: no headers or no place for the counts");
	if (!max_iters) return bh_set_error(BH_E_USAGE, "bh_em_host: max_iters must be at least 1");
	if (n_lines >= 0x80000000ull) return bh_set_error(BH_E_USAGE, "bh_em_host: %llu lines (limit 2^31 - 1)", (unsigned long long)n_lines);
	if (n_lines && (!lines || !group_w)) return bh_set_error(BH_E_USAGE, "bh_em_host: lines without a line array or without group weights");
	memset(counts, 0, (size_t)n_headers * 8);
	for (uint64_t i = 0; i < n_lines; ++i) {
		if (lines[i].group >= n_groups) return bh_set_error(BH_E_USAGE, "bh_em_host: line %llu names group %u of %u", (unsigned long long)i, lines[i].group, n_groups);
		if (lines[i].ref >= n_headers) return bh_set_error(BH_E_USAGE, "bh_em_host: line %llu names header %u of %u", (unsigned long long)i, lines[i].ref, n_headers);
	}
	if (!n_lines) return BH_OK;
	uint64_t *key = malloc(n_lines * 8);
	uint32_t *ref = malloc(n_lines * 4);
	EmSeg *seg = malloc(n_lines * sizeof(*seg));
	uint64_t *c = malloc((size_t)n_headers * 8), *nw = malloc((size_t)n_headers * 8), *base = calloc(n_headers, 8);
	int rc = BH_OK;
	if (!key || !ref || !seg || !c || !nw || !base) { rc = bh_set_error(BH_E_OOM, "OOM:abundance"); goto done; }
	/* the distinct (group, header) pairs of the groups that take part, headers ascending inside a group */
	uint64_t nk = 0, np = 0;
	for (uint64_t i = 0; i < n_lines; ++i) if (group_w[lines[i].group]) key[nk++] = (uint64_t)lines[i].group << 32 | lines[i].ref;
	qsort(key, nk, 8, u64_cmp);
	for (uint64_t i = 0; i < nk; ++i) if (!i || key[i] != key[i - 1]) key[np++] = key[i];
	info[1] = np;
	if (!np) goto done;
	/* one candidate set per group; equal sets merged into classes of summed weight */
	uint64_t ns = 0, total = 0;
	for (uint64_t i = 0; i < np; ++i) {
		ref[i] = (uint32_t)key[i];
		if (!i || (key[i] >> 32) != (key[i - 1] >> 32)) { seg[ns].start = (uint32_t)i; seg[ns].size = 0; seg[ns].w = group_w[key[i] >> 32]; total += seg[ns].w; ++ns; }
		++seg[ns - 1].size;
	}
	if (total > 0x7FFFFFFFull) { rc = bh_set_error(BH_E_USAGE, "bh_em_host: the participating groups hold %llu reads (limit 2^31 - 1)", (unsigned long long)total); goto done; }
	qsort_r(seg, ns, sizeof(*seg), seg_cmp, ref);
	uint64_t nc = 0;
	for (uint64_t s = 0; s < ns; ++s) {
		if (nc && !seg_cmp(&seg[nc - 1], &seg[s], ref)) seg[nc - 1].w += seg[s].w;
		else seg[nc++] = seg[s];
	}
	info[2] = nc;
	/* a class of one candidate gives the same W x ONE in every iteration */
	uint64_t nm = 0;
	for (uint64_t k = 0; k < nc; ++k) {
		if (seg[k].size == 1) base[ref[seg[k].start]] += (uint64_t)seg[k].w * EM_ONE;
		else seg[nm++] = seg[k];
	}
	for (uint32_t h = 0; h < n_headers; ++h) c[h] = EM_ONE;
	uint64_t t = 0, delta = 0; int conv = 0;
	while (t < max_iters && !conv) {
		memcpy(nw, base, (size_t)n_headers * 8);
		for (uint64_t k = 0; k < nm; ++k) {
			const uint32_t *r = ref + seg[k].start;
			uint64_t d = 0, sq = 0, tc = 0; uint32_t th = 0;
			for (uint32_t i = 0; i < seg[k].size; ++i) { d += c[r[i]]; if (!i || c[r[i]] > tc) { tc = c[r[i]]; th = r[i]; } }      /* (ascending headers: the first of equals is the lowest) */
			for (uint32_t i = 0; i < seg[k].size; ++i) {
				const uint64_t q = (uint64_t)(((double)c[r[i]] / (double)d) * 1073741824.0);
				sq += q;
				nw[r[i]] += seg[k].w * q;
			}
			nw[th] += seg[k].w * (EM_ONE - sq);
		}
		delta = 0;
		for (uint32_t h = 0; h < n_headers; ++h) { const uint64_t dl = nw[h] > c[h] ? nw[h] - c[h] : c[h] - nw[h]; if (dl > delta) delta = dl; }
		uint64_t *sw = c; c = nw; nw = sw;
		++t;
		conv = delta <= tol;
	}
	memcpy(counts, c, (size_t)n_headers * 8);
	info[0] = t; info[3] = delta; info[4] = (uint64_t)conv;
done:
	free(key); free(ref); free(seg); free(c); free(nw); free(base);
	if (rc) memset(info, 0, 8 * sizeof(uint64_t));
	return rc;
}

/* the device: ctx = the handle */
static int solve_device(void *ctx, uint32_t n_headers, uint32_t n_groups, const uint32_t *group_w, const BhipEmLine *lines, uint64_t n_lines, uint32_t max_iters,
                        uint64_t tol, uint64_t *counts, uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "abundance: the iterations run on the device and rank 0 has no device handle");
	const int rc = bhip_em_run(ctx, n_headers, n_groups, group_w, lines, n_lines, max_iters, tol, counts, info);
	if (rc) return bh_set_error(rc == BHIP_E_ARG ? BH_E_USAGE : BH_E_DEVICE, "abundance: %s", bhip_last_error());
	return BH_OK;
}

static char *sample_name(const char *path) {      /* base name without its last extension (as the coverage names its columns) */
	const char *b = strrchr(path, '/');
	b = b ? b + 1 : path;
	char *s = strdup(b);
	if (!s) return NULL;
	char *dot = strrchr(s, '.');
	if (dot && dot != s) *dot = 0;
	return s;
}

int bh_em_open_heads(const char *prefix, uint32_t n_headers, const char *const *heads, uint32_t max_iters, uint64_t tol, BhEm **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_em_open: no place for the object");
	*out = NULL;
	if (!prefix || !n_headers || !heads) return bh_set_error(BH_E_USAGE, "bh_em_open: no headers / no prefix");
	if (!max_iters) return bh_set_error(BH_E_USAGE, "ERROR: --abundance-iters must be at least 1");
	BhEm *em = calloc(1, sizeof(*em));
	if (!em) return bh_set_error(BH_E_OOM, "OOM:abundance");
	em->nH = n_headers; em->maxIters = max_iters; em->tol = tol;
	em->prefix = strdup(prefix);
	em->head = calloc(n_headers, sizeof(*em->head));
	int ok = em->prefix && em->head;
	for (uint32_t h = 0; ok && h < n_headers; ++h) ok = (em->head[h] = strdup(heads[h] ? heads[h] : "")) != NULL;
	if (!ok) { bh_em_close(em); return bh_set_error(BH_E_OOM, "OOM:abundance"); }
	*out = em;
	return BH_OK;
}

int bh_em_open(const BhDb *db, const char *prefix, uint32_t max_iters, uint64_t tol, BhEm **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_em_open: no place for the object");
	*out = NULL;
	if (!db || !prefix || !db->numRefHeads || !db->refMap || !db->refHead) return bh_set_error(BH_E_USAGE, "bh_em_open: no database / no prefix");
	const char **head = calloc(db->numRefHeads, sizeof(*head));
	if (!head) return bh_set_error(BH_E_OOM, "OOM:abundance");
	for (uint32_t i = 0; i < db->origTotR; ++i) if (db->refMap[i] < db->numRefHeads) head[db->refMap[i]] = db->refHead[i];      /* (the numbers the report's sink uses) */
	const int rc = bh_em_open_heads(prefix, db->numRefHeads, head, max_iters, tol, out);
	free(head);
	return rc;
}

void bh_em_set_solver(BhEm *em, bh_em_solver_fn fn, void *ctx) { if (em) { em->fn = fn; em->ctx = ctx; } }
void bh_em_abort(BhEm *em) { if (em && !em->dead) em->dead = BH_E_DEVICE; }
void bh_em_dims(const BhEm *em, uint32_t *n_columns, uint32_t *n_headers) {
	if (n_columns) *n_columns = em ? em->nCols + 1 : 0;
	if (n_headers) *n_headers = em ? em->nH : 0;
}

static int new_column(BhEm *em, const char *out_path) {
	char **nn = realloc(em->names, ((size_t)em->nCols + 1) * sizeof(*nn));
	if (nn) em->names = nn;
	uint64_t **nc = realloc(em->cols, ((size_t)em->nCols + 1) * sizeof(*nc));
	if (nc) em->cols = nc;
	char *nm = sample_name(out_path ? out_path : "sample");
	if (!nn || !nc || !nm) { free(nm); return bh_set_error(BH_E_OOM, "OOM:abundance"); }
	em->names[em->nCols] = nm; em->cols[em->nCols] = NULL;
	++em->nCols;
	return BH_OK;
}

int bh_em_sample_failed(BhEm *em, const char *out_path) {
	if (!em) return BH_OK;
	const int rc = new_column(em, out_path);
	if (!rc) printf(" --> abundance: sample '%s' failed alone: its column is all zero\n", em->names[em->nCols - 1]);
	return rc;
}

int bh_em_sample(BhEm *em, void *hh, const char *out_path, const uint32_t *reads, const BhipCovLine *lines, uint64_t n) {
	if (!em) return bh_set_error(BH_E_USAGE, "bh_em_sample: no abundance object");
	if (em->dead) return bh_set_error(em->dead, "abundance was ended by an earlier error");
	if (n && (!reads || !lines)) return bh_set_error(BH_E_USAGE, "bh_em_sample: placements without their query numbers");
	int rc = new_column(em, out_path);
	if (rc) return rc;
	/* group = the unique query's number, W = the reads of the unique query (the same on all its entries), ref = the entry's header */
	uint32_t nG = 0;
	for (uint64_t i = 0; i < n; ++i) if (reads[i] >= nG) nG = reads[i] + 1;
	uint32_t *gw = calloc((size_t)nG + 1, 4);
	BhipEmLine *ln = malloc((n + 1) * sizeof(*ln));
	uint64_t *col = calloc(em->nH, 8);
	if (!gw || !ln || !col) { free(gw); free(ln); free(col); em->dead = BH_E_OOM; return bh_set_error(BH_E_OOM, "OOM:abundance"); }
	uint64_t nreads = 0;
	for (uint64_t i = 0; i < n; ++i) {
		const uint32_t w = lines[i].w & 0x7FFFFFFFu;
		if (!gw[reads[i]]) nreads += w;
		gw[reads[i]] = w;
		ln[i].group = reads[i]; ln[i].ref = lines[i].ref;
	}
	uint64_t info[8] = {0};
	rc = em->fn ? em->fn(em->ctx, em->nH, nG, gw, ln, n, em->maxIters, em->tol, col, info) : solve_device(hh, em->nH, nG, gw, ln, n, em->maxIters, em->tol, col, info);
	free(gw); free(ln);
	if (rc) { free(col); em->dead = rc; return rc; }      /* (any error of the solver is final: nothing will be written) */
	em->cols[em->nCols - 1] = col;
	memcpy(em->info, info, sizeof info); em->reads = nreads; em->have_info = 1;
	return BH_OK;
}

int bh_em_stats(BhEm *em, uint64_t *cols) {
	if (!em || !cols) return bh_set_error(BH_E_USAGE, "bh_em_stats: no abundance object");
	if (em->dead) return bh_set_error(em->dead, "abundance was ended by an earlier error");
	memset(cols, 0, (size_t)em->nH * 8 * ((size_t)em->nCols + 1));
	for (uint32_t c = 0; c < em->nCols; ++c) if (em->cols[c]) {
		memcpy(cols + (size_t)em->nH * (c + 1), em->cols[c], (size_t)em->nH * 8);
		for (uint32_t h = 0; h < em->nH; ++h) cols[h] += em->cols[c][h];      /* Dataset: the integer sum of the sample columns */
	}
	return BH_OK;
}

typedef struct { const char *s; uint32_t h; } Row;
static int row_cmp(const void *a, const void *b) { return strcmp(((const Row *)a)->s, ((const Row *)b)->s); }

int bh_em_write(BhEm *em) {
	if (!em) return bh_set_error(BH_E_USAGE, "bh_em_write: no abundance object");
	if (em->dead) return bh_set_error(em->dead, "abundance was ended by an earlier error: no table is written");
	uint64_t *cols = malloc((size_t)em->nH * 8 * ((size_t)em->nCols + 1) + 8);
	Row *rows = malloc(((size_t)em->nH + 1) * sizeof(*rows));
	char *tmpn = NULL, *finn = NULL;
	int rc = cols && rows ? BH_OK : bh_set_error(BH_E_OOM, "OOM:abundance");
	if (!rc) rc = bh_em_stats(em, cols);
	if (!rc && (asprintf(&finn, "%sabundance.txt", em->prefix) < 0 || asprintf(&tmpn, "%sabundance.txt.tmp%ld", em->prefix, (long)getpid()) < 0)) rc = bh_set_error(BH_E_OOM, "OOM:abundance");
	if (!rc) {
		uint32_t nR = 0;
		for (uint32_t h = 0; h < em->nH; ++h) if (cols[h]) { rows[nR].s = em->head[h]; rows[nR].h = h; ++nR; }
		qsort(rows, nR, sizeof(*rows), row_cmp);
		FILE *f = fopen(tmpn, "wb");
		if (!f) rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", tmpn);
		else {
			setvbuf(f, NULL, _IOFBF, 1 << 20);
			fputs("#OTU ID\tDataset", f);
			for (uint32_t c = 0; c < em->nCols; ++c) fprintf(f, "\t%s", em->names[c]);
			fputc('\n', f);
			for (uint32_t r = 0; r < nR; ++r) {
				fputs(rows[r].s, f);
				for (uint32_t c = 0; c <= em->nCols; ++c) fprintf(f, "\t%.4f", (double)cols[(size_t)em->nH * c + rows[r].h] / 1073741824.0);
				fputc('\n', f);
			}
			if (ferror(f) | fclose(f)) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", tmpn);
			else if (rename(tmpn, finn)) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", tmpn, finn);
			if (rc) (void)unlink(tmpn);
		}
	}
	free(cols); free(rows); free(tmpn); free(finn);
	return rc;
}

/* one line on standard output: the last sample's figures (bhip_em_run's info) */
void bh_em_print_info(BhEm *em) {
	if (!em || !em->have_info || em->dead) return;
	printf("Abundance: %lu reads, %lu pairs, %lu classes, %lu iterations, %s (last delta %lu), device %.3f ms\n", (unsigned long)em->reads, (unsigned long)em->info[1],
	       (unsigned long)em->info[2], (unsigned long)em->info[0], em->info[4] ? "converged" : "not converged", (unsigned long)em->info[3], em->info[5] / 1e3);
}

void bh_em_last_info(const BhEm *em, uint64_t info[8], uint64_t *reads) {
	if (info) { if (em && em->have_info) memcpy(info, em->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t)); }
	if (reads) *reads = em && em->have_info ? em->reads : 0;
}

const uint64_t *bh_em_last_column(const BhEm *em) { return em && em->nCols && !em->dead ? em->cols[em->nCols - 1] : NULL; }

void bh_em_close(BhEm *em) {
	if (!em) return;
	for (uint32_t c = 0; c < em->nCols; ++c) { free(em->names[c]); free(em->cols[c]); }
	if (em->head) for (uint32_t h = 0; h < em->nH; ++h) free(em->head[h]);
	free(em->names); free(em->cols); free(em->prefix); free(em->head);
	free(em);
}
