/* bh_cov.c -- coverage and count tables per reference header and sample (burst_hip --coverage, host.Session(coverage=...)).
 *
 * The reference leaves this to helpers that run over the concatenated .b6 text: embalmlets/bcov.c (coverage, two 32-bit counters per
 * position of every reference and once more per sample) and embalmulate.c (the reference x sample count table).  Here the placements
 * come from the report itself (bh_report_view_sink), the statistics from the device (bhip_cov_*: sorted events, no per-position
 * arrays), and this file holds what is left: the lengths, the columns' names, the tables.
 *
 * Two deliberate departures from bcov.c:
 *   - a reverse-strand line (column 9 > column 10) covers [min - 1, max - 1) like a forward one; bcov's loop `for (s = rs; s < re; ...)`
 *     counts nothing for it (bcov.c:169-175);
 *   - a placement is unique when its read is on exactly one line of the sample's .b6; bcov compares the query names of neighbouring
 *     lines over the length of the first (bcov.c:162-168, 175, 192), which reads `q10` followed by `q100` as one query.
 * The sign convention of shared.txt / unique.txt is bcov's with its variance factor at 1 (bcov.c:217-222): the mean depth, negated
 * unless it exceeds the standard deviation of the depth. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

struct BhCov {
	const BhDb *db;
	char *prefix;
	uint32_t nH, pad, nCols;             /* nCols counts the samples (Dataset not included) */
	const char **head;                   /* [nH] header of every unique-header number */
	uint32_t *len; int have_len;
	char **names; uint8_t *added;        /* per sample: column name, 1 = its placements are on the device */
	void *hh; int begun, dead;
	bh_cov_tap_fn tap; void *tap_ctx;
};

static char *sample_name(const char *path) {      /* base name without its last extension */
	const char *b = strrchr(path, '/');
	b = b ? b + 1 : path;
	char *s = strdup(b);
	if (!s) return NULL;
	char *dot = strrchr(s, '.');
	if (dot && dot != s) *dot = 0;
	return s;
}

void bh_cov_extents_host(const BhDb *db, uint32_t *ext) {
	uint64_t w0 = 0;
	for (uint32_t c = 0; c < db->numRclumps; ++c) {
		const uint32_t L = db->clumpLen[c], rows = L / 2u + (L & 1);
		const uint8_t *p = db->packed + w0 * 16;
		for (uint32_t z = 0; z < 16; ++z) {
			uint32_t e = 0;
			for (uint32_t r = rows; r-- > 0;) {
				const uint8_t b = p[(uint64_t)r * 16 + z];
				if (b) { e = 2 * r + (b >> 4 ? 2 : 1); break; }
			}
			ext[16u * c + z] = e;
		}
		w0 += rows;
	}
}

int bh_cov_lengths_from_extents(const BhDb *db, const uint32_t *ext, uint32_t *len) {
	if (!db || !ext || !len) return bh_set_error(BH_E_USAGE, "bh_cov_lengths_from_extents: null argument");
	memset(len, 0, (size_t)db->numRefHeads * 4);
	for (uint32_t lane = 0; lane < db->totR; ++lane) {
		const uint32_t k0 = db->refDedupIx ? db->refDedupIx[lane] : lane, k1 = db->refDedupIx ? db->refDedupIx[lane + 1] : lane + 1;
		for (uint32_t k = k0; k < k1; ++k) {      /* the fragments this lane stands for (exact duplicates share it) */
			const uint32_t rix = db->tmpRIX[k], h = db->refMap ? db->refMap[rix] : rix;
			const uint64_t end = (uint64_t)(db->refStart ? db->refStart[rix] : 0) + ext[lane];
			if (h >= db->numRefHeads) return bh_set_error(BH_E_INTERNAL, "fragment %u maps to header %u of %u", rix, h, db->numRefHeads);
			if (end > len[h]) len[h] = end > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)end;
		}
	}
	return BH_OK;
}

typedef struct { const char *s; size_t n; uint32_t len; } LenRec;
static int lenrec_cmp(const void *a, const void *b) {
	const LenRec *x = a, *y = b;
	const int c = memcmp(x->s, y->s, x->n < y->n ? x->n : y->n);
	return c ? c : (x->n > y->n) - (x->n < y->n);
}
/* the table `name<TAB>length` of `file` looked up for every header: len[h] of heads[h]; `flag` names the option in the texts (--sam-lengths
 * reads the same table through here) */
int bh_cov_read_lengths(const char *file, const char *flag, uint32_t n_headers, const char *const *heads, uint32_t *len) {
	FILE *f = fopen(file, "rb");
	if (!f) return bh_set_error(BH_E_IO, "ERROR: Cannot open the lengths table: %s", file);
	fseek(f, 0, SEEK_END);
	const long sz = ftell(f);
	fseek(f, 0, SEEK_SET);
	char *txt = malloc((size_t)sz + 2);
	if (!txt) { fclose(f); return bh_set_error(BH_E_OOM, "OOM:coverage"); }
	if (fread(txt, 1, (size_t)sz, f) != (size_t)sz) { fclose(f); free(txt); return bh_set_error(BH_E_IO, "ERROR: Cannot read the lengths table: %s", file); }
	fclose(f);
	txt[sz] = 0;
	uint64_t n = 0, cap = 1024, line = 0;
	LenRec *R = malloc(cap * sizeof(*R));
	int rc = R ? BH_OK : bh_set_error(BH_E_OOM, "OOM:coverage");
	for (char *p = txt; !rc && p < txt + sz;) {
		char *e = strchr(p, '\n');
		if (!e) e = txt + sz;
		++line;
		if (e > p && !(e == p + 1 && *p == '\r')) {
			char *tab = memchr(p, '\t', (size_t)(e - p));
			if (!tab || tab == p) rc = bh_set_error(BH_E_USAGE, "ERROR: %s line %lu: expected 'name<TAB>length'", file, (unsigned long)line);
			else {
				if (n == cap) { LenRec *nr = realloc(R, (cap *= 2) * sizeof(*R)); if (!nr) { rc = bh_set_error(BH_E_OOM, "OOM:coverage"); break; } R = nr; }
				const unsigned long long v = strtoull(tab + 1, NULL, 10);
				R[n].s = p; R[n].n = (size_t)(tab - p); R[n].len = v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; ++n;
			}
		}
		p = e + 1;
	}
	if (!rc) {
		qsort(R, n, sizeof(*R), lenrec_cmp);
		for (uint32_t h = 0; h < n_headers && !rc; ++h) {
			const LenRec k = {heads[h], strlen(heads[h]), 0};
			const LenRec *m = n ? bsearch(&k, R, n, sizeof(*R), lenrec_cmp) : NULL;
			if (!m) rc = bh_set_error(BH_E_USAGE, "ERROR: %s %s has no length for reference '%s'", flag, file, heads[h]);
			else len[h] = m->len;
		}
	}
	free(R); free(txt);
	return rc;
}

/* the database's own extent of every header: from the lanes resident behind `hip_handle`, or (NULL) from the packed references in host memory */
int bh_cov_default_lengths(const BhDb *db, void *hip_handle, uint32_t *len) {
	uint32_t *ext = calloc((size_t)db->numRclumps * 16 + 1, 4);
	if (!ext) return bh_set_error(BH_E_OOM, "OOM:coverage");
	int rc = BH_OK;
	if (!hip_handle) bh_cov_extents_host(db, ext);
	else if (bhip_lane_extents(hip_handle, ext)) rc = bh_set_error(BH_E_DEVICE, "coverage: lane extents: %s", bhip_last_error());
	if (!rc) rc = bh_cov_lengths_from_extents(db, ext, len);
	free(ext);
	return rc;
}

int bh_cov_open(const BhDb *db, const char *prefix, const char *lengths_file, uint32_t pad, BhCov **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_cov_open: no place for the object");
	*out = NULL;
	if (!db || !prefix || !db->numRefHeads || !db->refMap || !db->refHead) return bh_set_error(BH_E_USAGE, "bh_cov_open: no database / no prefix");
	BhCov *cv = calloc(1, sizeof(*cv));
	if (!cv) return bh_set_error(BH_E_OOM, "OOM:coverage");
	cv->db = db; cv->nH = db->numRefHeads; cv->pad = pad;
	cv->prefix = strdup(prefix);
	cv->head = calloc(cv->nH, sizeof(*cv->head));
	cv->len = calloc(cv->nH, 4);
	if (!cv->prefix || !cv->head || !cv->len) { bh_cov_close(cv); return bh_set_error(BH_E_OOM, "OOM:coverage"); }
	for (uint32_t i = 0; i < db->origTotR; ++i) if (db->refMap[i] < cv->nH) cv->head[db->refMap[i]] = db->refHead[i];
	for (uint32_t h = 0; h < cv->nH; ++h) if (!cv->head[h]) cv->head[h] = "";
	if (lengths_file) {
		const int rc = bh_cov_read_lengths(lengths_file, "--coverage-lengths", cv->nH, cv->head, cv->len);
		if (rc) { bh_cov_close(cv); return rc; }
		cv->have_len = 1;
	}
	*out = cv;
	return BH_OK;
}

void bh_cov_set_tap(BhCov *cv, bh_cov_tap_fn fn, void *ctx) { if (cv) { cv->tap = fn; cv->tap_ctx = ctx; } }
void bh_cov_abort(BhCov *cv) { if (cv && !cv->dead) cv->dead = BH_E_DEVICE; }
void bh_cov_dims(const BhCov *cv, uint32_t *n_columns, uint32_t *n_headers) {
	if (n_columns) *n_columns = cv ? cv->nCols + 1 : 0;
	if (n_headers) *n_headers = cv ? cv->nH : 0;
}
const uint32_t *bh_cov_lengths(const BhCov *cv) { return cv && cv->have_len ? cv->len : NULL; }

/* the default lengths without a device: for runs in which no one handle holds the whole database (--shard db) */
int bh_cov_lengths_host(BhCov *cv) {
	if (!cv || cv->have_len) return BH_OK;
	const int rc = bh_cov_default_lengths(cv->db, NULL, cv->len);
	if (!rc) cv->have_len = 1;
	return rc;
}

static int new_column(BhCov *cv, const char *out_path) {
	char **nn = realloc(cv->names, ((size_t)cv->nCols + 1) * sizeof(*nn));
	if (nn) cv->names = nn;
	uint8_t *na = realloc(cv->added, (size_t)cv->nCols + 1);
	if (na) cv->added = na;
	char *nm = sample_name(out_path ? out_path : "sample");
	if (!nn || !na || !nm) { free(nm); return bh_set_error(BH_E_OOM, "OOM:coverage"); }
	cv->names[cv->nCols] = nm; cv->added[cv->nCols] = 0;
	++cv->nCols;
	return BH_OK;
}
static int dev_fail(BhCov *cv, const char *what) {
	cv->dead = BH_E_DEVICE;
	return bh_set_error(BH_E_DEVICE, "coverage: %s: %s", what, bhip_last_error());
}

int bh_cov_sample_failed(BhCov *cv, const char *out_path) {
	if (!cv) return BH_OK;
	const int rc = new_column(cv, out_path);
	if (!rc) printf(" --> coverage: sample '%s' failed alone: its column is all zero\n", cv->names[cv->nCols - 1]);
	return rc;
}

int bh_cov_sample(BhCov *cv, void *hh, const char *out_path, const BhipCovLine *lines, uint64_t n) {
	if (!cv) return bh_set_error(BH_E_USAGE, "bh_cov_sample: no coverage object");
	if (cv->dead) return bh_set_error(cv->dead, "coverage was ended by an earlier error");
	int rc = new_column(cv, out_path);
	if (rc) return rc;
	const uint32_t col = cv->nCols - 1;
	if (cv->tap && cv->tap(cv->tap_ctx, col, lines, n) == 1) return BH_OK;
	if (!hh) { cv->dead = BH_E_DEVICE; return bh_set_error(BH_E_DEVICE, "coverage: the statistics are computed on the device and rank 0 has no device handle"); }
	if (!cv->begun) {
		if (!cv->have_len) {      /* the database's own extents */
			rc = bh_cov_default_lengths(cv->db, hh, cv->len);
			if (rc == BH_E_DEVICE) cv->dead = BH_E_DEVICE;
			if (rc) return rc;
			cv->have_len = 1;
		}
		if (bhip_cov_begin(hh, cv->nH, cv->len, cv->pad)) return dev_fail(cv, "begin");
		cv->hh = hh; cv->begun = 1;
	}
	if (hh != cv->hh) return bh_set_error(BH_E_USAGE, "bh_cov_sample: a coverage stays on one device handle");
	if (bhip_cov_add(hh, col, lines, n)) return dev_fail(cv, "add");
	cv->added[col] = 1;
	return BH_OK;
}

int bh_cov_stats(BhCov *cv, uint64_t *shared, uint64_t *unique) {
	if (!cv) return bh_set_error(BH_E_USAGE, "bh_cov_stats: no coverage object");
	if (cv->dead) return bh_set_error(cv->dead, "coverage was ended by an earlier error");
	const size_t per = (size_t)cv->nH * 4;
	if (shared) memset(shared, 0, per * 8 * ((size_t)cv->nCols + 1));
	if (unique) memset(unique, 0, per * 8 * ((size_t)cv->nCols + 1));
	if (!cv->begun) return BH_OK;      /* (no sample reached the device: everything is zero) */
	if (bhip_cov_dataset_stats(cv->hh, shared, unique)) return dev_fail(cv, "Dataset statistics");
	for (uint32_t c = 0; c < cv->nCols; ++c)
		if (cv->added[c] && bhip_cov_sample_stats(cv->hh, c, shared ? shared + per * (c + 1) : NULL, unique ? unique + per * (c + 1) : NULL)) return dev_fail(cv, "sample statistics");
	return BH_OK;
}

typedef struct { const char *s; uint32_t h; } Row;
static int row_cmp(const void *a, const void *b) { return strcmp(((const Row *)a)->s, ((const Row *)b)->s); }

/* mean depth, negated unless it exceeds the standard deviation of the depth (bcov.c:217-222 with vf = 1), from the exact integers */
static double signed_mean(uint64_t tot, uint64_t sq, uint32_t L) {
	const double mean = (double)tot / L;
	if (L == 1 || !tot) return mean;      /* (no depth at all prints 0.0000, not the -0.0000 the negation would give) */
	const double ssd = (double)sq - (double)tot * (double)tot / L;
	return mean > sqrt(ssd / (L - 1)) ? mean : -mean;
}

int bh_cov_write_tables(const char *prefix, uint32_t nH, const char *const *head, const uint32_t *len, uint32_t nCols, const char *const *col_names,
                        const uint64_t *sh, const uint64_t *un) {
	static const char *const kind[5] = {"shared.txt", "unique.txt", "shared_binary.txt", "unique_binary.txt", "counts.txt"};
	if (!prefix || !head || !len || !nCols || !sh || !un) return bh_set_error(BH_E_USAGE, "bh_cov_write_tables: null argument");
	const size_t per = (size_t)nH * 4;
	Row *rows = malloc(((size_t)nH + 1) * sizeof(*rows));
	if (!rows) return bh_set_error(BH_E_OOM, "OOM:coverage");
	uint32_t nR = 0;
	for (uint32_t h = 0; h < nH; ++h) if (sh[4 * (size_t)h] > 0 && len[h]) { rows[nR].s = head[h]; rows[nR].h = h; ++nR; }      /* bcov's skip rule: Dataset shared depth 0 */
	qsort(rows, nR, sizeof(*rows), row_cmp);
	char *tmpn[5] = {0}, *finn[5] = {0}; FILE *f[5] = {0};
	int rc = BH_OK;
	for (int k = 0; k < 5 && !rc; ++k) {
		if (asprintf(&finn[k], "%s%s", prefix, kind[k]) < 0) { finn[k] = NULL; rc = bh_set_error(BH_E_OOM, "OOM:coverage"); break; }
		if (asprintf(&tmpn[k], "%s%s.tmp%ld", prefix, kind[k], (long)getpid()) < 0) { tmpn[k] = NULL; rc = bh_set_error(BH_E_OOM, "OOM:coverage"); break; }
		if (!(f[k] = fopen(tmpn[k], "wb"))) rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", tmpn[k]);
	}
	for (int k = 0; k < 5 && !rc; ++k) {
		setvbuf(f[k], NULL, _IOFBF, 1 << 20);
		fputs(k == 4 ? "#OTU ID\tDataset" : "#Coverage\tDataset", f[k]);
		for (uint32_t c = 1; c < nCols; ++c) fprintf(f[k], "\t%s", col_names && col_names[c] ? col_names[c] : "");
		fputc('\n', f[k]);
		for (uint32_t r = 0; r < nR; ++r) {
			const uint32_t h = rows[r].h, L = len[h];
			fputs(rows[r].s, f[k]);
			for (uint32_t c = 0; c < nCols; ++c) {
				const uint64_t *a = sh + per * c + 4 * (size_t)h, *b = un + per * c + 4 * (size_t)h;
				if (k == 0) fprintf(f[k], "\t%.4f", signed_mean(a[0], a[2], L));
				else if (k == 1) fprintf(f[k], "\t%.4f", signed_mean(b[0], b[2], L));
				else if (k == 2) fprintf(f[k], "\t%.4f", (double)a[1] / L);
				else if (k == 3) fprintf(f[k], "\t%.4f", (double)b[1] / L);
				else fprintf(f[k], "\t%llu", (unsigned long long)a[3]);
			}
			fputc('\n', f[k]);
		}
	}
	for (int k = 0; k < 5; ++k) if (f[k] && (ferror(f[k]) | fclose(f[k])) && !rc) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", tmpn[k]);
	for (int k = 0; k < 5 && !rc; ++k) if (rename(tmpn[k], finn[k])) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", tmpn[k], finn[k]);
	if (rc) for (int k = 0; k < 5; ++k) { if (tmpn[k]) (void)unlink(tmpn[k]); if (finn[k]) (void)unlink(finn[k]); }      /* all five or none */
	for (int k = 0; k < 5; ++k) { free(tmpn[k]); free(finn[k]); }
	free(rows);
	return rc;
}

int bh_cov_write(BhCov *cv) {
	if (!cv) return bh_set_error(BH_E_USAGE, "bh_cov_write: no coverage object");
	if (cv->dead) return bh_set_error(cv->dead, "coverage was ended by an earlier error: no tables are written");
	const size_t cells = (size_t)cv->nH * 4 * ((size_t)cv->nCols + 1);
	uint64_t *sh = malloc(cells * 8 + 8), *un = malloc(cells * 8 + 8);
	const char **names = calloc((size_t)cv->nCols + 2, sizeof(*names));
	int rc = sh && un && names ? BH_OK : bh_set_error(BH_E_OOM, "OOM:coverage");
	if (!rc) rc = bh_cov_stats(cv, sh, un);
	if (!rc) {
		for (uint32_t c = 0; c < cv->nCols; ++c) names[c + 1] = cv->names[c];
		rc = bh_cov_write_tables(cv->prefix, cv->nH, cv->head, cv->len, cv->nCols + 1, names, sh, un);
	}
	free(sh); free(un); free(names);
	return rc;
}

/* one line on standard output: what the coverage cost on the device (bhip_cov_info) */
void bh_cov_print_info(BhCov *cv) {
	uint64_t info[8];
	if (!cv || !cv->begun || cv->dead || bhip_cov_info(cv->hh, info)) return;
	printf("Coverage: %lu sample(s) on the device, sorts + scans + statistics kernels %.3f ms in all (%.3f ms per sample), event buffer peak %.2f MB of a cap of %.1f MB, %lu compaction(s)\n",
	       (unsigned long)info[7], info[6] / 1e3, info[7] ? info[6] / 1e3 / (double)info[7] : 0.0, info[1] / 1e6, info[3] / 1e6, (unsigned long)info[2]);
}

void bh_cov_close(BhCov *cv) {
	if (!cv) return;
	if (cv->begun && cv->hh) (void)bhip_cov_end(cv->hh);
	for (uint32_t c = 0; c < cv->nCols; ++c) free(cv->names[c]);
	free(cv->names); free(cv->added); free(cv->prefix); free(cv->head); free(cv->len);
	free(cv);
}
