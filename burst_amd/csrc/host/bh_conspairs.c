/* bh_conspairs.c -- sample-to-sample identity of the consensus rows of every reference (burst_hip --consensus PREFIX --consensus-pairs,
 * host.Session(consensus=..., consensus_pairs=True)).
 *
 * No reference counterpart.  The definition is bhip_consensus_pairs' (include/burst_hip.h "Consensus pairs"): a pure
 * function of the written PREFIXconsensus.fa.  bh_consensus_sample hands over the segments and letters of every (sample, header) whose
 * record it writes, instead of freeing them; this file keeps them in host memory (24 bytes per segment and a byte per covered position;
 * spilling is out of scope), makes ONE solver call on the reporting rank's handle when the run ends, and writes the three files under
 * temporary names, which bh_consensus_write renames together with the two consensus files.  bh_consensus_pairs_host is the definition once
 * more in plain sequential C (a dense row per (sample, header) over the header's covered extent and a double loop over the samples), which
 * the tests without a device and the yardstick use. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

struct BhConsPairs {
	char *tmp[3], *fin[3];
	uint32_t minCompared;
	int dead, written, renamed;
	bh_conspairs_solver_fn fn; void *ctx;
	BhipPairSeg *segs; uint64_t nSegs, capSegs;
	char *letters; uint64_t nLetters, capLetters;
	uint64_t *diag; uint32_t capDiag;      /* per sample: the comparable positions of its records */
	uint64_t nRecords;
	uint64_t info[8], devInfo[8]; int have_info;
};

static const char *const kSuffix[3] = {"consensus_pairs.txt", "consensus_identity.txt", "consensus_compared.txt"};

static int comparable(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == '-'; }

/* ---- the definition in plain C ---- */
typedef struct { uint64_t key; uint64_t seg0; uint32_t n_seg; } HostRow;      /* key = header << 16 | sample */
static int row_cmp(const void *a, const void *b) { const uint64_t x = ((const HostRow *)a)->key, y = ((const HostRow *)b)->key; return (x > y) - (x < y); }

int bh_consensus_pairs_host(void *unused, uint32_t n_samples, const BhipPairSeg *segs, uint64_t n_segs, const char *letters, uint64_t n_letters, uint32_t min_compared,
                            BhipPair *pairs, uint64_t pair_cap, uint64_t *n_pairs, uint64_t info[8]) {
	(void)unused;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!n_pairs || (n_segs && (!segs || !letters)) || (pair_cap && !pairs)) return bh_set_error(BH_E_USAGE, "bh_consensus_pairs_host: null argument");
	*n_pairs = 0;
	if (n_samples > 65535u) return bh_set_error(BH_E_USAGE, "bh_consensus_pairs_host: %u samples (at most 65535)", n_samples);
	if (!min_compared || min_compared > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "bh_consensus_pairs_host: min_compared %u (1 .. 2^31 - 1)", min_compared);
	if (n_segs >> 32) return bh_set_error(BH_E_USAGE, "bh_consensus_pairs_host: %llu segments (fewer than 2^32)", (unsigned long long)n_segs);
	uint64_t n_rows = 0;
	for (uint64_t i = 0; i < n_segs; ++i) {
		const BhipPairSeg *g = &segs[i], *p = i ? &segs[i - 1] : NULL;
		if (g->sample >= n_samples) return bh_set_error(BH_E_USAGE, "bh_consensus_pairs_host: segment %llu names sample %u of %u", (unsigned long long)i, g->sample, n_samples);
		if (!g->pos || !g->len) return bh_set_error(BH_E_USAGE, "bh_consensus_pairs_host: segment %llu has position %u and length %u (both >= 1)", (unsigned long long)i, g->pos, g->len);
		if ((uint64_t)g->pos + g->len > 0xFFFFFFFFull) return bh_set_error(BH_E_USAGE, "bh_consensus_pairs_host: segment %llu: position %u + length %u (at most 2^32 - 1)", (unsigned long long)i, g->pos, g->len);
		if (g->off > n_letters || g->len > n_letters - g->off)
			return bh_set_error(BH_E_USAGE, "bh_consensus_pairs_host: segment %llu owns letters %llu + %u of %llu", (unsigned long long)i, (unsigned long long)g->off, g->len, (unsigned long long)n_letters);
		if (p && (p->sample > g->sample || (p->sample == g->sample && p->header > g->header)))
			return bh_set_error(BH_E_USAGE, "bh_consensus_pairs_host: segments not ascending by (sample, header, pos) at segment %llu", (unsigned long long)i);
		if (p && p->sample == g->sample && p->header == g->header) {
			if ((uint64_t)g->pos < (uint64_t)p->pos + p->len)
				return bh_set_error(BH_E_USAGE, "bh_consensus_pairs_host: segment %llu at position %u starts before the end of the one before it (%u + %u): out of order or overlapping",
				                    (unsigned long long)i, g->pos, p->pos, p->len);
		} else ++n_rows;
	}
	info[0] = n_segs;
	if (n_samples < 2 || !n_segs) return BH_OK;
	HostRow *rows = malloc((size_t)n_rows * sizeof(*rows));
	if (!rows) return bh_set_error(BH_E_OOM, "OOM:conspairs");
	uint64_t nr = 0;
	for (uint64_t i = 0; i < n_segs; ++i) {
		if (!i || segs[i - 1].sample != segs[i].sample || segs[i - 1].header != segs[i].header) { rows[nr].key = (uint64_t)segs[i].header << 16 | segs[i].sample; rows[nr].seg0 = i; rows[nr].n_seg = 0; ++nr; }
		++rows[nr - 1].n_seg;
	}
	qsort(rows, (size_t)nr, sizeof(*rows), row_cmp);
	int rc = BH_OK;
	uint64_t found = 0;
	char *dense = NULL; uint64_t dense_cap = 0;
	for (uint64_t a = 0; a < nr && !rc;) {
		uint64_t b = a;
		while (b < nr && (rows[b].key >> 16) == (rows[a].key >> 16)) ++b;
		const uint64_t m = b - a;
		if (m < 2) { a = b; continue; }
		++info[1]; info[3] += m * (m - 1) / 2;
		/* the header's covered extent [lo, hi), a dense row per sample over it: 0 outside the segments */
		uint64_t lo = ~0ull, hi = 0;
		for (uint64_t r = a; r < b; ++r) {
			const BhipPairSeg *f = &segs[rows[r].seg0], *l = &segs[rows[r].seg0 + rows[r].n_seg - 1];
			if (f->pos < lo) lo = f->pos;
			if ((uint64_t)l->pos + l->len > hi) hi = (uint64_t)l->pos + l->len;
		}
		const uint64_t span = hi - lo;
		if (m * span > dense_cap) {
			char *d2 = realloc(dense, (size_t)(m * span));
			if (!d2) { rc = bh_set_error(BH_E_OOM, "OOM:conspairs"); break; }
			dense = d2; dense_cap = m * span;
		}
		memset(dense, 0, (size_t)(m * span));
		for (uint64_t r = a; r < b; ++r) for (uint32_t t = 0; t < rows[r].n_seg; ++t) {
			const BhipPairSeg *g = &segs[rows[r].seg0 + t];
			memcpy(dense + (r - a) * span + (g->pos - lo), letters + g->off, g->len);
		}
		for (uint64_t x = 0; x < span; ++x) { int any = 0; for (uint64_t r = 0; r < m && !any; ++r) any = dense[r * span + x] != 0; info[2] += (uint64_t)any; }
		for (uint64_t i = 0; i < m; ++i) for (uint64_t j = i + 1; j < m; ++j) {
			const char *x = dense + i * span, *y = dense + j * span;
			uint64_t compared = 0, same = 0;
			for (uint64_t t = 0; t < span; ++t) if (comparable(x[t]) && comparable(y[t])) { ++compared; same += x[t] == y[t]; }
			if (compared < min_compared) continue;
			if (found < pair_cap) {
				BhipPair *p = &pairs[found];
				p->header = (uint32_t)(rows[a].key >> 16); p->a = (uint32_t)(rows[a + i].key & 0xFFFFu); p->b = (uint32_t)(rows[a + j].key & 0xFFFFu); p->pad = 0;
				p->compared = (uint32_t)compared; p->same = (uint32_t)same;
			}
			++found;
		}
		a = b;
	}
	free(dense); free(rows);
	if (rc) return rc;
	*n_pairs = found;
	if (found > pair_cap) return BH_E_CAPACITY;      /* (what was written is not a result: the caller asks again with room) */
	info[4] = found;
	return BH_OK;
}

/* the device: ctx = the handle */
static int solve_device(void *ctx, uint32_t n_samples, const BhipPairSeg *segs, uint64_t n_segs, const char *letters, uint64_t n_letters, uint32_t min_compared,
                        BhipPair *pairs, uint64_t pair_cap, uint64_t *n_pairs, uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "consensus pairs: the pairs are counted on the device and rank 0 has no device handle");
	const int rc = bhip_consensus_pairs(ctx, n_samples, segs, n_segs, letters, n_letters, min_compared, pairs, pair_cap, n_pairs, info);
	if (rc == BHIP_E_CAPACITY) return BH_E_CAPACITY;
	if (rc) return bh_set_error(rc == BHIP_E_ARG || rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "consensus pairs: %s", bhip_last_error());
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

int bh_conspairs_check_min(uint64_t v) {
	if (!v || v > 0x7FFFFFFFull) return bh_set_error(BH_E_USAGE, "ERROR: --consensus-pairs-min takes 1 .. 2147483647");
	return BH_OK;
}

typedef struct { char *name; uint64_t i; } NameRow;
static int name_cmp(const void *a, const void *b) {
	const NameRow *x = a, *y = b;
	const int c = strcmp(x->name, y->name);
	return c ? c : (x->i > y->i) - (x->i < y->i);
}
/* (sorted, neighbours compared: the work follows n log n up to the 65 535 samples the primitive takes) */
int bh_conspairs_check_names(const char *const *out_paths, uint64_t n) {
	int rc = BH_OK;
	NameRow *nm = calloc(n ? n : 1, sizeof(*nm));
	if (!nm) return bh_set_error(BH_E_OOM, "OOM:conspairs");
	for (uint64_t i = 0; i < n && !rc; ++i) { nm[i].i = i; if (!(nm[i].name = sample_name(out_paths[i]))) rc = bh_set_error(BH_E_OOM, "OOM:conspairs"); }
	if (!rc) {
		qsort(nm, (size_t)n, sizeof(*nm), name_cmp);
		for (uint64_t j = 1; j < n; ++j) if (!strcmp(nm[j - 1].name, nm[j].name)) {
			rc = bh_set_error(BH_E_USAGE, "ERROR: --consensus-pairs: outputs '%s' and '%s' are both sample '%s'", out_paths[nm[j - 1].i], out_paths[nm[j].i], nm[j].name);
			break;
		}
	}
	for (uint64_t i = 0; i < n; ++i) free(nm[i].name);
	free(nm);
	return rc;
}

int bh_conspairs_open(const char *prefix, uint32_t min_compared, BhConsPairs **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_conspairs_open: no place for the object");
	*out = NULL;
	if (!prefix) return bh_set_error(BH_E_USAGE, "bh_conspairs_open: no prefix");
	const int rc = bh_conspairs_check_min(min_compared);
	if (rc) return rc;
	BhConsPairs *p = calloc(1, sizeof(*p));
	if (!p) return bh_set_error(BH_E_OOM, "OOM:conspairs");
	p->minCompared = min_compared;
	for (int k = 0; k < 3; ++k)
		if (asprintf(&p->fin[k], "%s%s", prefix, kSuffix[k]) < 0 || asprintf(&p->tmp[k], "%s%s.tmp%ld", prefix, kSuffix[k], (long)getpid()) < 0) { bh_conspairs_close(p); return bh_set_error(BH_E_OOM, "OOM:conspairs"); }
	*out = p;
	return BH_OK;
}

void bh_conspairs_set_solver(BhConsPairs *p, bh_conspairs_solver_fn fn, void *ctx) { if (p) { p->fn = fn; p->ctx = ctx; } }
void bh_conspairs_abort(BhConsPairs *p) { if (p && !p->dead) p->dead = BH_E_DEVICE; }

/* the segments of one written record (a sample's segments of one header, in order) with the letters their offsets point into */
int bh_conspairs_add(BhConsPairs *p, uint32_t sample, uint32_t header, const BhipConsSeg *segs, uint64_t n, const char *letters) {
	if (!p || !n) return BH_OK;
	if (p->dead) return bh_set_error(p->dead, "the consensus pairs were ended by an earlier error");
	if (p->written) return bh_set_error(BH_E_USAGE, "bh_conspairs_add: the files have been written");
	uint64_t nl = 0;
	for (uint64_t i = 0; i < n; ++i) {
		nl += segs[i].len;      /* (a record called through position 2^32 - 1 is one the primitive's keys cannot hold: said here, in the run's terms) */
		if ((uint64_t)segs[i].pos + segs[i].len > 0xFFFFFFFFull)
			return p->dead = bh_set_error(BH_E_USAGE, "ERROR: --consensus-pairs: a record of sample %u is covered through position %lu; the pairs take positions up to 4294967294", sample,
			                              (unsigned long)((uint64_t)segs[i].pos + segs[i].len - 1));
	}
	if (p->nSegs + n > p->capSegs) {
		uint64_t nc = p->capSegs ? p->capSegs * 2 : 1024;
		while (nc < p->nSegs + n) nc *= 2;
		BhipPairSeg *s2 = realloc(p->segs, nc * sizeof(*s2));
		if (!s2) return p->dead = bh_set_error(BH_E_OOM, "OOM:conspairs");
		p->segs = s2; p->capSegs = nc;
	}
	if (p->nLetters + nl > p->capLetters) {
		uint64_t nc = p->capLetters ? p->capLetters * 2 : (1u << 16);
		while (nc < p->nLetters + nl) nc *= 2;
		char *l2 = realloc(p->letters, nc);
		if (!l2) return p->dead = bh_set_error(BH_E_OOM, "OOM:conspairs");
		p->letters = l2; p->capLetters = nc;
	}
	if (sample >= p->capDiag) {
		uint32_t nc = p->capDiag ? p->capDiag : 16;
		while (nc <= sample) nc *= 2;
		uint64_t *d2 = realloc(p->diag, (size_t)nc * sizeof(*d2));
		if (!d2) return p->dead = bh_set_error(BH_E_OOM, "OOM:conspairs");
		memset(d2 + p->capDiag, 0, (size_t)(nc - p->capDiag) * sizeof(*d2));
		p->diag = d2; p->capDiag = nc;
	}
	for (uint64_t i = 0; i < n; ++i) {
		BhipPairSeg *g = &p->segs[p->nSegs++];
		g->sample = sample; g->header = header; g->pos = segs[i].pos; g->len = segs[i].len; g->off = p->nLetters;
		memcpy(p->letters + p->nLetters, letters + segs[i].off, segs[i].len);
		for (uint32_t t = 0; t < segs[i].len; ++t) p->diag[sample] += (uint64_t)comparable(p->letters[p->nLetters + t]);
		p->nLetters += segs[i].len;
	}
	++p->nRecords;
	return BH_OK;
}

/* the matrices are accumulated from the pair list, never as n_samples^2 sums: a cell per (row, column) that has a pair row, both ways round */
typedef struct { uint32_t r, c; uint64_t compared, same; } PairCell;
static int cell_cmp(const void *a, const void *b) {
	const PairCell *x = a, *y = b;
	return x->r != y->r ? (x->r > y->r) - (x->r < y->r) : (x->c > y->c) - (x->c < y->c);
}

static void put_cell_na(FILE *f, int na, int is_identity, uint64_t same, uint64_t compared) {
	if (is_identity) { if (na) fputs("\tNA", f); else fprintf(f, "\t%.6f", (double)same / (double)compared); }
	else if (na) fputs("\t0", f); else fprintf(f, "\t%lu", (unsigned long)compared);
}

/* the solver call and the three temporary files.  names, failed: per sample in study order; head, length: per unique-header number;
 * by_rank: the unique-header number of every header number the segments carry */
int bh_conspairs_write(BhConsPairs *p, void *hh, uint32_t n_samples, char *const *names, const uint8_t *failed, char *const *head, const uint32_t *by_rank, const uint32_t *length,
                       uint32_t n_headers) {
	if (!p) return bh_set_error(BH_E_USAGE, "bh_conspairs_write: no object");
	if (p->dead) return bh_set_error(p->dead, "the consensus pairs were ended by an earlier error: no file is written");
	if (p->written) return bh_set_error(BH_E_USAGE, "bh_conspairs_write: the files have been written");
	if (n_samples > 65535u) return p->dead = bh_set_error(BH_E_USAGE, "ERROR: --consensus-pairs takes at most 65535 samples (%u)", n_samples);
	/* room for every pair that can exist: per header m (m - 1) / 2 of its m records (the segments ascend by sample, then header) */
	uint64_t cap = 0;
	{
		uint32_t *cnt = calloc(n_headers ? n_headers : 1, sizeof(*cnt));
		if (!cnt) return p->dead = bh_set_error(BH_E_OOM, "OOM:conspairs");
		for (uint64_t i = 0; i < p->nSegs; ++i) {
			const BhipPairSeg *g = &p->segs[i];
			if (g->header >= n_headers) { free(cnt); return p->dead = bh_set_error(BH_E_INTERNAL, "consensus pairs: a kept segment names header %u of %u", g->header, n_headers); }
			if (!i || p->segs[i - 1].sample != g->sample || p->segs[i - 1].header != g->header) ++cnt[g->header];
		}
		for (uint32_t h = 0; h < n_headers; ++h) cap += (uint64_t)cnt[h] * (cnt[h] ? cnt[h] - 1 : 0) / 2;
		free(cnt);
	}
	BhipPair *pairs = malloc((size_t)(cap ? cap : 1) * sizeof(*pairs));
	PairCell *cells = NULL; uint64_t n_cells = 0;
	if (!pairs) return p->dead = bh_set_error(BH_E_OOM, "OOM:conspairs");
	uint64_t np = 0, dev[8] = {0};
	int rc = (p->fn ? p->fn : solve_device)(p->fn ? p->ctx : hh, n_samples, p->segs, p->nSegs, p->letters, p->nLetters, p->minCompared, pairs, cap, &np, dev);
	if (rc == BH_E_CAPACITY) rc = bh_set_error(BH_E_INTERNAL, "consensus pairs: %lu pairs do not fit the room for every pair that can exist (%lu)", (unsigned long)np, (unsigned long)cap);
	FILE *f[3] = {NULL, NULL, NULL};
	for (int k = 0; k < 3 && !rc; ++k) if (!(f[k] = fopen(p->tmp[k], "wb"))) rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", p->tmp[k]);
	if (!rc) {
		fputs("#Reference\tSampleA\tSampleB\tLength\tCompared\tSame\tDiffer\tIdentity\n", f[0]);
		for (uint64_t i = 0; i < np && !rc; ++i) {
			const BhipPair *q = &pairs[i];
			if (q->header >= n_headers || q->a >= q->b || q->b >= n_samples || q->same > q->compared || q->compared < p->minCompared ||
			    (i && (pairs[i - 1].header > q->header || (pairs[i - 1].header == q->header && (pairs[i - 1].a > q->a || (pairs[i - 1].a == q->a && pairs[i - 1].b >= q->b))))))
				{ rc = bh_set_error(BH_E_INTERNAL, "consensus pairs: pair %lu (header %u, samples %u and %u, %u of %u) is out of order or out of range", (unsigned long)i, q->header, q->a, q->b, q->same, q->compared); break; }
			const uint32_t h = by_rank[q->header];
			fprintf(f[0], "%s\t%s\t%s\t%u\t%u\t%u\t%u\t%.6f\n", head[h], names[q->a], names[q->b], length[h], q->compared, q->same, q->compared - q->same, (double)q->same / (double)q->compared);
		}
	}
	if (!rc && np) {      /* every pair row under (a, b) and (b, a), sorted, equal cells summed */
		if (!(cells = malloc((size_t)(2 * np) * sizeof(*cells)))) rc = bh_set_error(BH_E_OOM, "OOM:conspairs");
		else {
			for (uint64_t i = 0; i < np; ++i) {
				const PairCell ab = {pairs[i].a, pairs[i].b, pairs[i].compared, pairs[i].same}, ba = {pairs[i].b, pairs[i].a, pairs[i].compared, pairs[i].same};
				cells[2 * i] = ab; cells[2 * i + 1] = ba;
			}
			qsort(cells, (size_t)(2 * np), sizeof(*cells), cell_cmp);
			for (uint64_t i = 0; i < 2 * np; ++i) {
				if (n_cells && cells[n_cells - 1].r == cells[i].r && cells[n_cells - 1].c == cells[i].c) { cells[n_cells - 1].compared += cells[i].compared; cells[n_cells - 1].same += cells[i].same; }
				else cells[n_cells++] = cells[i];
			}
		}
	}
	for (int k = 1; k < 3 && !rc; ++k) {
		fputs(k == 1 ? "#Identity" : "#Compared", f[k]);
		for (uint32_t s = 0; s < n_samples; ++s) fprintf(f[k], "\t%s", names[s]);
		fputc('\n', f[k]);
		uint64_t at = 0;      /* the first cell not before (a, b): rows and columns ascend as the cells do */
		for (uint32_t a = 0; a < n_samples; ++a) {
			fputs(names[a], f[k]);
			for (uint32_t b = 0; b < n_samples; ++b) {
				if (a == b) {
					if (failed && failed[a]) fputs("\tNA", f[k]);
					else if (k == 1) fputs("\t1.000000", f[k]);
					else fprintf(f[k], "\t%lu", (unsigned long)(a < p->capDiag ? p->diag[a] : 0));
					continue;
				}
				while (at < n_cells && (cells[at].r < a || (cells[at].r == a && cells[at].c < b))) ++at;
				const int has = at < n_cells && cells[at].r == a && cells[at].c == b;
				if (failed && (failed[a] || failed[b])) fputs("\tNA", f[k]);
				else put_cell_na(f[k], !has, k == 1, has ? cells[at].same : 0, has ? cells[at].compared : 0);
			}
			fputc('\n', f[k]);
		}
	}
	for (int k = 0; k < 3; ++k) if (f[k]) { const int bad = ferror(f[k]) | fclose(f[k]); if (bad && !rc) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", p->tmp[k]); }
	free(pairs); free(cells);
	if (rc) { for (int k = 0; k < 3; ++k) (void)unlink(p->tmp[k]); return p->dead = rc; }
	uint32_t n_failed = 0;
	for (uint32_t s = 0; failed && s < n_samples; ++s) n_failed += failed[s] != 0;
	memcpy(p->devInfo, dev, sizeof dev);
	p->info[0] = n_samples - n_failed; p->info[1] = n_failed; p->info[2] = p->nRecords; p->info[3] = dev[1]; p->info[4] = dev[2]; p->info[5] = dev[3]; p->info[6] = np;
	p->info[7] = p->nSegs * sizeof(BhipPairSeg) + p->nLetters;
	p->have_info = 1; p->written = 1;
	free(p->segs); free(p->letters); p->segs = NULL; p->letters = NULL; p->nSegs = p->capSegs = p->nLetters = p->capLetters = 0;      /* (the kept rows are released) */
	return BH_OK;
}

int bh_conspairs_written(const BhConsPairs *p) { return p && p->written && !p->dead; }

/* the three files get their names (bh_consensus_write, after the two consensus files got theirs); on a failure none of the three stays */
int bh_conspairs_commit(BhConsPairs *p) {
	if (!p || !p->written || p->dead || p->renamed) return bh_set_error(BH_E_USAGE, "bh_conspairs_commit: nothing to name");
	int rc = BH_OK, k = 0;
	for (; k < 3 && !rc; ++k) if (rename(p->tmp[k], p->fin[k])) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", p->tmp[k], p->fin[k]);
	if (rc) { for (int j = 0; j + 1 < k; ++j) (void)unlink(p->fin[j]); for (int j = 0; j < 3; ++j) (void)unlink(p->tmp[j]); p->dead = rc; return rc; }
	p->renamed = 1;
	return BH_OK;
}

/* the collector becomes the consensus's: bh_consensus_sample hands it the rows, bh_consensus_pairs and bh_consensus_write finish it */
void bh_conspairs_attach(BhConsPairs *p, BhCons *cons) {
	static const BhConsPairsHooks hooks = {bh_conspairs_add, bh_conspairs_write, bh_conspairs_written, bh_conspairs_commit, bh_conspairs_abort};
	bh_consensus_set_pairs(cons, p, p ? &hooks : NULL);
}

/* one line on standard output */
void bh_conspairs_print_info(BhConsPairs *p) {
	if (!p || !p->have_info || p->dead) return;
	printf("ConsensusPairs: %lu samples done, %lu failed, %lu records, %lu headers with two or more, %lu union positions, %lu pairs examined, %lu written, %lu host bytes kept, device %.3f ms\n",
	       (unsigned long)p->info[0], (unsigned long)p->info[1], (unsigned long)p->info[2], (unsigned long)p->info[3], (unsigned long)p->info[4], (unsigned long)p->info[5],
	       (unsigned long)p->info[6], (unsigned long)p->info[7], p->devInfo[5] / 1e3);
}

/* [0] samples done [1] failed [2] records [3] headers with two or more [4] union positions [5] pairs examined [6] pairs written [7] host bytes kept;
 * device_us (may be NULL): the solver's microseconds */
void bh_conspairs_last_info(const BhConsPairs *p, uint64_t info[8], uint64_t *device_us) {
	if (info) { if (p && p->have_info) memcpy(info, p->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t)); }
	if (device_us) *device_us = p && p->have_info ? p->devInfo[5] : 0;
}

void bh_conspairs_close(BhConsPairs *p) {
	if (!p) return;
	for (int k = 0; k < 3; ++k) { if (p->tmp[k] && !p->renamed) (void)unlink(p->tmp[k]); free(p->tmp[k]); free(p->fin[k]); }
	free(p->segs); free(p->letters); free(p->diag);
	free(p);
}
