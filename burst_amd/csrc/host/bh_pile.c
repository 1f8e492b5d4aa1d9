/* bh_pile.c -- variant sites per sample from the alignment paths of the printed lines (burst_hip --variants,
 * host.Session(variants=...)).
 *
 * No reference counterpart.  The definition is bhip_pile_run's (include/burst_hip.h): per sample, every printed line
 * is a path on a header at a position; a site (header, position) counts the bases the lines show there.  The paths come from the tracer
 * the --cigar columns use (bh_paths.c hands every traced group to bh_pile_collect, so nothing is traced twice), the sites from ONE
 * bhip_pile_run per sample on the reporting rank's handle, and this file holds what is left: the lines of a sample, the order of the
 * headers, the table -- and bh_pile_host, the definition once more in plain C (one record per observed base, sorted and counted), which
 * the tests without a device and the yardstick use. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

struct BhPile {
	char *prefix, *tmpn, *finn; FILE *tmp;
	uint32_t nH, minDepth, minAlt; int uniqueOnly;
	char **head; uint32_t *rank, *byRank;      /* header of every unique-header number (copies); its place in strcmp order and back */
	int dead;
	bh_pile_solver_fn fn; void *ctx;
	/* the sample being collected */
	BhipPileLine *lines; uint64_t nLines, capLines, nPrinted;
	uint32_t *ops; uint64_t nOps, capOps;
	/* the rows so far */
	BhipPileSite *rows; uint32_t *rowSample; uint64_t nRows, capRows;
	char **names; uint32_t nSamples;
	uint64_t info[8], infoLines; int have_info;      /* of the last sample that was solved */
};

/* ---- the definition in plain C ---- */
typedef struct { uint64_t key; uint32_t w; uint8_t cls, ref, plain; } PileObs;      /* cls 0..3 A C G T, 4 Del, 5 Other, 6 insertion mark */
static int obs_cmp(const void *a, const void *b) { const uint64_t x = ((const PileObs *)a)->key, y = ((const PileObs *)b)->key; return (x > y) - (x < y); }
static uint64_t clump_words(uint32_t len) { return ((uint64_t)len + 1) / 2; }
static uint8_t ref_code(const BhPileRefs *R, const uint64_t *clump_off, uint32_t refIx, uint32_t col0) {
	const uint8_t b = R->packed[(clump_off[refIx >> 4] + (col0 >> 1)) * 16 + (refIx & 15u)];
	return (col0 & 1u) ? b >> 4 : b & 15u;
}

/* the checks of a solver's lines in plain C (bhip_pile_run's, `who` opens the texts); *n_obs: an upper bound of the records a walk writes */
int bh_pile_check_lines(const char *who, const BhPileRefs *R, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                        const uint32_t *ops, uint64_t n_ops, uint64_t *n_obs_out) {
	uint64_t n_obs = 0, wsum = 0;
	if (n_lines && (!R || !R->clump_len || !lines || !q_off || (n_ops && !ops))) return bh_set_error(BH_E_USAGE, "%s: null argument", who);
	for (uint64_t i = 0; i < n_lines; ++i) {
		const BhipPileLine *u = &lines[i];
		if (u->q >= n_queries || q_off[u->q + 1] < q_off[u->q]) return bh_set_error(BH_E_USAGE, "%s: line %llu names query %u of %u", who, (unsigned long long)i, u->q, n_queries);
		if (u->refIx >= 16ull * R->n_clumps || u->refIx >= R->tot_refs) return bh_set_error(BH_E_USAGE, "%s: line %llu names reference %u of %u", who, (unsigned long long)i, u->refIx, R->tot_refs);
		if (u->op_off > n_ops || u->n_ops > n_ops - u->op_off) return bh_set_error(BH_E_USAGE, "%s: line %llu owns ops %llu + %u of %llu", who, (unsigned long long)i, (unsigned long long)u->op_off, u->n_ops, (unsigned long long)n_ops);
		uint64_t on_q = 0, on_r = 0; uint32_t last = 0;
		for (uint32_t k = 0; k < u->n_ops; ++k) {
			const uint32_t word = ops[u->op_off + k], len = word >> 4, code = word & 15u;
			if (!len || code == last || (code != BHIP_OP_I && code != BHIP_OP_D && code != BHIP_OP_EQ && code != BHIP_OP_X))
				return bh_set_error(BH_E_USAGE, "%s: line %llu, op %u: word 0x%x is not a run of I, D, = or X, or repeats the op before it", who, (unsigned long long)i, k, word);
			last = code;
			if (code != BHIP_OP_D) on_q += len;
			if (code != BHIP_OP_I) on_r += len;
		}
		if (on_q != q_off[u->q + 1] - q_off[u->q]) return bh_set_error(BH_E_USAGE, "%s: line %llu: its ops consume %llu query symbols, query %u has %llu", who, (unsigned long long)i,
			(unsigned long long)on_q, u->q, (unsigned long long)(q_off[u->q + 1] - q_off[u->q]));
		if (u->ref_first < 1 || (uint64_t)u->ref_first - 1 + on_r > R->clump_len[u->refIx >> 4])
			return bh_set_error(BH_E_USAGE, "%s: line %llu: columns %u + %llu leave a clump of %u", who, (unsigned long long)i, u->ref_first, (unsigned long long)on_r, R->clump_len[u->refIx >> 4]);
		if (u->pos < 1 || (uint64_t)u->pos + on_r > 0xFFFFFFFFull) return bh_set_error(BH_E_USAGE, "%s: line %llu: position %u + %llu columns (1 .. 2^32 - 1)", who, (unsigned long long)i, u->pos, (unsigned long long)on_r);
		if (!u->w) return bh_set_error(BH_E_USAGE, "%s: line %llu has weight 0", who, (unsigned long long)i);
		wsum += u->w;
		if (wsum > 0x7FFFFFFFull) return bh_set_error(BH_E_USAGE, "%s: the lines stand for more than 2^31 - 1 reads (line %llu)", who, (unsigned long long)i);
		n_obs += on_r + u->n_ops;
	}
	if (n_obs_out) *n_obs_out = n_obs;
	return BH_OK;
}

int bh_pile_host(void *refs, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                 const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, uint32_t min_alt, BhipPileSite *sites, uint64_t cap, uint64_t *n_sites, uint64_t info[8]) {
	const BhPileRefs *R = refs;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!R || !R->packed || !R->clump_len || !n_sites || (n_lines && (!lines || !q_codes || !q_off)) || (n_ops && !ops) || (cap && !sites))
		return bh_set_error(BH_E_USAGE, "bh_pile_host: null argument");
	*n_sites = 0;
	if (!min_depth || !min_alt) return bh_set_error(BH_E_USAGE, "bh_pile_host: min_depth %u, min_alt %u (1 .. 2^31 - 1 each)", min_depth, min_alt);
	uint64_t n_obs = 0;
	{ const int rc = bh_pile_check_lines("bh_pile_host", R, q_off, n_queries, lines, n_lines, ops, n_ops, &n_obs); if (rc) return rc; }
	if (!n_lines) return BH_OK;
	uint64_t *clump_off = malloc(((size_t)R->n_clumps + 1) * 8);
	PileObs *ob = malloc((n_obs + 1) * sizeof(*ob));
	if (!clump_off || !ob) { free(clump_off); free(ob); return bh_set_error(BH_E_OOM, "OOM:variants"); }
	clump_off[0] = 0;
	for (uint32_t c = 0; c < R->n_clumps; ++c) clump_off[c + 1] = clump_off[c] + clump_words(R->clump_len[c]);
	/* one record per observation and per insertion mark */
	uint64_t n = 0;
	for (uint64_t i = 0; i < n_lines; ++i) {
		const BhipPileLine *u = &lines[i];
		const uint8_t *q = q_codes + q_off[u->q];
		const uint64_t hkey = (uint64_t)u->header << 32;
		uint32_t p = u->pos, col = u->ref_first - 1; uint64_t j = 0;
		for (uint32_t k = 0; k < u->n_ops; ++k) {
			const uint32_t word = ops[u->op_off + k], len = word >> 4, code = word & 15u;
			if (code == BHIP_OP_I) {
				if (k > 0 && k + 1 < u->n_ops) { PileObs *o = &ob[n++]; o->key = hkey | (p - 1); o->w = u->w; o->cls = 6; o->ref = ref_code(R, clump_off, u->refIx, col - 1); o->plain = 0; }
				j += len;
				continue;
			}
			for (uint32_t t = 0; t < len; ++t, ++p, ++col) {
				PileObs *o = &ob[n++];
				o->key = hkey | p; o->w = u->w; o->ref = ref_code(R, clump_off, u->refIx, col);
				if (code == BHIP_OP_D) { o->cls = 4; o->plain = 0; }
				else { const uint8_t s = q[j++] & 15u; const int acgt = s >= 1 && s <= 4; o->cls = acgt ? (uint8_t)(s - 1) : 5; o->plain = acgt && code == BHIP_OP_EQ; }
			}
		}
	}
	qsort(ob, n, sizeof(*ob), obs_cmp);
	uint64_t kept = 0;
	for (uint64_t a = 0; a < n;) {
		uint64_t b = a, cnt[7] = {0, 0, 0, 0, 0, 0, 0}, depth = 0; uint8_t ref = 15; int cand = 0;
		for (; b < n && ob[b].key == ob[a].key; ++b) {
			cnt[ob[b].cls] += ob[b].w;
			if (ob[b].ref < ref) ref = ob[b].ref;      /* (lanes that disagree: the smallest code) */
			if (!ob[b].plain) { cand = 1; ++info[0]; }
		}
		info[1] += (uint64_t)cand;
		for (int c = 0; c < 6; ++c) depth += cnt[c];
		if (ref >= 1 && ref <= 4 && depth >= min_depth && (depth - cnt[ref - 1] >= min_alt || cnt[6] >= min_alt)) {
			if (kept < cap) {
				BhipPileSite *s = &sites[kept];
				s->header = (uint32_t)(ob[a].key >> 32); s->pos = (uint32_t)ob[a].key; s->ref = ref; s->depth = (uint32_t)depth;
				for (int c = 0; c < 6; ++c) s->n[c] = (uint32_t)cnt[c];
				s->ins = (uint32_t)cnt[6];
			}
			++kept;
		}
		a = b;
	}
	free(clump_off); free(ob);
	*n_sites = kept;
	if (kept > cap) return BH_E_CAPACITY;
	info[2] = kept;
	return BH_OK;
}

/* the device: ctx = the handle */
static int solve_device(void *ctx, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines, const uint32_t *ops, uint64_t n_ops,
                        uint32_t min_depth, uint32_t min_alt, BhipPileSite *sites, uint64_t cap, uint64_t *n_sites, uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "variants: the sites are counted on the device and rank 0 has no device handle");
	const int rc = bhip_pile_run(ctx, q_codes, q_off, n_queries, lines, n_lines, ops, n_ops, min_depth, min_alt, sites, cap, n_sites, info);
	if (rc == BHIP_E_CAPACITY) return BH_E_CAPACITY;
	if (rc) return bh_set_error(rc == BHIP_E_ARG || rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "variants: %s", bhip_last_error());
	return BH_OK;
}

char *bh_pile_sample_name(const char *path) {      /* base name without its last extension (as the coverage names its columns) */
	const char *b = strrchr(path, '/');
	b = b ? b + 1 : path;
	char *s = strdup(b);
	if (!s) return NULL;
	char *dot = strrchr(s, '.');
	if (dot && dot != s) *dot = 0;
	return s;
}

typedef struct { const char *s; uint32_t h; } HeadRow;
static int head_cmp(const void *a, const void *b) {
	const HeadRow *x = a, *y = b;
	const int c = strcmp(x->s, y->s);
	return c ? c : (x->h > y->h) - (x->h < y->h);
}

int bh_pile_open_heads(const char *prefix, uint32_t n_headers, const char *const *heads, uint32_t min_depth, uint32_t min_alt, int unique_only, BhPile **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_pile_open: no place for the object");
	*out = NULL;
	if (!prefix || !n_headers || !heads) return bh_set_error(BH_E_USAGE, "bh_pile_open: no headers / no prefix");
	if (!min_depth || min_depth > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "ERROR: --variants-min-depth takes 1 .. 2147483647");
	if (!min_alt || min_alt > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "ERROR: --variants-min-alt takes 1 .. 2147483647");
	BhPile *pl = calloc(1, sizeof(*pl));
	if (!pl) return bh_set_error(BH_E_OOM, "OOM:variants");
	pl->nH = n_headers; pl->minDepth = min_depth; pl->minAlt = min_alt; pl->uniqueOnly = unique_only != 0;
	pl->prefix = strdup(prefix);
	pl->head = calloc(n_headers, sizeof(*pl->head));
	pl->rank = malloc((size_t)n_headers * 4); pl->byRank = malloc((size_t)n_headers * 4);
	HeadRow *rows = malloc((size_t)n_headers * sizeof(*rows));
	int ok = pl->prefix && pl->head && pl->rank && pl->byRank && rows;
	for (uint32_t h = 0; ok && h < n_headers; ++h) ok = (pl->head[h] = strdup(heads[h] ? heads[h] : "")) != NULL;
	if (ok && (asprintf(&pl->finn, "%svariants.txt", prefix) < 0 || asprintf(&pl->tmpn, "%svariants.txt.tmp%ld", prefix, (long)getpid()) < 0)) ok = 0;
	if (!ok) { free(rows); bh_pile_close(pl); return bh_set_error(BH_E_OOM, "OOM:variants"); }
	/* the device returns sites by ascending header number: the numbers it is given are the headers' places in strcmp order */
	for (uint32_t h = 0; h < n_headers; ++h) { rows[h].s = pl->head[h]; rows[h].h = h; }
	qsort(rows, n_headers, sizeof(*rows), head_cmp);
	for (uint32_t r = 0; r < n_headers; ++r) { pl->rank[rows[r].h] = r; pl->byRank[r] = rows[r].h; }
	free(rows);
	if (!(pl->tmp = fopen(pl->tmpn, "wb"))) { const int rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", pl->tmpn); bh_pile_close(pl); return rc; }
	setvbuf(pl->tmp, NULL, _IOFBF, 1 << 20);
	fputs("#Reference\tPosition\tRef\tSample\tDepth\tA\tC\tG\tT\tDel\tOther\tIns\n", pl->tmp);
	*out = pl;
	return BH_OK;
}

int bh_pile_open(const BhDb *db, const char *prefix, uint32_t min_depth, uint32_t min_alt, int unique_only, BhPile **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_pile_open: no place for the object");
	*out = NULL;
	if (!db || !prefix || !db->numRefHeads || !db->refMap || !db->refHead) return bh_set_error(BH_E_USAGE, "bh_pile_open: no database / no prefix");
	const char **head = calloc(db->numRefHeads, sizeof(*head));
	if (!head) return bh_set_error(BH_E_OOM, "OOM:variants");
	for (uint32_t i = 0; i < db->origTotR; ++i) if (db->refMap[i] < db->numRefHeads) head[db->refMap[i]] = db->refHead[i];      /* (the numbers the report's notes use) */
	const int rc = bh_pile_open_heads(prefix, db->numRefHeads, head, min_depth, min_alt, unique_only, out);
	free(head);
	return rc;
}

/* a collector alone (bh_vcf.c): no table, no file; the lines keep the header numbers they come with */
int bh_pile_open_lines(uint32_t n_headers, int unique_only, BhPile **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_pile_open_lines: no place for the object");
	*out = NULL;
	if (!n_headers) return bh_set_error(BH_E_USAGE, "bh_pile_open_lines: no headers");
	BhPile *pl = calloc(1, sizeof(*pl));
	if (!pl) return bh_set_error(BH_E_OOM, "OOM:variants");
	pl->nH = n_headers; pl->minDepth = pl->minAlt = 1; pl->uniqueOnly = unique_only != 0;
	pl->rank = malloc((size_t)n_headers * 4); pl->byRank = malloc((size_t)n_headers * 4);
	if (!pl->rank || !pl->byRank) { bh_pile_close(pl); return bh_set_error(BH_E_OOM, "OOM:variants"); }
	for (uint32_t h = 0; h < n_headers; ++h) pl->rank[h] = pl->byRank[h] = h;
	*out = pl;
	return BH_OK;
}
uint64_t bh_pile_lines(const BhPile *pl, const BhipPileLine **lines, const uint32_t **ops, uint64_t *n_ops, uint64_t *n_printed) {
	if (lines) *lines = pl ? pl->lines : NULL;
	if (ops) *ops = pl ? pl->ops : NULL;
	if (n_ops) *n_ops = pl ? pl->nOps : 0;
	if (n_printed) *n_printed = pl ? pl->nPrinted : 0;
	return pl ? pl->nLines : 0;
}
void bh_pile_drop_lines(BhPile *pl) { if (pl) pl->nLines = pl->nOps = pl->nPrinted = 0; }

void bh_pile_set_solver(BhPile *pl, bh_pile_solver_fn fn, void *ctx) { if (pl) { pl->fn = fn; pl->ctx = ctx; } }
void bh_pile_abort(BhPile *pl) { if (pl && !pl->dead) pl->dead = BH_E_DEVICE; }

static int die(BhPile *pl, int rc) { pl->dead = rc; return rc; }
static void drop_lines(BhPile *pl) { pl->nLines = pl->nOps = pl->nPrinted = 0; }

static int new_sample(BhPile *pl, const char *out_path) {
	char **nn = realloc(pl->names, ((size_t)pl->nSamples + 1) * sizeof(*nn));
	if (nn) pl->names = nn;
	char *nm = bh_pile_sample_name(out_path ? out_path : "sample");
	if (!nn || !nm) { free(nm); return bh_set_error(BH_E_OOM, "OOM:variants"); }
	pl->names[pl->nSamples++] = nm;
	return BH_OK;
}

/* a traced group of the report: the distinct records idx[0 .. nr) (ascending) with their requests, first columns and ops, and the notes
 * of the lines printed from them.  A line whose read is on other lines as well is left out under --variants-reads unique; consecutive
 * lines that show the same record on the same header at the same offset (a duplicate read's) are one entry of summed weight */
int bh_pile_collect(BhPile *pl, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t nr,
                    const BhPathBuf *bufs, uint64_t n_chunks) {
	if (!pl) return BH_OK;
	if (pl->dead) return bh_set_error(pl->dead, "variants were ended by an earlier error");
	const uint64_t base = pl->nOps, n_ops = nr ? off[nr] : 0;
	if (pl->nOps + n_ops > pl->capOps) {
		uint64_t nc = pl->capOps ? pl->capOps * 2 : (1u << 16);
		while (nc < pl->nOps + n_ops) nc *= 2;
		uint32_t *np = realloc(pl->ops, nc * sizeof(*np));
		if (!np) return die(pl, bh_set_error(BH_E_OOM, "OOM:variants"));
		pl->ops = np; pl->capOps = nc;
	}
	if (n_ops) memcpy(pl->ops + base, ops, n_ops * sizeof(*ops));
	pl->nOps += n_ops;
	for (uint64_t c = 0; c < n_chunks; ++c) for (uint64_t i = 0; i < bufs[c].n; ++i) {
		const BhPathLine *ln = &bufs[c].l[i];
		if (pl->uniqueOnly && !ln->uniq) continue;
		uint64_t lo = 0, hi = nr;
		while (lo + 1 < hi) { const uint64_t mid = (lo + hi) / 2; if (idx[mid] <= ln->hit) lo = mid; else hi = mid; }
		if (!nr || idx[lo] != ln->hit) return die(pl, bh_set_error(BH_E_INTERNAL, "variants: a printed line shows record %lu, which was not traced", (unsigned long)ln->hit));
		if (ln->header >= pl->nH) return die(pl, bh_set_error(BH_E_INTERNAL, "variants: a printed line names header %u of %u", ln->header, pl->nH));
		const uint64_t pos = (uint64_t)ln->refOff + first[lo];
		if (pos > 0xFFFFFFFFull) return die(pl, bh_set_error(BH_E_INTERNAL, "variants: position %lu does not fit 32 bits", (unsigned long)pos));
		++pl->nPrinted;
		BhipPileLine e;
		memset(&e, 0, sizeof e);
		e.q = req[lo].q; e.refIx = req[lo].refIx; e.ref_first = first[lo]; e.header = pl->rank[ln->header]; e.pos = (uint32_t)pos; e.w = 1;
		e.n_ops = (uint32_t)(off[lo + 1] - off[lo]); e.op_off = base + off[lo];
		if (pl->nLines) {
			BhipPileLine *p = &pl->lines[pl->nLines - 1];
			if (p->op_off == e.op_off && p->q == e.q && p->refIx == e.refIx && p->header == e.header && p->pos == e.pos && p->w < 0x7FFFFFFFu) { ++p->w; continue; }
		}
		if (pl->nLines == pl->capLines) {
			const uint64_t nc = pl->capLines ? pl->capLines * 2 : 4096;
			BhipPileLine *np = realloc(pl->lines, nc * sizeof(*np));
			if (!np) return die(pl, bh_set_error(BH_E_OOM, "OOM:variants"));
			pl->lines = np; pl->capLines = nc;
		}
		pl->lines[pl->nLines++] = e;
	}
	return BH_OK;
}

static int collect_cb(void *ctx, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t nr,
                      const BhPathBuf *bufs, uint64_t n_chunks) { return bh_pile_collect(ctx, idx, req, first, off, ops, nr, bufs, n_chunks); }
void bh_paths_set_pile(BhPaths *paths, BhPile *pl, int columns) { bh_paths_set_collector(paths, pl ? collect_cb : NULL, pl, columns); }

int bh_pile_sample_failed(BhPile *pl, const char *out_path) {
	if (!pl) return BH_OK;
	drop_lines(pl);
	const int rc = new_sample(pl, out_path);
	if (!rc) printf(" --> variants: sample '%s' failed alone: it has no rows\n", pl->names[pl->nSamples - 1]);
	return rc;
}

int bh_pile_sample(BhPile *pl, void *hh, const char *out_path, const uint8_t *q_codes, const uint64_t *q_off, uint64_t n_queries) {
	if (!pl) return bh_set_error(BH_E_USAGE, "bh_pile_sample: no variants object");
	if (pl->dead) return bh_set_error(pl->dead, "variants were ended by an earlier error");
	if (n_queries > 0xFFFFFFFFull) return die(pl, bh_set_error(BH_E_INTERNAL, "variants: %lu query entries", (unsigned long)n_queries));
	int rc = new_sample(pl, out_path);
	if (rc) return die(pl, rc);
	const uint32_t sample = pl->nSamples - 1;
	uint64_t cap = pl->nLines < 1024 ? 1024 : pl->nLines, n = 0, info[8] = {0};
	BhipPileSite *sites = NULL;
	for (int attempt = 0; attempt < 2; ++attempt) {      /* (the room grows once: the call says how many sites it has) */
		BhipPileSite *ns = realloc(sites, cap * sizeof(*ns));
		if (!ns) { free(sites); return die(pl, bh_set_error(BH_E_OOM, "OOM:variants")); }
		sites = ns;
		rc = (pl->fn ? pl->fn : solve_device)(pl->fn ? pl->ctx : hh, q_codes, q_off, (uint32_t)n_queries, pl->lines, pl->nLines, pl->ops, pl->nOps, pl->minDepth, pl->minAlt, sites, cap, &n, info);
		if (rc != BH_E_CAPACITY) break;
		if (attempt || n <= cap) { rc = bh_set_error(BH_E_INTERNAL, "variants: %lu sites do not fit the room the first call asked for", (unsigned long)n); break; }
		cap = n;
	}
	if (rc) { free(sites); return die(pl, rc); }      /* (any error of the solver is final: nothing will be written) */
	if (pl->nRows + n > pl->capRows) {
		uint64_t nc = pl->capRows ? pl->capRows * 2 : 4096;
		while (nc < pl->nRows + n) nc *= 2;
		BhipPileSite *nr = realloc(pl->rows, nc * sizeof(*nr)); if (nr) pl->rows = nr;
		uint32_t *nsm = realloc(pl->rowSample, nc * sizeof(*nsm)); if (nsm) pl->rowSample = nsm;
		if (!nr || !nsm) { free(sites); return die(pl, bh_set_error(BH_E_OOM, "OOM:variants")); }
		pl->capRows = nc;
	}
	/* the block of the sample: the sites come in (place of the header in strcmp order, position) order */
	for (uint64_t i = 0; i < n; ++i) {
		BhipPileSite s = sites[i];
		if (s.header >= pl->nH || s.ref > 15) { free(sites); return die(pl, bh_set_error(BH_E_INTERNAL, "variants: a site on header %u of %u", s.header, pl->nH)); }
		s.header = pl->byRank[s.header];
		fprintf(pl->tmp, "%s\t%u\t%c\t%s\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", pl->head[s.header], s.pos, ".ACGTNKMRYSWBVHD"[s.ref], pl->names[sample], s.depth,
		        s.n[0], s.n[1], s.n[2], s.n[3], s.n[4], s.n[5], s.ins);
		pl->rows[pl->nRows] = s; pl->rowSample[pl->nRows] = sample; ++pl->nRows;
	}
	free(sites);
	if (ferror(pl->tmp)) return die(pl, bh_set_error(BH_E_IO, "ERROR: write failed: %s", pl->tmpn));
	memcpy(pl->info, info, sizeof info); pl->infoLines = pl->nPrinted; pl->have_info = 1;
	drop_lines(pl);
	return BH_OK;
}

uint64_t bh_pile_rows(const BhPile *pl, BhipPileSite *rows, uint32_t *samples, uint64_t cap) {
	if (!pl) return 0;
	const uint64_t n = pl->nRows < cap ? pl->nRows : cap;
	if (rows && n) memcpy(rows, pl->rows, n * sizeof(*rows));
	if (samples && n) memcpy(samples, pl->rowSample, n * sizeof(*samples));
	return pl->nRows;
}

int bh_pile_write(BhPile *pl) {
	if (!pl) return bh_set_error(BH_E_USAGE, "bh_pile_write: no variants object");
	if (pl->dead) return bh_set_error(pl->dead, "variants were ended by an earlier error: no table is written");
	if (!pl->tmp) return bh_set_error(BH_E_USAGE, "bh_pile_write: the table has been written");
	FILE *f = pl->tmp; pl->tmp = NULL;
	int rc = BH_OK;
	if (ferror(f) | fclose(f)) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", pl->tmpn);
	else if (rename(pl->tmpn, pl->finn)) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", pl->tmpn, pl->finn);
	if (rc) { (void)unlink(pl->tmpn); pl->dead = rc; }
	return rc;
}

/* one line on standard output: the last sample's figures (bhip_pile_run's info) */
void bh_pile_print_info(BhPile *pl) {
	if (!pl || !pl->have_info || pl->dead) return;
	printf("Variants: %lu lines, %lu events, %lu candidate sites, %lu reported sites, device %.3f ms\n", (unsigned long)pl->infoLines, (unsigned long)pl->info[0],
	       (unsigned long)pl->info[1], (unsigned long)pl->info[2], pl->info[3] / 1e3);
}

void bh_pile_last_info(const BhPile *pl, uint64_t info[8], uint64_t *lines) {
	if (info) { if (pl && pl->have_info) memcpy(info, pl->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t)); }
	if (lines) *lines = pl && pl->have_info ? pl->infoLines : 0;
}

void bh_pile_close(BhPile *pl) {
	if (!pl) return;
	if (pl->tmp) { fclose(pl->tmp); if (pl->tmpn) (void)unlink(pl->tmpn); }      /* (not written: an abort, an error, or a caller that gave up) */
	for (uint32_t c = 0; c < pl->nSamples; ++c) free(pl->names[c]);
	if (pl->head) for (uint32_t h = 0; h < pl->nH; ++h) free(pl->head[h]);
	free(pl->names); free(pl->head); free(pl->rank); free(pl->byRank); free(pl->prefix); free(pl->tmpn); free(pl->finn);
	free(pl->lines); free(pl->ops); free(pl->rows); free(pl->rowSample);
	free(pl);
}
