/* bh_consensus.c -- consensus sequences per reference and sample from the alignment paths of the printed lines (burst_hip --consensus,
 * host.Session(consensus=...)).
 *
 * No reference counterpart.  The definition is bhip_consensus_run's (include/burst_hip.h): per sample, every printed
 * line is a path on a header at a position; every position the lines cover gets a letter, and the letters of a header become one record
 * in reference coordinates.  The paths come from the tracer the --cigar columns use (a collector beside --variants' and --sam's, so
 * nothing is traced twice), the segments and letters from ONE bhip_consensus_run per sample on the reporting rank's handle, and this file
 * holds what is left: the lines of a sample, the order of the headers, the lengths, the two files -- and bh_consensus_host, the definition
 * once more in plain C (one record per observed base, sorted and counted), which the tests without a device and the yardstick use. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

struct BhCons {
	char *tmpFa, *finFa, *tmpTx, *finTx; FILE *fa, *tx;
	uint32_t nH, minDepth, minBreadth; int uniqueOnly;
	char **head; uint32_t *rank, *byRank, *length;      /* header of every unique-header number (copies); its place in strcmp order and back; its length */
	int haveLengths; const BhDb *db;
	int dead;
	bh_cons_solver_fn fn; void *ctx;
	/* the sample being collected */
	BhipPileLine *lines; uint64_t nLines, capLines, nPrinted;
	uint32_t *ops; uint64_t nOps, capOps;
	/* the rows so far */
	BhConsRow *rows; uint64_t nRows, capRows;
	char **names; uint32_t nSamples;
	uint8_t *failed;                /* per sample: it failed alone (bh_consensus_sample_failed) */
	BhConsPairs *pairs; const BhConsPairsHooks *ph;      /* bh_consensus_set_pairs: NULL, or the collector every written record's segments and letters are handed to, and its entry points (bh_conspairs.c: this file links without it) */
	uint64_t info[8], infoLines, infoRecords; int have_info;      /* of the last sample that was solved */
};

/* ---- the definition in plain C ---- */
typedef struct { uint64_t key; uint32_t w; uint8_t cls, ref, plain; } ConsObs;      /* cls 0..3 A C G T, 4 Del, 5 Other, 6 insertion mark */
static int obs_cmp(const void *a, const void *b) { const uint64_t x = ((const ConsObs *)a)->key, y = ((const ConsObs *)b)->key; return (x > y) - (x < y); }
static uint8_t ref_code(const BhPileRefs *R, const uint64_t *clump_off, uint32_t refIx, uint32_t col0) {
	const uint8_t b = R->packed[(clump_off[refIx >> 4] + (col0 >> 1)) * 16 + (refIx & 15u)];
	return (col0 & 1u) ? b >> 4 : b & 15u;
}

int bh_consensus_host(void *refs, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                      const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, BhipConsSeg *segs, uint64_t seg_cap, uint64_t *n_segs,
                      char *letters, uint64_t letter_cap, uint64_t *n_letters, uint64_t info[8]) {
	const BhPileRefs *R = refs;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!R || !R->packed || !R->clump_len || !n_segs || !n_letters || (n_lines && (!lines || !q_codes || !q_off)) || (n_ops && !ops) || (seg_cap && !segs) || (letter_cap && !letters))
		return bh_set_error(BH_E_USAGE, "bh_consensus_host: null argument");
	*n_segs = *n_letters = 0;
	if (!min_depth || min_depth > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "bh_consensus_host: min_depth %u (1 .. 2^31 - 1)", min_depth);
	uint64_t n_obs = 0, wsum = 0;
	for (uint64_t i = 0; i < n_lines; ++i) {
		const BhipPileLine *u = &lines[i];
		if (u->q >= n_queries || q_off[u->q + 1] < q_off[u->q]) return bh_set_error(BH_E_USAGE, "bh_consensus_host: line %llu names query %u of %u", (unsigned long long)i, u->q, n_queries);
		if (u->refIx >= 16ull * R->n_clumps || u->refIx >= R->tot_refs) return bh_set_error(BH_E_USAGE, "bh_consensus_host: line %llu names reference %u of %u", (unsigned long long)i, u->refIx, R->tot_refs);
		if (u->op_off > n_ops || u->n_ops > n_ops - u->op_off) return bh_set_error(BH_E_USAGE, "bh_consensus_host: line %llu owns ops %llu + %u of %llu", (unsigned long long)i, (unsigned long long)u->op_off, u->n_ops, (unsigned long long)n_ops);
		uint64_t on_q = 0, on_r = 0; uint32_t last = 0;
		for (uint32_t k = 0; k < u->n_ops; ++k) {
			const uint32_t word = ops[u->op_off + k], len = word >> 4, code = word & 15u;
			if (!len || code == last || (code != BHIP_OP_I && code != BHIP_OP_D && code != BHIP_OP_EQ && code != BHIP_OP_X))
				return bh_set_error(BH_E_USAGE, "bh_consensus_host: line %llu, op %u: word 0x%x is not a run of I, D, = or X, or repeats the op before it", (unsigned long long)i, k, word);
			last = code;
			if (code != BHIP_OP_D) on_q += len;
			if (code != BHIP_OP_I) on_r += len;
		}
		if (on_q != q_off[u->q + 1] - q_off[u->q]) return bh_set_error(BH_E_USAGE, "bh_consensus_host: line %llu: its ops consume %llu query symbols, query %u has %llu", (unsigned long long)i,
			(unsigned long long)on_q, u->q, (unsigned long long)(q_off[u->q + 1] - q_off[u->q]));
		if (u->ref_first < 1 || (uint64_t)u->ref_first - 1 + on_r > R->clump_len[u->refIx >> 4])
			return bh_set_error(BH_E_USAGE, "bh_consensus_host: line %llu: columns %u + %llu leave a clump of %u", (unsigned long long)i, u->ref_first, (unsigned long long)on_r, R->clump_len[u->refIx >> 4]);
		if (u->pos < 1 || (uint64_t)u->pos + on_r > 0xFFFFFFFFull) return bh_set_error(BH_E_USAGE, "bh_consensus_host: line %llu: position %u + %llu columns (1 .. 2^32 - 1)", (unsigned long long)i, u->pos, (unsigned long long)on_r);
		if (!u->w) return bh_set_error(BH_E_USAGE, "bh_consensus_host: line %llu has weight 0", (unsigned long long)i);
		wsum += u->w;
		if (wsum > 0x7FFFFFFFull) return bh_set_error(BH_E_USAGE, "bh_consensus_host: the lines stand for more than 2^31 - 1 reads (line %llu)", (unsigned long long)i);
		n_obs += on_r + u->n_ops;
	}
	if (!n_lines) return BH_OK;
	uint64_t *clump_off = malloc(((size_t)R->n_clumps + 1) * 8);
	ConsObs *ob = malloc((n_obs + 1) * sizeof(*ob));
	if (!clump_off || !ob) { free(clump_off); free(ob); return bh_set_error(BH_E_OOM, "OOM:consensus"); }
	clump_off[0] = 0;
	for (uint32_t c = 0; c < R->n_clumps; ++c) clump_off[c + 1] = clump_off[c] + ((uint64_t)R->clump_len[c] + 1) / 2;
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
				if (k > 0 && k + 1 < u->n_ops) { ConsObs *o = &ob[n++]; o->key = hkey | (p - 1); o->w = u->w; o->cls = 6; o->ref = ref_code(R, clump_off, u->refIx, col - 1); o->plain = 0; }
				j += len;
				continue;
			}
			for (uint32_t t = 0; t < len; ++t, ++p, ++col) {
				ConsObs *o = &ob[n++];
				o->key = hkey | p; o->w = u->w; o->ref = ref_code(R, clump_off, u->refIx, col);
				if (code == BHIP_OP_D) { o->cls = 4; o->plain = 0; }
				else { const uint8_t s = q[j++] & 15u; const int acgt = s >= 1 && s <= 4; o->cls = acgt ? (uint8_t)(s - 1) : 5; o->plain = acgt && code == BHIP_OP_EQ; }
			}
		}
	}
	qsort(ob, n, sizeof(*ob), obs_cmp);
	/* every covered position has a record: a first pass counts segments and positions, a second one writes when there is room */
	uint64_t ns = 0, np = 0;
	for (uint64_t a = 0; a < n;) {
		uint64_t b = a;
		while (b < n && ob[b].key == ob[a].key) ++b;
		if (!a || ob[a].key != ob[a - 1].key + 1) ++ns;
		++np;
		a = b;
	}
	*n_segs = ns; *n_letters = np;
	info[2] = ns; info[3] = np;
	const int fits = ns <= seg_cap && np <= letter_cap && np <= 0x7FFFFFFFull;
	BhipConsSeg *g = NULL;
	uint64_t si = 0, li = 0;
	for (uint64_t a = 0; a < n;) {
		uint64_t b = a, cnt[7] = {0, 0, 0, 0, 0, 0, 0}, depth = 0; uint8_t ref = 15; int cand = 0;
		for (; b < n && ob[b].key == ob[a].key; ++b) {
			cnt[ob[b].cls] += ob[b].w;
			if (ob[b].ref < ref) ref = ob[b].ref;      /* (lanes that disagree: the smallest code) */
			if (!ob[b].plain) { cand = 1; ++info[0]; }      /* an event; a position with one is a candidate site */
		}
		info[1] += (uint64_t)cand;
		for (int c = 0; c < 6; ++c) depth += cnt[c];
		if (fits) {
			if (!a || ob[a].key != ob[a - 1].key + 1) {
				g = &segs[si++];
				memset(g, 0, sizeof *g);
				g->header = (uint32_t)(ob[a].key >> 32); g->pos = (uint32_t)ob[a].key; g->off = li;
			}
			char letter = 'N';
			if (depth >= min_depth) {
				++g->called;
				if (ref < 1 || ref > 4) { letter = "NACGTNKMRYSWBVHD"[ref]; ++g->ambig; }
				else {
					int win = ref - 1;
					for (int c = 0; c < 5; ++c) if (cnt[c] > cnt[win]) win = c;      /* only a larger count moves it: Ref among equals, else the first in the order */
					letter = "ACGT-"[win];
					if (win == ref - 1) ++g->same; else if (win == 4) ++g->del; else ++g->subst;
				}
				if (2 * cnt[6] > depth) ++g->ins_major;
			}
			letters[li++] = letter;
			++g->len;
		}
		a = b;
	}
	free(clump_off); free(ob);
	if (np > 0x7FFFFFFFull) return bh_set_error(BH_E_USAGE, "bh_consensus_host: the lines cover %llu positions (at most 2^31 - 1 in one call)", (unsigned long long)np);
	if (!fits) return BH_E_CAPACITY;
	return BH_OK;
}

/* the device: ctx = the handle */
static int solve_device(void *ctx, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines, const uint32_t *ops, uint64_t n_ops,
                        uint32_t min_depth, BhipConsSeg *segs, uint64_t seg_cap, uint64_t *n_segs, char *letters, uint64_t letter_cap, uint64_t *n_letters, uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "consensus: the letters are called on the device and rank 0 has no device handle");
	const int rc = bhip_consensus_run(ctx, q_codes, q_off, n_queries, lines, n_lines, ops, n_ops, min_depth, segs, seg_cap, n_segs, letters, letter_cap, n_letters, info);
	if (rc == BHIP_E_CAPACITY) return BH_E_CAPACITY;
	if (rc) return bh_set_error(rc == BHIP_E_ARG || rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "consensus: %s", bhip_last_error());
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

typedef struct { const char *s; uint32_t h; } HeadRow;
static int head_cmp(const void *a, const void *b) {
	const HeadRow *x = a, *y = b;
	const int c = strcmp(x->s, y->s);
	return c ? c : (x->h > y->h) - (x->h < y->h);
}

int bh_consensus_check_opts(uint32_t min_depth, uint32_t min_breadth) {
	if (!min_depth || min_depth > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "ERROR: --consensus-min-depth takes 1 .. 2147483647");
	if (min_breadth > 1000) return bh_set_error(BH_E_USAGE, "ERROR: --consensus-min-breadth takes 0 .. 1000 (permille of the reference's length)");
	return BH_OK;
}

/* lengths: of every header, or NULL (bh_consensus_open: the database's own extents, taken when the first sample ends) */
int bh_consensus_open_heads(const char *prefix, uint32_t n_headers, const char *const *heads, const uint32_t *lengths, uint32_t min_depth, uint32_t min_breadth, int unique_only, BhCons **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_consensus_open: no place for the object");
	*out = NULL;
	if (!prefix || !n_headers || !heads) return bh_set_error(BH_E_USAGE, "bh_consensus_open: no headers / no prefix");
	int rc = bh_consensus_check_opts(min_depth, min_breadth);
	if (rc) return rc;
	BhCons *cn = calloc(1, sizeof(*cn));
	if (!cn) return bh_set_error(BH_E_OOM, "OOM:consensus");
	cn->nH = n_headers; cn->minDepth = min_depth; cn->minBreadth = min_breadth; cn->uniqueOnly = unique_only != 0;
	cn->head = calloc(n_headers, sizeof(*cn->head));
	cn->rank = malloc((size_t)n_headers * 4); cn->byRank = malloc((size_t)n_headers * 4); cn->length = calloc(n_headers, 4);
	HeadRow *rows = malloc((size_t)n_headers * sizeof(*rows));
	int ok = cn->head && cn->rank && cn->byRank && cn->length && rows;
	for (uint32_t h = 0; ok && h < n_headers; ++h) ok = (cn->head[h] = strdup(heads[h] ? heads[h] : "")) != NULL;
	if (ok && (asprintf(&cn->finFa, "%sconsensus.fa", prefix) < 0 || asprintf(&cn->tmpFa, "%sconsensus.fa.tmp%ld", prefix, (long)getpid()) < 0 ||
	           asprintf(&cn->finTx, "%sconsensus.txt", prefix) < 0 || asprintf(&cn->tmpTx, "%sconsensus.txt.tmp%ld", prefix, (long)getpid()) < 0)) ok = 0;
	if (!ok) { free(rows); bh_consensus_close(cn); return bh_set_error(BH_E_OOM, "OOM:consensus"); }
	if (lengths) { memcpy(cn->length, lengths, (size_t)n_headers * 4); cn->haveLengths = 1; }
	/* the solver returns segments by ascending header number: the numbers it is given are the headers' places in strcmp order */
	for (uint32_t h = 0; h < n_headers; ++h) { rows[h].s = cn->head[h]; rows[h].h = h; }
	qsort(rows, n_headers, sizeof(*rows), head_cmp);
	for (uint32_t r = 0; r < n_headers; ++r) { cn->rank[rows[r].h] = r; cn->byRank[r] = rows[r].h; }
	free(rows);
	if (!(cn->fa = fopen(cn->tmpFa, "wb"))) { rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", cn->tmpFa); bh_consensus_close(cn); return rc; }
	if (!(cn->tx = fopen(cn->tmpTx, "wb"))) { rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", cn->tmpTx); bh_consensus_close(cn); return rc; }
	setvbuf(cn->fa, NULL, _IOFBF, 1 << 20);
	fputs("#Reference\tSample\tLength\tCovered\tCalled\tSame\tSubst\tDel\tAmbig\tInsMajor\tRecord\n", cn->tx);
	*out = cn;
	return BH_OK;
}

int bh_consensus_open(const BhDb *db, const char *prefix, const char *lengths_file, uint32_t min_depth, uint32_t min_breadth, int unique_only, BhCons **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_consensus_open: no place for the object");
	*out = NULL;
	if (!db || !prefix || !db->numRefHeads || !db->refMap || !db->refHead) return bh_set_error(BH_E_USAGE, "bh_consensus_open: no database / no prefix");
	int rc = bh_consensus_check_opts(min_depth, min_breadth);
	if (rc) return rc;
	const char **head = calloc(db->numRefHeads, sizeof(*head));
	uint32_t *len = lengths_file ? calloc(db->numRefHeads, 4) : NULL;
	if (!head || (lengths_file && !len)) { free(head); free(len); return bh_set_error(BH_E_OOM, "OOM:consensus"); }
	for (uint32_t i = 0; i < db->origTotR; ++i) if (db->refMap[i] < db->numRefHeads) head[db->refMap[i]] = db->refHead[i];      /* (the numbers the report's notes use) */
	if (lengths_file) rc = bh_cov_read_lengths(lengths_file, "--consensus-lengths", db->numRefHeads, head, len);      /* (before a file of ours exists) */
	if (!rc) rc = bh_consensus_open_heads(prefix, db->numRefHeads, head, len, min_depth, min_breadth, unique_only, out);
	if (!rc) (*out)->db = db;
	free(head); free(len);
	return rc;
}

void bh_consensus_set_solver(BhCons *cn, bh_cons_solver_fn fn, void *ctx) { if (cn) { cn->fn = fn; cn->ctx = ctx; } }
void bh_consensus_abort(BhCons *cn) { if (cn && !cn->dead) { cn->dead = BH_E_DEVICE; if (cn->pairs) cn->ph->abort(cn->pairs); } }
void bh_consensus_set_pairs(BhCons *cn, BhConsPairs *pairs, const BhConsPairsHooks *hooks) { if (cn) { cn->pairs = hooks ? pairs : NULL; cn->ph = hooks; } }

/* the end of the run with a pairs collector attached, before bh_consensus_write: ONE solver call over the rows of every written record on
 * the reporting rank's handle, and the three files under their temporary names */
int bh_consensus_pairs(BhCons *cn, void *hh) {
	if (!cn || !cn->pairs) return bh_set_error(BH_E_USAGE, "bh_consensus_pairs: no consensus with a pairs collector");
	if (cn->dead) return bh_set_error(cn->dead, "the consensus was ended by an earlier error: no file is written");
	if (!cn->fa || !cn->tx || cn->ph->written(cn->pairs)) return bh_set_error(BH_E_USAGE, "bh_consensus_pairs: the files have been written");
	const int rc = cn->ph->write(cn->pairs, hh, cn->nSamples, cn->names, cn->failed, cn->head, cn->byRank, cn->length, cn->nH);
	if (rc) cn->dead = rc;
	return rc;
}

static int die(BhCons *cn, int rc) { cn->dead = rc; return rc; }
static void drop_lines(BhCons *cn) { cn->nLines = cn->nOps = cn->nPrinted = 0; }

static int new_sample(BhCons *cn, const char *out_path) {
	char **nn = realloc(cn->names, ((size_t)cn->nSamples + 1) * sizeof(*nn));
	if (nn) cn->names = nn;
	uint8_t *nf = realloc(cn->failed, (size_t)cn->nSamples + 1);
	if (nf) cn->failed = nf;
	char *nm = sample_name(out_path ? out_path : "sample");
	if (!nn || !nf || !nm) { free(nm); return bh_set_error(BH_E_OOM, "OOM:consensus"); }
	cn->failed[cn->nSamples] = 0;
	cn->names[cn->nSamples++] = nm;
	return BH_OK;
}

/* a traced group of the report (as bh_pile_collect takes it): a line whose read is on other lines as well is left out under
 * --consensus-reads unique; consecutive lines that show the same record on the same header at the same offset (a duplicate read's) are
 * one entry of summed weight */
int bh_consensus_collect(BhCons *cn, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t nr,
                         const BhPathBuf *bufs, uint64_t n_chunks) {
	if (!cn) return BH_OK;
	if (cn->dead) return bh_set_error(cn->dead, "the consensus was ended by an earlier error");
	const uint64_t base = cn->nOps, n_ops = nr ? off[nr] : 0;
	if (cn->nOps + n_ops > cn->capOps) {
		uint64_t nc = cn->capOps ? cn->capOps * 2 : (1u << 16);
		while (nc < cn->nOps + n_ops) nc *= 2;
		uint32_t *np = realloc(cn->ops, nc * sizeof(*np));
		if (!np) return die(cn, bh_set_error(BH_E_OOM, "OOM:consensus"));
		cn->ops = np; cn->capOps = nc;
	}
	if (n_ops) memcpy(cn->ops + base, ops, n_ops * sizeof(*ops));
	cn->nOps += n_ops;
	for (uint64_t c = 0; c < n_chunks; ++c) for (uint64_t i = 0; i < bufs[c].n; ++i) {
		const BhPathLine *ln = &bufs[c].l[i];
		if (cn->uniqueOnly && !ln->uniq) continue;
		uint64_t lo = 0, hi = nr;
		while (lo + 1 < hi) { const uint64_t mid = (lo + hi) / 2; if (idx[mid] <= ln->hit) lo = mid; else hi = mid; }
		if (!nr || idx[lo] != ln->hit) return die(cn, bh_set_error(BH_E_INTERNAL, "consensus: a printed line shows record %lu, which was not traced", (unsigned long)ln->hit));
		if (ln->header >= cn->nH) return die(cn, bh_set_error(BH_E_INTERNAL, "consensus: a printed line names header %u of %u", ln->header, cn->nH));
		const uint64_t pos = (uint64_t)ln->refOff + first[lo];
		if (pos > 0xFFFFFFFFull) return die(cn, bh_set_error(BH_E_INTERNAL, "consensus: position %lu does not fit 32 bits", (unsigned long)pos));
		++cn->nPrinted;
		BhipPileLine e;
		memset(&e, 0, sizeof e);
		e.q = req[lo].q; e.refIx = req[lo].refIx; e.ref_first = first[lo]; e.header = cn->rank[ln->header]; e.pos = (uint32_t)pos; e.w = 1;
		e.n_ops = (uint32_t)(off[lo + 1] - off[lo]); e.op_off = base + off[lo];
		if (cn->nLines) {
			BhipPileLine *p = &cn->lines[cn->nLines - 1];
			if (p->op_off == e.op_off && p->q == e.q && p->refIx == e.refIx && p->header == e.header && p->pos == e.pos && p->w < 0x7FFFFFFFu) { ++p->w; continue; }
		}
		if (cn->nLines == cn->capLines) {
			const uint64_t nc = cn->capLines ? cn->capLines * 2 : 4096;
			BhipPileLine *np = realloc(cn->lines, nc * sizeof(*np));
			if (!np) return die(cn, bh_set_error(BH_E_OOM, "OOM:consensus"));
			cn->lines = np; cn->capLines = nc;
		}
		cn->lines[cn->nLines++] = e;
	}
	return BH_OK;
}

static int collect_cb(void *ctx, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t nr,
                      const BhPathBuf *bufs, char *const *text, const size_t *text_len, uint64_t n_chunks) {
	(void)text; (void)text_len;
	return bh_consensus_collect(ctx, idx, req, first, off, ops, nr, bufs, n_chunks);
}
int bh_paths_set_consensus(BhPaths *paths, BhCons *cn, int columns) { return bh_paths_add_collector(paths, collect_cb, cn, columns); }

int bh_consensus_sample_failed(BhCons *cn, const char *out_path) {
	if (!cn) return BH_OK;
	drop_lines(cn);
	const int rc = new_sample(cn, out_path);
	if (!rc) { cn->failed[cn->nSamples - 1] = 1; printf(" --> consensus: sample '%s' failed alone: it has no rows\n", cn->names[cn->nSamples - 1]); }
	return rc;
}

static void put_n(FILE *f, uint64_t n) {
	static const char ns[] = "NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN";
	for (; n >= 64; n -= 64) fwrite(ns, 1, 64, f);
	if (n) fwrite(ns, 1, (size_t)n, f);
}

int bh_consensus_sample(BhCons *cn, void *hh, const char *out_path, const uint8_t *q_codes, const uint64_t *q_off, uint64_t n_queries) {
	if (!cn) return bh_set_error(BH_E_USAGE, "bh_consensus_sample: no consensus object");
	if (cn->dead) return bh_set_error(cn->dead, "the consensus was ended by an earlier error");
	if (n_queries > 0xFFFFFFFFull) return die(cn, bh_set_error(BH_E_INTERNAL, "consensus: %lu query entries", (unsigned long)n_queries));
	int rc = new_sample(cn, out_path);
	if (rc) return die(cn, rc);
	const uint32_t sample = cn->nSamples - 1;
	if (!cn->haveLengths) {      /* no table: the database's own extents */
		if (!cn->db) return die(cn, bh_set_error(BH_E_USAGE, "bh_consensus_sample: no lengths"));
		if ((rc = bh_cov_default_lengths(cn->db, cn->fn ? NULL : hh, cn->length))) return die(cn, rc);
		cn->haveLengths = 1;
	}
	uint64_t seg_cap = cn->nLines < 1024 ? 1024 : cn->nLines, let_cap = 1u << 20, ns = 0, nl = 0, info[8] = {0};
	BhipConsSeg *segs = NULL; char *letters = NULL;
	for (int attempt = 0; attempt < 2; ++attempt) {      /* (the room grows once: the call says how much it needs) */
		BhipConsSeg *s2 = realloc(segs, seg_cap * sizeof(*s2)); if (s2) segs = s2;
		char *l2 = realloc(letters, let_cap); if (l2) letters = l2;
		if (!s2 || !l2) { free(segs); free(letters); return die(cn, bh_set_error(BH_E_OOM, "OOM:consensus")); }
		rc = (cn->fn ? cn->fn : solve_device)(cn->fn ? cn->ctx : hh, q_codes, q_off, (uint32_t)n_queries, cn->lines, cn->nLines, cn->ops, cn->nOps, cn->minDepth,
		                                        segs, seg_cap, &ns, letters, let_cap, &nl, info);
		if (rc != BH_E_CAPACITY) break;
		if (attempt || (ns <= seg_cap && nl <= let_cap)) { rc = bh_set_error(BH_E_INTERNAL, "consensus: %lu segments and %lu letters do not fit the room the first call asked for", (unsigned long)ns, (unsigned long)nl); break; }
		if (ns > seg_cap) seg_cap = ns;
		if (nl > let_cap) let_cap = nl;
	}
	if (rc) { free(segs); free(letters); return die(cn, rc); }      /* (any error of the solver is final: nothing will be written) */
	/* every segment inside its header's length, before a byte of the sample is written */
	uint64_t at = 0;
	for (uint64_t i = 0; i < ns && !rc; ++i) {
		const BhipConsSeg *g = &segs[i];
		if (g->header >= cn->nH || !g->pos || !g->len || g->off != at || g->off + g->len > nl || (i && (g->header < segs[i - 1].header || (g->header == segs[i - 1].header && g->pos <= segs[i - 1].pos + segs[i - 1].len))))
			rc = bh_set_error(BH_E_INTERNAL, "consensus: segment %lu on header %u of %u is out of order or out of range", (unsigned long)i, g->header, cn->nH);
		else if ((uint64_t)g->pos - 1 + g->len > cn->length[cn->byRank[g->header]])
			rc = bh_set_error(BH_E_USAGE, "ERROR: --consensus: a placement on '%s' ends at position %lu, beyond its length %u", cn->head[cn->byRank[g->header]],
			                  (unsigned long)((uint64_t)g->pos - 1 + g->len), cn->length[cn->byRank[g->header]]);
		at += g->len;
	}
	if (rc) { free(segs); free(letters); return die(cn, rc); }
	/* the block of the sample: the headers in strcmp order, as the segments come */
	uint64_t records = 0;
	for (uint64_t a = 0; a < ns;) {
		uint64_t b = a;
		BhConsRow row;
		memset(&row, 0, sizeof row);
		const uint32_t h = cn->byRank[segs[a].header], L = cn->length[h];
		row.header = h; row.sample = sample; row.length = L;
		for (; b < ns && segs[b].header == segs[a].header; ++b) {
			row.covered += segs[b].len; row.called += segs[b].called; row.same += segs[b].same; row.subst += segs[b].subst; row.del += segs[b].del;
			row.ambig += segs[b].ambig; row.ins_major += segs[b].ins_major;
		}
		row.record = row.called >= 1 && 1000ull * row.called >= (uint64_t)cn->minBreadth * L;
		if (row.record) {      /* N outside the segments, the segments copied: the record is never held as a whole */
			fprintf(cn->fa, ">%s|%s\n", cn->names[sample], cn->head[h]);
			uint64_t p = 0;      /* letters written so far */
			for (uint64_t s = a; s < b; ++s) {
				put_n(cn->fa, (uint64_t)segs[s].pos - 1 - p);
				fwrite(letters + segs[s].off, 1, segs[s].len, cn->fa);
				p = (uint64_t)segs[s].pos - 1 + segs[s].len;
			}
			put_n(cn->fa, L - p);
			fputc('\n', cn->fa);
			++records;
			if (cn->pairs && (rc = cn->ph->add(cn->pairs, sample, segs[a].header, segs + a, b - a, letters))) { free(segs); free(letters); return die(cn, rc); }      /* (kept: the row takes part) */
		}
		fprintf(cn->tx, "%s\t%s\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", cn->head[h], cn->names[sample], L, row.covered, row.called, row.same, row.subst, row.del, row.ambig,
		        row.ins_major, row.record);
		if (cn->nRows == cn->capRows) {
			const uint64_t nc = cn->capRows ? cn->capRows * 2 : 1024;
			BhConsRow *nr = realloc(cn->rows, nc * sizeof(*nr));
			if (!nr) { free(segs); free(letters); return die(cn, bh_set_error(BH_E_OOM, "OOM:consensus")); }
			cn->rows = nr; cn->capRows = nc;
		}
		cn->rows[cn->nRows++] = row;
		a = b;
	}
	free(segs); free(letters);
	if (ferror(cn->fa) || ferror(cn->tx)) return die(cn, bh_set_error(BH_E_IO, "ERROR: write failed: %s", ferror(cn->fa) ? cn->tmpFa : cn->tmpTx));
	memcpy(cn->info, info, sizeof info); cn->infoLines = cn->nPrinted; cn->infoRecords = records; cn->have_info = 1;
	drop_lines(cn);
	return BH_OK;
}

uint64_t bh_consensus_rows(const BhCons *cn, BhConsRow *rows, uint64_t cap) {
	if (!cn) return 0;
	const uint64_t n = cn->nRows < cap ? cn->nRows : cap;
	if (rows && n) memcpy(rows, cn->rows, n * sizeof(*rows));
	return cn->nRows;
}

/* both files get their names together, or neither */
int bh_consensus_write(BhCons *cn) {
	if (!cn) return bh_set_error(BH_E_USAGE, "bh_consensus_write: no consensus object");
	if (cn->dead) return bh_set_error(cn->dead, "the consensus was ended by an earlier error: no file is written");
	if (!cn->fa || !cn->tx) return bh_set_error(BH_E_USAGE, "bh_consensus_write: the files have been written");
	if (cn->pairs && !cn->ph->written(cn->pairs)) return bh_set_error(BH_E_USAGE, "bh_consensus_write: a pairs collector is attached and bh_consensus_pairs has not run");
	FILE *fa = cn->fa, *tx = cn->tx; cn->fa = cn->tx = NULL;
	int rc = BH_OK;
	const int bad_fa = ferror(fa) | fclose(fa), bad_tx = ferror(tx) | fclose(tx);
	if (bad_fa || bad_tx) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", bad_fa ? cn->tmpFa : cn->tmpTx);
	else if (rename(cn->tmpFa, cn->finFa)) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", cn->tmpFa, cn->finFa);
	else if (rename(cn->tmpTx, cn->finTx)) { rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", cn->tmpTx, cn->finTx); (void)unlink(cn->finFa); }
	if (!rc && cn->pairs && (rc = cn->ph->commit(cn->pairs))) { (void)unlink(cn->finFa); (void)unlink(cn->finTx); }      /* (all five, or none) */
	if (rc) { (void)unlink(cn->tmpFa); (void)unlink(cn->tmpTx); cn->dead = rc; }
	return rc;
}

/* one line on standard output: the last sample's figures (bhip_consensus_run's info) */
void bh_consensus_print_info(BhCons *cn) {
	if (!cn || !cn->have_info || cn->dead) return;
	printf("Consensus: %lu lines, %lu events, %lu candidate sites, %lu segments, %lu covered positions, %lu records written, device %.3f ms\n", (unsigned long)cn->infoLines,
	       (unsigned long)cn->info[0], (unsigned long)cn->info[1], (unsigned long)cn->info[2], (unsigned long)cn->info[3], (unsigned long)cn->infoRecords, cn->info[4] / 1e3);
}

void bh_consensus_last_info(const BhCons *cn, uint64_t info[8], uint64_t *lines, uint64_t *records) {
	if (info) { if (cn && cn->have_info) memcpy(info, cn->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t)); }
	if (lines) *lines = cn && cn->have_info ? cn->infoLines : 0;
	if (records) *records = cn && cn->have_info ? cn->infoRecords : 0;
}

void bh_consensus_close(BhCons *cn) {
	if (!cn) return;
	if (cn->fa) { fclose(cn->fa); if (cn->tmpFa) (void)unlink(cn->tmpFa); }      /* (not written: an abort, an error, or a caller that gave up) */
	if (cn->tx) { fclose(cn->tx); if (cn->tmpTx) (void)unlink(cn->tmpTx); }
	for (uint32_t c = 0; c < cn->nSamples; ++c) free(cn->names[c]);
	if (cn->head) for (uint32_t h = 0; h < cn->nH; ++h) free(cn->head[h]);
	free(cn->names); free(cn->head); free(cn->rank); free(cn->byRank); free(cn->length); free(cn->tmpFa); free(cn->finFa); free(cn->tmpTx); free(cn->finTx);
	free(cn->lines); free(cn->ops); free(cn->rows); free(cn->failed);
	free(cn);
}
