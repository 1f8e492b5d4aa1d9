/* bh_chimera.c -- de-novo two-parent chimera check of the reads of a query file from the lines it prints against itself and their
 * alignment paths (burst_hip --chimeras, host.Session(chimeras=...)).
 *
 * No reference counterpart: the definition is bhip_chimera_run's (include/burst_hip.h), a pure integer function of
 * the printed lines and their paths.  The per-read profiles are computed on the device; this file holds what is left: the reads (names,
 * weights and `;size=N` through bh_cluster.c's name table, lengths), the traced groups of the report turned into lines, the table and the
 * `Chimeras:` line -- and bh_chimera_host, the definition once more in plain sequential C, which the tests without a device and the
 * yardstick use. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define NO_NODE 0xFFFFFFFFu
#define MAX_EDITS 254u

struct BhChimera {
	char *prefix; int use_sizes, dead;
	uint32_t skew, min_seg, min_gain;
	bh_chimera_solver_fn fn; void *ctx;
	BhCluster *tab;                      /* the reads' names and weights (bh_cluster.c's table) */
	uint32_t n; uint32_t *len;           /* reads (nodes) in file order, their lengths */
	const BhQueries *Q; uint32_t *node_of, *hdr_node; uint32_t n_hdr;      /* bh_chimera_begin: read of heads[j], read named by header h */
	BhipChimLine *lines; uint64_t nL, capL;
	uint32_t *ops; uint64_t nOps, capOps;
	uint64_t printed, foreign;
	BhipChimera *res; int solved;
	uint64_t info[8];
};

/* ---- the definition in plain sequential C ---- */
typedef struct { uint64_t key, val; } HostPair;
static int hpair_cmp(const void *a, const void *b) {
	const HostPair *x = a, *y = b;
	if (x->key != y->key) return x->key < y->key ? -1 : 1;
	return (x->val > y->val) - (x->val < y->val);
}
static int u64_cmp(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return (x > y) - (x < y); }

/* what bhip_chimera_run checks before it touches the device; edits[i] = the line's number of edit positions */
static int check_lines(uint32_t n_nodes, const uint32_t *len, const BhipChimLine *lines, uint64_t n_lines, const uint32_t *ops, uint64_t n_ops, uint32_t skew,
                       uint32_t min_seg, uint32_t min_gain, uint32_t *edits) {
	if (!skew || !min_seg || !min_gain) return bh_set_error(BH_E_USAGE, "bh_chimera_host: skew %u, min_seg %u, min_gain %u (each at least 1)", skew, min_seg, min_gain);
	if (n_nodes == NO_NODE || n_lines >= ((uint64_t)1 << 32)) return bh_set_error(BH_E_USAGE, "bh_chimera_host: %u nodes, %llu lines (fewer than 2^32 - 1 nodes, fewer than 2^32 lines)", n_nodes, (unsigned long long)n_lines);
	for (uint64_t i = 0; i < n_lines; ++i) {
		const BhipChimLine *l = &lines[i];
		if (l->q >= n_nodes || l->r >= n_nodes) return bh_set_error(BH_E_USAGE, "bh_chimera_host: line %llu names node %u -> %u of %u", (unsigned long long)i, l->q, l->r, n_nodes);
		if (!len[l->q] || len[l->q] > BHIP_MAX_QLEN) return bh_set_error(BH_E_USAGE, "bh_chimera_host: line %llu: read %u has %u symbols (1 .. %d)", (unsigned long long)i, l->q, len[l->q], BHIP_MAX_QLEN);
		if (l->op_off > n_ops || l->n_ops > n_ops - l->op_off) return bh_set_error(BH_E_USAGE, "bh_chimera_host: line %llu: ops %llu + %u leave the %llu given", (unsigned long long)i, (unsigned long long)l->op_off, l->n_ops, (unsigned long long)n_ops);
		uint64_t used = 0, ed = 0;
		for (uint32_t k = 0; k < l->n_ops; ++k) {
			const uint32_t w = ops[l->op_off + k], code = w & 15u, run = w >> 4;
			if (!run || (code != BHIP_OP_EQ && code != BHIP_OP_X && code != BHIP_OP_I && code != BHIP_OP_D)) return bh_set_error(BH_E_USAGE, "bh_chimera_host: line %llu: op word %u (0x%x) is no run of I/D/=/X", (unsigned long long)i, k, w);
			if (code != BHIP_OP_D) used += run;
			if (code != BHIP_OP_EQ) ed += run;
		}
		if (used != len[l->q]) return bh_set_error(BH_E_USAGE, "bh_chimera_host: line %llu: its ops consume %llu symbols, read %u has %u", (unsigned long long)i, (unsigned long long)used, l->q, len[l->q]);
		if (ed > MAX_EDITS) return bh_set_error(BH_E_USAGE, "bh_chimera_host: line %llu: %llu edits (at most %u)", (unsigned long long)i, (unsigned long long)ed, MAX_EDITS);
		edits[i] = (uint32_t)ed;
	}
	return BH_OK;
}

int bh_chimera_host(void *unused, uint32_t n_nodes, const uint32_t *weights, const uint32_t *len, const BhipChimLine *lines, uint64_t n_lines, const uint32_t *ops,
                    uint64_t n_ops, uint32_t skew, uint32_t min_seg, uint32_t min_gain, BhipChimera *out, uint64_t info[8]) {
	(void)unused;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (n_nodes && (!weights || !len || !out)) return bh_set_error(BH_E_USAGE, "bh_chimera_host: nodes without weights, lengths or a place for the result");
	if ((n_lines && !lines) || (n_ops && !ops)) return bh_set_error(BH_E_USAGE, "bh_chimera_host: lines or ops without their array");
	uint32_t *edits = malloc((n_lines + 1) * 4);
	if (!edits) return bh_set_error(BH_E_OOM, "OOM:chimeras");
	int rc = check_lines(n_nodes, len, lines, n_lines, ops, n_ops, skew, min_seg, min_gain, edits);
	if (rc) { free(edits); return rc; }
	info[5] = n_lines; info[6] = n_nodes;
	if (n_nodes) memset(out, 0, (size_t)n_nodes * sizeof(*out));
	if (!n_nodes || !n_lines) { free(edits); return BH_OK; }
	uint64_t *ord = malloc((size_t)n_nodes * 8);
	uint32_t *rank = malloc((size_t)n_nodes * 4), *order = malloc((size_t)n_nodes * 4);
	HostPair *hp = malloc((n_lines + 1) * sizeof(*hp));
	uint32_t *pos = malloc(256 * 4), *L = malloc(((size_t)BHIP_MAX_QLEN + 1) * 4);
	uint64_t *bl = malloc(((size_t)BHIP_MAX_QLEN + 1) * 8), *br = malloc(((size_t)BHIP_MAX_QLEN + 1) * 8);
	if (!ord || !rank || !order || !hp || !pos || !L || !bl || !br) { rc = bh_set_error(BH_E_OOM, "OOM:chimeras"); goto done; }
	/* priority: the larger weight first, the smaller number among equals */
	for (uint32_t i = 0; i < n_nodes; ++i) ord[i] = (uint64_t)(~weights[i]) << 32 | i;
	qsort(ord, n_nodes, 8, u64_cmp);
	for (uint32_t p = 0; p < n_nodes; ++p) { order[p] = (uint32_t)ord[p]; rank[order[p]] = p; }
	/* the lines towards candidate parents, per (q, r) the one with the fewest edits, the first among equals */
	uint64_t nk = 0, kept = 0;
	for (uint64_t i = 0; i < n_lines; ++i) {
		const uint32_t q = lines[i].q, r = lines[i].r;
		if (q == r || (uint64_t)weights[r] < (uint64_t)skew * (uint64_t)weights[q]) continue;
		hp[nk].key = (uint64_t)q << 32 | r; hp[nk].val = (uint64_t)edits[i] << 32 | i; ++nk;
	}
	qsort(hp, nk, sizeof(*hp), hpair_cmp);
	for (uint64_t i = 0; i < nk; ++i) if (!i || hp[i].key != hp[i - 1].key) hp[kept++] = hp[i];
	info[0] = kept;
	/* read by read: its lines are hp[a .. b) */
	for (uint64_t a = 0, b; a < kept; a = b) {
		const uint32_t q = (uint32_t)(hp[a].key >> 32), m = len[q];
		for (b = a; b < kept && (uint32_t)(hp[b].key >> 32) == q; ++b) { }
		if (b - a < 2 || (uint64_t)m < 2 * (uint64_t)min_seg) continue;      /* not evaluated */
		uint32_t single = ~0u;
		for (uint32_t c = 0; c <= m; ++c) bl[c] = br[c] = ~(uint64_t)0;
		for (uint64_t i = a; i < b; ++i) {
			const BhipChimLine *l = &lines[(uint32_t)hp[i].val];
			const uint32_t E = (uint32_t)(hp[i].val >> 32), rk = rank[(uint32_t)hp[i].key];
			uint32_t j = 0, e = 0;
			for (uint32_t k = 0; k < l->n_ops; ++k) {
				const uint32_t w = ops[l->op_off + k], code = w & 15u, run = w >> 4;
				for (uint32_t t = 0; t < run; ++t) {
					if (code == BHIP_OP_X || code == BHIP_OP_I) { pos[e++] = 2 * j + 1; ++j; }
					else if (code == BHIP_OP_D) pos[e++] = 2 * j;
					else ++j;
				}
			}
			if (l->flags & 1u) for (uint32_t t = 0; t < e; ++t) pos[t] = 2 * m - pos[t];      /* the path of the reverse-complement entry, mirrored */
			if (E < single) single = E;
			for (uint32_t c = 0; c <= m; ++c) {      /* L[c] for every cut, no cleverness */
				L[c] = 0;
				for (uint32_t t = 0; t < e; ++t) L[c] += pos[t] <= 2 * c;
			}
			for (uint32_t c = min_seg; c <= m - min_seg; ++c) {
				const uint64_t kl = (uint64_t)L[c] << 32 | rk, kr = (uint64_t)(E - L[c]) << 32 | rk;
				if (kl < bl[c]) bl[c] = kl;
				if (kr < br[c]) br[c] = kr;
			}
		}
		uint32_t cut = min_seg;
		uint64_t model = (bl[cut] >> 32) + (br[cut] >> 32);
		for (uint32_t c = min_seg + 1; c <= m - min_seg; ++c) { const uint64_t v = (bl[c] >> 32) + (br[c] >> 32); if (v < model) { model = v; cut = c; } }
		BhipChimera *o = &out[q];
		o->single = single; o->model = (uint32_t)model; o->cut = cut;
		o->a = order[(uint32_t)bl[cut]]; o->ea = (uint32_t)(bl[cut] >> 32);
		o->b = order[(uint32_t)br[cut]]; o->eb = (uint32_t)(br[cut] >> 32);
		o->role = single - o->model >= min_gain ? 2u : 1u;
		++info[1]; info[2] += o->role == 2;
		if (o->role == 2 && o->a == o->b) { rc = bh_set_error(BH_E_INTERNAL, "bh_chimera_host: read %u is chimeric with parent %u on both sides", q, o->a); goto done; }
	}
done:
	free(edits); free(ord); free(rank); free(order); free(hp); free(pos); free(L); free(bl); free(br);
	return rc;
}

/* the device: ctx = the handle */
static int solve_device(void *ctx, uint32_t n_nodes, const uint32_t *weights, const uint32_t *len, const BhipChimLine *lines, uint64_t n_lines, const uint32_t *ops,
                        uint64_t n_ops, uint32_t skew, uint32_t min_seg, uint32_t min_gain, BhipChimera *out, uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "chimeras: the profiles are computed on the device and rank 0 has no device handle");
	const int rc = bhip_chimera_run(ctx, n_nodes, weights, len, lines, n_lines, ops, n_ops, skew, min_seg, min_gain, out);
	if (rc) return bh_set_error(rc == BHIP_E_ARG ? BH_E_USAGE : rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "chimeras: %s", bhip_last_error());
	(void)bhip_chimera_info(ctx, info);
	return BH_OK;
}

int bh_chimera_open(const char *prefix, int use_sizes, uint32_t skew, uint32_t min_seg, uint32_t min_gain, BhChimera **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_chimera_open: no place for the object");
	*out = NULL;
	if (!prefix) return bh_set_error(BH_E_USAGE, "bh_chimera_open: no prefix");
	if (!skew || skew > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "ERROR: --chimera-skew takes 1 .. 2147483647");
	if (!min_seg || min_seg > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "ERROR: --chimera-min-seg takes 1 .. 2147483647");
	if (!min_gain || min_gain > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "ERROR: --chimera-min-gain takes 1 .. 2147483647");
	BhChimera *ch = calloc(1, sizeof(*ch));
	if (!ch) return bh_set_error(BH_E_OOM, "OOM:chimeras");
	ch->use_sizes = use_sizes != 0; ch->skew = skew; ch->min_seg = min_seg; ch->min_gain = min_gain;
	ch->prefix = strdup(prefix);
	if (!ch->prefix || bh_cluster_open("", use_sizes, &ch->tab)) { free(ch->prefix); free(ch); return bh_set_error(BH_E_OOM, "OOM:chimeras"); }
	*out = ch;
	return BH_OK;
}
void bh_chimera_set_solver(BhChimera *ch, bh_chimera_solver_fn fn, void *ctx) { if (ch) { ch->fn = fn; ch->ctx = ctx; } }
void bh_chimera_abort(BhChimera *ch) { if (ch && !ch->dead) ch->dead = BH_E_DEVICE; }
static int die(BhChimera *ch, int rc) { if (!ch->dead) ch->dead = rc; return rc; }

static void drop_reads(BhChimera *ch) {
	free(ch->len); free(ch->res); free(ch->node_of); free(ch->hdr_node);
	ch->len = NULL; ch->res = NULL; ch->node_of = ch->hdr_node = NULL; ch->Q = NULL;
	ch->n = ch->n_hdr = 0; ch->nL = ch->nOps = 0; ch->printed = ch->foreign = 0; ch->solved = 0;
	memset(ch->info, 0, sizeof ch->info);
}

int bh_chimera_names(BhChimera *ch, const char *const *names, const uint32_t *lens, uint32_t n) {
	if (!ch) return bh_set_error(BH_E_USAGE, "bh_chimera_names: no chimera object");
	if (ch->dead) return bh_set_error(ch->dead, "the chimera check was ended by an earlier error");
	if (n && (!names || !lens)) return bh_set_error(BH_E_USAGE, "bh_chimera_names: no names or no lengths");
	drop_reads(ch);
	const int rc = bh_cluster_names_as(ch->tab, names, n, "--chimeras", "--chimera-sizes");
	if (rc) return die(ch, rc);
	ch->len = malloc(((size_t)n + 1) * 4); ch->res = calloc((size_t)n + 1, sizeof(*ch->res));
	if (!ch->len || !ch->res) return die(ch, bh_set_error(BH_E_OOM, "OOM:chimeras"));
	if (n) memcpy(ch->len, lens, (size_t)n * 4);
	ch->n = n;
	return BH_OK;
}

/* room for one more line and n_ops more op words */
static int grow(BhChimera *ch, uint64_t n_ops) {
	if (ch->nL == ch->capL) {
		const uint64_t nc = ch->capL ? ch->capL * 2 : 4096;
		BhipChimLine *nl = realloc(ch->lines, nc * sizeof(*nl));
		if (!nl) return die(ch, bh_set_error(BH_E_OOM, "OOM:chimeras"));
		ch->lines = nl; ch->capL = nc;
	}
	if (ch->nOps + n_ops > ch->capOps) {
		uint64_t nc = ch->capOps ? ch->capOps * 2 : (1u << 16);
		while (nc < ch->nOps + n_ops) nc *= 2;
		uint32_t *no = realloc(ch->ops, nc * sizeof(*no));
		if (!no) return die(ch, bh_set_error(BH_E_OOM, "OOM:chimeras"));
		ch->ops = no; ch->capOps = nc;
	}
	if (ch->nL >= 0xFFFFFFFFull) return die(ch, bh_set_error(BH_E_USAGE, "ERROR: --chimeras takes fewer than 2^32 lines between reads"));
	return BH_OK;
}
static void push_line(BhChimera *ch, uint32_t q, uint32_t r, int reverse, uint32_t n_ops, uint64_t op_off) {
	const BhipChimLine l = {q, r, reverse ? 1u : 0u, n_ops, op_off};
	ch->lines[ch->nL++] = l;
}

int bh_chimera_line(BhChimera *ch, uint32_t q, const char *ref_name, size_t ref_len, int reverse, const uint32_t *ops, uint32_t n_ops) {
	if (!ch || !ref_name || (n_ops && !ops)) return bh_set_error(BH_E_USAGE, "bh_chimera_line: no chimera object, no name or no ops");
	if (ch->dead) return bh_set_error(ch->dead, "the chimera check was ended by an earlier error");
	if (q >= ch->n) return bh_set_error(BH_E_USAGE, "bh_chimera_line: read %u of %u", q, ch->n);
	++ch->printed; ch->solved = 0;
	const uint32_t r = bh_cluster_find(ch->tab, ref_name, ref_len);
	if (r == NO_NODE) { ++ch->foreign; return BH_OK; }
	const int rc = grow(ch, n_ops);
	if (rc) return rc;
	if (n_ops) memcpy(ch->ops + ch->nOps, ops, (size_t)n_ops * 4);
	push_line(ch, q, r, reverse, n_ops, ch->nOps);
	ch->nOps += n_ops;
	return BH_OK;
}

/* the lines of a .b6 file written with --cigar: columns 1, 2, 9, 10 and the last (the CIGAR text in =XID) */
int bh_chimera_add_b6(BhChimera *ch, const char *path) {
	if (!ch || !path) return bh_set_error(BH_E_USAGE, "bh_chimera_add_b6: no chimera object or no file");
	if (ch->dead) return bh_set_error(ch->dead, "the chimera check was ended by an earlier error");
	FILE *f = fopen(path, "rb");
	if (!f) return bh_set_error(BH_E_IO, "ERROR: Cannot open %s", path);
	char *line = NULL; size_t cap = 0; ssize_t len; uint64_t no = 0; int rc = BH_OK;
	uint32_t *w = NULL; size_t wcap = 0;
	while (!rc && (len = getline(&line, &cap, f)) >= 0) {
		++no;
		while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
		if (!len) continue;
		const char *col[32]; size_t cl_len[32]; int nc = 0;
		for (char *p = line; nc < 32;) {
			char *t = strchr(p, '\t');
			col[nc] = p; cl_len[nc] = t ? (size_t)(t - p) : strlen(p); ++nc;
			if (!t) break;
			p = t + 1;
		}
		if (nc < 14) { rc = bh_set_error(BH_E_USAGE, "ERROR: %s line %llu has fewer than 14 columns: --chimeras reads the output of --cigar", path, (unsigned long long)no); break; }
		const uint32_t q = bh_cluster_find(ch->tab, col[0], cl_len[0]);
		if (q == NO_NODE) { rc = bh_set_error(BH_E_USAGE, "ERROR: %s line %llu: column 1 names no read of the query file", path, (unsigned long long)no); break; }
		const long long st = strtoll(col[8], NULL, 10), ed = strtoll(col[9], NULL, 10);
		const char *c = col[nc - 1];
		size_t nw = 0;
		while (*c) {
			uint64_t v = 0; const char *d = c;
			while (*c >= '0' && *c <= '9' && v < ((uint64_t)1 << 28)) v = v * 10 + (uint64_t)(*c++ - '0');
			const uint32_t code = *c == '=' ? BHIP_OP_EQ : *c == 'X' ? BHIP_OP_X : *c == 'I' ? BHIP_OP_I : *c == 'D' ? BHIP_OP_D : 0u;
			if (c == d || !v || v >= ((uint64_t)1 << 28) || !code) { rc = bh_set_error(BH_E_USAGE, "ERROR: %s line %llu: the last column is no CIGAR in =XID", path, (unsigned long long)no); break; }
			++c;
			if (nw == wcap) { const size_t ncap = wcap ? wcap * 2 : 64; uint32_t *nn = realloc(w, ncap * 4); if (!nn) { rc = bh_set_error(BH_E_OOM, "OOM:chimeras"); break; } w = nn; wcap = ncap; }
			w[nw++] = (uint32_t)v << 4 | code;
		}
		if (!rc) rc = bh_chimera_line(ch, q, col[1], cl_len[1], st > ed, w, (uint32_t)nw);
	}
	free(line); free(w); fclose(f);
	if (rc) die(ch, rc);
	return rc;
}

/* before a run's report: the reads of Q in file order with their lengths, and which read every header of the database names */
int bh_chimera_begin(BhChimera *ch, const BhDb *db, const BhQueries *Q) {
	if (!ch || !db || !Q) return bh_set_error(BH_E_USAGE, "bh_chimera_begin: no chimera object / database / queries");
	if (ch->dead) return bh_set_error(ch->dead, "the chimera check was ended by an earlier error");
	if (Q->totQ >= NO_NODE) return die(ch, bh_set_error(BH_E_USAGE, "ERROR: --chimeras takes fewer than 2^32 - 1 reads"));
	const uint64_t n = Q->totQ;
	const char **names = malloc((n + 1) * sizeof(*names));
	uint32_t *node_of = malloc((n + 1) * 4), *lens = malloc((n + 1) * 4);
	int rc = names && node_of && lens ? BH_OK : bh_set_error(BH_E_OOM, "OOM:chimeras");
	if (!rc) rc = bh_cluster_file_order(Q, names, node_of);
	if (!rc) {
		for (uint64_t i = 0; i < Q->numUniq; ++i) for (uint64_t j = Q->offset[i]; j < Q->offset[i + 1]; ++j) lens[node_of[j]] = Q->len[i];
		rc = bh_chimera_names(ch, names, lens, (uint32_t)n);
	}
	free(names); free(lens);
	if (rc) { free(node_of); return die(ch, rc); }
	ch->node_of = node_of; ch->Q = Q;
	/* the notes of the printed lines name a reference by its header number (RefMap, or the reference itself without one) */
	uint32_t n_hdr = 0;
	for (uint32_t i = 0; i < db->origTotR; ++i) { const uint32_t h = db->refMap ? db->refMap[i] : i; if (h != NO_NODE && h + 1 > n_hdr) n_hdr = h + 1; }
	ch->hdr_node = malloc(((size_t)n_hdr + 1) * 4);
	if (!ch->hdr_node) return die(ch, bh_set_error(BH_E_OOM, "OOM:chimeras"));
	memset(ch->hdr_node, 0xFF, ((size_t)n_hdr + 1) * 4);
	ch->n_hdr = n_hdr;
	for (uint32_t i = 0; i < db->origTotR; ++i) {
		const uint32_t h = db->refMap ? db->refMap[i] : i;
		if (h >= n_hdr || ch->hdr_node[h] != NO_NODE || !db->refHead || !db->refHead[i]) continue;
		ch->hdr_node[h] = bh_cluster_find(ch->tab, db->refHead[i], strlen(db->refHead[i]));
	}
	return BH_OK;
}

/* a traced group of the report (bh_paths_emit): the distinct records idx[0 .. nr) (ascending) with their requests and ops, and the notes
 * of the lines printed from them, in file order.  FORAGE prints, per unique query, every read's lines one read after the other: the
 * notes of a unique query are one run, which its reads share in equal parts */
static int collect(void *ctx, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t nr,
                   const BhPathBuf *bufs, uint64_t n_chunks) {
	BhChimera *ch = ctx;
	(void)first;
	if (!ch) return BH_OK;
	if (ch->dead) return bh_set_error(ch->dead, "the chimera check was ended by an earlier error");
	const BhQueries *Q = ch->Q;
	if (!Q || !ch->node_of) return die(ch, bh_set_error(BH_E_INTERNAL, "chimeras: lines before bh_chimera_begin"));
	const uint64_t base = ch->nOps, n_ops = nr ? off[nr] : 0;
	int rc = grow(ch, n_ops);
	if (rc) return rc;
	if (n_ops) memcpy(ch->ops + base, ops, n_ops * sizeof(*ops));
	ch->nOps += n_ops;
	ch->solved = 0;
	#define RECORD_OF(ln, lo) do { uint64_t lo_ = 0, hi_ = nr; while (lo_ + 1 < hi_) { const uint64_t mid_ = (lo_ + hi_) / 2; if (idx[mid_] <= (ln)->hit) lo_ = mid_; else hi_ = mid_; } \
		if (!nr || idx[lo_] != (ln)->hit) return die(ch, bh_set_error(BH_E_INTERNAL, "chimeras: a printed line shows record %lu, which was not traced", (unsigned long)(ln)->hit)); \
		if (req[lo_].q >= Q->numEntries) return die(ch, bh_set_error(BH_E_INTERNAL, "chimeras: a record of query entry %u of %lu", req[lo_].q, (unsigned long)Q->numEntries)); \
		lo = lo_; } while (0)
	for (uint64_t c = 0; c < n_chunks; ++c) for (uint64_t i = 0, e; i < bufs[c].n; i = e) {
		uint64_t lo;
		RECORD_OF(&bufs[c].l[i], lo);
		const uint32_t uq = Q->six[req[lo].q];
		for (e = i + 1; e < bufs[c].n; ++e) { uint64_t l2; RECORD_OF(&bufs[c].l[e], l2); if (Q->six[req[l2].q] != uq) break; }
		if (uq >= Q->numUniq) return die(ch, bh_set_error(BH_E_INTERNAL, "chimeras: unique query %u of %lu", uq, (unsigned long)Q->numUniq));
		const uint64_t reads = Q->offset[uq + 1] - Q->offset[uq];
		if (!reads || (e - i) % reads) return die(ch, bh_set_error(BH_E_INTERNAL, "chimeras: %lu lines for the %lu reads of unique query %u", (unsigned long)(e - i), (unsigned long)reads, uq));
		const uint64_t per = (e - i) / reads;
		for (uint64_t k = i; k < e; ++k) {
			const BhPathLine *ln = &bufs[c].l[k];
			RECORD_OF(ln, lo);
			++ch->printed;
			const uint32_t r = ln->header < ch->n_hdr ? ch->hdr_node[ln->header] : NO_NODE;
			if (r == NO_NODE) { ++ch->foreign; continue; }
			if ((rc = grow(ch, 0))) return rc;
			push_line(ch, ch->node_of[Q->offset[uq] + (k - i) / per], r, Q->rc[req[lo].q] != 0, (uint32_t)(off[lo + 1] - off[lo]), base + off[lo]);
		}
	}
	#undef RECORD_OF
	return BH_OK;
}
void bh_paths_set_chimera(BhPaths *paths, BhChimera *ch, int columns) { bh_paths_set_collector(paths, ch ? collect : NULL, ch, columns); }

int bh_chimera_solve(BhChimera *ch, void *hh) {
	if (!ch) return bh_set_error(BH_E_USAGE, "bh_chimera_solve: no chimera object");
	if (ch->dead) return bh_set_error(ch->dead, "the chimera check was ended by an earlier error");
	if (ch->n && !ch->res) return bh_set_error(BH_E_USAGE, "bh_chimera_solve: no reads");
	uint64_t info[8] = {0};
	const uint32_t *w = bh_cluster_weights(ch->tab);
	const int rc = ch->fn ? ch->fn(ch->ctx, ch->n, w, ch->len, ch->lines, ch->nL, ch->ops, ch->nOps, ch->skew, ch->min_seg, ch->min_gain, ch->res, info)
	                      : solve_device(hh, ch->n, w, ch->len, ch->lines, ch->nL, ch->ops, ch->nOps, ch->skew, ch->min_seg, ch->min_gain, ch->res, info);
	if (rc) return die(ch, rc);      /* (any error of the solver is final: nothing will be written) */
	memcpy(ch->info, info, sizeof info);
	ch->solved = 1;
	return BH_OK;
}

uint32_t bh_chimera_reads(const BhChimera *ch) { return ch ? ch->n : 0; }
int bh_chimera_result(const BhChimera *ch, BhipChimera *out, uint32_t *weights) {
	if (!ch || !ch->solved) return bh_set_error(BH_E_USAGE, "bh_chimera_result: nothing has been checked");
	if (out && ch->n) memcpy(out, ch->res, (size_t)ch->n * sizeof(*out));
	if (weights && ch->n) memcpy(weights, bh_cluster_weights(ch->tab), (size_t)ch->n * 4);
	return BH_OK;
}
void bh_chimera_last_info(const BhChimera *ch, uint64_t info[8], uint64_t *lines, uint64_t *foreign) {
	if (info) { if (ch && ch->solved) memcpy(info, ch->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t)); }
	if (lines) *lines = ch ? ch->printed : 0;
	if (foreign) *foreign = ch ? ch->foreign : 0;
}

/* PREFIXchimeras.txt, under a temporary name first */
int bh_chimera_write(BhChimera *ch) {
	if (!ch) return bh_set_error(BH_E_USAGE, "bh_chimera_write: no chimera object");
	if (ch->dead) return bh_set_error(ch->dead, "the chimera check was ended by an earlier error: no table is written");
	if (!ch->solved) return bh_set_error(BH_E_USAGE, "bh_chimera_write: nothing has been checked");
	char *fin = NULL, *tmp = NULL;
	if (asprintf(&fin, "%schimeras.txt", ch->prefix) < 0) fin = NULL;
	if (asprintf(&tmp, "%schimeras.txt.tmp%ld", ch->prefix, (long)getpid()) < 0) tmp = NULL;
	int rc = fin && tmp ? BH_OK : bh_set_error(BH_E_OOM, "OOM:chimeras");
	if (!rc) {
		FILE *f = fopen(tmp, "wb");
		if (!f) rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", tmp);
		else {
			setvbuf(f, NULL, _IOFBF, 1 << 20);
			const uint32_t *w = bh_cluster_weights(ch->tab);
			fputs("#Read\tRole\tSingle\tModel\tCut\tParentA\tEditsA\tParentB\tEditsB\tWeight\n", f);
			for (uint32_t i = 0; i < ch->n; ++i) {
				const BhipChimera *o = &ch->res[i];
				if (!o->role) fprintf(f, "%s\t-\t0\t0\t0\t*\t0\t*\t0\t%u\n", bh_cluster_name(ch->tab, i), w[i]);
				else fprintf(f, "%s\t%c\t%u\t%u\t%u\t%s\t%u\t%s\t%u\t%u\n", bh_cluster_name(ch->tab, i), o->role == 2 ? 'Y' : 'N', o->single, o->model, o->cut,
				             bh_cluster_name(ch->tab, o->a), o->ea, bh_cluster_name(ch->tab, o->b), o->eb, w[i]);
			}
			if (ferror(f) | fclose(f)) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", tmp);
			if (!rc && rename(tmp, fin)) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", tmp, fin);
			if (rc) (void)unlink(tmp);
		}
	}
	free(fin); free(tmp);
	return rc;
}

/* one line on standard output */
void bh_chimera_print_info(BhChimera *ch) {
	if (!ch || !ch->solved || ch->dead) return;
	printf("Chimeras: %u reads, %llu lines, %llu foreign lines, %llu pairs kept, %llu reads evaluated, %llu chimeric, device %.3f ms\n", ch->n,
	       (unsigned long long)ch->printed, (unsigned long long)ch->foreign, (unsigned long long)ch->info[0], (unsigned long long)ch->info[1],
	       (unsigned long long)ch->info[2], ch->info[3] / 1e3);
}

void bh_chimera_close(BhChimera *ch) {
	if (!ch) return;
	drop_reads(ch);
	bh_cluster_close(ch->tab);
	free(ch->lines); free(ch->ops); free(ch->prefix);
	free(ch);
}
