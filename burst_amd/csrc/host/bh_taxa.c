/* bh_taxa.c -- taxon tables per sample: every read goes to the lowest common ancestor of the taxonomies of the references it was
 * placed on (burst_hip --taxa, host.Session(taxa=...)).
 *
 * The reference's embalmlets/embalmulate.c writes a taxa table from column 13 of BEST output and its README leaves the tied references of
 * ALLPATHS output to the user.  The definition is bhip_taxa_run's (include/burst_hip.h); the groups are the
 * abundance's (bh_em.c: one per unique query of the report's sink), the sort and the per-group reduction run on the device, and this file
 * holds what is left: the tree of the map's strings (bh_taxa_tree), the columns and the tables -- and bh_taxa_host / bh_taxa_rollup_host,
 * the definition once more in plain C, which counts the candidates below every ancestor and is what the tests without a device and the
 * yardstick use. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define TAXA_MAX_DEPTH 64u

/* ---- the tree of the map's strings ---- */
typedef struct { const char *s; uint32_t len, h; } Pre;      /* a header's string without its trailing ';' */
/* byte order with ';' below every other byte: a string is then followed at once by everything that continues it with ';', its subtree,
 * so the nodes met while walking the sorted strings stand in preorder */
static int pre_cmp(const void *a, const void *b) {
	const Pre *x = a, *y = b;
	const uint32_t m = x->len < y->len ? x->len : y->len;
	for (uint32_t i = 0; i < m; ++i) {
		const int cx = x->s[i] == ';' ? -1 : (unsigned char)x->s[i], cy = y->s[i] == ';' ? -1 : (unsigned char)y->s[i];
		if (cx != cy) return cx < cy ? -1 : 1;
	}
	return (x->len > y->len) - (x->len < y->len);
}
/* the leading levels two strings share: a level ends where a string has ';' or ends */
static uint32_t shared_levels(const Pre *p, const Pre *f) {
	uint32_t k = 0;
	for (uint32_t i = 0;; ++i) {
		const int ep = i == p->len || p->s[i] == ';', ef = i == f->len || f->s[i] == ';';
		if (ep && ef) ++k;
		if (i == p->len || i == f->len || p->s[i] != f->s[i]) return k;
	}
}

/* the taxonomy of a header without its trailing ';'; length 0 = no taxonomy */
static const char *header_tax(const BhTax *map, const char *head, int ncbi, uint32_t *len) {
	const char *t = bh_tax_lookup(map, head ? head : "", ncbi);
	size_t l = strlen(t);
	while (l && t[l - 1] == ';') --l;
	if (l == 10 && !memcmp(t, "Unassigned", 10)) l = 0;
	*len = (uint32_t)l;
	return t;
}

void bh_taxa_tree_free(BhTaxaTree *t) {
	if (!t) return;
	if (t->name) for (uint32_t v = 0; v < t->n_nodes; ++v) free(t->name[v]);
	free(t->name); free(t->parent); free(t->depth); free(t->header_node);
	memset(t, 0, sizeof *t);
}

int bh_taxa_tree(uint32_t n_headers, const char *const *heads, const BhTax *map, int ncbi, BhTaxaTree *out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_taxa_tree: no place for the tree");
	memset(out, 0, sizeof *out);
	if (!n_headers || !heads || !map) return bh_set_error(BH_E_USAGE, "bh_taxa_tree: no headers or no taxonomy map");      /* (a map without a line: every header at the root) */
	Pre *full = malloc(((size_t)n_headers + 1) * sizeof(*full));
	int rc = BH_OK;
	uint64_t nf = 0, nd = 0;
	if (!full) return bh_set_error(BH_E_OOM, "OOM:taxa");
	for (uint32_t h = 0; h < n_headers; ++h) {
		Pre f; f.h = h;
		f.s = header_tax(map, heads[h], ncbi, &f.len);
		if (!f.len) continue;      /* (the root) */
		uint32_t levels = 1;
		for (uint32_t i = 0; i < f.len; ++i) levels += f.s[i] == ';';
		if (levels > TAXA_MAX_DEPTH) { rc = bh_set_error(BH_E_USAGE, "ERROR: the taxonomy of '%s' has %u levels (limit %u)", heads[h] ? heads[h] : "", levels, TAXA_MAX_DEPTH); goto done; }
		full[nf++] = f;
	}
	qsort(full, nf, sizeof(*full), pre_cmp);
	/* a string adds the nodes of the levels it does not share with the string before it: counted, then made */
	for (uint64_t i = 0; i < nf; ++i) {
		uint32_t levels = 1;
		for (uint32_t k = 0; k < full[i].len; ++k) levels += full[i].s[k] == ';';
		nd += levels - (i ? shared_levels(&full[i - 1], &full[i]) : 0);
	}
	if (nd + 1 > 0x7FFFFFFFull) { rc = bh_set_error(BH_E_USAGE, "ERROR: the taxonomy has %llu nodes (limit 2^31 - 1)", (unsigned long long)nd + 1); goto done; }
	const uint32_t nN = (uint32_t)nd + 1;
	out->n_nodes = nN; out->n_headers = n_headers;
	out->name = calloc(nN, sizeof(*out->name)); out->parent = calloc(nN, 4); out->depth = calloc(nN, 4); out->header_node = calloc(n_headers, 4);
	if (!out->name || !out->parent || !out->depth || !out->header_node || !(out->name[0] = strdup("Unassigned"))) { rc = bh_set_error(BH_E_OOM, "OOM:taxa"); goto done; }
	uint32_t stack[TAXA_MAX_DEPTH + 1], sp = 0, v = 0;      /* the nodes of the levels of the string before, root excluded */
	for (uint64_t i = 0; i < nf; ++i) {
		const Pre *f = &full[i];
		sp = i ? shared_levels(&full[i - 1], f) : 0;
		uint32_t k = 0;
		for (uint32_t e = 0; e <= f->len; ++e) {
			if (e < f->len && f->s[e] != ';') continue;
			if (++k <= sp) continue;      /* (level k ends at e) */
			++v;
			out->parent[v] = k > 1 ? stack[k - 2] : 0;
			out->depth[v] = k;
			stack[k - 1] = v;
			if (!(out->name[v] = strndup(f->s, e))) { rc = bh_set_error(BH_E_OOM, "OOM:taxa"); goto done; }
		}
		out->header_node[f->h] = stack[k - 1];
	}
done:
	free(full);
	if (rc) bh_taxa_tree_free(out);
	return rc;
}

/* ---- the definition in plain C ---- */
/* the checks of bhip_taxa_run on the tree; depth[] filled */
static int check_tree(const char *who, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, uint32_t *depth) {
	if (!n_nodes || !parent || n_nodes > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "%s: no tree", who);
	if (n_headers && !header_node) return bh_set_error(BH_E_USAGE, "%s: headers without their nodes", who);
	if (parent[0]) return bh_set_error(BH_E_USAGE, "%s: node 0 is the root and its own parent", who);
	depth[0] = 0;
	for (uint32_t v = 1; v < n_nodes; ++v) {
		const uint32_t p = parent[v];
		if (p >= v) return bh_set_error(BH_E_USAGE, "%s: node %u has parent %u: not a preorder numbering", who, v, p);
		uint32_t x = v - 1;
		while (x > p) x = parent[x];
		if (x != p) return bh_set_error(BH_E_USAGE, "%s: the parent %u of node %u is no ancestor of node %u: not a preorder numbering", who, p, v, v - 1);
		depth[v] = depth[p] + 1;
		if (depth[v] > TAXA_MAX_DEPTH) return bh_set_error(BH_E_USAGE, "%s: node %u lies %u levels deep (limit %u)", who, v, depth[v], TAXA_MAX_DEPTH);
	}
	for (uint32_t h = 0; h < n_headers; ++h)
		if (header_node[h] >= n_nodes) return bh_set_error(BH_E_USAGE, "%s: header %u names node %u of %u", who, h, header_node[h], n_nodes);
	return BH_OK;
}
static int u64_cmp(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return (x > y) - (x < y); }
static void clade_of(uint32_t n_nodes, const uint32_t *parent, const uint64_t *own, uint64_t *clade) {
	memcpy(clade, own, (size_t)n_nodes * 8);
	for (uint32_t v = n_nodes - 1; v > 0; --v) clade[parent[v]] += clade[v];      /* (children have larger numbers than their parent) */
}

int bh_taxa_host(void *unused, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, uint32_t n_groups, const uint32_t *group_w,
                 const BhipEmLine *lines, uint64_t n_lines, uint32_t agree, uint32_t *group_node, uint64_t *own, uint64_t *clade, uint64_t info[8]) {
	(void)unused;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!own || !clade) return bh_set_error(BH_E_USAGE, "bh_taxa_host: no place for the counts");
	if (agree < 501 || agree > 1000) return bh_set_error(BH_E_USAGE, "bh_taxa_host: agree %u outside 501 .. 1000", agree);
	if (n_lines >= 0x80000000ull) return bh_set_error(BH_E_USAGE, "bh_taxa_host: %llu lines (limit 2^31 - 1)", (unsigned long long)n_lines);
	if (n_lines && (!lines || !group_w)) return bh_set_error(BH_E_USAGE, "bh_taxa_host: lines without a line array or without group weights");
	uint32_t *depth = malloc(((size_t)n_nodes + 1) * 4), *cnt = NULL, *touched = NULL;
	uint64_t *key = NULL;
	if (!depth) return bh_set_error(BH_E_OOM, "OOM:taxa");
	int rc = check_tree("bh_taxa_host", n_nodes, parent, n_headers, header_node, depth);
	if (rc) goto done;
	for (uint64_t i = 0; i < n_lines; ++i) {
		if (lines[i].group >= n_groups) { rc = bh_set_error(BH_E_USAGE, "bh_taxa_host: line %llu names group %u of %u", (unsigned long long)i, lines[i].group, n_groups); goto done; }
		if (lines[i].ref >= n_headers) { rc = bh_set_error(BH_E_USAGE, "bh_taxa_host: line %llu names header %u of %u", (unsigned long long)i, lines[i].ref, n_headers); goto done; }
	}
	memset(own, 0, (size_t)n_nodes * 8); memset(clade, 0, (size_t)n_nodes * 8);
	if (group_node) memset(group_node, 0xFF, (size_t)n_groups * 4);
	if (!n_lines) goto done;
	key = malloc(n_lines * 8); cnt = calloc(n_nodes, 4); touched = malloc((size_t)n_nodes * 4);
	if (!key || !cnt || !touched) { rc = bh_set_error(BH_E_OOM, "OOM:taxa"); goto done; }
	for (uint64_t i = 0; i < n_lines; ++i) key[i] = (uint64_t)lines[i].group << 32 | lines[i].ref;
	qsort(key, n_lines, 8, u64_cmp);
	uint64_t np = 0;
	for (uint64_t i = 0; i < n_lines; ++i) if (!i || key[i] != key[i - 1]) key[np++] = key[i];
	info[0] = np;
	for (uint64_t a = 0; a < np;) {
		uint64_t b = a;
		const uint32_t g = (uint32_t)(key[a] >> 32);
		while (b < np && (uint32_t)(key[b] >> 32) == g) ++b;
		const uint64_t n = b - a, t = (agree * n + 999) / 1000;
		/* the candidates below every ancestor; the deepest node that holds t of them (two of one depth cannot both: t > n / 2) */
		uint32_t nt = 0, best = 0;
		for (uint64_t i = a; i < b; ++i)
			for (uint32_t v = header_node[(uint32_t)key[i]];; v = parent[v]) { if (!cnt[v]++) touched[nt++] = v; if (!v) break; }
		for (uint32_t k = 0; k < nt; ++k) { const uint32_t v = touched[k]; if (cnt[v] >= t && depth[v] > depth[best]) best = v; cnt[v] = 0; }
		if (group_node) group_node[g] = best;
		own[best] += group_w[g];
		++info[1]; info[2] += group_w[g];
		if (depth[best] > info[4]) info[4] = depth[best];
		a = b;
	}
	info[3] = own[0];
	clade_of(n_nodes, parent, own, clade);
done:
	free(depth); free(key); free(cnt); free(touched);
	if (rc) memset(info, 0, 8 * sizeof(uint64_t));
	return rc;
}

int bh_taxa_rollup_host(void *unused, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, const uint64_t *header_count,
                        uint64_t *own, uint64_t *clade) {
	(void)unused;
	if (!own || !clade || (n_headers && !header_count)) return bh_set_error(BH_E_USAGE, "bh_taxa_rollup_host: no counts or no place for the sums");
	uint32_t *depth = malloc(((size_t)n_nodes + 1) * 4);
	if (!depth) return bh_set_error(BH_E_OOM, "OOM:taxa");
	const int rc = check_tree("bh_taxa_rollup_host", n_nodes, parent, n_headers, header_node, depth);
	free(depth);
	if (rc) return rc;
	memset(own, 0, (size_t)n_nodes * 8);
	for (uint32_t h = 0; h < n_headers; ++h) own[header_node[h]] += header_count[h];
	clade_of(n_nodes, parent, own, clade);
	return BH_OK;
}

/* ---- the columns and the tables ---- */
/* a sample's column: the nodes with an own count and the nodes with a rolled-up abundance count.  The clade sums follow from them (clade_of),
 * so a study keeps what its samples hit, not samples x nodes cells */
typedef struct { uint64_t n[2]; uint32_t *ix[2]; uint64_t *val[2]; } TaxaCol;      /* [0] own, [1] own_em */
struct BhTaxa {
	char *prefix; uint32_t agree;
	BhTaxaTree tree;
	uint32_t nCols;
	char **names; TaxaCol **cols;        /* per sample: column name; its counts, or NULL = the sample failed alone */
	int have_em;                         /* some sample came with its abundance counts: the abundance level files are written */
	int dead;
	bh_taxa_run_fn run; bh_taxa_rollup_fn rollup; void *ctx;
	uint64_t info[8]; int have_info;     /* of the last sample */
};

static void col_free(TaxaCol *c) { if (c) { for (int k = 0; k < 2; ++k) { free(c->ix[k]); free(c->val[k]); } free(c); } }
static int col_keep(TaxaCol *c, int k, const uint64_t *dense, uint32_t n_nodes) {
	uint64_t n = 0;
	for (uint32_t v = 0; v < n_nodes; ++v) n += dense[v] != 0;
	c->ix[k] = malloc((n + 1) * 4); c->val[k] = malloc((n + 1) * 8);
	if (!c->ix[k] || !c->val[k]) return bh_set_error(BH_E_OOM, "OOM:taxa");
	c->n[k] = 0;
	for (uint32_t v = 0; v < n_nodes; ++v) if (dense[v]) { c->ix[k][c->n[k]] = v; c->val[k][c->n[k]++] = dense[v]; }
	return BH_OK;
}
/* own (k = 0) or own_em (k = 1) of a column, and its subtree sums, as whole vectors; a failed sample: zeros */
static void col_dense(const BhTaxa *tx, const TaxaCol *c, int k, uint64_t *own, uint64_t *clade) {
	memset(own, 0, (size_t)tx->tree.n_nodes * 8);
	if (c) for (uint64_t i = 0; i < c->n[k]; ++i) own[c->ix[k][i]] = c->val[k][i];
	clade_of(tx->tree.n_nodes, tx->tree.parent, own, clade);
}

static int run_device(void *ctx, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, uint32_t n_groups, const uint32_t *group_w,
                      const BhipEmLine *lines, uint64_t n_lines, uint32_t agree, uint32_t *group_node, uint64_t *own, uint64_t *clade, uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "taxa: the groups are reduced on the device and rank 0 has no device handle");
	const int rc = bhip_taxa_run(ctx, n_nodes, parent, n_headers, header_node, n_groups, group_w, lines, n_lines, agree, group_node, own, clade, info);
	if (rc) return bh_set_error(rc == BHIP_E_ARG ? BH_E_USAGE : BH_E_DEVICE, "taxa: %s", bhip_last_error());
	return BH_OK;
}
static int rollup_device(void *ctx, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, const uint64_t *header_count,
                         uint64_t *own, uint64_t *clade) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "taxa: the counts are summed on the device and rank 0 has no device handle");
	const int rc = bhip_taxa_rollup(ctx, n_nodes, parent, n_headers, header_node, header_count, own, clade);
	if (rc) return bh_set_error(rc == BHIP_E_ARG ? BH_E_USAGE : BH_E_DEVICE, "taxa: %s", bhip_last_error());
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

int bh_taxa_check_opts(const char *tax_file, int agree_given, long long agree) {
	if (!tax_file) return bh_set_error(BH_E_USAGE, "ERROR: --taxa needs the taxonomy map: add -b <file>");
	if (agree_given && (agree < 501 || agree > 1000)) return bh_set_error(BH_E_USAGE, "ERROR: --taxa-agree takes the permille of a read's references that must agree (501 .. 1000)");
	return BH_OK;
}

int bh_taxa_open_heads(const char *prefix, uint32_t n_headers, const char *const *heads, const BhTax *map, int ncbi, uint32_t agree, BhTaxa **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_taxa_open: no place for the object");
	*out = NULL;
	if (!prefix) return bh_set_error(BH_E_USAGE, "bh_taxa_open: no prefix");
	if (agree < 501 || agree > 1000) return bh_set_error(BH_E_USAGE, "ERROR: --taxa-agree takes the permille of a read's references that must agree (501 .. 1000)");
	BhTaxa *tx = calloc(1, sizeof(*tx));
	if (!tx) return bh_set_error(BH_E_OOM, "OOM:taxa");
	tx->agree = agree;
	int rc = bh_taxa_tree(n_headers, heads, map, ncbi, &tx->tree);
	if (!rc && !(tx->prefix = strdup(prefix))) rc = bh_set_error(BH_E_OOM, "OOM:taxa");
	if (rc) { bh_taxa_close(tx); return rc; }
	*out = tx;
	return BH_OK;
}

int bh_taxa_open(const BhDb *db, const char *prefix, const BhTax *map, int ncbi, uint32_t agree, BhTaxa **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_taxa_open: no place for the object");
	*out = NULL;
	if (!db || !prefix || !db->numRefHeads || !db->refMap || !db->refHead) return bh_set_error(BH_E_USAGE, "bh_taxa_open: no database / no prefix");
	const char **head = calloc(db->numRefHeads, sizeof(*head));
	if (!head) return bh_set_error(BH_E_OOM, "OOM:taxa");
	for (uint32_t i = 0; i < db->origTotR; ++i) if (db->refMap[i] < db->numRefHeads) head[db->refMap[i]] = db->refHead[i];      /* (the numbers the report's sink uses) */
	const int rc = bh_taxa_open_heads(prefix, db->numRefHeads, head, map, ncbi, agree, out);
	free(head);
	return rc;
}

void bh_taxa_set_solver(BhTaxa *tx, bh_taxa_run_fn run, bh_taxa_rollup_fn rollup, void *ctx) { if (tx) { tx->run = run; tx->rollup = rollup; tx->ctx = ctx; } }
void bh_taxa_abort(BhTaxa *tx) { if (tx && !tx->dead) tx->dead = BH_E_DEVICE; }
const BhTaxaTree *bh_taxa_tree_of(const BhTaxa *tx) { return tx ? &tx->tree : NULL; }
void bh_taxa_dims(const BhTaxa *tx, uint32_t *n_columns, uint32_t *n_nodes) {
	if (n_columns) *n_columns = tx ? tx->nCols + 1 : 0;
	if (n_nodes) *n_nodes = tx ? tx->tree.n_nodes : 0;
}

static int new_column(BhTaxa *tx, const char *out_path) {
	char **nn = realloc(tx->names, ((size_t)tx->nCols + 1) * sizeof(*nn));
	if (nn) tx->names = nn;
	TaxaCol **nc = realloc(tx->cols, ((size_t)tx->nCols + 1) * sizeof(*nc));
	if (nc) tx->cols = nc;
	char *nm = sample_name(out_path ? out_path : "sample");
	if (!nn || !nc || !nm) { free(nm); return bh_set_error(BH_E_OOM, "OOM:taxa"); }
	tx->names[tx->nCols] = nm; tx->cols[tx->nCols] = NULL;
	++tx->nCols;
	return BH_OK;
}

int bh_taxa_sample_failed(BhTaxa *tx, const char *out_path) {
	if (!tx) return BH_OK;
	const int rc = new_column(tx, out_path);
	if (!rc) printf(" --> taxa: sample '%s' failed alone: its column is all zero\n", tx->names[tx->nCols - 1]);
	return rc;
}

int bh_taxa_sample(BhTaxa *tx, void *hh, const char *out_path, const uint32_t *reads, const BhipCovLine *lines, uint64_t n, const uint64_t *em_counts) {
	if (!tx) return bh_set_error(BH_E_USAGE, "bh_taxa_sample: no taxa object");
	if (tx->dead) return bh_set_error(tx->dead, "taxa was ended by an earlier error");
	if (n && (!reads || !lines)) return bh_set_error(BH_E_USAGE, "bh_taxa_sample: placements without their query numbers");
	int rc = new_column(tx, out_path);
	if (rc) return rc;
	const BhTaxaTree *T = &tx->tree;
	/* group = the unique query's number, W = its reads (the same on all its entries), ref = the entry's header: the abundance's groups */
	uint32_t nG = 0;
	for (uint64_t i = 0; i < n; ++i) if (reads[i] >= nG) nG = reads[i] + 1;
	uint32_t *gw = calloc((size_t)nG + 1, 4);
	BhipEmLine *ln = malloc((n + 1) * sizeof(*ln));
	uint64_t *col = calloc((size_t)T->n_nodes * 4, 8);      /* (the solvers' whole vectors: kept only where they hold a count) */
	TaxaCol *keep = calloc(1, sizeof(*keep));
	if (!gw || !ln || !col || !keep) { free(gw); free(ln); free(col); free(keep); tx->dead = BH_E_OOM; return bh_set_error(BH_E_OOM, "OOM:taxa"); }
	for (uint64_t i = 0; i < n; ++i) { gw[reads[i]] = lines[i].w & 0x7FFFFFFFu; ln[i].group = reads[i]; ln[i].ref = lines[i].ref; }
	uint64_t info[8] = {0};
	uint64_t *own = col, *clade = col + T->n_nodes, *own_em = col + 2 * (size_t)T->n_nodes, *clade_em = col + 3 * (size_t)T->n_nodes;
	rc = tx->run ? tx->run(tx->ctx, T->n_nodes, T->parent, T->n_headers, T->header_node, nG, gw, ln, n, tx->agree, NULL, own, clade, info)
	             : run_device(hh, T->n_nodes, T->parent, T->n_headers, T->header_node, nG, gw, ln, n, tx->agree, NULL, own, clade, info);
	free(gw); free(ln);
	if (!rc && em_counts) {
		rc = tx->rollup ? tx->rollup(tx->ctx, T->n_nodes, T->parent, T->n_headers, T->header_node, em_counts, own_em, clade_em)
		                : rollup_device(hh, T->n_nodes, T->parent, T->n_headers, T->header_node, em_counts, own_em, clade_em);
		tx->have_em = 1;
	}
	if (!rc) rc = col_keep(keep, 0, own, T->n_nodes);
	if (!rc) rc = col_keep(keep, 1, own_em, T->n_nodes);
	free(col);
	if (rc) { col_free(keep); tx->dead = rc; return rc; }      /* (any error of the solver is final: nothing will be written) */
	tx->cols[tx->nCols - 1] = keep;
	memcpy(tx->info, info, sizeof info); tx->have_info = 1;
	return BH_OK;
}

/* cols: [4][nCols + 1][n_nodes] -- own, clade, own_em, clade_em; column 0 = Dataset, the integer sum of the sample columns */
int bh_taxa_stats(BhTaxa *tx, uint64_t *cols) {
	if (!tx || !cols) return bh_set_error(BH_E_USAGE, "bh_taxa_stats: no taxa object");
	if (tx->dead) return bh_set_error(tx->dead, "taxa was ended by an earlier error");
	const size_t nN = tx->tree.n_nodes, nC = (size_t)tx->nCols + 1;
	memset(cols, 0, nN * nC * 4 * 8);
	for (uint32_t c = 0; c < tx->nCols; ++c)
		for (int k = 0; k < 2; ++k) {
			uint64_t *own = cols + ((size_t)2 * k * nC + c + 1) * nN, *clade = cols + (((size_t)2 * k + 1) * nC + c + 1) * nN;
			uint64_t *own0 = cols + (size_t)2 * k * nC * nN, *clade0 = cols + ((size_t)2 * k + 1) * nC * nN;
			col_dense(tx, tx->cols[c], k, own, clade);
			for (size_t v = 0; v < nN; ++v) { own0[v] += own[v]; clade0[v] += clade[v]; }
		}
	return BH_OK;
}

/* what the tables print: the nodes with a Dataset clade count (every printed row is one of them), and their cells of own, clade, clade_em */
typedef struct { uint32_t nR, nC; uint32_t *node; uint64_t *val[3]; } TaxaCells;      /* val[kind][c * nR + r] */
typedef struct { const char *s; uint32_t r; } Row;
static int row_cmp(const void *a, const void *b) { return strcmp(((const Row *)a)->s, ((const Row *)b)->s); }

/* one table under its temporary name: kind 0 = the rows with a Dataset own count, their own counts; 1 / 2 = the rows of `level`, clade / clade_em */
static int write_table(const BhTaxa *tx, const char *tmpn, const TaxaCells *T, int kind, uint32_t level, Row *rows) {
	uint32_t nR = 0;
	for (uint32_t r = 0; r < T->nR; ++r)
		if (kind ? tx->tree.depth[T->node[r]] == level : T->val[0][r] != 0) { rows[nR].s = tx->tree.name[T->node[r]]; rows[nR].r = r; ++nR; }
	qsort(rows, nR, sizeof(*rows), row_cmp);
	FILE *f = fopen(tmpn, "wb");
	if (!f) return bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", tmpn);
	setvbuf(f, NULL, _IOFBF, 1 << 20);
	fputs("#OTU ID\tDataset", f);
	for (uint32_t c = 0; c < tx->nCols; ++c) fprintf(f, "\t%s", tx->names[c]);
	fputc('\n', f);
	for (uint32_t r = 0; r < nR; ++r) {
		fputs(rows[r].s, f);
		for (uint32_t c = 0; c < T->nC; ++c) {
			const uint64_t x = T->val[kind][(size_t)c * T->nR + rows[r].r];
			if (kind == 2) fprintf(f, "\t%.4f", (double)x / 1073741824.0); else fprintf(f, "\t%llu", (unsigned long long)x);
		}
		fputc('\n', f);
	}
	if (ferror(f) | fclose(f)) { (void)unlink(tmpn); return bh_set_error(BH_E_IO, "ERROR: write failed: %s", tmpn); }
	return BH_OK;
}

/* the cells of the printed rows, sample by sample: a few whole vectors at a time, never samples x nodes */
static int cells_of(const BhTaxa *tx, TaxaCells *T, uint32_t *deepest) {
	const size_t nN = tx->tree.n_nodes;
	memset(T, 0, sizeof *T);
	T->nC = tx->nCols + 1;
	uint64_t *own = malloc(nN * 8), *clade = malloc(nN * 8), *sum = calloc(nN, 8);
	int rc = own && clade && sum ? BH_OK : bh_set_error(BH_E_OOM, "OOM:taxa");
	if (!rc) {
		for (uint32_t c = 0; c < tx->nCols; ++c) if (tx->cols[c]) for (uint64_t i = 0; i < tx->cols[c]->n[0]; ++i) sum[tx->cols[c]->ix[0][i]] += tx->cols[c]->val[0][i];
		clade_of(tx->tree.n_nodes, tx->tree.parent, sum, clade);
		for (size_t v = 0; v < nN; ++v) if (clade[v]) { ++T->nR; if (tx->tree.depth[v] > *deepest) *deepest = tx->tree.depth[v]; }
		T->node = malloc(((size_t)T->nR + 1) * 4);
		for (int k = 0; k < 3; ++k) T->val[k] = calloc((size_t)T->nR * T->nC + 1, 8);
		if (!T->node || !T->val[0] || !T->val[1] || !T->val[2]) rc = bh_set_error(BH_E_OOM, "OOM:taxa");
	}
	if (!rc) {
		uint32_t r = 0;
		for (size_t v = 0; v < nN; ++v) if (clade[v]) T->node[r++] = (uint32_t)v;
		for (uint32_t c = 0; c < tx->nCols; ++c)
			for (int k = 0; k < 2; ++k) {
				if (k && !tx->have_em) continue;
				col_dense(tx, tx->cols[c], k, own, clade);
				for (r = 0; r < T->nR; ++r) {
					const uint32_t v = T->node[r];
					if (!k) { T->val[0][(size_t)(c + 1) * T->nR + r] = own[v]; T->val[0][r] += own[v]; }
					T->val[1 + k][(size_t)(c + 1) * T->nR + r] = clade[v]; T->val[1 + k][r] += clade[v];
				}
			}
	}
	free(own); free(clade); free(sum);
	return rc;
}

int bh_taxa_write(BhTaxa *tx, uint32_t *n_levels, uint32_t *n_em_levels) {
	if (n_levels) *n_levels = 0;
	if (n_em_levels) *n_em_levels = 0;
	if (!tx) return bh_set_error(BH_E_USAGE, "bh_taxa_write: no taxa object");
	if (tx->dead) return bh_set_error(tx->dead, "taxa was ended by an earlier error: no table is written");
	TaxaCells T;
	uint32_t nF = 0, D = 0;
	int rc = cells_of(tx, &T, &D);
	Row *rows = rc ? NULL : malloc(((size_t)T.nR + 1) * sizeof(*rows));
	char **tmpn = NULL, **finn = NULL;
	if (!rc && !rows) rc = bh_set_error(BH_E_OOM, "OOM:taxa");
	if (!rc) {
		const uint32_t Dem = tx->have_em ? D : 0, total = 1 + D + Dem;      /* (the abundance level files: the same rows, level by level) */
		tmpn = calloc(total, sizeof(*tmpn)); finn = calloc(total, sizeof(*finn));
		if (!tmpn || !finn) rc = bh_set_error(BH_E_OOM, "OOM:taxa");
		/* every table under its temporary name first; renamed together when all of them stand */
		for (uint32_t k = 0; !rc && k < total; ++k) {
			const int kind = !k ? 0 : k > D ? 2 : 1; const uint32_t level = kind == 2 ? k - D : k;
			const int ok = !k ? asprintf(&finn[k], "%staxa.txt", tx->prefix) : asprintf(&finn[k], kind == 2 ? "%staxa_abundance_L%u.txt" : "%staxa_L%u.txt", tx->prefix, level);
			if (ok < 0) { finn[k] = NULL; rc = bh_set_error(BH_E_OOM, "OOM:taxa"); break; }
			if (asprintf(&tmpn[k], "%s.tmp%ld", finn[k], (long)getpid()) < 0) { tmpn[k] = NULL; rc = bh_set_error(BH_E_OOM, "OOM:taxa"); break; }
			rc = write_table(tx, tmpn[k], &T, kind, level, rows);
			if (!rc) nF = k + 1;
		}
		for (uint32_t k = 0; !rc && k < nF; ++k) if (rename(tmpn[k], finn[k])) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", tmpn[k], finn[k]);
		if (rc) for (uint32_t k = 0; k < nF; ++k) (void)unlink(tmpn[k]);
		for (uint32_t k = 0; tmpn && finn && k < total; ++k) { free(tmpn[k]); free(finn[k]); }
		if (!rc) { if (n_levels) *n_levels = D; if (n_em_levels) *n_em_levels = Dem; }
	}
	free(T.node); for (int k = 0; k < 3; ++k) free(T.val[k]);
	free(rows); free(tmpn); free(finn);
	return rc;
}

/* one line on standard output: the last sample's figures (bhip_taxa_run's info) */
void bh_taxa_print_info(BhTaxa *tx) {
	if (!tx || !tx->have_info || tx->dead) return;
	printf("Taxa: %lu reads, %lu groups, %lu pairs, %lu reads at the root, deepest level %lu, device %.3f ms\n", (unsigned long)tx->info[2], (unsigned long)tx->info[1],
	       (unsigned long)tx->info[0], (unsigned long)tx->info[3], (unsigned long)tx->info[4], tx->info[5] / 1e3);
}

void bh_taxa_last_info(const BhTaxa *tx, uint64_t info[8]) {
	if (!info) return;
	if (tx && tx->have_info) memcpy(info, tx->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t));
}

void bh_taxa_close(BhTaxa *tx) {
	if (!tx) return;
	for (uint32_t c = 0; c < tx->nCols; ++c) { free(tx->names[c]); col_free(tx->cols[c]); }
	free(tx->names); free(tx->cols); free(tx->prefix);
	bh_taxa_tree_free(&tx->tree);
	free(tx);
}
