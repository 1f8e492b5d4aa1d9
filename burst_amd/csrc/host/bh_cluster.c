/* bh_cluster.c -- greedy centroid clusters of the reads of a query file from the lines it prints against itself
 * (burst_hip --cluster, host.Session(cluster=...)).
 *
 * No reference counterpart: the reference's README lists clustering "as an output mode" as planned and names the recipe (the queries as
 * their own references in FORAGE, clusters picked from that hit graph).  The definition is bhip_cluster_run's (include/burst_hip.h,
 * DESIGN.md section 7e): a pure function of the printed lines.  The greedy order is resolved on the device; this file holds what is left:
 * the table of read names (hash, `;size=N` suffix, duplicate check), the lines turned into edges, the two tables and the `Clusters:`
 * line -- and bh_cluster_host, the definition once more in plain sequential C, which the tests without a device and the yardstick use. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define NO_NODE 0xFFFFFFFFu

struct BhCluster {
	char *prefix; int use_sizes, dead;
	bh_cluster_solver_fn fn; void *ctx;
	uint32_t n;                          /* reads (nodes), in file order */
	char *blob; char **name;             /* copies of the names */
	uint32_t *w;                         /* weights */
	uint32_t *tab; uint64_t mask;        /* open-addressing hash of the names: node + 1, 0 = free */
	BhipClusterEdge *edges; uint64_t nE, capE;
	uint64_t lines, foreign;
	uint32_t *centroid, *edits; int solved;
	uint64_t info[8];
};

/* ---- the definition in plain sequential C ---- */
typedef struct { uint64_t key; uint32_t edits; } HostEdge;
static int hedge_cmp(const void *a, const void *b) {
	const HostEdge *x = a, *y = b;
	if (x->key != y->key) return x->key < y->key ? -1 : 1;
	return (x->edits > y->edits) - (x->edits < y->edits);
}
static int u64_cmp(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return (x > y) - (x < y); }

int bh_cluster_host(void *unused, uint32_t n_nodes, const uint32_t *weights, const BhipClusterEdge *edges, uint64_t n_edges, uint32_t *centroid, uint32_t *edits,
                    uint64_t info[8]) {
	(void)unused;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (n_nodes && (!weights || !centroid || !edits)) return bh_set_error(BH_E_USAGE, "bh_cluster_host: nodes without weights or without a place for the result");
	if (n_edges && !edges) return bh_set_error(BH_E_USAGE, "bh_cluster_host: edges without an edge array");
	if (n_nodes == NO_NODE || n_edges >= ((uint64_t)1 << 32)) return bh_set_error(BH_E_USAGE, "bh_cluster_host: %u nodes, %llu edges (fewer than 2^32 - 1 nodes, fewer than 2^32 edges)", n_nodes, (unsigned long long)n_edges);
	for (uint64_t i = 0; i < n_edges; ++i) if (edges[i].q >= n_nodes || edges[i].r >= n_nodes)
		return bh_set_error(BH_E_USAGE, "bh_cluster_host: edge %llu names node %u -> %u of %u", (unsigned long long)i, edges[i].q, edges[i].r, n_nodes);
	info[5] = n_edges; info[6] = n_nodes;
	if (!n_nodes) return BH_OK;
	uint64_t *ord = malloc((size_t)n_nodes * 8);
	uint32_t *rank = malloc((size_t)n_nodes * 4), *order = malloc((size_t)n_nodes * 4);
	uint8_t *is_centroid = calloc(n_nodes, 1);
	HostEdge *he = malloc((n_edges + 1) * sizeof(*he));
	uint64_t *off = calloc((size_t)n_nodes + 1, 8);
	int rc = BH_OK;
	if (!ord || !rank || !order || !is_centroid || !he || !off) { rc = bh_set_error(BH_E_OOM, "OOM:cluster"); goto done; }
	/* priority: the larger weight first, the smaller number among equals */
	for (uint32_t i = 0; i < n_nodes; ++i) ord[i] = (uint64_t)(~weights[i]) << 32 | i;
	qsort(ord, n_nodes, 8, u64_cmp);
	for (uint32_t p = 0; p < n_nodes; ++p) { order[p] = (uint32_t)ord[p]; rank[order[p]] = p; }
	/* the edges that can matter, each (q, r) once with its smallest edits, the targets of a read ascending in priority */
	uint64_t nk = 0, kept = 0;
	for (uint64_t i = 0; i < n_edges; ++i) {
		const uint32_t q = edges[i].q, r = edges[i].r;
		if (q == r || rank[r] >= rank[q]) continue;
		he[nk].key = (uint64_t)q << 32 | rank[r]; he[nk].edits = edges[i].edits; ++nk;
	}
	qsort(he, nk, sizeof(*he), hedge_cmp);
	for (uint64_t i = 0; i < nk; ++i) if (!i || he[i].key != he[i - 1].key) he[kept++] = he[i];      /* (the first of equal keys holds the smallest edits) */
	for (uint64_t i = 0; i < kept; ++i) ++off[(he[i].key >> 32) + 1];
	for (uint32_t q = 0; q < n_nodes; ++q) off[q + 1] += off[q];
	/* the reads in priority order */
	uint64_t n_centroids = 0;
	for (uint32_t p = 0; p < n_nodes; ++p) {
		const uint32_t q = order[p];
		uint64_t best = ~(uint64_t)0;
		for (uint64_t i = off[q]; i < off[q + 1]; ++i) {
			const uint32_t t = (uint32_t)he[i].key;
			if (!is_centroid[t]) continue;
			const uint64_t c = (uint64_t)he[i].edits << 32 | t;
			if (c < best) best = c;
		}
		if (best == ~(uint64_t)0) { is_centroid[p] = 1; centroid[q] = q; edits[q] = 0; ++n_centroids; }
		else { centroid[q] = order[(uint32_t)best]; edits[q] = (uint32_t)(best >> 32); }
	}
	info[1] = kept; info[2] = n_centroids;
done:
	free(ord); free(rank); free(order); free(is_centroid); free(he); free(off);
	return rc;
}

/* the device: ctx = the handle */
static int solve_device(void *ctx, uint32_t n_nodes, const uint32_t *weights, const BhipClusterEdge *edges, uint64_t n_edges, uint32_t *centroid, uint32_t *edits,
                        uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "cluster: the greedy order is resolved on the device and rank 0 has no device handle");
	const int rc = bhip_cluster_run(ctx, n_nodes, weights, edges, n_edges, centroid, edits);
	if (rc) return bh_set_error(rc == BHIP_E_ARG ? BH_E_USAGE : rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "cluster: %s", bhip_last_error());
	(void)bhip_cluster_info(ctx, info);
	return BH_OK;
}

int bh_cluster_open(const char *prefix, int use_sizes, BhCluster **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_cluster_open: no place for the object");
	*out = NULL;
	if (!prefix) return bh_set_error(BH_E_USAGE, "bh_cluster_open: no prefix");
	BhCluster *cl = calloc(1, sizeof(*cl));
	if (!cl) return bh_set_error(BH_E_OOM, "OOM:cluster");
	cl->use_sizes = use_sizes != 0;
	if (!(cl->prefix = strdup(prefix))) { free(cl); return bh_set_error(BH_E_OOM, "OOM:cluster"); }
	*out = cl;
	return BH_OK;
}
void bh_cluster_set_solver(BhCluster *cl, bh_cluster_solver_fn fn, void *ctx) { if (cl) { cl->fn = fn; cl->ctx = ctx; } }
void bh_cluster_abort(BhCluster *cl) { if (cl && !cl->dead) cl->dead = BH_E_DEVICE; }

static void drop_names(BhCluster *cl) {
	free(cl->blob); free(cl->name); free(cl->w); free(cl->tab); free(cl->centroid); free(cl->edits);
	cl->blob = NULL; cl->name = NULL; cl->w = NULL; cl->tab = NULL; cl->centroid = cl->edits = NULL;
	cl->n = 0; cl->nE = 0; cl->lines = cl->foreign = 0; cl->solved = 0;
	memset(cl->info, 0, sizeof cl->info);
}
static uint64_t name_hash(const char *s, size_t len) {
	uint64_t h = 0xcbf29ce484222325ull;
	for (size_t i = 0; i < len; ++i) { h ^= (uint8_t)s[i]; h *= 0x100000001b3ull; }
	return h ^ h >> 29;
}
/* the N of a trailing `;size=N` or `;size=N;`: 0 = no such suffix, -1 = a suffix whose number is not 1 .. 2^32 - 1 */
static int64_t size_suffix(const char *s) {
	size_t e = strlen(s);
	if (e && s[e - 1] == ';') --e;
	size_t d = e;
	while (d && s[d - 1] >= '0' && s[d - 1] <= '9') --d;
	if (d == e || d < 6 || memcmp(s + d - 6, ";size=", 6)) return 0;
	uint64_t v = 0;
	for (size_t i = d; i < e; ++i) { v = v * 10 + (uint64_t)(s[i] - '0'); if (v > 0xFFFFFFFFull) return -1; }
	return v ? (int64_t)v : -1;
}
static uint32_t lookup(const BhCluster *cl, const char *s, size_t len) {
	if (!cl->tab) return NO_NODE;
	for (uint64_t h = name_hash(s, len) & cl->mask;; h = (h + 1) & cl->mask) {
		const uint32_t v = cl->tab[h];
		if (!v) return NO_NODE;
		const char *o = cl->name[v - 1];
		if (!strncmp(o, s, len) && !o[len]) return v - 1;
	}
}

int bh_cluster_names(BhCluster *cl, const char *const *names, uint32_t n) { return bh_cluster_names_as(cl, names, n, "--cluster", "--cluster-sizes"); }
uint32_t bh_cluster_find(const BhCluster *cl, const char *s, size_t len) { return cl ? lookup(cl, s, len) : NO_NODE; }
const char *bh_cluster_name(const BhCluster *cl, uint32_t node) { return cl && node < cl->n ? cl->name[node] : NULL; }
const uint32_t *bh_cluster_weights(const BhCluster *cl) { return cl ? cl->w : NULL; }

/* (the same under another flag's name: bh_chimera.c keeps its reads in such a table) */
int bh_cluster_names_as(BhCluster *cl, const char *const *names, uint32_t n, const char *flag, const char *sizes_flag) {
	if (!cl) return bh_set_error(BH_E_USAGE, "bh_cluster_names: no cluster object");
	if (cl->dead) return bh_set_error(cl->dead, "clustering was ended by an earlier error");
	if (n && !names) return bh_set_error(BH_E_USAGE, "bh_cluster_names: no names");
	if (n == NO_NODE) return bh_set_error(BH_E_USAGE, "bh_cluster_names: fewer than 2^32 - 1 reads");
	drop_names(cl);
	size_t tot = 0;
	for (uint32_t i = 0; i < n; ++i) tot += strlen(names[i] ? names[i] : "") + 1;
	uint64_t ts = 16;
	while (ts < (uint64_t)n * 2 + 2) ts *= 2;
	cl->blob = malloc(tot + 1); cl->name = malloc(((size_t)n + 1) * sizeof(*cl->name)); cl->w = malloc(((size_t)n + 1) * 4);
	cl->tab = calloc(ts, 4); cl->mask = ts - 1;
	cl->centroid = malloc(((size_t)n + 1) * 4); cl->edits = malloc(((size_t)n + 1) * 4);
	if (!cl->blob || !cl->name || !cl->w || !cl->tab || !cl->centroid || !cl->edits) { drop_names(cl); cl->dead = BH_E_OOM; return bh_set_error(BH_E_OOM, "OOM:cluster"); }
	cl->n = n;
	char *p = cl->blob;
	for (uint32_t i = 0; i < n; ++i) {
		const char *s = names[i] ? names[i] : "";
		const size_t len = strlen(s);
		memcpy(p, s, len + 1); cl->name[i] = p; p += len + 1;
		const uint32_t other = lookup(cl, s, len);
		if (other != NO_NODE) {
			cl->dead = BH_E_USAGE;
			return bh_set_error(BH_E_USAGE, "ERROR: %s needs every read named once: reads %u and %u of the query file are both named '%s'", flag, other + 1, i + 1, s);
		}
		uint64_t h = name_hash(s, len) & cl->mask;
		while (cl->tab[h]) h = (h + 1) & cl->mask;
		cl->tab[h] = i + 1;
		cl->w[i] = 1;
		if (cl->use_sizes) {
			const int64_t v = size_suffix(s);
			if (v < 0) { cl->dead = BH_E_USAGE; return bh_set_error(BH_E_USAGE, "ERROR: %s: the size of read '%s' is not a number 1 .. 4294967295", sizes_flag, s); }
			if (v) cl->w[i] = (uint32_t)v;
		}
	}
	return BH_OK;
}

static int push_edge(BhCluster *cl, uint32_t q, uint32_t r, uint32_t edits) {
	if (cl->nE == cl->capE) {
		const uint64_t nc = cl->capE ? cl->capE * 2 : 4096;
		BhipClusterEdge *ne = realloc(cl->edges, nc * sizeof(*ne));
		if (!ne) { cl->dead = BH_E_OOM; return bh_set_error(BH_E_OOM, "OOM:cluster"); }
		cl->edges = ne; cl->capE = nc;
	}
	if (cl->nE >= 0xFFFFFFFFull) { cl->dead = BH_E_USAGE; return bh_set_error(BH_E_USAGE, "ERROR: --cluster takes fewer than 2^32 lines between reads"); }
	const BhipClusterEdge e = {q, r, edits};
	cl->edges[cl->nE++] = e;
	return BH_OK;
}

/* `count` printed lines of read q whose column 2 is ref_name and whose column 11 is edits */
int bh_cluster_line(BhCluster *cl, uint32_t q, const char *ref_name, size_t ref_len, uint32_t edits, uint64_t count) {
	if (!cl || !ref_name) return bh_set_error(BH_E_USAGE, "bh_cluster_line: no cluster object or no name");
	if (cl->dead) return bh_set_error(cl->dead, "clustering was ended by an earlier error");
	if (q >= cl->n) return bh_set_error(BH_E_USAGE, "bh_cluster_line: read %u of %u", q, cl->n);
	cl->lines += count; cl->solved = 0;
	const uint32_t r = lookup(cl, ref_name, ref_len);
	if (r == NO_NODE) { cl->foreign += count; return BH_OK; }
	if (r == q) return BH_OK;
	return push_edge(cl, q, r, edits);
}

/* the lines of a .b6 file: columns 1, 2 and 11 */
int bh_cluster_add_b6(BhCluster *cl, const char *path) {
	if (!cl || !path) return bh_set_error(BH_E_USAGE, "bh_cluster_add_b6: no cluster object or no file");
	if (cl->dead) return bh_set_error(cl->dead, "clustering was ended by an earlier error");
	FILE *f = fopen(path, "rb");
	if (!f) return bh_set_error(BH_E_IO, "ERROR: Cannot open %s", path);
	char *line = NULL; size_t cap = 0; ssize_t len; uint64_t no = 0; int rc = BH_OK;
	while (!rc && (len = getline(&line, &cap, f)) >= 0) {
		++no;
		while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
		if (!len) continue;
		const char *col[12]; size_t cl_len[12]; int nc = 0;
		for (char *p = line; nc < 12;) {
			char *t = strchr(p, '\t');
			col[nc] = p; cl_len[nc] = t ? (size_t)(t - p) : strlen(p); ++nc;
			if (!t) break;
			p = t + 1;
		}
		if (nc < 11) { rc = bh_set_error(BH_E_USAGE, "ERROR: %s line %llu has fewer than 11 columns", path, (unsigned long long)no); break; }
		const uint32_t q = lookup(cl, col[0], cl_len[0]);
		if (q == NO_NODE) { rc = bh_set_error(BH_E_USAGE, "ERROR: %s line %llu: column 1 names no read of the query file", path, (unsigned long long)no); break; }
		char *end = NULL; const unsigned long long ed = strtoull(col[10], &end, 10);
		if (end == col[10] || (size_t)(end - col[10]) != cl_len[10] || ed > 0xFFFFFFFFull) { rc = bh_set_error(BH_E_USAGE, "ERROR: %s line %llu: column 11 is not a number of edits", path, (unsigned long long)no); break; }
		rc = bh_cluster_line(cl, q, col[1], cl_len[1], (uint32_t)ed, 1);
	}
	free(line); fclose(f);
	if (rc && !cl->dead) cl->dead = rc;
	return rc;
}

int bh_cluster_solve(BhCluster *cl, void *hh) {
	if (!cl) return bh_set_error(BH_E_USAGE, "bh_cluster_solve: no cluster object");
	if (cl->dead) return bh_set_error(cl->dead, "clustering was ended by an earlier error");
	uint64_t info[8] = {0};
	const int rc = cl->fn ? cl->fn(cl->ctx, cl->n, cl->w, cl->edges, cl->nE, cl->centroid, cl->edits, info)
	                      : solve_device(hh, cl->n, cl->w, cl->edges, cl->nE, cl->centroid, cl->edits, info);
	if (rc) { cl->dead = rc; return rc; }      /* (any error of the solver is final: nothing will be written) */
	memcpy(cl->info, info, sizeof info);
	cl->solved = 1;
	return BH_OK;
}

typedef struct { const char *p; uint64_t j; } HeadAt;
static int headat_cmp(const void *a, const void *b) {
	const HeadAt *x = a, *y = b;
	if (x->p != y->p) return (uintptr_t)x->p < (uintptr_t)y->p ? -1 : 1;
	return (x->j > y->j) - (x->j < y->j);
}

/* the reads of Q in file order (their names lie in the file's text in that order): names[k] = the k-th read's, node_of[j] = the place of
 * heads[j]; both with room for totQ + 1 */
int bh_cluster_file_order(const BhQueries *Q, const char **names, uint32_t *node_of) {
	const uint64_t n = Q->totQ;
	HeadAt *at = malloc((n + 1) * sizeof(*at));
	if (!at) return bh_set_error(BH_E_OOM, "OOM:cluster");
	for (uint64_t j = 0; j < n; ++j) { at[j].p = Q->heads[j]; at[j].j = j; }
	qsort(at, n, sizeof(*at), headat_cmp);
	for (uint64_t k = 0; k < n; ++k) { names[k] = at[k].p; node_of[at[k].j] = (uint32_t)k; }
	free(at);
	return BH_OK;
}

/* a finished run: the reads of Q in file order (their names lie in the file's text in that order), the lines from the report's sink
 * (filled with want_re), solved on `hh` */
int bh_cluster_sample(BhCluster *cl, void *hh, const BhDb *db, const BhQueries *Q, const BhPlaceSink *sink) {
	if (!cl || !db || !Q || !sink) return bh_set_error(BH_E_USAGE, "bh_cluster_sample: no cluster object / database / queries / lines");
	if (cl->dead) return bh_set_error(cl->dead, "clustering was ended by an earlier error");
	if (sink->n && (!sink->uq || !sink->re)) return bh_set_error(BH_E_USAGE, "bh_cluster_sample: the report's lines came without their references and edits");
	if (Q->totQ >= NO_NODE) return bh_set_error(BH_E_USAGE, "ERROR: --cluster takes fewer than 2^32 - 1 reads");
	const uint64_t n = Q->totQ;
	const char **names = malloc((n + 1) * sizeof(*names));
	uint32_t *node_of = malloc((n + 1) * 4);
	int rc = names && node_of ? BH_OK : bh_set_error(BH_E_OOM, "OOM:cluster");
	if (!rc) rc = bh_cluster_file_order(Q, names, node_of);
	if (!rc) rc = bh_cluster_names(cl, names, (uint32_t)n);
	for (uint64_t k = 0; !rc && k < sink->n; ++k) {
		const uint64_t i = sink->uq[k];
		if (i >= Q->numUniq) { rc = bh_set_error(BH_E_INTERNAL, "bh_cluster_sample: entry %llu names query %llu of %llu", (unsigned long long)k, (unsigned long long)i, (unsigned long long)Q->numUniq); break; }
		const char *rn = db->refHead[sink->re[k] >> 32];
		const size_t rl = strlen(rn);
		for (uint64_t j = Q->offset[i]; !rc && j < Q->offset[i + 1]; ++j) rc = bh_cluster_line(cl, node_of[j], rn, rl, (uint32_t)sink->re[k], 1);
	}
	free(names); free(node_of);
	if (rc) { if (!cl->dead) cl->dead = rc; return rc; }
	return bh_cluster_solve(cl, hh);
}

uint32_t bh_cluster_reads(const BhCluster *cl) { return cl ? cl->n : 0; }
int bh_cluster_result(const BhCluster *cl, uint32_t *centroid, uint32_t *edits, uint32_t *weights) {
	if (!cl || !cl->solved) return bh_set_error(BH_E_USAGE, "bh_cluster_result: nothing has been clustered");
	if (centroid) memcpy(centroid, cl->centroid, (size_t)cl->n * 4);
	if (edits) memcpy(edits, cl->edits, (size_t)cl->n * 4);
	if (weights) memcpy(weights, cl->w, (size_t)cl->n * 4);
	return BH_OK;
}
void bh_cluster_last_info(const BhCluster *cl, uint64_t info[8], uint64_t *lines, uint64_t *foreign) {
	if (info) { if (cl && cl->solved) memcpy(info, cl->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t)); }
	if (lines) *lines = cl ? cl->lines : 0;
	if (foreign) *foreign = cl ? cl->foreign : 0;
}

/* PREFIXclusters.txt and PREFIXcluster_sizes.txt, both under temporary names first, renamed together */
int bh_cluster_write(BhCluster *cl) {
	if (!cl) return bh_set_error(BH_E_USAGE, "bh_cluster_write: no cluster object");
	if (cl->dead) return bh_set_error(cl->dead, "clustering was ended by an earlier error: no table is written");
	if (!cl->solved) return bh_set_error(BH_E_USAGE, "bh_cluster_write: nothing has been clustered");
	const uint32_t n = cl->n;
	uint64_t *reads = calloc((size_t)n + 1, 8), *wsum = calloc((size_t)n + 1, 8), *ord = malloc(((size_t)n + 1) * 8);
	char *fin[2] = {NULL, NULL}, *tmp[2] = {NULL, NULL};
	int rc = reads && wsum && ord ? BH_OK : bh_set_error(BH_E_OOM, "OOM:cluster");
	if (!rc && (asprintf(&fin[0], "%sclusters.txt", cl->prefix) < 0 || asprintf(&tmp[0], "%sclusters.txt.tmp%ld", cl->prefix, (long)getpid()) < 0 ||
	            asprintf(&fin[1], "%scluster_sizes.txt", cl->prefix) < 0 || asprintf(&tmp[1], "%scluster_sizes.txt.tmp%ld", cl->prefix, (long)getpid()) < 0))
		rc = bh_set_error(BH_E_OOM, "OOM:cluster");
	int made = 0;
	if (!rc) {
		FILE *f = fopen(tmp[0], "wb");
		if (!f) rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", tmp[0]);
		else {
			made = 1;
			setvbuf(f, NULL, _IOFBF, 1 << 20);
			fputs("#Read\tCentroid\tRole\tEdits\tWeight\n", f);
			for (uint32_t i = 0; i < n; ++i) {
				const uint32_t c = cl->centroid[i];
				fprintf(f, "%s\t%s\t%c\t%u\t%u\n", cl->name[i], cl->name[c], c == i ? 'C' : 'M', cl->edits[i], cl->w[i]);
				++reads[c]; wsum[c] += cl->w[i];
			}
			if (ferror(f) | fclose(f)) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", tmp[0]);
		}
	}
	if (!rc) {
		uint32_t nc = 0;
		for (uint32_t i = 0; i < n; ++i) if (cl->centroid[i] == i) ord[nc++] = (uint64_t)(~cl->w[i]) << 32 | i;      /* priority order */
		qsort(ord, nc, 8, u64_cmp);
		FILE *f = fopen(tmp[1], "wb");
		if (!f) rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", tmp[1]);
		else {
			made = 2;
			setvbuf(f, NULL, _IOFBF, 1 << 20);
			fputs("#OTU ID\tReads\tWeight\n", f);
			for (uint32_t k = 0; k < nc; ++k) { const uint32_t c = (uint32_t)ord[k]; fprintf(f, "%s\t%llu\t%llu\n", cl->name[c], (unsigned long long)reads[c], (unsigned long long)wsum[c]); }
			if (ferror(f) | fclose(f)) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", tmp[1]);
		}
	}
	if (!rc && (rename(tmp[0], fin[0]) || rename(tmp[1], fin[1]))) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s / %s to %s / %s", tmp[0], tmp[1], fin[0], fin[1]);
	if (rc) { if (made >= 1) (void)unlink(tmp[0]); if (made >= 2) (void)unlink(tmp[1]); }
	free(reads); free(wsum); free(ord);
	for (int k = 0; k < 2; ++k) { free(fin[k]); free(tmp[k]); }
	return rc;
}

/* one line on standard output */
void bh_cluster_print_info(BhCluster *cl) {
	if (!cl || !cl->solved || cl->dead) return;
	printf("Clusters: %u reads, %llu lines, %llu foreign lines, %llu edges kept, %llu centroids, %llu rounds, device %.3f ms\n", cl->n, (unsigned long long)cl->lines,
	       (unsigned long long)cl->foreign, (unsigned long long)cl->info[1], (unsigned long long)cl->info[2], (unsigned long long)cl->info[0], cl->info[3] / 1e3);
}

void bh_cluster_close(BhCluster *cl) {
	if (!cl) return;
	drop_names(cl);
	free(cl->edges); free(cl->prefix);
	free(cl);
}
