/* bh_vcf.c -- VCF output beside the .b6: SNVs and indel alleles per sample from the alignment paths of the printed lines (burst_hip --vcf,
 * host.Session(vcf=True)).
 *
 * No reference counterpart.  The alleles are bhip_alleles_run's (include/burst_hip.h "Indel alleles"), the SNVs a
 * subset of bhip_pile_run's sites.  A converter from the variants table cannot write these records: the table has Ins and Del counts but
 * no alleles, and a deletion's REF needs the deleted reference letters, which sit packed on the device.  The paths come from the tracer
 * the --cigar columns use (one more collector beside --sam's, --variants' and --consensus': nothing is traced twice), the lines of a
 * sample are kept by bh_pile.c's collector (bh_pile_open_lines: the same lines, weights and unique-read rule as --variants), the sites and
 * alleles from ONE bhip_pile_run and ONE bhip_alleles_run per sample on the reporting rank's handle, and this file holds what is left: the
 * merge of the two ordered lists into records, the file -- and bh_alleles_host, the definition once more in plain sequential C (one
 * record per allele run, sorted and counted), which the tests without a device and the yardstick use. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static const char VCF_LETTERS[] = "NACGTNNNNNNNNNNN";      /* VCF allows nothing but A C G T N in REF and ALT */

struct BhVcf {
	const BhDb *db;
	uint32_t nH, minDepth, minAlt; char **sn; uint32_t *len; int have_len;
	BhPile *lines;                     /* the sample being collected (bh_pile.c's collector) */
	int dead;
	bh_pile_solver_fn pile_fn; void *pile_ctx;
	bh_alleles_solver_fn al_fn; void *al_ctx;
	uint64_t info[12]; int have_info;  /* of the last sample that was written */
	BhVcfStudy *study;                 /* bh_vcf_set_study: NULL, or the study VCF every sample's (1, 1) lists are handed to (bh_vcfstudy.c) */
};

/* ---- the definition in plain C ---- */
typedef struct { uint64_t k1, k2, line; uint32_t w, col; } AlRec;      /* col: the 0-based lane column behind the anchor's */
static int rec_cmp(const void *a, const void *b) {
	const AlRec *x = a, *y = b;
	if (x->k1 != y->k1) return x->k1 < y->k1 ? -1 : 1;
	if (x->k2 != y->k2) return x->k2 < y->k2 ? -1 : 1;
	return (x->line > y->line) - (x->line < y->line);
}
static uint8_t ref_code(const BhPileRefs *R, const uint64_t *clump_off, uint32_t refIx, uint32_t col0) {
	const uint8_t b = R->packed[(clump_off[refIx >> 4] + (col0 >> 1)) * 16 + (refIx & 15u)];
	return (col0 & 1u) ? b >> 4 : b & 15u;
}

int bh_alleles_host(void *refs, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                    const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, uint32_t min_alt, BhipAllele *alleles, uint64_t cap, uint64_t *n_alleles,
                    uint8_t *codes, uint64_t code_cap, uint64_t *n_codes, uint64_t info[8]) {
	const BhPileRefs *R = refs;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if (!R || !R->packed || !R->clump_len || !n_alleles || !n_codes || (n_lines && (!lines || !q_codes || !q_off)) || (n_ops && !ops) || (cap && !alleles) || (code_cap && !codes))
		return bh_set_error(BH_E_USAGE, "bh_alleles_host: null argument");
	*n_alleles = *n_codes = 0;
	if (!min_depth || min_depth > 0x7FFFFFFFu || !min_alt || min_alt > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "bh_alleles_host: min_depth %u, min_alt %u (1 .. 2^31 - 1 each)", min_depth, min_alt);
	uint64_t n_obs = 0;
	int rc = bh_pile_check_lines("bh_alleles_host", R, q_off, n_queries, lines, n_lines, ops, n_ops, &n_obs);
	if (rc) return rc;
	if (!n_lines) return BH_OK;
	uint64_t n_runs = 0;
	for (uint64_t i = 0; i < n_lines; ++i) n_runs += lines[i].n_ops;
	uint64_t *clump_off = malloc(((size_t)R->n_clumps + 1) * 8);
	AlRec *rec = malloc((n_runs + 1) * sizeof(*rec));
	uint64_t *anc = malloc((n_runs + 1) * 8), *depth = calloc(n_runs + 1, 8);
	if (!clump_off || !rec || !anc || !depth) { free(clump_off); free(rec); free(anc); free(depth); return bh_set_error(BH_E_OOM, "OOM:vcf"); }
	clump_off[0] = 0;
	for (uint32_t c = 0; c < R->n_clumps; ++c) clump_off[c + 1] = clump_off[c] + ((uint64_t)R->clump_len[c] + 1) / 2;
	/* one record per allele run */
	uint64_t n = 0;
	for (uint64_t i = 0; i < n_lines; ++i) {
		const BhipPileLine *u = &lines[i];
		const uint8_t *q = q_codes + q_off[u->q];
		uint32_t p = u->pos, col = u->ref_first - 1, prev = 0; uint64_t j = 0;
		for (uint32_t k = 0; k < u->n_ops; ++k) {
			const uint32_t word = ops[u->op_off + k], len = word >> 4, code = word & 15u;
			if (code == BHIP_OP_I || code == BHIP_OP_D) {
				if (k == 0 || k + 1 == u->n_ops) ++info[3];
				else if (prev == BHIP_OP_I || prev == BHIP_OP_D) ++info[4];
				else if (code == BHIP_OP_I && len > 15) ++info[5];
				else {
					AlRec *r = &rec[n++];
					r->k1 = (uint64_t)u->header << 32 | (p - 1); r->line = i; r->w = u->w; r->col = col;
					if (code == BHIP_OP_D) r->k2 = len;
					else { r->k2 = (uint64_t)len << 60; for (uint32_t t = 0; t < len; ++t) r->k2 |= (uint64_t)(q[j + t] & 15u) << (56 - 4 * t); }
				}
			}
			if (code != BHIP_OP_I) { p += len; col += len; }
			if (code != BHIP_OP_D) j += len;
			prev = code;
		}
	}
	info[0] = n;
	qsort(rec, n, sizeof(*rec), rec_cmp);
	/* Depth of every anchor: each line adds its weight to the anchors inside its range */
	uint64_t na = 0;
	for (uint64_t a = 0; a < n; ++a) if (!na || anc[na - 1] != rec[a].k1) anc[na++] = rec[a].k1;
	for (uint64_t i = 0; i < n_lines && na; ++i) {
		uint64_t span = 0;
		for (uint32_t k = 0; k < lines[i].n_ops; ++k) if ((ops[lines[i].op_off + k] & 15u) != BHIP_OP_I) span += ops[lines[i].op_off + k] >> 4;
		const uint64_t first = (uint64_t)lines[i].header << 32 | lines[i].pos, behind = first + span;
		uint64_t lo = 0, hi = na;
		while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (anc[mid] < first) lo = mid + 1; else hi = mid; }
		for (; lo < na && anc[lo] < behind; ++lo) depth[lo] += lines[i].w;
	}
	/* the runs of equal (anchor, allele): a first pass counts, a second one writes when there is room */
	uint64_t kept = 0, n_del = 0;
	for (int pass = 0; pass < 2; ++pass) {
		uint64_t ai = 0, ki = 0, ci = 0;
		for (uint64_t a = 0; a < n;) {
			uint64_t b = a, count = 0;
			for (; b < n && rec[b].k1 == rec[a].k1 && rec[b].k2 == rec[a].k2; ++b) count += rec[b].w;
			while (anc[ai] != rec[a].k1) ++ai;
			if (!pass) ++info[1];
			if (depth[ai] >= min_depth && count >= min_alt) {
				const uint64_t nd = (rec[a].k2 >> 60) ? 0 : (rec[a].k2 & 0xFFFFFFFFull);
				if (pass) {
					const BhipPileLine *u = &lines[rec[a].line];      /* (the smallest line that carries it) */
					BhipAllele *o = &alleles[ki];
					memset(o, 0, sizeof *o);
					o->header = (uint32_t)(rec[a].k1 >> 32); o->pos = (uint32_t)rec[a].k1; o->allele = rec[a].k2; o->depth = (uint32_t)depth[ai]; o->count = (uint32_t)count;
					o->ref = ref_code(R, clump_off, u->refIx, rec[a].col - 1); o->code_off = ci;
					for (uint64_t t = 0; t < nd; ++t) codes[ci + t] = ref_code(R, clump_off, u->refIx, rec[a].col + (uint32_t)t);
				}
				++ki; ci += nd;
			}
			a = b;
		}
		kept = ki; n_del = ci;
		if (kept > cap || n_del > code_cap) break;
	}
	free(clump_off); free(rec); free(anc); free(depth);
	*n_alleles = kept; *n_codes = n_del;
	if (kept > cap || n_del > code_cap) return BH_E_CAPACITY;
	info[2] = kept;
	return BH_OK;
}

/* the device: ctx = the handle */
static int pile_device(void *ctx, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines, const uint32_t *ops, uint64_t n_ops,
                       uint32_t min_depth, uint32_t min_alt, BhipPileSite *sites, uint64_t cap, uint64_t *n_sites, uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "vcf: the sites are counted on the device and rank 0 has no device handle");
	const int rc = bhip_pile_run(ctx, q_codes, q_off, n_queries, lines, n_lines, ops, n_ops, min_depth, min_alt, sites, cap, n_sites, info);
	if (rc == BHIP_E_CAPACITY) return BH_E_CAPACITY;
	if (rc) return bh_set_error(rc == BHIP_E_ARG || rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "vcf: %s", bhip_last_error());
	return BH_OK;
}
static int alleles_device(void *ctx, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines, const uint32_t *ops, uint64_t n_ops,
                          uint32_t min_depth, uint32_t min_alt, BhipAllele *alleles, uint64_t cap, uint64_t *n_alleles, uint8_t *codes, uint64_t code_cap, uint64_t *n_codes, uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "vcf: the alleles are counted on the device and rank 0 has no device handle");
	const int rc = bhip_alleles_run(ctx, q_codes, q_off, n_queries, lines, n_lines, ops, n_ops, min_depth, min_alt, alleles, cap, n_alleles, codes, code_cap, n_codes, info);
	if (rc == BHIP_E_CAPACITY) return BH_E_CAPACITY;
	if (rc) return bh_set_error(rc == BHIP_E_ARG || rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "vcf: %s", bhip_last_error());
	return BH_OK;
}

int bh_vcf_check_opts(uint32_t min_depth, uint32_t min_alt) {
	if (!min_depth || min_depth > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "ERROR: --vcf-min-depth takes 1 .. 2147483647");
	if (!min_alt || min_alt > 0x7FFFFFFFu) return bh_set_error(BH_E_USAGE, "ERROR: --vcf-min-alt takes 1 .. 2147483647");
	return BH_OK;
}

/* lengths: of every header, or NULL (bh_vcf_open: the database's own extents, taken when the first sample ends) */
int bh_vcf_open_heads(uint32_t n_headers, const char *const *heads, const uint32_t *lengths, uint32_t min_depth, uint32_t min_alt, int unique_only, BhVcf **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_vcf_open: no place for the object");
	*out = NULL;
	if (!n_headers || !heads) return bh_set_error(BH_E_USAGE, "bh_vcf_open: no headers");
	int rc = bh_vcf_check_opts(min_depth, min_alt);
	if (rc) return rc;
	BhVcf *v = calloc(1, sizeof(*v));
	if (!v) return bh_set_error(BH_E_OOM, "OOM:vcf");
	v->nH = n_headers; v->minDepth = min_depth; v->minAlt = min_alt;
	v->len = calloc(n_headers, 4);
	if (!v->len) { bh_vcf_close(v); return bh_set_error(BH_E_OOM, "OOM:vcf"); }
	if ((rc = bh_sam_names("--vcf", n_headers, heads, &v->sn)) || (rc = bh_pile_open_lines(n_headers, unique_only, &v->lines))) { bh_vcf_close(v); return rc; }
	if (lengths) { memcpy(v->len, lengths, (size_t)n_headers * 4); v->have_len = 1; }
	*out = v;
	return BH_OK;
}

int bh_vcf_open(const BhDb *db, const char *lengths_file, uint32_t min_depth, uint32_t min_alt, int unique_only, BhVcf **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_vcf_open: no place for the object");
	*out = NULL;
	if (!db || !db->numRefHeads || !db->refMap || !db->refHead) return bh_set_error(BH_E_USAGE, "bh_vcf_open: no database / no reference headers");
	const char **head = calloc(db->numRefHeads, sizeof(*head));
	if (!head) return bh_set_error(BH_E_OOM, "OOM:vcf");
	for (uint32_t i = 0; i < db->origTotR; ++i) if (db->refMap[i] < db->numRefHeads) head[db->refMap[i]] = db->refHead[i];      /* (the numbers the report's notes use) */
	for (uint32_t h = 0; h < db->numRefHeads; ++h) if (!head[h]) head[h] = "";
	int rc = bh_vcf_open_heads(db->numRefHeads, head, NULL, min_depth, min_alt, unique_only, out);
	if (!rc) {
		(*out)->db = db;
		if (lengths_file && !(rc = bh_cov_read_lengths(lengths_file, "--vcf-lengths", db->numRefHeads, head, (*out)->len))) (*out)->have_len = 1;
		if (rc) { bh_vcf_close(*out); *out = NULL; }
	}
	free(head);
	return rc;
}

void bh_vcf_set_solver(BhVcf *v, bh_pile_solver_fn pile_fn, void *pile_ctx, bh_alleles_solver_fn al_fn, void *al_ctx) {
	if (v) { v->pile_fn = pile_fn; v->pile_ctx = pile_ctx; v->al_fn = al_fn; v->al_ctx = al_ctx; }
}
void bh_vcf_set_study(BhVcf *v, BhVcfStudy *study) { if (v) v->study = study; }
void bh_vcf_abort(BhVcf *v) { if (v && !v->dead) v->dead = BH_E_DEVICE; if (v) bh_vcfstudy_abort(v->study); }
void bh_vcf_sample_failed(BhVcf *v) { if (v) bh_pile_drop_lines(v->lines); }      /* (no OUT.vcf of a sample that failed) */
int bh_vcf_study_sample_failed(BhVcf *v, const char *out_path) { return v && v->study ? bh_vcfstudy_sample_failed(v->study, out_path) : BH_OK; }
static int die(BhVcf *v, int rc) { v->dead = rc; bh_vcfstudy_abort(v->study); return rc; }

/* what the study file shares with OUT.vcf: the contig names, the lengths (no table: the database's own extents, as --sam takes them), the
 * header block in front of the column line (study: the NS line as well) */
uint32_t bh_vcf_n_headers(const BhVcf *v) { return v ? v->nH : 0; }
const char *bh_vcf_contig(const BhVcf *v, uint32_t h) { return v && h < v->nH ? v->sn[h] : ""; }
int bh_vcf_ensure_lengths(BhVcf *v, void *hh) {
	if (!v) return bh_set_error(BH_E_USAGE, "bh_vcf_ensure_lengths: no vcf object");
	if (v->have_len) return BH_OK;
	if (!v->db) return bh_set_error(BH_E_USAGE, "bh_vcf_sample: no reference lengths");
	const int rc = bh_cov_default_lengths(v->db, v->al_fn ? NULL : hh, v->len);
	if (!rc) v->have_len = 1;
	return rc;
}
void bh_vcf_write_header(const BhVcf *v, FILE *f, int study) {
	fputs("##fileformat=VCFv4.2\n##source=burst_hip\n", f);
	for (uint32_t h = 0; h < v->nH; ++h) fprintf(f, "##contig=<ID=%s,length=%u>\n", v->sn[h], v->len[h]);
	fputs("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Reads observing the position\">\n", f);
	if (study) fputs("##INFO=<ID=NS,Number=1,Type=Integer,Description=\"Samples with a read observing the position\">\n", f);
	fputs("##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Reads observing the position\">\n"
	      "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Reads per allele, reference first\">\n", f);
}

int bh_vcf_collect(BhVcf *v, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t nr,
                   const BhPathBuf *bufs, uint64_t n_chunks) {
	if (!v) return BH_OK;
	if (v->dead) return bh_set_error(v->dead, "the VCF output was ended by an earlier error");
	const int rc = bh_pile_collect(v->lines, idx, req, first, off, ops, nr, bufs, n_chunks);
	return rc ? die(v, rc) : BH_OK;
}
static int collect_cb(void *ctx, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t nr,
                      const BhPathBuf *bufs, char *const *text, const size_t *text_len, uint64_t n_chunks) {
	(void)text; (void)text_len;
	return bh_vcf_collect(ctx, idx, req, first, off, ops, nr, bufs, n_chunks);
}
int bh_paths_set_vcf(BhPaths *paths, BhVcf *v, int columns) { return bh_paths_add_collector(paths, collect_cb, v, columns); }

/* the records of one sample: the two ordered lists merged.  Returns 0, or 1 for a list that is out of order or out of range */
static int write_records(const BhVcf *v, FILE *f, const BhipPileSite *sites, uint64_t ns, const BhipAllele *al, uint64_t na, const uint8_t *codes, uint64_t nc, uint64_t counts[3]) {
	uint64_t si = 0, ai = 0, last = 0;
	while (si < ns || ai < na) {
		const uint64_t ks = si < ns ? (uint64_t)sites[si].header << 32 | sites[si].pos : ~0ull, ka = ai < na ? (uint64_t)al[ai].header << 32 | al[ai].pos : ~0ull;
		if (si < ns && ks <= ka) {      /* at one position the SNV record first */
			const BhipPileSite *s = &sites[si++];
			if (s->header >= v->nH || ks < last) return 1;
			last = ks;
			if (s->ref < 1 || s->ref > 4 || s->depth < v->minDepth) continue;
			int any = 0;
			for (uint32_t b = 0; b < 4; ++b) if (b != s->ref - 1 && s->n[b] >= v->minAlt) any = 1;
			if (!any) continue;
			fprintf(f, "%s\t%u\t.\t%c\t", v->sn[s->header], s->pos, VCF_LETTERS[s->ref]);
			for (uint32_t b = 0, k = 0; b < 4; ++b) if (b != s->ref - 1 && s->n[b] >= v->minAlt) { if (k++) fputc(',', f); fputc("ACGT"[b], f); }
			fprintf(f, "\t.\t.\tDP=%u\tDP:AD\t%u:%u", s->depth, s->depth, s->n[s->ref - 1]);
			for (uint32_t b = 0; b < 4; ++b) if (b != s->ref - 1 && s->n[b] >= v->minAlt) fprintf(f, ",%u", s->n[b]);
			fputc('\n', f);
			++counts[0];
			continue;
		}
		const BhipAllele *a = &al[ai++];
		const uint32_t n_ins = (uint32_t)(a->allele >> 60);
		const uint64_t n_del = n_ins ? 0 : (a->allele & 0xFFFFFFFFull);
		if (a->header >= v->nH || ka < last || a->ref > 15 || a->count > a->depth || (!n_ins && (!n_del || a->code_off > nc || n_del > nc - a->code_off))) return 1;
		last = ka;
		const char anchor = VCF_LETTERS[a->ref];
		fprintf(f, "%s\t%u\t.\t%c", v->sn[a->header], a->pos, anchor);
		for (uint64_t t = 0; t < n_del; ++t) fputc(VCF_LETTERS[codes[a->code_off + t] & 15u], f);
		fprintf(f, "\t%c", anchor);
		for (uint32_t t = 0; t < n_ins; ++t) fputc(VCF_LETTERS[(a->allele >> (56 - 4 * t)) & 15u], f);
		fprintf(f, "\t.\t.\tDP=%u\tDP:AD\t%u:%u,%u\n", a->depth, a->depth, a->depth - a->count, a->count);
		++counts[n_ins ? 2 : 1];
	}
	return 0;
}

int bh_vcf_sample(BhVcf *v, void *hh, const char *out_path, const uint8_t *q_codes, const uint64_t *q_off, uint64_t n_queries) {
	if (!v || !out_path) return bh_set_error(BH_E_USAGE, "bh_vcf_sample: no vcf object / no output");
	if (v->dead) return bh_set_error(v->dead, "the VCF output was ended by an earlier error");
	if (n_queries > 0xFFFFFFFFull) return die(v, bh_set_error(BH_E_INTERNAL, "vcf: %lu query entries", (unsigned long)n_queries));
	int rc;
	if ((rc = bh_vcf_ensure_lengths(v, hh))) return die(v, rc);
	/* with a study attached the solvers are asked at (1, 1): everything the sample observes that is not plain, which the study keeps; the
	 * thresholds are then applied here (write_records does it for the sites, the alleles are filtered below), so OUT.vcf has the same bytes */
	const uint32_t askDepth = v->study ? 1u : v->minDepth, askAlt = v->study ? 1u : v->minAlt;
	const BhipPileLine *lines = NULL; const uint32_t *ops = NULL; uint64_t n_ops = 0, n_printed = 0;
	const uint64_t n_lines = bh_pile_lines(v->lines, &lines, &ops, &n_ops, &n_printed);
	uint64_t site_cap = n_lines < 1024 ? 1024 : n_lines, ns = 0, pinfo[8] = {0};
	uint64_t al_cap = site_cap, code_cap = 1u << 16, na = 0, nc = 0, ainfo[8] = {0};
	BhipPileSite *sites = NULL; BhipAllele *al = NULL; uint8_t *codes = NULL;
	#define VCF_FAIL(code) do { free(sites); free(al); free(codes); return die(v, (code)); } while (0)
	for (int attempt = 0; attempt < 2; ++attempt) {      /* (the room grows once: the call says how many sites it has) */
		BhipPileSite *s2 = realloc(sites, site_cap * sizeof(*s2));
		if (!s2) VCF_FAIL(bh_set_error(BH_E_OOM, "OOM:vcf"));
		sites = s2;
		rc = (v->pile_fn ? v->pile_fn : pile_device)(v->pile_fn ? v->pile_ctx : hh, q_codes, q_off, (uint32_t)n_queries, lines, n_lines, ops, n_ops, askDepth, askAlt, sites, site_cap, &ns, pinfo);
		if (rc != BH_E_CAPACITY) break;
		if (attempt || ns <= site_cap) { rc = bh_set_error(BH_E_INTERNAL, "vcf: %lu sites do not fit the room the first call asked for", (unsigned long)ns); break; }
		site_cap = ns;
	}
	if (rc) VCF_FAIL(rc);
	for (int attempt = 0; attempt < 2; ++attempt) {
		BhipAllele *a2 = realloc(al, al_cap * sizeof(*a2)); if (a2) al = a2;
		uint8_t *c2 = realloc(codes, code_cap); if (c2) codes = c2;
		if (!a2 || !c2) VCF_FAIL(bh_set_error(BH_E_OOM, "OOM:vcf"));
		rc = (v->al_fn ? v->al_fn : alleles_device)(v->al_fn ? v->al_ctx : hh, q_codes, q_off, (uint32_t)n_queries, lines, n_lines, ops, n_ops, askDepth, askAlt, al, al_cap, &na,
		                                            codes, code_cap, &nc, ainfo);
		if (rc != BH_E_CAPACITY) break;
		if (attempt || (na <= al_cap && nc <= code_cap)) { rc = bh_set_error(BH_E_INTERNAL, "vcf: %lu alleles and %lu codes do not fit the room the first call asked for", (unsigned long)na, (unsigned long)nc); break; }
		if (na > al_cap) al_cap = na;
		if (nc > code_cap) code_cap = nc;
	}
	if (rc) VCF_FAIL(rc);
	BhipAllele *al_all = NULL; uint64_t na_all = na;      /* (study: the (1, 1) list is kept whole, OUT.vcf takes the alleles that pass) */
	if (v->study) {
		if (!(al_all = malloc((na ? na : 1) * sizeof(*al_all)))) VCF_FAIL(bh_set_error(BH_E_OOM, "OOM:vcf"));
		memcpy(al_all, al, na * sizeof(*al));
		uint64_t k = 0;
		for (uint64_t i = 0; i < na; ++i) if (al[i].depth >= v->minDepth && al[i].count >= v->minAlt) al[k++] = al[i];      /* (code_off still points into the whole code list) */
		na = k; ainfo[2] = k;
	}
	/* OUT.vcf under a temporary name */
	char *finn = NULL, *tmpn = NULL, *name = bh_pile_sample_name(out_path);
	if (!name || asprintf(&finn, "%s.vcf", out_path) < 0) { finn = NULL; free(name); free(al_all); VCF_FAIL(bh_set_error(BH_E_OOM, "OOM:vcf")); }
	if (asprintf(&tmpn, "%s.vcf.tmp%ld", out_path, (long)getpid()) < 0) { free(name); free(finn); free(al_all); VCF_FAIL(bh_set_error(BH_E_OOM, "OOM:vcf")); }
	FILE *f = fopen(tmpn, "wb");
	if (!f) {      /* (the sample's own error: the object stays usable) */
		rc = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", tmpn);
		free(name); free(finn); free(tmpn); free(sites); free(al); free(codes); free(al_all);
		bh_pile_drop_lines(v->lines);
		(void)bh_vcfstudy_sample_failed(v->study, out_path);
		return bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s.vcf.tmp%ld", out_path, (long)getpid());
	}
	setvbuf(f, NULL, _IOFBF, 1 << 20);
	bh_vcf_write_header(v, f, 0);
	fprintf(f, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n", name);
	uint64_t counts[3] = {0, 0, 0};
	const int bad = write_records(v, f, sites, ns, al, na, codes, nc, counts);
	free(name);
	rc = BH_OK;
	if (bad) rc = bh_set_error(BH_E_INTERNAL, "vcf: a site or an allele is out of order or out of range");
	if ((ferror(f) | fclose(f)) && !rc) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", tmpn);
	if (!rc && rename(tmpn, finn)) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", tmpn, finn);
	if (rc) (void)unlink(tmpn);
	free(finn); free(tmpn);
	if (v->study) {      /* the sample has its OUT.vcf: the study keeps its ranges and its (1, 1) lists; without one its column is '.' */
		if (rc == BH_E_IO) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); (void)bh_vcfstudy_sample_failed(v->study, out_path); bh_set_error(rc, "%s", msg); }
		else if (!rc) rc = bh_vcfstudy_add(v->study, out_path, lines, n_lines, ops, sites, ns, al_all, na_all, codes, nc, v->minDepth, v->minAlt);
	}
	free(sites); free(al); free(codes); free(al_all);
	bh_pile_drop_lines(v->lines);
	if (rc) { if (rc != BH_E_IO && rc != BH_E_USAGE) die(v, rc); return rc; }
	v->info[0] = n_printed; v->info[1] = ainfo[0]; v->info[2] = ainfo[1]; v->info[3] = ainfo[2]; v->info[4] = counts[0]; v->info[5] = counts[1]; v->info[6] = counts[2];
	v->info[7] = ainfo[3]; v->info[8] = ainfo[4]; v->info[9] = ainfo[5]; v->info[10] = ainfo[6] + pinfo[3]; v->info[11] = ainfo[7] > pinfo[4] ? ainfo[7] : pinfo[4];
	v->have_info = 1;
	return BH_OK;
	#undef VCF_FAIL
}

/* one line on standard output: the last sample's figures */
void bh_vcf_print_info(BhVcf *v) {
	if (!v || !v->have_info || v->dead) return;
	printf("Vcf: %lu lines, %lu allele events, %lu distinct alleles, records written %lu SNV / %lu Del / %lu Ins, skipped runs %lu end / %lu adjacent / %lu long, device %.3f ms\n",
	       (unsigned long)v->info[0], (unsigned long)v->info[1], (unsigned long)v->info[2], (unsigned long)v->info[4], (unsigned long)v->info[5], (unsigned long)v->info[6],
	       (unsigned long)v->info[7], (unsigned long)v->info[8], (unsigned long)v->info[9], v->info[10] / 1e3);
}
void bh_vcf_last_info(const BhVcf *v, uint64_t info[12]) {
	if (!info) return;
	if (v && v->have_info) memcpy(info, v->info, 12 * sizeof(uint64_t)); else memset(info, 0, 12 * sizeof(uint64_t));
}

void bh_vcf_close(BhVcf *v) {
	if (!v) return;
	bh_sam_names_free(v->sn, v->nH);
	bh_pile_close(v->lines);
	free(v->len);
	free(v);
}
