/* bh_vcfstudy.c -- the study VCF: every sample's counts at every record that any sample reports (burst_hip --vcf --vcf-study PREFIX,
 * host.Session(vcf=True, vcf_study=PREFIX)).
 *
 * No reference counterpart.  The definition is include/burst_hip.h "Site counts" and DESIGN.md section 7k.  The single-sample OUT.vcf files
 * cannot be merged afterwards: where one sample reports a record and another one's file has no line, the other sample may show the
 * reference base, have no read, or have two reads where --vcf-min-depth wants four -- and the depth that tells these apart exists only
 * while the run holds the sample's lines.  So bh_vcf_sample, with this object attached, asks its two solvers at thresholds (1, 1), filters
 * for OUT.vcf on the host, and hands over what this file keeps per sample in host memory: a range of 16 bytes per line, the (1, 1) sites and
 * alleles, and the records the sample reports with the codes of its Dels.  At the end of the run the reported records of all samples are
 * merged in the order of OUT.vcf, ONE bhip_site_counts call per sample on the reporting rank's handle fills that sample's column, and
 * PREFIXstudy.vcf is written under a temporary name and renamed.  Also here: bh_site_counts_host, the primitive once more in plain
 * sequential C (a loop over all ranges per record), which the tests without a device and the yardstick use. */
#define _GNU_SOURCE
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static const char STUDY_LETTERS[] = "NACGTNNNNNNNNNNN";

/* a record one sample reports: allele 0 = an SNV (alt: bit b for ALT base b), else the allele word (a Del owns codes[code_off .. + n)) */
typedef struct { uint64_t key, allele; uint32_t ref, alt; uint64_t code_off; } StudyRec;
typedef struct {
	char *name, *path; int failed;
	BhipCountRange *ranges; uint64_t nr;
	BhipPileSite *sites; uint64_t ns;
	BhipAllele *al; uint64_t na;
	StudyRec *rec; uint64_t nrec;
	uint8_t *codes; uint64_t nc;
} StudySample;

struct BhVcfStudy {
	char *finn, *tmpn;
	StudySample *s; uint32_t n, cap;
	int dead, written;
	bh_sitecounts_solver_fn fn; void *ctx;
	uint64_t info[8]; int have_info;
};

/* ---- the definition in plain C ---- */
static uint64_t key_of(uint32_t header, uint32_t pos) { return (uint64_t)header << 32 | pos; }
int bh_site_counts_host(void *unused, const BhipCountRange *ranges, uint64_t n_ranges, const BhipPileSite *sites, uint64_t n_sites, const BhipAllele *alleles, uint64_t n_alleles,
                        const BhipCountRecord *records, uint64_t n_records, BhipCountCell *cells, uint64_t info[8]) {
	(void)unused;
	uint64_t local[8];
	if (!info) info = local;
	memset(info, 0, 8 * sizeof(uint64_t));
	if ((n_ranges && !ranges) || (n_sites && !sites) || (n_alleles && !alleles) || (n_records && (!records || !cells))) return bh_set_error(BH_E_USAGE, "bh_site_counts_host: null argument");
	if ((n_ranges | n_sites | n_alleles | n_records) >> 32) return bh_set_error(BH_E_USAGE, "bh_site_counts_host: a count of 2^32 or more");
	uint64_t wsum = 0;
	for (uint64_t i = 0; i < n_ranges; ++i) {
		if (ranges[i].pos < 1 || (uint64_t)ranges[i].pos + ranges[i].span > 0xFFFFFFFFull)
			return bh_set_error(BH_E_USAGE, "bh_site_counts_host: range %lu: position %u + span %u (1 .. 2^32 - 1)", (unsigned long)i, ranges[i].pos, ranges[i].span);
		if (!ranges[i].w) return bh_set_error(BH_E_USAGE, "bh_site_counts_host: range %lu has weight 0", (unsigned long)i);
		if ((wsum += ranges[i].w) > 0x7FFFFFFFull) return bh_set_error(BH_E_USAGE, "bh_site_counts_host: the ranges stand for more than 2^31 - 1 reads (range %lu)", (unsigned long)i);
	}
	for (uint64_t i = 1; i < n_sites; ++i)
		if (key_of(sites[i - 1].header, sites[i - 1].pos) >= key_of(sites[i].header, sites[i].pos)) return bh_set_error(BH_E_USAGE, "bh_site_counts_host: sites not strictly ascending by (header, pos) at site %lu", (unsigned long)i);
	for (uint64_t i = 1; i < n_alleles; ++i) {
		const uint64_t a = key_of(alleles[i - 1].header, alleles[i - 1].pos), b = key_of(alleles[i].header, alleles[i].pos);
		if (a > b || (a == b && alleles[i - 1].allele >= alleles[i].allele)) return bh_set_error(BH_E_USAGE, "bh_site_counts_host: alleles not strictly ascending by (header, pos, allele) at allele %lu", (unsigned long)i);
	}
	for (uint64_t i = 0; i < n_records; ++i) {
		if (!records[i].pos) return bh_set_error(BH_E_USAGE, "bh_site_counts_host: record %lu has position 0", (unsigned long)i);
		if (!records[i].allele && (records[i].ref < 1 || records[i].ref > 4)) return bh_set_error(BH_E_USAGE, "bh_site_counts_host: site record %lu has ref %u (1 .. 4)", (unsigned long)i, records[i].ref);
	}
	for (uint64_t i = 0; i < n_records; ++i) {
		const BhipCountRecord *r = &records[i];
		BhipCountCell *c = &cells[i];
		memset(c, 0, sizeof *c);
		uint64_t depth = 0;
		for (uint64_t k = 0; k < n_ranges; ++k)
			if (ranges[k].header == r->header && ranges[k].pos <= r->pos && (uint64_t)r->pos < (uint64_t)ranges[k].pos + ranges[k].span) depth += ranges[k].w;
		c->depth = (uint32_t)depth;
		if (!r->allele) {
			uint64_t k = 0;
			while (k < n_sites && !(sites[k].header == r->header && sites[k].pos == r->pos)) ++k;
			if (k < n_sites) memcpy(c->n, sites[k].n, 4 * sizeof(uint32_t)); else c->n[r->ref - 1] = (uint32_t)depth;
		} else {
			for (uint64_t k = 0; k < n_alleles; ++k)
				if (alleles[k].header == r->header && alleles[k].pos == r->pos && alleles[k].allele == r->allele) { c->count = alleles[k].count; break; }
		}
	}
	info[0] = n_ranges; info[1] = n_records;
	return BH_OK;
}

/* the device: ctx = the handle */
static int counts_device(void *ctx, const BhipCountRange *ranges, uint64_t n_ranges, const BhipPileSite *sites, uint64_t n_sites, const BhipAllele *alleles, uint64_t n_alleles,
                         const BhipCountRecord *records, uint64_t n_records, BhipCountCell *cells, uint64_t info[8]) {
	if (!ctx) return bh_set_error(BH_E_DEVICE, "vcf study: the counts are taken on the device and rank 0 has no device handle");
	const int rc = bhip_site_counts(ctx, ranges, n_ranges, sites, n_sites, alleles, n_alleles, records, n_records, cells, info);
	if (rc) return bh_set_error(rc == BHIP_E_ARG || rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "vcf study: %s", bhip_last_error());
	return BH_OK;
}

int bh_vcfstudy_open(const char *prefix, BhVcfStudy **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_vcfstudy_open: no place for the object");
	*out = NULL;
	if (!prefix) return bh_set_error(BH_E_USAGE, "bh_vcfstudy_open: no prefix");
	BhVcfStudy *st = calloc(1, sizeof(*st));
	if (!st) return bh_set_error(BH_E_OOM, "OOM:vcfstudy");
	if (asprintf(&st->finn, "%sstudy.vcf", prefix) < 0) st->finn = NULL;
	if (asprintf(&st->tmpn, "%sstudy.vcf.tmp%ld", prefix, (long)getpid()) < 0) st->tmpn = NULL;
	if (!st->finn || !st->tmpn) { bh_vcfstudy_close(st); return bh_set_error(BH_E_OOM, "OOM:vcfstudy"); }
	*out = st;
	return BH_OK;
}
void bh_vcfstudy_set_solver(BhVcfStudy *st, bh_sitecounts_solver_fn fn, void *ctx) { if (st) { st->fn = fn; st->ctx = ctx; } }
void bh_vcfstudy_abort(BhVcfStudy *st) { if (st && !st->dead) st->dead = BH_E_DEVICE; }

/* two outputs of one sample name: BH_E_USAGE that names both (the command line asks before a device is touched) */
int bh_vcfstudy_check_names(const char *const *out_paths, uint64_t n) {
	int rc = BH_OK;
	char **nm = calloc(n ? n : 1, sizeof(*nm));
	if (!nm) return bh_set_error(BH_E_OOM, "OOM:vcfstudy");
	for (uint64_t i = 0; i < n && !rc; ++i) {
		if (!(nm[i] = bh_pile_sample_name(out_paths[i]))) { rc = bh_set_error(BH_E_OOM, "OOM:vcfstudy"); break; }
		for (uint64_t k = 0; k < i; ++k) if (!strcmp(nm[i], nm[k])) { rc = bh_set_error(BH_E_USAGE, "ERROR: --vcf-study: outputs '%s' and '%s' are both sample '%s'", out_paths[k], out_paths[i], nm[i]); break; }
	}
	for (uint64_t i = 0; i < n; ++i) free(nm[i]);
	free(nm);
	return rc;
}

static void sample_free(StudySample *s) { free(s->name); free(s->path); free(s->ranges); free(s->sites); free(s->al); free(s->rec); free(s->codes); memset(s, 0, sizeof *s); }
static int new_sample(BhVcfStudy *st, const char *out_path, StudySample **out) {
	if (st->n == st->cap) {
		const uint32_t cap = st->cap ? 2 * st->cap : 16;
		StudySample *s2 = realloc(st->s, (size_t)cap * sizeof(*s2));
		if (!s2) return bh_set_error(BH_E_OOM, "OOM:vcfstudy");
		st->s = s2; st->cap = cap;
	}
	StudySample *s = &st->s[st->n];
	memset(s, 0, sizeof *s);
	s->name = bh_pile_sample_name(out_path); s->path = strdup(out_path);
	if (!s->name || !s->path) { sample_free(s); return bh_set_error(BH_E_OOM, "OOM:vcfstudy"); }
	for (uint32_t k = 0; k < st->n; ++k) if (!strcmp(st->s[k].name, s->name)) {
		const int rc = bh_set_error(BH_E_USAGE, "ERROR: --vcf-study: outputs '%s' and '%s' are both sample '%s'", st->s[k].path, out_path, s->name);
		sample_free(s);
		return rc;
	}
	++st->n;
	*out = s;
	return BH_OK;
}

int bh_vcfstudy_sample_failed(BhVcfStudy *st, const char *out_path) {
	if (!st || st->dead || st->written) return BH_OK;
	StudySample *s = NULL;
	const int rc = new_sample(st, out_path ? out_path : "sample", &s);
	if (rc) return rc;
	s->failed = 1;
	printf(" --> vcf study: sample '%s' failed alone: its column is '.'\n", s->name);
	return BH_OK;
}

static void *dup_mem(const void *p, size_t bytes) { void *q = malloc(bytes ? bytes : 1); if (q && bytes) memcpy(q, p, bytes); return q; }

/* the end of a sample that has its OUT.vcf: its lines as ranges, its (1, 1) lists, the records it reports at (min_depth, min_alt) */
int bh_vcfstudy_add(BhVcfStudy *st, const char *out_path, const BhipPileLine *lines, uint64_t n_lines, const uint32_t *ops, const BhipPileSite *sites, uint64_t ns,
                    const BhipAllele *al, uint64_t na, const uint8_t *codes, uint64_t nc, uint32_t min_depth, uint32_t min_alt) {
	if (!st) return BH_OK;
	if (st->dead) return bh_set_error(st->dead, "the study VCF was ended by an earlier error");
	if (st->written) return bh_set_error(BH_E_USAGE, "bh_vcfstudy_add: the study VCF has been written");
	if (!out_path || (n_lines && (!lines || !ops)) || (ns && !sites) || (na && !al)) return bh_set_error(BH_E_USAGE, "bh_vcfstudy_add: null argument");
	StudySample *s = NULL;
	int rc = new_sample(st, out_path, &s);
	if (rc) return rc;      /* (a usage error: the sample's own) */
	s->nr = n_lines; s->ns = ns; s->na = na;
	s->ranges = malloc((n_lines ? n_lines : 1) * sizeof(*s->ranges));
	s->sites = dup_mem(sites, ns * sizeof(*sites)); s->al = dup_mem(al, na * sizeof(*al));
	s->rec = malloc((ns + na + 1) * sizeof(*s->rec));
	uint64_t n_codes = 0;
	for (uint64_t i = 0; i < na; ++i) if (!(al[i].allele >> 60) && al[i].depth >= min_depth && al[i].count >= min_alt) n_codes += al[i].allele & 0xFFFFFFFFull;
	s->codes = malloc(n_codes ? n_codes : 1);
	if (!s->ranges || !s->sites || !s->al || !s->rec || !s->codes) { sample_free(s); --st->n; return st->dead = bh_set_error(BH_E_OOM, "OOM:vcfstudy"); }
	for (uint64_t i = 0; i < n_lines; ++i) {
		uint64_t span = 0;
		for (uint32_t k = 0; k < lines[i].n_ops; ++k) if ((ops[lines[i].op_off + k] & 15u) != BHIP_OP_I) span += ops[lines[i].op_off + k] >> 4;
		s->ranges[i].header = lines[i].header; s->ranges[i].pos = lines[i].pos; s->ranges[i].span = (uint32_t)span; s->ranges[i].w = lines[i].w;
	}
	uint64_t n = 0;
	for (uint64_t i = 0; i < ns; ++i) {      /* (the rule of OUT.vcf's SNV records) */
		const BhipPileSite *x = &sites[i];
		if (x->ref < 1 || x->ref > 4 || x->depth < min_depth) continue;
		uint32_t alt = 0;
		for (uint32_t b = 0; b < 4; ++b) if (b != x->ref - 1 && x->n[b] >= min_alt) alt |= 1u << b;
		if (!alt) continue;
		StudyRec *r = &s->rec[n++];
		r->key = key_of(x->header, x->pos); r->allele = 0; r->ref = x->ref; r->alt = alt; r->code_off = 0;
	}
	for (uint64_t i = 0; i < na; ++i) {
		const BhipAllele *a = &al[i];
		if (a->depth < min_depth || a->count < min_alt) continue;
		const uint64_t n_del = (a->allele >> 60) ? 0 : (a->allele & 0xFFFFFFFFull);
		if (!a->allele || a->code_off > nc || n_del > nc - a->code_off) { sample_free(s); --st->n; return st->dead = bh_set_error(BH_E_INTERNAL, "vcf study: an allele is out of range"); }
		StudyRec *r = &s->rec[n++];
		r->key = key_of(a->header, a->pos); r->allele = a->allele; r->ref = a->ref & 15u; r->alt = 0; r->code_off = s->nc;
		if (n_del) { memcpy(s->codes + s->nc, codes + a->code_off, n_del); s->nc += n_del; }
	}
	s->nrec = n;
	return BH_OK;
}

static int rec_cmp(const void *a, const void *b) {
	const StudyRec *x = a, *y = b;
	if (x->key != y->key) return x->key < y->key ? -1 : 1;
	return (x->allele > y->allele) - (x->allele < y->allele);
}
typedef struct { StudyRec r; const uint8_t *codes; } Merged;
static int merged_cmp(const void *a, const void *b) { return rec_cmp(&((const Merged *)a)->r, &((const Merged *)b)->r); }

int bh_vcfstudy_write(BhVcfStudy *st, BhVcf *vcf, void *hh) {
	if (!st || !vcf) return bh_set_error(BH_E_USAGE, "bh_vcfstudy_write: no study / no vcf object");
	if (st->dead) return bh_set_error(st->dead, "the study VCF was ended by an earlier error: no file is written");
	if (st->written) return bh_set_error(BH_E_USAGE, "bh_vcfstudy_write: the study VCF has been written");
	int rc = bh_vcf_ensure_lengths(vcf, hh);
	if (rc) return st->dead = rc;
	const uint32_t nS = st->n, nH = bh_vcf_n_headers(vcf);
	/* 1. the reported records of all samples, merged in the order of OUT.vcf: (header, pos), the SNV first (word 0), then the alleles by word */
	uint64_t total = 0, kept = 0, n_done = 0;
	for (uint32_t i = 0; i < nS; ++i) { total += st->s[i].nrec; if (!st->s[i].failed) ++n_done; }
	Merged *m = malloc((total ? total : 1) * sizeof(*m));
	if (!m) return st->dead = bh_set_error(BH_E_OOM, "OOM:vcfstudy");
	uint64_t n = 0;
	for (uint32_t i = 0; i < nS; ++i) for (uint64_t k = 0; k < st->s[i].nrec; ++k) { m[n].r = st->s[i].rec[k]; m[n].codes = st->s[i].codes + st->s[i].rec[k].code_off; ++n; }
	qsort(m, n, sizeof(*m), merged_cmp);      /* (equal records are interchangeable: the database is the same for all samples) */
	uint64_t nrec = 0;
	for (uint64_t i = 0; i < n; ++i) {
		if (nrec && m[nrec - 1].r.key == m[i].r.key && m[nrec - 1].r.allele == m[i].r.allele) { m[nrec - 1].r.alt |= m[i].r.alt; continue; }
		m[nrec++] = m[i];
	}
	BhipCountRecord *recs = malloc((nrec ? nrec : 1) * sizeof(*recs));
	BhipCountCell *cells = malloc(((uint64_t)nS * nrec + 1) * sizeof(*cells));
	if (!recs || !cells) { free(m); free(recs); free(cells); return st->dead = bh_set_error(BH_E_OOM, "OOM:vcfstudy"); }
	for (uint64_t i = 0; i < nrec; ++i) {
		recs[i].header = (uint32_t)(m[i].r.key >> 32); recs[i].pos = (uint32_t)m[i].r.key; recs[i].allele = m[i].r.allele; recs[i].ref = m[i].r.allele ? 0 : m[i].r.ref; recs[i].pad = 0;
		if (recs[i].header >= nH) rc = bh_set_error(BH_E_INTERNAL, "vcf study: a record names header %u of %u", recs[i].header, nH);
	}
	/* 2. one call per sample; a list that comes back inconsistent is final */
	uint64_t us = 0;
	for (uint32_t i = 0; i < nS && !rc; ++i) {
		const StudySample *s = &st->s[i];
		BhipCountCell *c = cells + (uint64_t)i * nrec;
		if (s->failed) { memset(c, 0, nrec * sizeof(*c)); continue; }
		uint64_t info[8] = {0};
		rc = (st->fn ? st->fn : counts_device)(st->fn ? st->ctx : hh, s->ranges, s->nr, s->sites, s->ns, s->al, s->na, recs, nrec, c, info);
		us += info[2];
		for (uint64_t k = 0; k < nrec && !rc; ++k)
			if (recs[k].allele ? c[k].count > c[k].depth : c[k].n[recs[k].ref - 1] > c[k].depth)
				rc = bh_set_error(BH_E_INTERNAL, "vcf study: sample '%s' counts more reads on an allele than observe %u:%u", s->name, recs[k].header, recs[k].pos);
		kept += s->nr * sizeof(*s->ranges) + s->ns * sizeof(*s->sites) + s->na * sizeof(*s->al) + s->nrec * sizeof(*s->rec) + s->nc;
	}
	if (rc) { free(m); free(recs); free(cells); return st->dead = rc; }
	/* 3. the file, under a temporary name */
	FILE *f = fopen(st->tmpn, "wb");
	if (!f) { free(m); free(recs); free(cells); return st->dead = bh_set_error(BH_E_IO, "ERROR: Cannot open output: %s", st->tmpn); }
	setvbuf(f, NULL, _IOFBF, 1 << 20);
	bh_vcf_write_header(vcf, f, 1);
	fputs("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT", f);
	for (uint32_t i = 0; i < nS; ++i) fprintf(f, "\t%s", st->s[i].name);
	fputc('\n', f);
	uint64_t counts[3] = {0, 0, 0};
	for (uint64_t k = 0; k < nrec; ++k) {
		const StudyRec *r = &m[k].r;
		const uint32_t n_ins = (uint32_t)(r->allele >> 60);
		const uint64_t n_del = n_ins ? 0 : (r->allele & 0xFFFFFFFFull);
		uint64_t dp = 0; uint32_t nsamp = 0;
		for (uint32_t i = 0; i < nS; ++i) if (!st->s[i].failed) { const uint32_t d = cells[(uint64_t)i * nrec + k].depth; dp += d; nsamp += d >= 1; }
		fprintf(f, "%s\t%u\t.\t%c", bh_vcf_contig(vcf, recs[k].header), recs[k].pos, STUDY_LETTERS[r->ref & 15u]);
		if (!r->allele) {
			fputc('\t', f);
			for (uint32_t b = 0, j = 0; b < 4; ++b) if (r->alt >> b & 1u) { if (j++) fputc(',', f); fputc("ACGT"[b], f); }
			++counts[0];
		} else {
			for (uint64_t t = 0; t < n_del; ++t) fputc(STUDY_LETTERS[m[k].codes[t] & 15u], f);
			fprintf(f, "\t%c", STUDY_LETTERS[r->ref & 15u]);
			for (uint32_t t = 0; t < n_ins; ++t) fputc(STUDY_LETTERS[(r->allele >> (56 - 4 * t)) & 15u], f);
			++counts[n_ins ? 2 : 1];
		}
		fprintf(f, "\t.\t.\tDP=%lu;NS=%u\tDP:AD", (unsigned long)dp, nsamp);
		for (uint32_t i = 0; i < nS; ++i) {
			const BhipCountCell *c = &cells[(uint64_t)i * nrec + k];
			if (st->s[i].failed) { fputs("\t.", f); continue; }
			if (!r->allele) {
				fprintf(f, "\t%u:%u", c->depth, c->n[r->ref - 1]);
				for (uint32_t b = 0; b < 4; ++b) if (r->alt >> b & 1u) fprintf(f, ",%u", c->n[b]);
			} else fprintf(f, "\t%u:%u,%u", c->depth, c->depth - c->count, c->count);
		}
		fputc('\n', f);
	}
	free(m); free(recs); free(cells);
	rc = BH_OK;
	if (ferror(f) | fclose(f)) rc = bh_set_error(BH_E_IO, "ERROR: write failed: %s", st->tmpn);
	if (!rc && rename(st->tmpn, st->finn)) rc = bh_set_error(BH_E_IO, "ERROR: Cannot rename %s to %s", st->tmpn, st->finn);
	if (rc) { (void)unlink(st->tmpn); return st->dead = rc; }
	st->written = 1;
	st->info[0] = n_done; st->info[1] = nS - n_done; st->info[2] = counts[0]; st->info[3] = counts[1]; st->info[4] = counts[2]; st->info[5] = n_done * nrec; st->info[6] = kept; st->info[7] = us;
	st->have_info = 1;
	for (uint32_t i = 0; i < nS; ++i) { StudySample *s = &st->s[i]; free(s->ranges); free(s->sites); free(s->al); free(s->rec); free(s->codes); s->ranges = NULL; s->sites = NULL; s->al = NULL; s->rec = NULL; s->codes = NULL; }
	return BH_OK;
}

const char *bh_vcfstudy_path(const BhVcfStudy *st) { return st ? st->finn : NULL; }

/* one line on standard output: the figures of the file */
void bh_vcfstudy_print_info(BhVcfStudy *st) {
	if (!st || !st->have_info || st->dead) return;
	printf("VcfStudy: %lu samples done, %lu failed, records %lu SNV / %lu Del / %lu Ins, %lu cells, %lu host bytes kept, device %.3f ms\n", (unsigned long)st->info[0],
	       (unsigned long)st->info[1], (unsigned long)st->info[2], (unsigned long)st->info[3], (unsigned long)st->info[4], (unsigned long)st->info[5], (unsigned long)st->info[6], st->info[7] / 1e3);
}
void bh_vcfstudy_last_info(const BhVcfStudy *st, uint64_t info[8]) {
	if (!info) return;
	if (st && st->have_info) memcpy(info, st->info, 8 * sizeof(uint64_t)); else memset(info, 0, 8 * sizeof(uint64_t));
}

void bh_vcfstudy_close(BhVcfStudy *st) {
	if (!st) return;
	for (uint32_t i = 0; i < st->n; ++i) sample_free(&st->s[i]);
	free(st->s);
	if (st->tmpn) (void)unlink(st->tmpn);      /* (a file that was not renamed leaves no temporary file) */
	free(st->finn); free(st->tmpn);
	free(st);
}
