/* main.c -- `burst_hip`: the reference's command line (burst.c:4902-5164) in front of the MI355X device path.
 *
 *   burst_hip -r DB.edx -a DB.acx -q reads.fa -o out.b6 -m {BEST|ALLPATHS|CAPITALIST|FORAGE|ANY} -i 0.97 [-fr] [-y] [-w]
 *   burst_hip -r refs.fa -q reads.fa -o out.b6 [-s [len]]            direct FASTA (exhaustive, no accelerator)
 *   burst_hip -r refs.fa -d [QUICK|DNA|RNA] [qLen] -o DB.edx [-a DB.acx] [-s [len]] [-dp N] -i 0.97      database construction
 *   burst_hip -r DB.edx (-a DB.acx | -ad) --samples LIST -m ... -i ...    a list of `queries<TAB>output` against the one resident database (bh_session.c)
 *   burst_hip -r DB.edx (-a DB.acx | -ad) -q R1.fq --mates R2.fq -o out.b6 -m ALLPATHS|FORAGE -i ... [--insert-min N] [--insert-max N]
 *             [--mates-orientation fr|rf|ff] [--mates-report all|best]      paired-end reads: the concordant combinations of the two mates' placements (bh_mates.c)
 *   ... -q / -o or --samples ... --coverage PREFIX [--coverage-lengths FILE] [--coverage-pad N]      coverage and count tables per reference and sample (bh_cov.c)
 *   ... -q / -o or --samples ... --abundance PREFIX [--abundance-iters N] [--abundance-tol UNITS]   multi-mapped reads split over their references by EM (bh_em.c)
 *   ... -q / -o or --samples ... -b MAP --taxa PREFIX [--taxa-agree PERMILLE]   taxon tables: a read to the lowest common ancestor of its references (bh_taxa.c)
 *   burst_hip -r reads.fa|reads.edx [-a|-ad ...] -q reads.fa -o self.b6 -m FORAGE -i ... [-fr] --cluster PREFIX [--cluster-sizes]      greedy centroid clusters of the reads from their self-hits (bh_cluster.c)
 *   burst_hip -r reads.fa|reads.edx [-a|-ad ...] -q reads.fa -o self.b6 -m FORAGE -i ... [-fr] --chimeras PREFIX [--chimera-sizes] [--chimera-skew S]
 *             [--chimera-min-seg G] [--chimera-min-gain D]      de-novo two-parent chimera check of the reads from their self-hits and the hits' paths (bh_chimera.c)
 *   ... -q / -o or --samples ... --variants PREFIX [--variants-min-depth N] [--variants-min-alt N] [--variants-reads all|unique]   variant sites per sample (bh_pile.c)
 *   ... -q / -o or --samples ... --consensus PREFIX [--consensus-min-depth N] [--consensus-min-breadth PERMILLE] [--consensus-reads all|unique] [--consensus-lengths FILE]   consensus per reference and sample (bh_consensus.c)
 *   ... --consensus PREFIX --consensus-pairs [--consensus-pairs-min N]   PREFIXconsensus_pairs.txt, _identity.txt, _compared.txt: every two samples' consensus rows compared per reference (bh_conspairs.c)
 *   ... --vcf --vcf-study PREFIX       PREFIXstudy.vcf: every sample's DP:AD at every record any sample's OUT.vcf has (bh_vcfstudy.c)
 *   ... -q / -o or --samples ... --vcf [--vcf-min-depth N] [--vcf-min-alt N] [--vcf-reads all|unique] [--vcf-lengths FILE]   OUT.vcf beside every .b6 output OUT: SNVs and indel alleles (bh_vcf.c)
 *   ... -q / -o or --samples ... --sam [--sam-unmapped] [--sam-lengths FILE]      OUT.sam beside every .b6 output OUT, with NM and MD tags (bh_sam.c)
 *
 * Flags not on the hot path (-f fingerprints, -p prepass, -x alphabet, -hr) are refused with the
 * reference's exit code 1.  Extra flags: --device N, --batch N (unique queries per device call), -k {12|15}.
 */
#define _GNU_SOURCE      /* getline */
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <omp.h>
#include <pthread.h>
#include <unistd.h>

#define BH_MAX_GPUS BH_MAX_RANKS
static double wall(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
static int code_to_exit(int rc) { return rc == BH_E_USAGE ? 1 : rc == BH_E_IO ? 2 : rc == BH_E_OOM ? 3 : 4; }
#define DIE(rc) do { fprintf(stderr, "%s\n", bh_last_error()); return code_to_exit(rc); } while (0)
#define NEEDARG(name) do { if (++i == argc || argv[i][0] == '-') { printf("ERROR: %s requires an argument\n", name); return 1; } } while (0)

/* make_accelerator (burst.c:3304-3532): on the device when there is one (tuples of every lane, radix sort, fold: bhip_init
 * with K and no tables, then bhip_acx_export), else -- or with --host-acx / -sa -- by the host builder.  Same bytes either way. */
static int build_accelerator(BhDb *db, int K, int z, int device, int on_host, int skip_ambig) {
	if (!on_host && !skip_ambig) {
		void *hh = NULL;
		uint8_t *keep = NULL;      /* a -d DNA database: the builder sees every lane cut at its fragment length (bh_db_trim_lanes) */
		int rc = bh_db_trim_lanes(db, &keep);
		if (rc) return rc;
		if (!bh_device_open_ex(db, device, z, K, &hh)) {
			rc = bh_acx_from_device(db, hh, K, z);
			bhip_destroy(hh);
			bh_db_untrim_lanes(db, keep);
			if (!rc) printf(" --> accelerator built on device %d\n", device);
			return rc;
		}
		bh_db_untrim_lanes(db, keep);
		printf(" --> no device accelerator build (%s); using the host builder\n", bh_last_error());
	}
	return bh_acx_build_ex(db, K, z, skip_ambig);
}

/* the query pipeline (process_queries, burst.c:2980-3223) on a thread of its own: with an .edx database nothing in it depends on
 * the database, so the file is read, indexed, sorted and de-duplicated while the main thread reads the database and brings it
 * onto the devices */
typedef struct { const char *fn; float thres; int do_rc, incl_ws, do_accel, K, z, skip_ambig; BhQueries *Q; int rc; char err[512]; double secs; } Ingest;
static void *ingest_main(void *p) {
	Ingest *a = p;
	const double t0 = wall();
	a->rc = bh_queries_load(a->fn, a->thres, a->do_rc, a->incl_ws, a->do_accel, a->K, a->z, a->skip_ambig, a->Q);
	if (a->rc) snprintf(a->err, sizeof a->err, "%s", bh_last_error());
	a->secs = wall() - t0;
	return NULL;
}

/* the database onto the devices of the n_gpus ranks (one host thread each): replicated, or -- shard_db -- rank r the clumps of shard
 * r % n_shards (slices[r], ranks[r].c0); prints the device lines; returns 0 or the exit code */
static int open_devices(const BhDb *db, int n_gpus, const int *dev_list, int shard_db, int n_shards, int accel_dev, int K, int z,
                        void **hhs, BhMultiRank *ranks, BhDb *slices) {
	int rcs[BH_MAX_GPUS]; char errs[BH_MAX_GPUS][512];
	for (int r = 0; r < BH_MAX_GPUS; ++r) rcs[r] = BH_E_INTERNAL;
	int shared_dev = 0;
	for (int a = 0; a < n_gpus; ++a) for (int b = a + 1; b < n_gpus; ++b) shared_dev |= dev_list[a] == dev_list[b];
	omp_set_dynamic(0);
	/* A replicated database whose accelerator is built on the devices (-ad): the ranks build it TOGETHER, each the lists of 1/N of the words,
	 * and complete each other's tables device to device (bhip_build_accelerator_shared + bhip_team_share; BURST_HIP_SOLO_BUILD=1: every
	 * rank builds the whole thing as before).  The gates of the devices are held here, around the ranks: ranks on one device meet inside. */
	void *team = NULL;
	const int coop = n_gpus > 1 && !shard_db && accel_dev && !db->hasAcx && !getenv("BURST_HIP_SOLO_BUILD");
	if (coop && bhip_team_create(n_gpus, &team)) { fprintf(stderr, "libburst_hip: %s\n", bhip_last_error()); return 4; }
	if (coop) {
		for (int a = 0; a < n_gpus; ++a) { int seen = 0; for (int b = 0; b < a; ++b) seen |= dev_list[a] == dev_list[b]; if (!seen) bh_device_gate(dev_list[a], 1); }
		printf("Accelerator: built by the %d ranks together (word ranges, device-to-device exchange)\n", n_gpus);
	}
	#pragma omp parallel num_threads(n_gpus)
	{
		const int r = omp_get_thread_num();
		const BhDb *part = db;
		rcs[r] = BH_OK;
		if (coop) {
			if (omp_get_num_threads() != n_gpus) rcs[r] = BH_E_INTERNAL;      /* (no team: nobody enters the exchange) */
			else if ((rcs[r] = bh_device_open_shared(db, dev_list[r], z, K, r, n_gpus, bhip_team_share, team, &hhs[r]))) snprintf(errs[r], sizeof errs[r], "%s", bh_last_error());
		} else {
		if (shard_db) {      /* this rank's clumps: a view of the clump area + (with an .acx) the lists restricted to it */
			uint32_t c0, c1;
			bh_clump_shard(db, n_shards, r % n_shards, &c0, &c1);
			ranks[r].c0 = c0;
			if ((rcs[r] = bh_db_slice(db, c0, c1, &slices[r]))) snprintf(errs[r], sizeof errs[r], "%s", bh_last_error());
			part = &slices[r];
		}
		/* ranks that share a device (--devices 0,0,...: diagnostics on a one-GPU machine) open their handles one after the other:
		 * the accelerator build sizes its scratch from the memory that is free when it starts */
		if (!rcs[r] && shared_dev) {
			#pragma omp critical (bh_device_open)
			if ((rcs[r] = bh_device_open_ex(part, dev_list[r], z, accel_dev ? K : 0, &hhs[r]))) snprintf(errs[r], sizeof errs[r], "%s", bh_last_error());
		} else if (!rcs[r] && (rcs[r] = bh_device_open_ex(part, dev_list[r], z, accel_dev ? K : 0, &hhs[r]))) snprintf(errs[r], sizeof errs[r], "%s", bh_last_error());
		}
	}
	if (coop) for (int a = 0; a < n_gpus; ++a) { int seen = 0; for (int b = 0; b < a; ++b) seen |= dev_list[a] == dev_list[b]; if (!seen) bh_device_gate(dev_list[a], 0); }
	if (team) bhip_team_destroy(team);
	for (int r = 0; r < n_gpus; ++r) if (rcs[r]) { fprintf(stderr, "%s\n", rcs[r] == BH_E_INTERNAL ? "OpenMP did not start one host thread per GPU" : errs[r]); return 4; }
	for (int r = 0; r < n_gpus; ++r) { char nm[256]; int ncu = 0; uint64_t hbm = 0; if (!bhip_device_info(hhs[r], nm, sizeof nm, &ncu, &hbm)) printf("Device %d: %s, %d CUs, %.0f GiB\n", dev_list[r], nm, ncu, hbm / 1073741824.0); }
	if (shard_db) for (int r = 0; r < n_gpus; ++r) printf("Rank %d: replica group %d, clumps [%u, %u)\n", r, r / n_shards, ranks[r].c0, ranks[r].c0 + slices[r].numRclumps);
	return 0;
}

static void print_taxa_written(const char *prefix, uint32_t n_levels, uint32_t n_em_levels) {
	printf("Taxon tables written: %staxa.txt, %staxa_L<k>.txt for k = 1 .. %u", prefix, prefix, n_levels);
	if (n_em_levels) printf(", %staxa_abundance_L<k>.txt likewise", prefix);
	putchar('\n');
}

/* ---- --samples LIST: a list of query files against one resident database, each to its own .b6 (bh_session.c) ---- */
typedef struct {
	const char *ref_FN, *xcel_FN, *tax_FN, *list_FN;
	BhMode mode; float thres; int z, do_rc, incl_ws, do_accel, accel_dev, K, skip_ambig, rep_flags, threads, device;
	int n_gpus, n_gpus_given, n_dev_list, *dev_list, shard_db, n_shards; uint64_t batch; BhTaxOpts *txo;
	const char *cov_prefix, *cov_lengths; uint32_t cov_pad; int cigar;
	const char *q1_FN, *mates_FN, *out_FN;      /* --mates: the one pair of -q / --mates / -o in place of a list (list_FN = NULL) */
	BhMatesOpts mates; int mates_opts_given;
	const char *em_prefix; uint32_t em_iters; uint64_t em_tol;
	const char *var_prefix; uint32_t var_min_depth, var_min_alt; int var_unique;
	int sam, sam_unmapped; const char *sam_lengths;
	const char *cons_prefix; uint32_t cons_min_depth, cons_min_breadth; int cons_unique; const char *cons_lengths;
	int vcf; uint32_t vcf_min_depth, vcf_min_alt; int vcf_unique; const char *vcf_lengths;
	const char *taxa_prefix; uint32_t taxa_agree;
	const char *vcf_study;
	int cons_pairs; uint32_t cons_pairs_min;
} SamplesArgs;
typedef struct { char *q, *o, *m; int line; } Sample;      /* m: the mates file of a three-field line, or NULL */

/* `queries<TAB>output` or `queries<TAB>output<TAB>mates` per line; blank lines and lines that start with '#' are skipped.  Returns 0 or the exit code. */
static int read_sample_list(const SamplesArgs *a, Sample **out, int *n_out) {
	FILE *f = fopen(a->list_FN, "rb");
	if (!f) { fprintf(stderr, "ERROR: Cannot open sample list: %s\n", a->list_FN); return 2; }
	Sample *S = NULL; int n = 0, cap = 0, line = 0;
	char *buf = NULL; size_t bcap = 0;
	while (getline(&buf, &bcap, f) >= 0) {
		++line;
		size_t len = strlen(buf);
		while (len && (buf[len - 1] == '\n' || buf[len - 1] == '\r')) buf[--len] = 0;
		if (!len || buf[0] == '#') continue;
		char *tab = strchr(buf, '\t');
		char *tab2 = tab ? strchr(tab + 1, '\t') : NULL;
		if (!tab || tab == buf || !tab[1] || tab2 == tab + 1 || (tab2 && (!tab2[1] || strchr(tab2 + 1, '\t')))) { printf("ERROR: %s line %d: expected 'queries<TAB>output' or 'queries<TAB>output<TAB>mates'\n", a->list_FN, line); fclose(f); return 1; }
		*tab = 0;
		if (tab2) *tab2 = 0;
		if (n == cap) { cap = cap ? 2 * cap : 64; S = realloc(S, (size_t)cap * sizeof(*S)); if (!S) { fclose(f); fputs("OOM:samples\n", stderr); return 3; } }
		S[n].q = strdup(buf); S[n].o = strdup(tab + 1); S[n].m = tab2 ? strdup(tab2 + 1) : NULL; S[n].line = line;
		if (!S[n].q || !S[n].o || (tab2 && !S[n].m)) { fclose(f); fputs("OOM:samples\n", stderr); return 3; }
		++n;
	}
	free(buf); fclose(f);
	if (!n) { printf("ERROR: %s names no sample\n", a->list_FN); return 1; }
	for (int i = 0; i < n; ++i) {
		for (int k = 0; k < i; ++k) if (!strcmp(S[i].o, S[k].o)) { printf("ERROR: %s line %d: output '%s' is the output of line %d already\n", a->list_FN, S[i].line, S[i].o, S[k].line); return 1; }
		for (int k = 0; k < n; ++k) if (!strcmp(S[i].o, S[k].q) || (S[k].m && !strcmp(S[i].o, S[k].m))) { printf("ERROR: %s line %d: output '%s' is the query file of line %d\n", a->list_FN, S[i].line, S[i].o, S[k].line); return 1; }
		if (!strcmp(S[i].o, a->ref_FN) || (a->xcel_FN && !strcmp(S[i].o, a->xcel_FN)) || !strcmp(S[i].o, a->list_FN)) {
			printf("ERROR: %s line %d: output '%s' is the database, the accelerator or the list itself\n", a->list_FN, S[i].line, S[i].o); return 1;
		}
	}
	*out = S; *n_out = n;
	return 0;
}

/* the consensus of a run: closed on every way out, so that a run that ends on an error leaves neither file nor temporary file */
static BhCons *g_cons;
static BhConsPairs *g_conspairs;      /* --consensus-pairs: the collector of the consensus's written rows */
static void close_consensus(void) { bh_consensus_close(g_cons); g_cons = NULL; bh_conspairs_close(g_conspairs); g_conspairs = NULL; }
static void cons_atexit(void) { close_consensus(); }
/* opened before a device is touched: the lengths table is checked against the database's headers.  pairs_min: 0, or --consensus-pairs-min */
static int open_consensus(const BhDb *db, const char *prefix, const char *lengths, uint32_t min_depth, uint32_t min_breadth, int unique, uint32_t pairs_min) {
	if (!db->refMap || !db->numRefHeads) { puts("ERROR: --consensus needs the reference headers of the database"); return 1; }
	int rc = bh_consensus_open(db, prefix, lengths, min_depth, min_breadth, unique, &g_cons);
	if (!rc && pairs_min && !(rc = bh_conspairs_open(prefix, pairs_min, &g_conspairs))) bh_conspairs_attach(g_conspairs, g_cons);
	atexit(cons_atexit);
	if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; }
	if (rc) { fprintf(stderr, "%s\n", bh_last_error()); return code_to_exit(rc); }
	return 0;
}
/* the end of a run with --consensus: with --consensus-pairs the one call on rank 0's handle and the three files, then all files get their
 * names together.  Returns 0 or the exit code */
static int write_consensus(void *hh, const char *prefix) {
	int rc = g_conspairs ? bh_consensus_pairs(g_cons, hh) : BH_OK;
	if (!rc) rc = bh_consensus_write(g_cons);
	if (rc) { if (rc == BH_E_USAGE) puts(bh_last_error()); else fprintf(stderr, "%s\n", bh_last_error()); fflush(NULL); return code_to_exit(rc); }
	if (g_conspairs) bh_conspairs_print_info(g_conspairs);
	printf("Consensus written: %sconsensus.fa, %sconsensus.txt\n", prefix, prefix);
	if (g_conspairs) printf("Consensus pairs written: %sconsensus_pairs.txt, %sconsensus_identity.txt, %sconsensus_compared.txt\n", prefix, prefix, prefix);
	return 0;
}
/* the VCF writer of a run: closed on every way out */
static BhVcf *g_vcf;
static void vcf_atexit(void) { bh_vcf_close(g_vcf); g_vcf = NULL; }
/* opened before a device is touched: two headers of one name, a lengths table without a header */
static int open_vcf(const BhDb *db, const char *lengths, uint32_t min_depth, uint32_t min_alt, int unique) {
	if (!db->refMap || !db->numRefHeads) { puts("ERROR: --vcf needs the reference headers of the database"); return 1; }
	const int rc = bh_vcf_open(db, lengths, min_depth, min_alt, unique, &g_vcf);
	if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; }
	if (rc) { fprintf(stderr, "%s\n", bh_last_error()); return code_to_exit(rc); }
	atexit(vcf_atexit);
	return 0;
}
/* the study VCF of a run: closed on every way out, so that a run that ends on an error leaves neither file nor temporary file */
static BhVcfStudy *g_vcfstudy;
static void vcfstudy_atexit(void) { bh_vcfstudy_close(g_vcfstudy); g_vcfstudy = NULL; }
static int open_vcfstudy(const char *prefix) {
	const int rc = bh_vcfstudy_open(prefix, &g_vcfstudy);
	if (rc) { fprintf(stderr, "%s\n", bh_last_error()); return code_to_exit(rc); }
	bh_vcf_set_study(g_vcf, g_vcfstudy);
	atexit(vcfstudy_atexit);
	return 0;
}
/* the end of a run with --vcf-study: the file, its line on standard output.  Returns 0 or the exit code */
static int write_vcfstudy(void *hh, const char *prefix) {
	const int rc = bh_vcfstudy_write(g_vcfstudy, g_vcf, hh);
	if (rc) { if (rc == BH_E_USAGE) puts(bh_last_error()); else fprintf(stderr, "%s\n", bh_last_error()); return code_to_exit(rc); }
	bh_vcfstudy_print_info(g_vcfstudy);
	printf("Study VCF written: %sstudy.vcf\n", prefix);
	return 0;
}
static int samples_main(SamplesArgs *a) {
	Sample *S = NULL; int nS = 0, rc;
	if (a->list_FN) { const int e = read_sample_list(a, &S, &nS); if (e) return e; }
	else {      /* --mates: a session of one pair */
		if (!(S = calloc(1, sizeof(*S))) || !(S[0].q = strdup(a->q1_FN)) || !(S[0].o = strdup(a->out_FN)) || !(S[0].m = strdup(a->mates_FN))) { fputs("OOM:samples\n", stderr); return 3; }
		nS = 1;
	}
	int any_mates = 0;
	for (int i = 0; i < nS; ++i) any_mates |= S[i].m != NULL;
	/* what a pair of mate files needs, checked before a device is touched */
	if (a->mates_opts_given && !any_mates) { puts("ERROR: --insert-min, --insert-max, --mates-orientation and --mates-report go with --mates (or a --samples line with a mates file)"); return 1; }
	if (any_mates && a->mode != BH_ALLPATHS && a->mode != BH_FORAGE) { puts("ERROR: mates are joined from the placements of -m ALLPATHS or -m FORAGE (BEST, CAPITALIST and ANY discard the ties the join needs)"); return 1; }
	if (any_mates && !a->do_rc) { puts("ERROR: a --samples line with a mates file needs both strands searched: add -fr"); return 1; }
	if (any_mates && (a->cigar || a->cov_prefix)) { puts("ERROR: --cigar and --coverage of paired output are out of scope: neither goes with mates"); return 1; }
	if (any_mates && a->em_prefix) { puts("ERROR: --abundance of paired output is out of scope: it does not go with mates"); return 1; }
	if (any_mates && a->taxa_prefix) { puts("ERROR: --taxa of paired output is out of scope: it does not go with mates"); return 1; }
	if (any_mates && a->var_prefix) { puts("ERROR: --variants of paired output are out of scope: they do not go with mates"); return 1; }
	if (any_mates && a->cons_prefix) { puts("ERROR: --consensus of paired output is out of scope: it does not go with mates"); return 1; }
	if (any_mates && a->vcf) { puts("ERROR: --vcf of paired output is out of scope: it does not go with mates"); return 1; }
	if (a->vcf_study) {      /* (two samples of one name would share a column: refused before a device is touched) */
		const char **outs = calloc((size_t)nS, sizeof(*outs));
		if (!outs) { fputs("OOM:samples\n", stderr); return 3; }
		for (int i = 0; i < nS; ++i) outs[i] = S[i].o;
		rc = bh_vcfstudy_check_names(outs, (uint64_t)nS);
		free(outs);
		if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; }
		if (rc) DIE(rc);
	}
	if (a->cons_pairs) {      /* (two samples of one name would share a row and a column of the matrices: refused before a device is touched) */
		const char **outs = calloc((size_t)nS, sizeof(*outs));
		if (!outs) { fputs("OOM:samples\n", stderr); return 3; }
		for (int i = 0; i < nS; ++i) outs[i] = S[i].o;
		rc = bh_conspairs_check_names(outs, (uint64_t)nS);
		free(outs);
		if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; }
		if (rc) DIE(rc);
	}
	if (any_mates && a->sam) { puts("ERROR: --sam of paired output (paired flags, RNEXT, TLEN) is out of scope: it does not go with mates"); return 1; }
	const int usedb = bh_is_edx(a->ref_FN);
	if (usedb < 0) DIE(usedb);
	/* direct FASTA references: their clumps depend on the longest query (burst.c:5151) -- there is nothing to keep resident */
	if (!usedb && !a->list_FN) { puts("ERROR: --mates needs an .edx database (FASTA references are clumped per query file: nothing would stay resident between the mates)"); return 1; }
	if (!usedb) { puts("ERROR: --samples needs an .edx database (the clumps of FASTA references depend on the queries: nothing would stay resident)"); return 1; }
	int K = a->K, shard_db = a->shard_db, n_shards = a->n_shards;
	const int n_gpus = a->n_gpus;
	if (n_gpus > BH_MAX_GPUS) { printf("ERROR: --gpus %d (max %d)\n", n_gpus, BH_MAX_GPUS); return 1; }
	if (shard_db && !n_shards) n_shards = n_gpus;
	if (!shard_db || n_shards < 2) { shard_db = 0; n_shards = 1; }
	/* more shards than devices: one upload per shard per search -- nothing stays resident either (out of scope for --samples) */
	if (shard_db && n_gpus == 1 && n_shards > 1 && !a->list_FN) { puts("ERROR: --mates needs a resident device handle: it does not go with the serial-shards path (--gpus 1 --shards S)"); return 1; }
	if (shard_db && n_gpus == 1 && n_shards > 1) { puts("ERROR: --samples does not take the serial-shards path (--gpus 1 --shards S uploads every shard for every search)"); return 1; }
	if (n_gpus % n_shards) { printf("ERROR: --shards %d does not divide --gpus %d\n", n_shards, n_gpus); return 1; }
	if (a->threads > 0) omp_set_num_threads(a->threads);
	const double start = wall();
	double tp = start;
	#define PHASE(name) do { const double t_ = wall(); printf(" [%-28s %8.3f s]\n", name, t_ - tp); tp = t_; } while (0)
	BhDb db; memset(&db, 0, sizeof db);
	BhTax taxonomy; memset(&taxonomy, 0, sizeof taxonomy);
	void *hhs[BH_MAX_GPUS]; BhMultiRank ranks[BH_MAX_GPUS]; BhDb slices[BH_MAX_GPUS];
	memset(hhs, 0, sizeof hhs); memset(ranks, 0, sizeof ranks); memset(slices, 0, sizeof slices);
	int dev_list[BH_MAX_GPUS];
	for (int r = 0; r < n_gpus; ++r) dev_list[r] = a->n_dev_list ? a->dev_list[r] : (a->n_gpus_given ? r : a->device);
	for (int r = 0; r < n_gpus; ++r) ranks[r].rank = r;
	if (a->do_accel && a->accel_dev && !K) K = 12;
	if (a->tax_FN) {                                                                 /* burst.c:5142-5149 (the session copies the options) */
		if ((rc = bh_tax_load(a->tax_FN, &taxonomy))) DIE(rc);
		a->txo->tax = &taxonomy;
	}
	/* the session first: the first sample is parsed on its ingest thread beside the database phases (as the single -q is) */
	BhSessionOpts so; memset(&so, 0, sizeof so);
	so.mode = a->mode; so.thres = a->thres; so.do_rc = a->do_rc; so.incl_ws = a->incl_ws; so.z = a->z; so.do_accel = a->do_accel; so.K = K;
	so.skip_ambig = a->skip_ambig; so.rep_flags = a->rep_flags; so.batch = a->batch; so.shard_db = shard_db ? n_shards : 0; so.tax = a->tax_FN ? a->txo : NULL;
	so.ingest_ahead = 1; so.verbose = 1; so.cigar = a->cigar; so.mates = a->mates;
	BhSession *ses = NULL;
	if ((rc = bh_session_open(&db, ranks, n_gpus, n_gpus, NULL, NULL, &so, &ses))) DIE(rc);
	bh_queries_sort_device(dev_list[0]);      /* large query files are sorted on the (first) search device */
	bh_session_prefetch(ses, S[0].q);
	#define DIES(rc) do { bh_session_close(ses); DIE(rc); } while (0)
	puts("\nEDB database provided. Parsing...");
	if ((rc = bh_edx_read(a->ref_FN, &db))) DIES(rc);
	if (db.xalpha) { bh_session_close(ses); fputs("ERROR: DB made with Xalpha; queries can't use Xalpha.\n", stderr); return 1; }
	printf(" --> EDB: %u refs [%u orig], %u clumps, %u maxR\n", db.totR, db.origTotR, db.numRclumps, db.maxLenR);
	if (a->do_accel && a->accel_dev) printf(" --> [Accel] K=%d, built on the device from the database\n", K);
	else if (a->do_accel) {
		if ((rc = bh_acx_read(a->xcel_FN, K, a->z, &db))) DIES(rc);      /* K = 0: 12 or 15, whichever the file's exact size says */
		K = db.K;
		printf(" --> [Accel] K=%d, %s format, %u ambiguous clumps\n", K, db.acxFmt ? "LARGE" : "SMALL", db.badSz);
	}
	PHASE("database read");
	BhCov *cov = NULL;
	if (a->cov_prefix) {      /* (the lengths table is checked against the database's headers before a device is touched) */
		if ((rc = bh_cov_open(&db, a->cov_prefix, a->cov_lengths, a->cov_pad, &cov))) DIES(rc);
		bh_session_set_coverage(ses, cov);
	}
	BhEm *em = NULL;
	if (a->em_prefix) {
		if ((rc = bh_em_open(&db, a->em_prefix, a->em_iters, a->em_tol, &em))) DIES(rc);
		bh_session_set_abundance(ses, em);
	}
	BhTaxa *taxa = NULL;
	if (a->taxa_prefix) {      /* (the tree of the map's strings is built, and a string of too many levels refused, before a device is touched) */
		if ((rc = bh_taxa_open(&db, a->taxa_prefix, &taxonomy, a->txo->ncbi, a->taxa_agree, &taxa)) || (rc = bh_session_set_taxa(ses, taxa))) { if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); bh_session_close(ses); return 1; } DIES(rc); }
	}
	BhSam *sam = NULL;
	if (a->sam) {      /* (the names and the lengths table are checked against the database's headers before a device is touched) */
		if ((rc = bh_sam_open(&db, a->sam_lengths, a->sam_unmapped, &sam)) || (rc = bh_session_set_sam(ses, sam))) { if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); bh_session_close(ses); return 1; } DIES(rc); }
	}
	if (a->cons_prefix) {
		const int e = open_consensus(&db, a->cons_prefix, a->cons_lengths, a->cons_min_depth, a->cons_min_breadth, a->cons_unique, a->cons_pairs ? a->cons_pairs_min : 0);
		if (e) { bh_session_close(ses); return e; }
		if ((rc = bh_session_set_consensus(ses, g_cons))) { if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); bh_session_close(ses); return 1; } DIES(rc); }
	}
	if (a->vcf) {
		const int e = open_vcf(&db, a->vcf_lengths, a->vcf_min_depth, a->vcf_min_alt, a->vcf_unique);
		if (e) { bh_session_close(ses); return e; }
		if ((rc = bh_session_set_vcf(ses, g_vcf))) { if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); bh_session_close(ses); return 1; } DIES(rc); }
		if (a->vcf_study) { const int e2 = open_vcfstudy(a->vcf_study); if (e2) { bh_session_close(ses); return e2; } }
	}
	if (shard_db && (uint32_t)n_shards > db.numRclumps) { bh_session_close(ses); puts("ERROR: more database shards than clumps"); return 1; }
	{ const int e = open_devices(&db, n_gpus, dev_list, shard_db, n_shards, a->accel_dev, K, a->z, hhs, ranks, slices); if (e) { bh_session_close(ses); return e; } }
	for (int r = 0; r < n_gpus; ++r) ranks[r].hh = hhs[r];
	PHASE("device database upload");
	BhPile *pile = NULL;      /* (opened last: its table grows under a temporary name from here on) */
	if (a->var_prefix) {
		if ((rc = bh_pile_open(&db, a->var_prefix, a->var_min_depth, a->var_min_alt, a->var_unique, &pile))) DIES(rc);
		bh_session_set_variants(ses, pile);
	}
	int n_failed = 0, first_fail = 0, n_done = 0;
	for (int i = 0; i < nS; ++i) {
		if (S[i].m) printf("Sample %d/%d: %s + %s -> %s\n", i + 1, nS, S[i].q, S[i].m, S[i].o);
		else printf("Sample %d/%d: %s -> %s\n", i + 1, nS, S[i].q, S[i].o);
		/* (a pair prefetches its own second file; the sample after a pair is read when its turn comes) */
		if (i + 1 < nS && !S[i].m) bh_session_prefetch(ses, S[i + 1].q);
		BhSampleResult res;
		rc = S[i].m ? bh_session_run_mates(ses, S[i].q, S[i].m, S[i].o, &res) : bh_session_run(ses, S[i].q, S[i].o, &res);
		if (rc) {
			printf("Sample %d/%d FAILED (exit code %d): %s\n", i + 1, nS, code_to_exit(rc), res.err);
			if (!n_failed++) first_fail = code_to_exit(rc);
			/* usage and I/O errors are the sample's own; after anything else nothing more is started on a device */
			if (bh_session_ended(ses)) { n_failed += nS - 1 - i; printf("The session ends here: %d sample(s) not started\n", nS - 1 - i); break; }
		} else ++n_done;
		fflush(stdout);
	}
	if (cov && !bh_session_ended(ses)) {
		tp = wall();
		if ((rc = bh_cov_write(cov))) { fprintf(stderr, "%s\n", bh_last_error()); if (!first_fail) first_fail = code_to_exit(rc); }
		else { printf("Coverage tables written: %sshared.txt, %sunique.txt, %sshared_binary.txt, %sunique_binary.txt, %scounts.txt\n", a->cov_prefix, a->cov_prefix, a->cov_prefix, a->cov_prefix, a->cov_prefix); PHASE("coverage tables"); bh_cov_print_info(cov); }
	} else if (cov) puts("No coverage tables are written: the run ended on an error");
	if (em && !bh_session_ended(ses)) {
		tp = wall();
		if ((rc = bh_em_write(em))) { fprintf(stderr, "%s\n", bh_last_error()); if (!first_fail) first_fail = code_to_exit(rc); }
		else { printf("Abundance table written: %sabundance.txt\n", a->em_prefix); PHASE("abundance table"); }
	} else if (em) puts("No abundance table is written: the run ended on an error");
	if (taxa && !bh_session_ended(ses)) {
		uint32_t nl = 0, nel = 0;
		tp = wall();
		if ((rc = bh_taxa_write(taxa, &nl, &nel))) { fprintf(stderr, "%s\n", bh_last_error()); if (!first_fail) first_fail = code_to_exit(rc); }
		else { print_taxa_written(a->taxa_prefix, nl, nel); PHASE("taxon tables"); }
	} else if (taxa) puts("No taxon tables are written: the run ended on an error");
	if (pile && !bh_session_ended(ses)) {
		if ((rc = bh_pile_write(pile))) { fprintf(stderr, "%s\n", bh_last_error()); if (!first_fail) first_fail = code_to_exit(rc); }
		else printf("Variants table written: %svariants.txt\n", a->var_prefix);
	} else if (pile) puts("No variants table is written: the run ended on an error");
	bh_pile_close(pile); pile = NULL;      /* (a table that was not written leaves no temporary file) */
	if (g_cons && !bh_session_ended(ses)) {
		tp = wall();      /* (with --consensus-pairs: one bhip_consensus_pairs call on rank 0's handle before the files get their names) */
		const int e = write_consensus(hhs[0], a->cons_prefix);
		if (e) { if (!first_fail) first_fail = e; } else if (g_conspairs) PHASE("consensus pairs");
	} else if (g_cons) puts("No consensus is written: the run ended on an error");
	close_consensus();
	if (g_vcfstudy && !bh_session_ended(ses)) {      /* one bhip_site_counts call per sample on rank 0's handle, then the file */
		tp = wall();
		const int e = write_vcfstudy(hhs[0], a->vcf_study);
		if (e) { if (!first_fail) first_fail = e; } else PHASE("study VCF");
	} else if (g_vcfstudy) puts("No study VCF is written: the run ended on an error");
	bh_vcfstudy_close(g_vcfstudy); g_vcfstudy = NULL;
	bh_vcf_close(g_vcf); g_vcf = NULL;     /* (every sample's file was renamed or removed when the sample ended) */
	bh_sam_close(sam); sam = NULL;         /* (every sample's file was renamed or removed when the sample ended) */
	printf("\nSamples: %d done, %d failed. Alignment time: %f seconds\n", n_done, n_failed, wall() - start);
	fflush(NULL);
	#undef PHASE
	#undef DIES
	if (!getenv("BURST_HOST_TEARDOWN")) _exit(first_fail);      /* (as the single-sample path: the operating system releases a finished process's memory faster) */
	bh_session_close(ses);
	bh_cov_close(cov); bh_em_close(em); bh_taxa_close(taxa);
	for (int r = 0; r < n_gpus; ++r) { bhip_destroy(hhs[r]); bh_run_free(&ranks[r].run); if (slices[r].numRclumps) bh_db_free(&slices[r]); }
	bh_db_free(&db); bh_tax_free(&taxonomy);
	for (int i = 0; i < nS; ++i) { free(S[i].q); free(S[i].o); free(S[i].m); }
	free(S);
	return first_fail;
}

/* the single-sample path's SAM writer: closed on every way out of the run, so that a run that ends on an error leaves no file */
static BhSam *g_sam;
static void sam_atexit(void) { bh_sam_close(g_sam); g_sam = NULL; }

static void usage(void) {
	puts("\nburst_hip: BURST-compatible optimal aligner, MI355X (gfx950) device path");
	puts("--references (-r) <name>: FASTA/edx DB of reference sequences [required]");
	puts("--accelerator (-a) <name>: Creates/uses a helper DB (acx) [optional]");
	puts("--queries (-q) <name>: FASTA file of queries to search [required if aligning]");
	puts("--output (-o) <name>: Blast6/edx file for output alignments/database [required]");
	puts("--forwardreverse (-fr), --whitespace (-w), --nwildcard (-y), --mode (-m) BEST|ALLPATHS|CAPITALIST|FORAGE|ANY");
	puts("--makedb (-d) [name qLen], --id (-i) <decimal>, --threads (-t) <int>, --shear (-s) [len], --noprogress");
	puts("   -d DNA|RNA with -s: the compressive build (shears start at duplicated regions; marks on the device, else the host)");
	puts("--dbpartition (-dp) <int>: -d DNA marks in this many slices of the references (less memory)");
	puts("--taxonomy (-b) <name>, --taxacut (-bc) <num>, --taxa_ncbi (-bn), --taxasuppress (-bs) [STRICT]: taxonomy column (interpolated in CAPITALIST)");
	puts("--gpus <int> [--devices a,b,...] [--gather host|rccl]: shard the queries over the GPUs of this node; every rank's records reach host");
	puts("   memory over its own PCIe link and meet there (host, default) or are gathered over RCCL / xGMI to rank 0's device first (rccl)");
	puts("--shard queries|db: with --gpus, cut the queries (database replicated; default) or the database (every rank holds a range of");
	puts("                    clumps and aligns all queries; one all-reduce of the per-query minimum) -- for databases beyond one device");
	puts("--shards <S>: database shards (implies --shard db; default = --gpus): the ranks form gpus / S replica groups of S shards, the queries cut over the groups");
	puts("--device <int>, --batch <int>, -k <12|15>, --make-acx <name> (with -r DB.edx: rebuild the accelerator of a database)");
	puts("--accelerator-device (-ad): no .acx file, the device builds the accelerator from the .edx (word length -k, default 12)");
	puts("--samples <list>: align a list of query files against the one resident database, each to its own output; one sample per line,");
	puts("                  'queries<TAB>output' (in place of -q / -o; needs -r DB.edx; the database is read, uploaded and indexed once)");
	puts("--mates <name>: paired-end reads: -q holds mate 1, --mates mate 2 (paired by name, a trailing /1 or /2 ignored); -o gets every concordant");
	puts("    combination of a line of mate 1 and a line of mate 2 on the same reference as those two lines, each followed by the fragment's leftmost");
	puts("    position and its length.  Needs -r DB.edx and -m ALLPATHS or FORAGE; -fr is implied.  In a --samples list: a third field on the line;");
	puts("    such a list needs -fr given (it holds for every line: the two-field lines run as the flags say)");
	puts("--insert-min <int> (0), --insert-max <int> (1000): bounds of the fragment length; --mates-orientation fr|rf|ff (fr); --mates-report all|best (all)");
	puts("--cigar: with -q / -o or --samples, two further columns per line: the leftmost 1-based reference position of the alignment path and");
	puts("    its CIGAR in =XID (I: query symbol without a reference column, D: reference column without a query symbol)");
	puts("--coverage <prefix> [--coverage-lengths <file>] [--coverage-pad <int>]: with -q / -o or --samples, leave coverage and count tables per");
	puts("                  reference and sample next to the .b6 files: <prefix>shared.txt, unique.txt, shared_binary.txt, unique_binary.txt,");
	puts("                  counts.txt; lengths from a 'name<TAB>length' table, else the database's own extent of every reference");
	puts("--abundance <prefix> [--abundance-iters <int>] [--abundance-tol <units>]: with -q / -o or --samples, leave <prefix>abundance.txt: per reference and");
	puts("                  sample the reads, a read placed on several references split over them by expectation-maximisation (every -m mode; ALLPATHS");
	puts("                  gives it the ties); at most --abundance-iters iterations (1000), until no count moves by more than --abundance-tol (1024)");
	puts("                  units of 2^-30 read");
	puts("--variants <prefix> [--variants-min-depth <int>] [--variants-min-alt <int>] [--variants-reads all|unique]: with -q / -o or --samples, leave");
	puts("                  <prefix>variants.txt: per sample the reference positions where its reads differ from the reference, with the reads per base");
	puts("                  (Depth, A, C, G, T, Del, Other) and the insertions behind the position (Ins), counted from the alignment paths of the");
	puts("                  printed lines; a position is listed when its reference base is A/C/G/T, Depth >= --variants-min-depth (4) and the reads");
	puts("                  that differ, or Ins, are >= --variants-min-alt (2); --variants-reads unique counts only reads printed on one line");
	puts("--consensus <prefix> [--consensus-min-depth <int>] [--consensus-min-breadth <permille>] [--consensus-reads all|unique] [--consensus-lengths <file>]:");
	puts("                  with -q / -o or --samples, leave <prefix>consensus.fa and <prefix>consensus.txt: per sample and reference header the sequence the");
	puts("                  sample's reads show, in REFERENCE coordinates (every record has the reference's length, from a 'name<TAB>length' table as");
	puts("                  --coverage-lengths takes, else the database's own extent): at a position with Depth >= --consensus-min-depth (4) the largest of");
	puts("                  the counts A, C, G, T, Del of --variants (the reference's base among equals, then that order; - for Del; the reference's own");
	puts("                  letter where it is an ambiguity code), N elsewhere.  Insertions are counted (InsMajor), not written.  A record is written when");
	puts("                  a position was called and 1000 * Called >= --consensus-min-breadth (0) * length; the table has a row per covered (sample,");
	puts("                  header).  --consensus-reads unique counts only reads printed on one line.  Refuses what --variants refuses");
	puts("--consensus-pairs [--consensus-pairs-min <int>]: with --consensus, compare the written records of every reference between every two samples and");
	puts("                  leave <prefix>consensus_pairs.txt (per reference and pair a < b in study order: Length, Compared = positions where both rows");
	puts("                  show one of A C G T -, Same, Differ, Identity = Same / Compared; rows with Compared >= --consensus-pairs-min (1)),");
	puts("                  <prefix>consensus_identity.txt (samples x samples, sum Same / sum Compared over the pair's rows, NA without one) and");
	puts("                  <prefix>consensus_compared.txt (the sums Compared; the diagonal is the sample's own comparable positions).  N and ambiguity");
	puts("                  letters are never compared.  A sample that failed alone reads NA throughout.  Two samples of one name are refused");
	puts("--vcf [--vcf-min-depth <int>] [--vcf-min-alt <int>] [--vcf-reads all|unique] [--vcf-lengths <file>]: with -q / -o or --samples, leave OUT.vcf");
	puts("                  beside every output OUT (VCFv4.2, one sample, no genotypes): a contig line per reference (ID and length as --sam's @SQ), and from");
	puts("                  the alignment paths of the printed lines three kinds of records at positions with Depth >= --vcf-min-depth (4): an SNV where the");
	puts("                  reference base is A/C/G/T and another base has >= --vcf-min-alt (2) reads; a deletion, REF the base before it and the deleted");
	puts("                  reference bases; an insertion of at most 15 bases, ALT the base before it and the inserted bases -- each indel allele with");
	puts("                  >= --vcf-min-alt reads.  INFO DP=Depth, sample field DP:AD (for an indel AD's first number is the observing reads without this");
	puts("                  allele).  An indel at an end of a path or directly behind the other kind is no allele; nothing is left-aligned.  --vcf-reads");
	puts("                  unique counts only reads printed on one line.  Refuses what --variants refuses, and --cluster and --chimeras");
	puts("--vcf-study <prefix>: with --vcf, leave <prefix>study.vcf as well: one multi-sample VCF with a record wherever at least one sample's OUT.vcf has");
	puts("                  one (an SNV's ALT is the union of the samples' ALTs) and a column per sample in study order, named as the coverage tables name");
	puts("                  them.  Every sample's DP:AD is given at every record with no threshold applied: a sample that shows the reference there has its");
	puts("                  reads on the first AD number, one without a read prints 0:0,0, one that failed alone prints '.'.  INFO DP=<sum of the depths>;");
	puts("                  NS=<samples with a read there>.  No pooled call and no genotypes; -q / -o is a study of one sample.  Two samples of one name are");
	puts("                  refused.  OUT.vcf keeps its bytes");
	puts("--cluster <prefix> [--cluster-sizes]: with -q reads -r the same reads (FASTA or .edx) -m FORAGE, greedy centroid clusters of the reads from the");
	puts("                  lines they print against each other: the reads in the order of their weight (1, or with --cluster-sizes the N of a trailing");
	puts("                  ;size=N of the name), ties in file order; a read with a line to an earlier centroid joins the one with the fewest edits, any");
	puts("                  other read is a centroid.  Leaves <prefix>clusters.txt (per read) and <prefix>cluster_sizes.txt (per centroid)");
	puts("--chimeras <prefix> [--chimera-sizes] [--chimera-skew S] [--chimera-min-seg G] [--chimera-min-gain D]: with -q reads -r the same reads -m FORAGE, a de-novo");
	puts("                  two-parent chimera check.  Weights and priority as in --cluster (--chimera-sizes: the N of a trailing ;size=N).  A candidate parent");
	puts("                  of a read weighs at least S (2) times as much; per (read, parent) the line with the fewest edits counts, the first among equals.");
	puts("                  The edit positions of its alignment path, in read orientation, give for every cut c in [G, length - G] (G = 16) the edits left");
	puts("                  (positions <= 2c in doubled coordinates) and right of it.  Model = the smallest sum over the cuts of the fewest edits left over all");
	puts("                  parents and the fewest right (ties: higher priority, smaller cut); Single = the fewest edits of one line.  Role Y when");
	puts("                  Single - Model >= D (3), else N; - = not evaluated (fewer than two parents with a line, or no cut).  Leaves <prefix>chimeras.txt");
	puts("--sam [--sam-unmapped] [--sam-lengths <file>]: with -q / -o or --samples, leave OUT.sam beside every output OUT: @HD, one @SQ per reference");
	puts("                  header (SN = the header up to its first white space; LN from a 'name<TAB>length' table as --coverage-lengths takes, else");
	puts("                  the database's own extent), @PG, and one record per printed line in the order of the lines: FLAG 0x10 for a reverse line,");
	puts("                  0x100 on every line of a read but its first; POS and CIGAR (=XID) as --cigar prints them; MAPQ 255; SEQ of the strand");
	puts("                  that was aligned; QUAL *; NM:i: = column 11; MD:Z: = samtools calmd's string over the path, a match being an '=' op: the");
	puts("                  count of matches, then the reference base under every X, ^ and the reference bases under every D, the count again, also");
	puts("                  when it is 0 (3=2D1X4= gives 3^AC0T4; I adds nothing).  --sam-unmapped: behind them one FLAG 4 record per read without a");
	puts("                  line, in query-file order.  Refuses what --cigar refuses, and --mates");
	puts("--taxa <prefix> [--taxa-agree <permille>]: with -q / -o or --samples and -b <map>, leave taxon tables per sample: every read goes to the lowest");
	puts("                  common ancestor of the taxonomies of the references it was placed on (at least <permille> of them, 501 .. 1000, default 1000:");
	puts("                  all of them): <prefix>taxa.txt, <prefix>taxa_L<k>.txt per level, with --abundance also <prefix>taxa_abundance_L<k>.txt");
	puts("--host-acx: build accelerators (-d ... -a, --make-acx) with the host builder instead of the device");
}

int main(int argc, char **argv) {
	BhMode mode = BH_CAPITALIST;                    /* burst.c:81 */
	float thres = 0.97f;                            /* burst.c:93 */
	int xalpha = 0, cigar = 0;
	int dna_db = 0, dpart = 0;
	int z = 1, do_rc = 0, incl_ws = 0, makedb = 0, do_shear = 0, do_accel = 0, dedupe = 0, device = 0, K = 0, skip_ambig = 0, threads = 0, rep_flags = 0;
	long shear_amt = 500, db_qlen = 500;            /* burst.c:94 */
	uint32_t latency = 16;                          /* burst.c:83 */
	int n_gpus = 1, n_gpus_given = 0, gather_host = 1, n_dev_list = 0, dev_list[BH_MAX_GPUS], accel_dev = 0, host_acx = 0, shard_db = 0, n_shards = 0;
	uint64_t batch = 1u << 21;      /* unique queries per device batch: the fixed cost of a batch (launches, synchronisation) is about 1 ms of device time */
	const char *ref_FN = 0, *query_FN = 0, *output_FN = 0, *xcel_FN = 0, *mkacx_FN = 0, *tax_FN = 0, *samples_FN = 0, *cov_prefix = 0, *cov_lengths = 0;
	uint32_t cov_pad = 0;
	const char *taxa_prefix = 0; long long taxa_agree = 1000; int taxa_agree_given = 0;
	const char *em_prefix = 0; uint32_t em_iters = 1000; uint64_t em_tol = 1024; int em_opts_given = 0;
	const char *var_prefix = 0; uint32_t var_min_depth = 4, var_min_alt = 2; int var_unique = 0, var_opts_given = 0;
	const char *mates_FN = 0; BhMatesOpts mopts = {BHIP_MATES_FR, 0, 1000, BHIP_MATES_ALL}; int mates_opts_given = 0;
	const char *clu_prefix = 0; int clu_sizes = 0;
	int sam = 0, sam_unmapped = 0; const char *sam_lengths = 0;
	const char *vcf_study = 0;
	int vcf = 0, vcf_unique = 0, vcf_opts_given = 0; uint32_t vcf_min_depth = 4, vcf_min_alt = 2; const char *vcf_lengths = 0;
	const char *cons_prefix = 0, *cons_lengths = 0; uint32_t cons_min_depth = 4, cons_min_breadth = 0; int cons_unique = 0, cons_opts_given = 0;
	int cons_pairs = 0, cons_pairs_min_given = 0; uint32_t cons_pairs_min = 1;
	const char *chi_prefix = 0; int chi_sizes = 0, chi_opts_given = 0; uint32_t chi_skew = 2, chi_min_seg = 16, chi_min_gain = 3;
	BhTax taxonomy; memset(&taxonomy, 0, sizeof taxonomy);
	BhTaxOpts txo; memset(&txo, 0, sizeof txo); txo.taxacut = 10;   /* burst.c:92 */
	setenv("GPU_MAX_HW_QUEUES", "8", 0);      /* HIP runtime: hardware queues for the library's four streams (read when the runtime starts) */
	printf("This is burst_hip [MI355X device path; BURST v1.0 semantics]\n");
	if (argc < 2) { usage(); return 1; }
	for (int i = 1; i < argc; ++i) {
		const char *a = argv[i];
		if (!strcmp(a, "--references") || !strcmp(a, "-r")) { NEEDARG("--references"); ref_FN = argv[i]; }
		else if (!strcmp(a, "--queries") || !strcmp(a, "-q")) { NEEDARG("--queries"); query_FN = argv[i]; }
		else if (!strcmp(a, "--output") || !strcmp(a, "-o")) { NEEDARG("--output"); output_FN = argv[i]; }
		else if (!strcmp(a, "--accelerator") || !strcmp(a, "-a")) { NEEDARG("--accelerator"); xcel_FN = argv[i]; do_accel = 1; }
		else if (!strcmp(a, "--accelerator-device") || !strcmp(a, "-ad")) { accel_dev = 1; do_accel = 1; }
		else if (!strcmp(a, "--host-acx")) host_acx = 1;
		else if (!strcmp(a, "--forwardreverse") || !strcmp(a, "-fr")) do_rc = 1;
		else if (!strcmp(a, "--whitespace") || !strcmp(a, "-w")) incl_ws = 1;
		else if (!strcmp(a, "--npenalize") || !strcmp(a, "-n")) z = 1;
		else if (!strcmp(a, "--nwildcard") || !strcmp(a, "-y")) z = 0;
		else if (!strcmp(a, "--mode") || !strcmp(a, "-m")) {
			NEEDARG("--mode");
			if (!strcmp(argv[i], "BEST")) mode = BH_BEST; else if (!strcmp(argv[i], "ALLPATHS")) mode = BH_ALLPATHS;
			else if (!strcmp(argv[i], "CAPITALIST")) mode = BH_CAPITALIST; else if (!strcmp(argv[i], "FORAGE")) mode = BH_FORAGE;
			else if (!strcmp(argv[i], "ANY")) mode = BH_ANY;
			else { printf("Unsupported run mode '%s'\n", argv[i]); return 1; }
		}
		else if (!strcmp(a, "--makedb") || !strcmp(a, "-d")) {
			makedb = 1;
			if (i + 1 != argc && argv[i + 1][0] != '-' && !atol(argv[i + 1])) {
				++i;
				if (strcmp(argv[i], "DNA") && strcmp(argv[i], "RNA") && strcmp(argv[i], "QUICK")) { printf("Unsupported makedb mode '%s'\n", argv[i]); return 1; }
				dna_db = strcmp(argv[i], "QUICK") != 0;
			}
			if (i + 1 != argc && argv[i + 1][0] != '-') { db_qlen = atol(argv[++i]); if (db_qlen <= 0) { fprintf(stderr, "ERROR: bad max query length '%s'\n", argv[i]); return 1; } }
		}
		else if (!strcmp(a, "--id") || !strcmp(a, "-i")) {
			NEEDARG("--id"); thres = (float)atof(argv[i]);
			if (thres > 1.f || thres < 0.f) { puts("Invalid id range [0-1]"); return 1; }
			if (thres < 0.01f) thres = 0.01f;
		}
		else if (!strcmp(a, "--threads") || !strcmp(a, "-t")) { NEEDARG("--threads"); threads = atoi(argv[i]); }
		else if (!strcmp(a, "--shear") || !strcmp(a, "-s")) {
			do_shear = 1;
			if (i + 1 != argc && argv[i + 1][0] != '-') { shear_amt = atol(argv[++i]); if (shear_amt < 0) { printf("ERROR: bad shear length '%s'\n", argv[i]); return 1; } }
			if (!shear_amt) do_shear = 0;
		}
		else if (!strcmp(a, "--unique") || !strcmp(a, "-u")) dedupe = 1;
		else if (!strcmp(a, "--skipambig") || !strcmp(a, "-sa")) skip_ambig = 1;
		else if (!strcmp(a, "--noprogress")) { }
		else if (!strcmp(a, "--no-dupe-hunt")) rep_flags |= BH_REP_NO_DUPE_HUNT;   /* diagnostics: print every (hit, reference) expansion */
		else if (!strcmp(a, "--samples")) { NEEDARG("--samples"); samples_FN = argv[i]; }
		else if (!strcmp(a, "--make-acx")) { NEEDARG("--make-acx"); mkacx_FN = argv[i]; }
		else if (!strcmp(a, "--coverage")) { NEEDARG("--coverage"); cov_prefix = argv[i]; }
		else if (!strcmp(a, "--taxa")) { NEEDARG("--taxa"); taxa_prefix = argv[i]; }
		else if (!strcmp(a, "--taxa-agree")) {
			NEEDARG("--taxa-agree");
			char *end = NULL; taxa_agree = strtoll(argv[i], &end, 10);
			if (!*argv[i] || *end) taxa_agree = -1;
			taxa_agree_given = 1;
		}
		else if (!strcmp(a, "--abundance")) { NEEDARG("--abundance"); em_prefix = argv[i]; }
		else if (!strcmp(a, "--abundance-iters") || !strcmp(a, "--abundance-tol")) {
			const int is_tol = !strcmp(a, "--abundance-tol");
			NEEDARG(a);
			char *end = NULL; const unsigned long long v = strtoull(argv[i], &end, 10);
			if (!*argv[i] || *argv[i] == '-' || *end || (!is_tol && (!v || v > 0xFFFFFFFFull))) { printf("ERROR: %s takes %s\n", a, is_tol ? "a count of units of 2^-30 read (0 ..)" : "a number of iterations (1 .. 4294967295)"); return 1; }
			if (is_tol) em_tol = v; else em_iters = (uint32_t)v;
			em_opts_given = 1;
		}
		else if (!strcmp(a, "--cigar")) cigar = 1;
		else if (!strcmp(a, "--vcf")) vcf = 1;
		else if (!strcmp(a, "--vcf-min-depth") || !strcmp(a, "--vcf-min-alt")) {
			const int is_alt = !strcmp(a, "--vcf-min-alt");
			NEEDARG(a);
			char *end = NULL; const unsigned long long v = strtoull(argv[i], &end, 10);
			if (!*argv[i] || *end || argv[i][0] == '-' || !v || v > 0x7FFFFFFFull) { puts(is_alt ? "ERROR: --vcf-min-alt takes 1 .. 2147483647" : "ERROR: --vcf-min-depth takes 1 .. 2147483647"); return 1; }
			if (is_alt) vcf_min_alt = (uint32_t)v; else vcf_min_depth = (uint32_t)v;
			vcf_opts_given = 1;
		}
		else if (!strcmp(a, "--vcf-reads")) {
			NEEDARG("--vcf-reads"); vcf_opts_given = 1;
			if (!strcmp(argv[i], "all")) vcf_unique = 0; else if (!strcmp(argv[i], "unique")) vcf_unique = 1; else { puts("ERROR: --vcf-reads all|unique"); return 1; }
		}
		else if (!strcmp(a, "--vcf-study")) { NEEDARG("--vcf-study"); vcf_study = argv[i]; }
		else if (!strcmp(a, "--vcf-lengths")) { NEEDARG("--vcf-lengths"); vcf_lengths = argv[i]; vcf_opts_given = 1; }
		else if (!strcmp(a, "--sam")) sam = 1;
		else if (!strcmp(a, "--sam-unmapped")) sam_unmapped = 1;
		else if (!strcmp(a, "--sam-lengths")) { NEEDARG("--sam-lengths"); sam_lengths = argv[i]; }
		else if (!strcmp(a, "--cluster")) { NEEDARG("--cluster"); clu_prefix = argv[i]; }
		else if (!strcmp(a, "--cluster-sizes")) clu_sizes = 1;
		else if (!strcmp(a, "--chimeras")) { NEEDARG("--chimeras"); chi_prefix = argv[i]; }
		else if (!strcmp(a, "--chimera-sizes")) { chi_sizes = 1; chi_opts_given = 1; }
		else if (!strcmp(a, "--chimera-skew") || !strcmp(a, "--chimera-min-seg") || !strcmp(a, "--chimera-min-gain")) {
			NEEDARG(a);
			char *end = NULL; const unsigned long long v = strtoull(argv[i], &end, 10);
			if (!*argv[i] || *argv[i] == '-' || *end || !v || v > 0x7FFFFFFFull) { printf("ERROR: %s takes a number 1 .. 2147483647\n", a); return 1; }
			if (!strcmp(a, "--chimera-skew")) chi_skew = (uint32_t)v; else if (!strcmp(a, "--chimera-min-seg")) chi_min_seg = (uint32_t)v; else chi_min_gain = (uint32_t)v;
			chi_opts_given = 1;
		}
		else if (!strcmp(a, "--variants")) { NEEDARG("--variants"); var_prefix = argv[i]; }
		else if (!strcmp(a, "--variants-min-depth") || !strcmp(a, "--variants-min-alt")) {
			const int is_alt = !strcmp(a, "--variants-min-alt");
			NEEDARG(a);
			char *end = NULL; const unsigned long long v = strtoull(argv[i], &end, 10);
			if (!*argv[i] || *end || !v || v > 0x7FFFFFFFull) { printf("ERROR: %s takes a number of reads (1 .. 2147483647)\n", a); return 1; }
			if (is_alt) var_min_alt = (uint32_t)v; else var_min_depth = (uint32_t)v;
			var_opts_given = 1;
		}
		else if (!strcmp(a, "--variants-reads")) {
			NEEDARG("--variants-reads"); var_opts_given = 1;
			if (!strcmp(argv[i], "all")) var_unique = 0; else if (!strcmp(argv[i], "unique")) var_unique = 1; else { puts("ERROR: --variants-reads all|unique"); return 1; }
		}
		else if (!strcmp(a, "--consensus")) { NEEDARG("--consensus"); cons_prefix = argv[i]; }
		else if (!strcmp(a, "--consensus-min-depth") || !strcmp(a, "--consensus-min-breadth")) {
			const int is_breadth = !strcmp(a, "--consensus-min-breadth");
			NEEDARG(a);
			char *end = NULL; const unsigned long long v = strtoull(argv[i], &end, 10);
			if (!*argv[i] || *end || (is_breadth ? v > 1000 : !v || v > 0x7FFFFFFFull)) { puts(is_breadth ? "ERROR: --consensus-min-breadth takes 0 .. 1000 (permille of the reference's length)" : "ERROR: --consensus-min-depth takes 1 .. 2147483647"); return 1; }
			if (is_breadth) cons_min_breadth = (uint32_t)v; else cons_min_depth = (uint32_t)v;
			cons_opts_given = 1;
		}
		else if (!strcmp(a, "--consensus-reads")) {
			NEEDARG("--consensus-reads"); cons_opts_given = 1;
			if (!strcmp(argv[i], "all")) cons_unique = 0; else if (!strcmp(argv[i], "unique")) cons_unique = 1; else { puts("ERROR: --consensus-reads all|unique"); return 1; }
		}
		else if (!strcmp(a, "--consensus-lengths")) { NEEDARG("--consensus-lengths"); cons_lengths = argv[i]; cons_opts_given = 1; }
		else if (!strcmp(a, "--consensus-pairs")) cons_pairs = 1;
		else if (!strcmp(a, "--consensus-pairs-min")) {
			NEEDARG("--consensus-pairs-min");
			char *end = NULL; const unsigned long long v = strtoull(argv[i], &end, 10);
			if (!*argv[i] || *end || bh_conspairs_check_min(v)) { puts("ERROR: --consensus-pairs-min takes 1 .. 2147483647"); return 1; }
			cons_pairs_min = (uint32_t)v; cons_pairs_min_given = 1;
		}
		else if (!strcmp(a, "--mates")) { NEEDARG("--mates"); mates_FN = argv[i]; }
		else if (!strcmp(a, "--insert-min") || !strcmp(a, "--insert-max")) {
			const int is_max = !strcmp(a, "--insert-max");
			NEEDARG(a);
			char *end = NULL; const unsigned long long v = strtoull(argv[i], &end, 10);
			if (!*argv[i] || *end || v > 0xFFFFFFFFull) { printf("ERROR: %s takes a length (0 .. 4294967295)\n", a); return 1; }
			if (is_max) mopts.ins_max = (uint32_t)v; else mopts.ins_min = (uint32_t)v;
			mates_opts_given = 1;
		}
		else if (!strcmp(a, "--mates-orientation")) {
			NEEDARG("--mates-orientation"); mates_opts_given = 1;
			if (!strcmp(argv[i], "fr")) mopts.orientation = BHIP_MATES_FR; else if (!strcmp(argv[i], "rf")) mopts.orientation = BHIP_MATES_RF;
			else if (!strcmp(argv[i], "ff")) mopts.orientation = BHIP_MATES_FF; else { puts("ERROR: --mates-orientation fr|rf|ff"); return 1; }
		}
		else if (!strcmp(a, "--mates-report")) {
			NEEDARG("--mates-report"); mates_opts_given = 1;
			if (!strcmp(argv[i], "all")) mopts.report = BHIP_MATES_ALL; else if (!strcmp(argv[i], "best")) mopts.report = BHIP_MATES_BEST;
			else { puts("ERROR: --mates-report all|best"); return 1; }
		}
		else if (!strcmp(a, "--coverage-lengths")) { NEEDARG("--coverage-lengths"); cov_lengths = argv[i]; }
		else if (!strcmp(a, "--coverage-pad")) { NEEDARG("--coverage-pad"); cov_pad = (uint32_t)strtoul(argv[i], 0, 10); }
		else if (!strcmp(a, "--device")) { NEEDARG("--device"); device = atoi(argv[i]); }
		else if (!strcmp(a, "--gpus")) { NEEDARG("--gpus"); n_gpus = atoi(argv[i]); n_gpus_given = 1; if (n_gpus < 1) { puts("ERROR: --gpus must be >= 1"); return 1; } }
		else if (!strcmp(a, "--devices")) {      /* explicit device of every rank, e.g. 0,1,2,3 (the same device twice only with --gather host) */
			NEEDARG("--devices");
			for (char *t = strtok(argv[i], ","); t && n_dev_list < BH_MAX_GPUS; t = strtok(NULL, ",")) dev_list[n_dev_list++] = atoi(t);
		}
		else if (!strcmp(a, "--gather")) { NEEDARG("--gather"); gather_host = !strcmp(argv[i], "host"); if (!gather_host && strcmp(argv[i], "rccl")) { puts("ERROR: --gather rccl|host"); return 1; } }
		else if (!strcmp(a, "--shard")) { NEEDARG("--shard"); shard_db = !strcmp(argv[i], "db"); if (!shard_db && strcmp(argv[i], "queries")) { puts("ERROR: --shard queries|db"); return 1; } }
		else if (!strcmp(a, "--shards")) { NEEDARG("--shards"); n_shards = atoi(argv[i]); if (n_shards < 1) { puts("ERROR: --shards must be >= 1"); return 1; } shard_db = 1; }
		else if (!strcmp(a, "--batch")) { NEEDARG("--batch"); batch = strtoull(argv[i], 0, 10); }
		else if (!strcmp(a, "-k")) { NEEDARG("-k"); K = atoi(argv[i]); if (K != 12 && K != 15) { puts("ERROR: -k must be 12 or 15"); return 1; } }
		else if (!strcmp(a, "--help") || !strcmp(a, "-h")) { usage(); return 1; }
		else if (!strcmp(a, "--taxonomy") || !strcmp(a, "-b")) {                       /* burst.c:4949-4954 */
			if (++i == argc || argv[i][0] == '-') { puts("ERROR: --taxonomy requires filename argument"); return 1; }
			tax_FN = argv[i];
			printf(" --> Assigning taxonomy based on mapping file: %s\n", tax_FN);
		}
		else if (!strcmp(a, "--taxacut") || !strcmp(a, "-bc")) {                        /* burst.c:5001-5014 */
			if (++i == argc || argv[i][0] == '-') { puts("ERROR: --taxacut requires numeric argument"); return 1; }
			int temp = atoi(argv[i]);
			if (temp < 2) { double fl = 1.0 / (1.0 - atof(argv[i])); temp = (int)(fl + 0.5); printf(" --> Taxacut: converting %s to %d...\n", argv[i], temp); }
			if (temp < 2) { fputs("ERROR: taxacut must be >= 2\n", stderr); return 1; }
			txo.taxacut = (uint32_t)temp;
			printf(" --> Ignoring 1/%d disagreeing taxonomy calls\n", temp);
		}
		else if (!strcmp(a, "--taxa_ncbi") || !strcmp(a, "-bn")) { txo.ncbi = 1; printf(" --> Using NCBI header formatting for taxonomy lookups\n"); }
		else if (!strcmp(a, "--taxasuppress") || !strcmp(a, "-bs")) {                   /* burst.c:5023-5031 */
			txo.suppress = 1;
			if (i + 1 != argc && argv[i + 1][0] != '-') {
				if (!strcmp(argv[++i], "STRICT")) txo.strict = 1;
				else { fprintf(stderr, "ERROR: Unrecognized taxasuppress '%s'\n", argv[i]); return 1; }
			}
			printf(" --> Surpressing taxonomic specificity by alignment identity%s\n", txo.strict ? " [STRICT]" : "");
		}
		else if (!strcmp(a, "--cache") || !strcmp(a, "-c")) {                           /* burst.c:5079-5084 */
			if (++i == argc || argv[i][0] == '-') { puts("ERROR: --cache requires integer argument"); return 1; }
			printf(" --> Cached matrix lines (%d) are a CPU-side optimisation; ignored on the device path\n", atoi(argv[i]));
		}
		else if (!strcmp(a, "--latency") || !strcmp(a, "-l")) {                         /* burst.c:5085-5090 */
			if (++i == argc || argv[i][0] == '-') { puts("ERROR: --latency requires integer argument"); return 1; }
			latency = (uint32_t)atoi(argv[i]);
			printf(" --> Setting clump formation latency to %d bases\n", atoi(argv[i]));
		}
		else if (!strcmp(a, "--dbpartition") || !strcmp(a, "-dp")) {                    /* burst.c:4986-4993 */
			if (++i == argc || argv[i][0] == '-') { puts("ERROR: --dbpartition requires integer argument"); return 1; }
			const int temp = atoi(argv[i]);
			if (temp < 0) { fputs("ERROR: numb partitions must be >= 1\n", stderr); return 1; }
			dpart = temp;
			printf(" --> Partitioning database into %d slices\n", temp);
		}
		else if (!strcmp(a, "--clustradius") || !strcmp(a, "-cr")) {
			printf("ERROR: option %s tunes the reference's fingerprints (-f), which burst_hip does not include\n", a); return 1;
		}
		else if (!strcmp(a, "--xalphabet") || !strcmp(a, "-x")) { xalpha = 1; printf(" --> Allowing any alphabet (unambiguous ID matching)\n"); }
		else if (!strcmp(a, "--fingerprint") || !strcmp(a, "-f") || !strcmp(a, "--prepass") ||
		         !strcmp(a, "-p") || !strcmp(a, "--heuristic") || !strcmp(a, "-hr")) {
			printf("ERROR: option %s is outside the device hot path and not supported by burst_hip\n", a); return 1;
		}
		else { printf("ERROR: Unrecognized command-line option: %s\n", a); puts("See help by running with just '-h'"); return 1; }
	}
	if (n_dev_list && !n_gpus_given) { n_gpus = n_dev_list; n_gpus_given = 1; }
	if (n_dev_list && n_dev_list != n_gpus) { puts("ERROR: --devices must name one device per --gpus rank"); return 1; }
	if ((cov_lengths || cov_pad) && !cov_prefix) { puts("ERROR: --coverage-lengths and --coverage-pad go with --coverage <prefix>"); return 1; }
	if (cov_prefix && (makedb || mkacx_FN || xalpha)) { puts("ERROR: --coverage works from the lines of an alignment run: it does not go with -d, --make-acx or -x"); return 1; }
	if (taxa_agree_given && !taxa_prefix) { puts("ERROR: --taxa-agree goes with --taxa <prefix>"); return 1; }
	if (taxa_prefix && bh_taxa_check_opts(tax_FN, taxa_agree_given, taxa_agree)) { puts(bh_last_error()); return 1; }
	if (taxa_prefix && (makedb || mkacx_FN || xalpha)) { puts("ERROR: --taxa works from the lines of an alignment run: it does not go with -d, --make-acx or -x"); return 1; }
	if (taxa_prefix && shard_db && n_gpus == 1 && n_shards > 1) { puts("ERROR: --taxa needs a resident device handle: it does not go with the serial-shards path (--gpus 1 --shards S)"); return 1; }
	if (taxa_prefix && mates_FN) { puts("ERROR: --taxa of paired output is out of scope: it does not go with --mates"); return 1; }
	if (taxa_prefix && !samples_FN && !(ref_FN && query_FN && output_FN)) { puts("ERROR: --taxa goes with an alignment run: -r, -q and -o, or --samples"); return 1; }
	if (em_opts_given && !em_prefix) { puts("ERROR: --abundance-iters and --abundance-tol go with --abundance <prefix>"); return 1; }
	if (em_prefix && (makedb || mkacx_FN || xalpha)) { puts("ERROR: --abundance works from the lines of an alignment run: it does not go with -d, --make-acx or -x"); return 1; }
	if (em_prefix && shard_db && n_gpus == 1 && n_shards > 1) { puts("ERROR: --abundance needs a resident device handle: it does not go with the serial-shards path (--gpus 1 --shards S)"); return 1; }
	if (em_prefix && mates_FN) { puts("ERROR: --abundance of paired output is out of scope: it does not go with --mates"); return 1; }
	/* (refused before a device is touched: the paths are traced on ONE handle that holds the whole database in the nucleotide alphabet) */
	if (cigar && (makedb || mkacx_FN || xalpha)) { puts("ERROR: --cigar adds the alignment paths to the lines of an alignment run: it does not go with -d, --make-acx or -x"); return 1; }
	if (cigar && (shard_db || n_shards)) { puts("ERROR: --cigar traces the paths on rank 0's handle, which must hold the whole database: it does not go with --shard db or --shards"); return 1; }
	if (cigar && !gather_host) { puts("ERROR: --cigar takes the host gather only (drop --gather rccl)"); return 1; }
	/* (--sam writes its records from the same paths, traced on the same handle: it refuses what --cigar refuses, and paired output) */
	if ((sam_unmapped || sam_lengths) && !sam) { puts("ERROR: --sam-unmapped and --sam-lengths go with --sam"); return 1; }
	if (sam && (makedb || mkacx_FN || xalpha)) { puts("ERROR: --sam writes the records of an alignment run: it does not go with -d, --make-acx or -x"); return 1; }
	if (sam && (shard_db || n_shards)) { puts("ERROR: --sam traces the paths on rank 0's handle, which must hold the whole database: it does not go with --shard db or --shards"); return 1; }
	if (sam && !gather_host) { puts("ERROR: --sam takes the host gather only (drop --gather rccl)"); return 1; }
	if (sam && mates_FN) { puts("ERROR: --sam of paired output (paired flags, RNEXT, TLEN) is out of scope: it does not go with --mates"); return 1; }
	/* (--variants counts from the same paths, traced on the same handle: it refuses what --cigar refuses) */
	if (var_opts_given && !var_prefix) { puts("ERROR: --variants-min-depth, --variants-min-alt and --variants-reads go with --variants <prefix>"); return 1; }
	if (var_prefix && (makedb || mkacx_FN || xalpha)) { puts("ERROR: --variants counts from the lines of an alignment run: it does not go with -d, --make-acx or -x"); return 1; }
	if (var_prefix && (shard_db || n_shards)) { puts("ERROR: --variants traces the paths on rank 0's handle, which must hold the whole database: it does not go with --shard db or --shards"); return 1; }
	if (var_prefix && !gather_host) { puts("ERROR: --variants takes the host gather only (drop --gather rccl)"); return 1; }
	if (var_prefix && mates_FN) { puts("ERROR: --variants of paired output are out of scope: they do not go with --mates"); return 1; }
	/* (--consensus calls from the same paths, traced on the same handle: it refuses what --variants refuses, and the self-alignment outputs) */
	if (cons_opts_given && !cons_prefix) { puts("ERROR: --consensus-min-depth, --consensus-min-breadth, --consensus-reads and --consensus-lengths go with --consensus <prefix>"); return 1; }
	if ((cons_pairs || cons_pairs_min_given) && !cons_prefix) { puts("ERROR: --consensus-pairs and --consensus-pairs-min go with --consensus <prefix>"); return 1; }
	if (cons_pairs_min_given && !cons_pairs) { puts("ERROR: --consensus-pairs-min goes with --consensus-pairs"); return 1; }
	if (cons_prefix && (makedb || mkacx_FN || xalpha)) { puts("ERROR: --consensus calls from the lines of an alignment run: it does not go with -d, --make-acx or -x"); return 1; }
	if (cons_prefix && (shard_db || n_shards)) { puts("ERROR: --consensus traces the paths on rank 0's handle, which must hold the whole database: it does not go with --shard db or --shards"); return 1; }
	if (cons_prefix && !gather_host) { puts("ERROR: --consensus takes the host gather only (drop --gather rccl)"); return 1; }
	if (cons_prefix && mates_FN) { puts("ERROR: --consensus of paired output is out of scope: it does not go with --mates"); return 1; }
	if (cons_prefix && (clu_prefix || chi_prefix)) { puts("ERROR: --consensus does not go with --cluster or --chimeras: per-reference outputs of a self-alignment are out of scope"); return 1; }
	if (cons_prefix && !samples_FN && !(ref_FN && query_FN && output_FN)) { puts("ERROR: --consensus goes with an alignment run: -r, -q and -o, or --samples"); return 1; }
	/* (--vcf counts from the same paths, traced on the same handle: it refuses what --variants refuses, and the self-alignment outputs) */
	if (vcf_opts_given && !vcf) { puts("ERROR: --vcf-min-depth, --vcf-min-alt, --vcf-reads and --vcf-lengths go with --vcf"); return 1; }
	if (vcf_study && !vcf) { puts("ERROR: --vcf-study goes with --vcf"); return 1; }
	if (vcf && (makedb || mkacx_FN || xalpha)) { puts("ERROR: --vcf calls from the lines of an alignment run: it does not go with -d, --make-acx or -x"); return 1; }
	if (vcf && (shard_db || n_shards)) { puts("ERROR: --vcf traces the paths on rank 0's handle, which must hold the whole database: it does not go with --shard db or --shards"); return 1; }
	if (vcf && !gather_host) { puts("ERROR: --vcf takes the host gather only (drop --gather rccl)"); return 1; }
	if (vcf && mates_FN) { puts("ERROR: --vcf of paired output is out of scope: it does not go with --mates"); return 1; }
	if (vcf && (clu_prefix || chi_prefix)) { puts("ERROR: --vcf does not go with --cluster or --chimeras: per-reference outputs of a self-alignment are out of scope"); return 1; }
	if (vcf && !samples_FN && !(ref_FN && query_FN && output_FN)) { puts("ERROR: --vcf goes with an alignment run: -r, -q and -o, or --samples"); return 1; }
	/* (--cluster picks clusters from the lines one query file prints against itself: refused before a device is touched whatever would
	 * discard those lines, print other files' lines, or leave rank 0 without the whole report) */
	if (clu_sizes && !clu_prefix) { puts("ERROR: --cluster-sizes goes with --cluster <prefix>"); return 1; }
	if (clu_prefix && (makedb || mkacx_FN || xalpha)) { puts("ERROR: --cluster works from the lines of an alignment run: it does not go with -d, --make-acx or -x"); return 1; }
	if (clu_prefix && mode != BH_FORAGE) { puts("ERROR: --cluster needs every relationship under the identity cutoff: run it with -m FORAGE (the other modes discard them)"); return 1; }
	if (clu_prefix && samples_FN) { puts("ERROR: --cluster takes one query file aligned against itself: it does not go with --samples"); return 1; }
	if (clu_prefix && mates_FN) { puts("ERROR: --cluster takes one query file aligned against itself: it does not go with --mates"); return 1; }
	if (clu_prefix && (shard_db || n_shards)) { puts("ERROR: --cluster needs the whole report on rank 0: it does not go with --shard db or --shards"); return 1; }
	if (clu_prefix && !gather_host) { puts("ERROR: --cluster takes the host gather only (drop --gather rccl)"); return 1; }
	if (clu_prefix && taxa_prefix) { puts("ERROR: --cluster does not go with --taxa: per-reference tables of a self-alignment are out of scope"); return 1; }
	if (clu_prefix && (cov_prefix || em_prefix || var_prefix)) { puts("ERROR: --cluster does not go with --coverage, --abundance or --variants: per-reference tables of a self-alignment are out of scope"); return 1; }
	/* (--chimeras works from the same lines as --cluster, and from their paths: the same refusals, before a device is touched) */
	if (chi_opts_given && !chi_prefix) { puts("ERROR: --chimera-sizes, --chimera-skew, --chimera-min-seg and --chimera-min-gain go with --chimeras <prefix>"); return 1; }
	if (chi_prefix && (makedb || mkacx_FN || xalpha)) { puts("ERROR: --chimeras works from the lines of an alignment run: it does not go with -d, --make-acx or -x"); return 1; }
	if (chi_prefix && mode != BH_FORAGE) { puts("ERROR: --chimeras needs every relationship under the identity cutoff: run it with -m FORAGE (the other modes discard them)"); return 1; }
	if (chi_prefix && samples_FN) { puts("ERROR: --chimeras takes one query file aligned against itself: it does not go with --samples"); return 1; }
	if (chi_prefix && mates_FN) { puts("ERROR: --chimeras takes one query file aligned against itself: it does not go with --mates"); return 1; }
	if (chi_prefix && (shard_db || n_shards)) { puts("ERROR: --chimeras needs the whole report on rank 0: it does not go with --shard db or --shards"); return 1; }
	if (chi_prefix && !gather_host) { puts("ERROR: --chimeras takes the host gather only (drop --gather rccl)"); return 1; }
	if (chi_prefix && taxa_prefix) { puts("ERROR: --chimeras does not go with --taxa: per-reference tables of a self-alignment are out of scope"); return 1; }
	if (chi_prefix && (cov_prefix || em_prefix || var_prefix)) { puts("ERROR: --chimeras does not go with --coverage, --abundance or --variants: per-reference tables of a self-alignment are out of scope"); return 1; }
	if (mates_opts_given && mopts.ins_min > mopts.ins_max) { puts("ERROR: --insert-min is larger than --insert-max"); return 1; }
	if (mates_opts_given && !mates_FN && !samples_FN) { puts("ERROR: --insert-min, --insert-max, --mates-orientation and --mates-report go with --mates"); return 1; }
	if (mates_FN) {
		/* a session of one pair (bh_session_run_mates), beside the single-sample path below; everything here is checked before a device is touched */
		if (samples_FN) { puts("ERROR: --mates goes with -q / -o; in a --samples list the mates file is the third field of a line"); return 1; }
		if (makedb || mkacx_FN) { puts("ERROR: --mates joins the lines of an alignment run: it does not go with -d or --make-acx"); return 1; }
		if (xalpha) { puts("ERROR: --mates does not take -x (raw alphabets work against FASTA references only, and have no reverse strand)"); return 1; }
		if (!ref_FN || !query_FN || !output_FN) { puts("ERROR: --mates needs -r DB.edx, -q (mate 1) and -o"); return 1; }
		if (!gather_host) { puts("ERROR: --mates takes the host gather only (drop --gather rccl)"); return 1; }
		if (accel_dev && xcel_FN) { puts("ERROR: -ad builds the accelerator on the device; drop -a"); return 1; }
		if (!strcmp(mates_FN, query_FN) || !strcmp(output_FN, query_FN) || !strcmp(output_FN, mates_FN)) { puts("ERROR: -q, --mates and -o must be three different files"); return 1; }
		do_rc = 1;      /* (implied: one mate of a pair lies on the reverse strand) */
	}
	if (samples_FN || mates_FN) {
		/* per sample what a separate invocation writes; everything checked here is checked before a device is touched.  Out of scope:
		 * per-sample identity / mode, FASTA references, -x, serial shards and the RCCL gather (refused below and in samples_main) */
		if (samples_FN && (query_FN || output_FN || makedb || mkacx_FN)) { puts("ERROR: --samples names the query files and outputs itself: it does not go with -q, -o, -d or --make-acx"); return 1; }
		if (!ref_FN) { puts("ERROR: --samples needs -r DB.edx"); return 1; }
		if (samples_FN && xalpha) { puts("ERROR: --samples does not take -x (raw alphabets work against FASTA references only)"); return 1; }
		if (!gather_host) { puts("ERROR: --samples takes the host gather only (drop --gather rccl)"); return 1; }
		if (accel_dev && xcel_FN) { puts("ERROR: -ad builds the accelerator on the device; drop -a"); return 1; }
		SamplesArgs sa = {ref_FN, xcel_FN, tax_FN, samples_FN, mode, thres, z, do_rc, incl_ws, do_accel, accel_dev, K, skip_ambig, rep_flags, threads, device,
		                  n_gpus, n_gpus_given, n_dev_list, dev_list, shard_db, n_shards, batch, &txo, cov_prefix, cov_lengths, cov_pad, cigar,
		                  query_FN, mates_FN, output_FN, mopts, mates_opts_given, em_prefix, em_iters, em_tol,
		                  var_prefix, var_min_depth, var_min_alt, var_unique, sam, sam_unmapped, sam_lengths,
		                  cons_prefix, cons_min_depth, cons_min_breadth, cons_unique, cons_lengths,
		                  vcf, vcf_min_depth, vcf_min_alt, vcf_unique, vcf_lengths, taxa_prefix, (uint32_t)taxa_agree, vcf_study, cons_pairs, cons_pairs_min};
		return samples_main(&sa);
	}
	if (mkacx_FN) {   /* (re)build an accelerator for an existing .edx:  burst_hip -r DB.edx --make-acx DB.acx [-k 12|15] [-y] */
		if (!ref_FN) { puts("ERROR: --make-acx needs -r DB.edx"); return 1; }
		BhDb db; int rc0;
		if ((rc0 = bh_edx_read(ref_FN, &db))) DIE(rc0);
		if ((rc0 = build_accelerator(&db, K ? K : 12, z, device, host_acx, skip_ambig))) DIE(rc0);
		if ((rc0 = bh_acx_write(&db, mkacx_FN))) DIE(rc0);
		printf("Accelerator written: K=%d, %s format, %u ambiguous clumps\n", db.K, db.acxFmt ? "LARGE" : "SMALL", db.badSz);
		bh_db_free(&db);
		return 0;
	}
	if (!ref_FN || !output_FN) { puts("ERROR: --references and --output are required"); return 1; }
	if (threads > 0) omp_set_num_threads(threads);
	FILE *output = fopen(output_FN, "wb");
	if (!output) { fprintf(stderr, "ERROR: Cannot open output: %s\n", output_FN); return 2; }
	const double start = wall();
	int rc;
	if (makedb && xalpha) { puts("ERROR: -x with -d: a database nibble-packs its symbols whatever the alphabet (burst.c:2810-2824): -x works against FASTA references only"); return 1; }
	if (makedb) {
		fclose(output);
		int e = bh_is_edx(ref_FN);
		if (e < 0) DIE(e);
		if (e) { fputs("ERROR: DBs can't make DBs.\n", stderr); return 1; }
		BhDb db;
		if (!do_shear) db_qlen = 0;                                             /* burst.c:5121 */
		double tw = wall();
		if (dna_db && do_shear) {
			/* the compressive build (burst.c:1859-2108).  Without -s the reference reaches RefLen unset and crashes: the QUICK layout below */
			BhDnaStats st;
			if ((rc = bh_db_from_fasta_dna(ref_FN, (uint32_t)db_qlen, thres, shear_amt, (uint32_t)dpart, 1, latency, device, &db, &st))) DIE(rc);
			printf("Compressive build [shear %u, ov %u, window %u, %u partition%s]: max chain %llu, max sh %llu, %llu fragments\n", st.shear, st.ov, st.W,
			       st.partitions, st.partitions == 1 ? "" : "s", (unsigned long long)st.maxChain, (unsigned long long)st.maxSh, (unsigned long long)st.fragments);
			if (st.device >= 0) printf(" --> duplicate marks computed on device %d (%llu eligible positions, %llu chunk%s, %llu by the exact path, peak %.2f GB)\n", st.device,
			                           (unsigned long long)st.eligible, (unsigned long long)st.chunks, st.chunks == 1 ? "" : "s", (unsigned long long)st.exactChunks, st.peakDeviceBytes / 1e9);
			else printf(" --> duplicate marks computed on the host (%s)\n", st.note[0] ? st.note : "no device asked for");
			printf(" [parse %.3f s] [marks %.3f s: upload %.3f, sort %.3f, classify %.3f, mark %.3f] [shear %.3f s] [order/dedupe/clumps %.3f s]\n", st.secParse, st.secMarks,
			       st.secUpload, st.secSort, st.secClassify, st.secMark, st.secShear, st.secStages);
		} else if ((rc = bh_db_from_fasta_ex(ref_FN, (uint32_t)db_qlen, thres, do_shear, shear_amt, 1, latency, &db))) DIE(rc);
		puts("Writing database...");
		tw = wall();
		if ((rc = bh_edx_write(&db, output_FN, db_qlen, thres))) DIE(rc);
		printf("Database written: %u refs [%u orig], %u clumps, %u maxR [write %.3f s]\n", db.totR, db.origTotR, db.numRclumps, db.maxLenR, wall() - tw);
		if (do_accel) {
			if (!K) K = 12;
			if (accel_dev || !xcel_FN) { puts("ERROR: -ad builds the accelerator at search time; give -a <name> to write one"); return 1; }
			printf("Generating accelerator '%s' (K=%d)\n", xcel_FN, K);
			tw = wall();
			if ((rc = build_accelerator(&db, K, z, device, host_acx, skip_ambig))) DIE(rc);
			if ((rc = bh_acx_write(&db, xcel_FN))) DIE(rc);
			printf(" [accelerator %.3f s]\n", wall() - tw);
		}
		bh_db_free(&db);
		return 0;
	}
	if (!query_FN) { puts("ERROR: --queries is required when aligning"); return 1; }
	BhDb db; memset(&db, 0, sizeof db);
	double tp = wall();
	#define PHASE(name) do { const double t_ = wall(); printf(" [%-28s %8.3f s]\n", name, t_ - tp); tp = t_; } while (0)
	int usedb = bh_is_edx(ref_FN);
	if (usedb < 0) DIE(usedb);
	if (xalpha) {
		/* -x: raw symbols compared for equality (aded_xalpha / reScoreM_xalpha, burst.c:696-697, 894, 1099).  Upstream that only works
		 * against FASTA references (a database nibble-packs every symbol whatever the alphabet, burst.c:2810-2824) and on the forward
		 * strand (its reverse complement indexes a 16-entry table with the raw byte, burst.c:168, 3102): the same here, said aloud. */
		if (usedb) { fputs("ERROR: DB made without Xalpha; queries can't use Xalpha.\n", stderr); return 1; }      /* (the reference's message, burst.c:2859-2862) */
		if (do_rc) { puts("ERROR: -x compares raw symbols: there is no reverse complement of an arbitrary alphabet (drop -fr)"); return 1; }
		uint8_t map[256];
		int n_sym = 0;
		if ((rc = bh_alphabet_from_files(ref_FN, query_FN, map, &n_sym))) { fprintf(stderr, "%s\n", bh_last_error()); return rc == BH_E_IO ? 2 : 1; }
		printf(" --> Alphabet of %d symbols\n", n_sym);
		bh_set_alphabet(map);
	}
	BhQueries Q; memset(&Q, 0, sizeof Q);
	Ingest ing = {query_FN, thres, do_rc, incl_ws, do_accel, K ? K : (accel_dev || !do_accel ? 12 : 0), z, skip_ambig, &Q, 0, "", 0.0};
	pthread_t ing_thread; int ing_running = 0;
	bh_queries_sort_device(n_dev_list ? dev_list[0] : (n_gpus_given ? 0 : device));      /* large query files are sorted on the (first) search device */
	if (usedb && !getenv("BURST_HOST_SERIAL_INGEST")) ing_running = !pthread_create(&ing_thread, NULL, ingest_main, &ing);
	const int ing_started = ing_running;
	#define JOIN_INGEST() do { if (ing_running) { pthread_join(ing_thread, NULL); ing_running = 0; } } while (0)
	#define DIEJ(rc) do { JOIN_INGEST(); DIE(rc); } while (0)
	if (usedb) {
		puts("\nEDB database provided. Parsing...");
		if ((rc = bh_edx_read(ref_FN, &db))) DIEJ(rc);
		if (db.xalpha) { JOIN_INGEST(); fputs("ERROR: DB made with Xalpha; queries can't use Xalpha.\n", stderr); return 1; }
		printf(" --> EDB: %u refs [%u orig], %u clumps, %u maxR\n", db.totR, db.origTotR, db.numRclumps, db.maxLenR);
	}
	if (do_accel && accel_dev) {
		if (!usedb) { fputs("ERROR: an accelerator needs an .edx database\n", stderr); return 1; }
		if (!K) K = 12;
		printf(" --> [Accel] K=%d, built on the device from the database\n", K);
	} else if (do_accel) {
		if (!usedb) { fputs("ERROR: an accelerator needs an .edx database\n", stderr); return 1; }
		if ((rc = bh_acx_read(xcel_FN, K, z, &db))) DIEJ(rc);      /* K = 0: 12 or 15, whichever the file's exact size says */
		K = db.K;
		printf(" --> [Accel] K=%d, %s format, %u ambiguous clumps\n", K, db.acxFmt ? "LARGE" : "SMALL", db.badSz);
	}
	if (tax_FN) {                                                                    /* burst.c:5142-5149 */
		if ((rc = bh_tax_load(tax_FN, &taxonomy))) DIEJ(rc);
		txo.tax = &taxonomy;
	}
	PHASE("database read");
	if (!usedb) {      /* direct FASTA references: their clumps depend on the longest query (burst.c:5151), the queries come first */
		ingest_main(&ing);
		if (ing.rc) { fprintf(stderr, "%s\n", ing.err); return code_to_exit(ing.rc); }
		printf("Parsed %lu queries, %lu unique [min %u, max %u, maxED %u]; clear %lu, ambiguous %lu, bad %lu\n", (unsigned long)Q.totQ,
		       (unsigned long)Q.numUniq, Q.minLen, Q.maxLen, Q.maxED, (unsigned long)Q.nClear, (unsigned long)Q.nAmbig, (unsigned long)Q.nBad);
		PHASE("queries parsed, sorted");
		if ((rc = bh_db_from_fasta_ex(ref_FN, Q.maxLen, thres, do_shear, shear_amt, dedupe, latency, &db))) DIE(rc);
		printf("There are %u references and hence %u clumps\n", db.totR, db.numRclumps);
	}
	/* Multi-GPU (--gpus N): one host thread and one device handle per GPU (bh_search_multi, bh_multi.c).  --shard queries (default):
	 * the database replicated, unique queries [r U / N, (r+1) U / N) on rank r (a forward entry and its reverse complement stay
	 * together); --shard db: every rank holds a range of the database's clumps and aligns all queries, the per-query minimum is
	 * combined over the ranks.  Then the records meet where the reference's consolidation (incl. CAPITALIST's global vote) runs,
	 * in host memory.  The ranks are threads of this process and every rank's records are in host memory already when its last
	 * batch ends (copied behind each batch over the rank's own PCIe link), so the default hand-over is a concatenation there
	 * (--gather host).  --gather rccl takes them over RCCL / xGMI to rank 0's device first (bhip_comm_gather_hits: ncclAllGather of
	 * the counts + grouped ncclSend / ncclRecv; minima by ncclAllReduce MIN) -- N shares through rank 0's one PCIe link: the path
	 * for ranks that cannot see each other's memory.  --gpus 1 --gather rccl takes the RCCL path with one rank. */
	if (n_gpus > BH_MAX_GPUS) { printf("ERROR: --gpus %d (max %d)\n", n_gpus, BH_MAX_GPUS); return 1; }
	void *hhs[BH_MAX_GPUS];
	BhMultiRank ranks[BH_MAX_GPUS]; BhDb slices[BH_MAX_GPUS]; uint64_t ru0[BH_MAX_GPUS], ru1[BH_MAX_GPUS];
	memset(hhs, 0, sizeof hhs); memset(ranks, 0, sizeof ranks); memset(slices, 0, sizeof slices);
	void *comm = NULL;
	const int use_rccl = n_gpus_given && !gather_host;
	if (shard_db && !n_shards) n_shards = n_gpus;
	if (!shard_db || n_shards < 2) { shard_db = 0; n_shards = 1; }
	if (cov_prefix && shard_db && n_gpus == 1 && n_shards > 1) { JOIN_INGEST(); puts("ERROR: --coverage needs a resident device handle: it does not go with the serial-shards path (--gpus 1 --shards S)"); return 1; }
	BhCov *cov = NULL;
	if (cov_prefix && (rc = bh_cov_open(&db, cov_prefix, cov_lengths, cov_pad, &cov))) DIEJ(rc);      /* (before a device is touched) */
	BhEm *em = NULL;
	if (em_prefix && (rc = bh_em_open(&db, em_prefix, em_iters, em_tol, &em))) DIEJ(rc);
	BhTaxa *taxa = NULL;      /* (the tree of the map's strings: a string of too many levels is refused before a device is touched) */
	if (taxa_prefix && (rc = bh_taxa_open(&db, taxa_prefix, &taxonomy, txo.ncbi, (uint32_t)taxa_agree, &taxa))) { JOIN_INGEST(); if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; } DIE(rc); }
	if (cons_prefix) { const int e = open_consensus(&db, cons_prefix, cons_lengths, cons_min_depth, cons_min_breadth, cons_unique, cons_pairs ? cons_pairs_min : 0); if (e) { JOIN_INGEST(); return e; } }
	if (vcf) { const int e = open_vcf(&db, vcf_lengths, vcf_min_depth, vcf_min_alt, vcf_unique); if (e) { JOIN_INGEST(); return e; } }
	if (vcf_study) { const int e = open_vcfstudy(vcf_study); if (e) { JOIN_INGEST(); return e; } }
	if (sam) {      /* (before a device is touched: two headers of one name, a lengths table without a header) */
		if ((rc = bh_sam_open(&db, sam_lengths, sam_unmapped, &g_sam))) { JOIN_INGEST(); if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; } DIE(rc); }
		atexit(sam_atexit);      /* (whichever way the run ends before bh_sam_end: no file, no temporary file) */
	}
	if (shard_db && n_gpus == 1 && n_shards > 1 && !use_rccl) {
		/* more shards than devices: the shards take turns on the one device (bh_search_serial_shards) -- a database larger than the
		 * device's memory, at the price of one upload per shard */
		if ((uint32_t)n_shards > db.numRclumps) { puts("ERROR: more database shards than clumps"); return 1; }
		if (n_shards > BH_MAX_GPUS) { printf("ERROR: --shards %d (max %d)\n", n_shards, BH_MAX_GPUS); return 1; }
		if (!n_dev_list) dev_list[0] = device;
		JOIN_INGEST();
		if (!ing_started && usedb) ingest_main(&ing);
		if (ing.rc) { fprintf(stderr, "%s\n", ing.err); return code_to_exit(ing.rc); }
		if (usedb && do_accel && !ing.K) bh_queries_bins(&Q, do_accel, K, z);
		printf("Parsed %lu queries, %lu unique [min %u, max %u, maxED %u]; clear %lu, ambiguous %lu, bad %lu\n", (unsigned long)Q.totQ,
		       (unsigned long)Q.numUniq, Q.minLen, Q.maxLen, Q.maxED, (unsigned long)Q.nClear, (unsigned long)Q.nAmbig, (unsigned long)Q.nBad);
		if (db.shear && (uint32_t)(Q.maxLen / thres) > db.shear) { fputs("ERROR: DB incompatible with selected queries/identity.\n", stderr); return 1; }
		bh_queries_pin(&Q);
		PHASE("queries parsed, page-locked");
		BhRun srun; memset(&srun, 0, sizeof srun);
		double secs[BH_MAX_GPUS], ups[BH_MAX_GPUS];
		const double ts0 = wall();
		if ((rc = bh_search_serial_shards(&db, dev_list[0], n_shards, z, accel_dev ? K : 0, &Q, mode, batch, &srun, secs, ups))) { fprintf(stderr, "%s\n", bh_last_error()); return rc == BH_E_USAGE ? 1 : 4; }
		printf("serial shards: %d shard(s) taking turns on device %d; upload (+ accelerator build) per shard [s]:", n_shards, dev_list[0]);
		for (int r = 0; r < n_shards; ++r) printf(" %.3f", ups[r]);
		printf("; align phase per shard [s]:");
		for (int r = 0; r < n_shards; ++r) printf(" %.4f", secs[r]);
		printf("\n");
		printf("Search complete [%f s, %u batches, %lu candidate (query, clump) pairs, %lu hits]. Consolidating results...\n", wall() - ts0, srun.nBatches,
		       (unsigned long)srun.total.n_pairs, (unsigned long)srun.nHits);
		PHASE("search (all shards, uploads included)");
		uint64_t slines = 0;
		setvbuf(output, NULL, _IOFBF, 1 << 22);
		BhRunView sview; memset(&sview, 0, sizeof sview);
		sview.base = srun.hits; sview.n_runs = 1; sview.off[0] = 0; sview.n[0] = srun.nHits; sview.total = srun.nHits;
		if ((rc = bh_report_view(output, &db, &Q, &sview, mode, (do_accel ? 0 : BH_REP_MERGED_LIST) | rep_flags, tax_FN ? &txo : NULL, &slines))) DIE(rc);
		if (fclose(output)) { fprintf(stderr, "ERROR: write failed: %s\n", output_FN); return 2; }
		printf("Wrote %lu alignments\n", (unsigned long)slines);
		PHASE("consolidation, output");
		printf("\nAlignment time: %f seconds\n", wall() - start);
		fflush(NULL);
		_exit(0);
	}
	if (shard_db && n_gpus == 1 && n_shards > 1) { printf("ERROR: --gpus 1 --shards %d takes the shards in turns on one device, which has no exchange: drop --gather rccl\n", n_shards); return 1; }
	if (n_gpus % n_shards) { printf("ERROR: --shards %d does not divide --gpus %d\n", n_shards, n_gpus); return 1; }
	const int n_groups = n_gpus / n_shards;
	if (shard_db && (uint32_t)n_shards > db.numRclumps) { puts("ERROR: more database shards than clumps"); return 1; }
	if (!n_dev_list) for (int r = 0; r < n_gpus; ++r) dev_list[r] = n_gpus_given ? r : device;
	if (use_rccl && bhip_comm_create(n_gpus, dev_list, &comm)) { fprintf(stderr, "libburst_hip: %s\n", bhip_last_error()); return 4; }
	{ const int e = open_devices(&db, n_gpus, dev_list, shard_db, n_shards, accel_dev, K, z, hhs, ranks, slices); if (e) return e; }
	PHASE("device database upload");
	if (usedb) {
		JOIN_INGEST();
		if (!ing_started) ingest_main(&ing);      /* (no thread: read them now) */
		if (ing.rc) { fprintf(stderr, "%s\n", ing.err); return code_to_exit(ing.rc); }
		if (do_accel && !ing.K) bh_queries_bins(&Q, do_accel, K, z);        /* K came with the accelerator file */
		printf("Parsed %lu queries, %lu unique [min %u, max %u, maxED %u]; clear %lu, ambiguous %lu, bad %lu\n", (unsigned long)Q.totQ,
		       (unsigned long)Q.numUniq, Q.minLen, Q.maxLen, Q.maxED, (unsigned long)Q.nClear, (unsigned long)Q.nAmbig, (unsigned long)Q.nBad);
		if (db.shear && (uint32_t)(Q.maxLen / thres) > db.shear) {                /* burst.c:5152-5156 */
			fputs("ERROR: DB incompatible with selected queries/identity.\n", stderr); return 1;
		}
		printf(" [%-28s %8.3f s%s; waited for %.3f s]\n", "queries parsed, sorted", ing.secs, ing_started ? ", on a thread beside the database phases" : "", wall() - tp);
		tp = wall();
	}
	bh_queries_pin(&Q);
	PHASE("query arrays page-locked");
	for (int r = 0; r < n_gpus; ++r) {
		ranks[r].rank = r; ranks[r].hh = hhs[r];
		const int grp = r / n_shards;      /* the ranks of a replica group align the same queries, each against its shard */
		ru0[r] = Q.numUniq * (uint64_t)grp / (uint64_t)n_groups; ru1[r] = Q.numUniq * (uint64_t)(grp + 1) / (uint64_t)n_groups;
		ranks[r].r0 = &ru0[r]; ranks[r].r1 = &ru1[r]; ranks[r].n_ranges = 1;
	}
	BhRun block; memset(&block, 0, sizeof block);
	if (n_gpus > 1 && !use_rccl && !shard_db) {
		/* the ranks' record buffers as slices of ONE page-locked block: what they deliver is then read where it lies (a view over the
		 * block, bh_report_view) instead of being concatenated first */
		uint64_t off[BH_MAX_GPUS + 1]; off[0] = 0;
		const uint64_t strands = Q.numEntries > Q.numUniq ? 2 : 1;
		for (int r = 0; r < n_gpus; ++r) { const uint64_t n = ru1[r] - ru0[r]; off[r + 1] = off[r] + n * strands + n / 2 + (1u << 20); }
		if (!bh_run_reserve(&block, off[n_gpus])) for (int r = 0; r < n_gpus; ++r) { ranks[r].run.hits = block.hits + off[r]; ranks[r].run.capHits = off[r + 1] - off[r]; ranks[r].run.hitsPinned = 2; }
	}
	{	/* device and record buffers for the batches to come (allocations synchronise the device: not inside the search), sized from
		 * the batches that will really be staged: their entry count and their symbols (one long read among millions of short ones
		 * must not size every buffer for n_entries x max_len) */
		const uint64_t strands = Q.numEntries > Q.numUniq ? 2 : 1;
		#pragma omp parallel num_threads(n_gpus)
		{
			const int r = omp_get_thread_num();
			const uint64_t n = ru1[r] - ru0[r], B = n < batch ? n : batch;
			uint64_t sym = 0;
			for (uint64_t u = ru0[r]; u < ru1[r]; u += B ? B : 1) {
				const uint64_t e = u + B < ru1[r] ? u + B : ru1[r];
				uint64_t sy = Q.qoff[e] - Q.qoff[u];
				if (strands == 2) sy += Q.qoff[Q.numUniq + e] - Q.qoff[Q.numUniq + u];
				if (sy > sym) sym = sy;
			}
			if (!ranks[r].run.hits) bh_run_reserve(&ranks[r].run, n * strands + n / 2 + (1u << 20));      /* (no slice of the block below) */
			if (B && bhip_reserve_symbols(hhs[r], (uint32_t)(B * strands), Q.maxLen, sym))      /* last: it ends with a warm-up pass, the search follows at once */
				fprintf(stderr, " --> WARNING: batch buffers not reserved on device %d (%s); they are allocated batch by batch\n", dev_list[r], bhip_last_error());
		}
	}
	BhRun run; memset(&run, 0, sizeof run);
	BhRunView view; memset(&view, 0, sizeof view);
	/* several ranks: the buffer their records meet in, made here and not inside the search (page-locked when a device copy lands
	 * in it, i.e. with the RCCL gather; bh_search_multi grows it if the job brings more) */
	if ((n_gpus > 1 || use_rccl) && !block.hits) { const uint64_t cap = Q.numEntries + Q.numEntries / 2 + (1u << 20); if (use_rccl) bh_run_reserve(&run, cap); else bh_run_reserve_plain(&run, cap); }
	PHASE("batch buffers");
	const double t0 = wall();
	uint64_t cnts[BH_MAX_GPUS]; memset(cnts, 0, sizeof cnts);
	if (n_gpus == 1 && !use_rccl) {
		if ((rc = bh_align_ranges_reuse(hhs[0], &Q, &ru0[0], &ru1[0], 1, mode, batch, &ranks[0].run))) { fprintf(stderr, "%s\n", bh_last_error()); return rc == BH_E_USAGE ? 1 : 4; }
		run = ranks[0].run; memset(&ranks[0].run, 0, sizeof ranks[0].run);
		view.base = run.hits; view.n_runs = 1; view.off[0] = 0; view.n[0] = run.nHits; view.total = run.nHits;
	} else {
		if ((rc = bh_search_multi_ex(ranks, n_gpus, n_gpus, comm, NULL, &Q, mode, batch, shard_db ? n_shards : 0, &run, cnts, &view))) { fprintf(stderr, "%s\n", bh_last_error()); return rc == BH_E_USAGE ? 1 : 4; }
		printf("%s: %d rank(s)%s, records per rank:", use_rccl ? "RCCL gather" : "host gather", n_gpus, shard_db ? ", database-sharded" : "");
		for (int r = 0; r < n_gpus; ++r) printf(" %lu", (unsigned long)cnts[r]);
		printf("; align phase per rank [s]:");
		for (int r = 0; r < n_gpus; ++r) printf(" %.4f", ranks[r].secSearch);
		printf("\n");
		for (int r = 0; r < n_gpus; ++r) run.total.n_pairs += ranks[r].run.total.n_pairs;
	}
	const double t1 = wall();
	printf("Search complete [%f s, %u batches, %lu candidate (query, clump) pairs, %lu hits]. Consolidating results...\n", t1 - t0, run.nBatches,
	       (unsigned long)run.total.n_pairs, (unsigned long)run.nHits);
	PHASE("search (all batches)");
	uint64_t lines = 0;
	setvbuf(output, NULL, _IOFBF, 1 << 22);
	BhPlaceSink sink; memset(&sink, 0, sizeof sink);
	BhPaths *paths = NULL;
	if ((cigar || var_prefix || cons_prefix || vcf || chi_prefix || sam) && (rc = bh_paths_open(hhs[0], &paths))) DIE(rc);      /* (rank 0's handle, as the coverage) */
	BhPile *pile = NULL;      /* a study of one sample; opened here: its temporary file exists from now until it is renamed or the object is closed */
	#define DIEP(rc) do { bh_pile_close(pile); DIE(rc); } while (0)
	if (var_prefix) {
		if (!db.refMap || !db.numRefHeads) { puts("ERROR: --variants needs the reference headers of the database"); return 1; }
		if ((rc = bh_pile_open(&db, var_prefix, var_min_depth, var_min_alt, var_unique, &pile))) DIE(rc);
		bh_paths_set_pile(paths, pile, cigar);
	}
	BhCluster *clu = NULL;
	if (clu_prefix && (rc = bh_cluster_open(clu_prefix, clu_sizes, &clu))) DIE(rc);
	sink.want_re = clu != NULL;
	BhChimera *chi = NULL;      /* its lines come from the traced groups of the report: a usage error -- two reads of one name -- ends the run before it */
	if (chi_prefix) {
		if ((rc = bh_chimera_open(chi_prefix, chi_sizes, chi_skew, chi_min_seg, chi_min_gain, &chi)) || (rc = bh_chimera_begin(chi, &db, &Q))) { if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; } DIE(rc); }
		bh_paths_set_chimera(paths, chi, cigar);
	}
	if (sam) {
		if ((rc = bh_sam_begin(g_sam, hhs[0], &Q, output_FN))) DIEP(rc);
		if ((rc = bh_paths_set_sam(paths, g_sam, cigar))) DIEP(rc);
	}
	if (g_cons && (rc = bh_paths_set_consensus(paths, g_cons, cigar))) DIEP(rc);
	if (g_vcf && (rc = bh_paths_set_vcf(paths, g_vcf, cigar))) DIEP(rc);
	if ((rc = bh_report_view_paths(output, &db, &Q, &view, mode, (do_accel ? 0 : BH_REP_MERGED_LIST) | rep_flags, tax_FN ? &txo : NULL, &lines, cov || em || clu || taxa ? &sink : NULL, paths))) DIEP(rc);
	if (fclose(output)) { fprintf(stderr, "ERROR: write failed: %s\n", output_FN); return 2; }      /* (the last buffer of the report: a full disk must not end in exit code 0) */
	printf("Wrote %lu alignments\n", (unsigned long)lines);
	if (paths && cigar) bh_paths_print_info(paths, hhs[0]);
	PHASE("consolidation, output");
	if (pile) {     /* first of the tables: a failure below must not leave its temporary file */
		if ((rc = bh_pile_sample(pile, hhs[0], output_FN, Q.codes, Q.qoff, Q.numEntries)) || (rc = bh_pile_write(pile))) DIEP(rc);
		bh_pile_print_info(pile);
		printf("Variants table written: %svariants.txt\n", var_prefix);
		PHASE("variants");
		bh_pile_close(pile); pile = NULL;
	}
	if (g_cons) {   /* a study of one sample: its block, then both files get their names (a failure: the exit handler removes the temporary files) */
		if ((rc = bh_consensus_sample(g_cons, hhs[0], output_FN, Q.codes, Q.qoff, Q.numEntries)) || (g_conspairs && (rc = bh_consensus_pairs(g_cons, hhs[0]))) || (rc = bh_consensus_write(g_cons)))
			{ if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; } DIE(rc); }
		bh_consensus_print_info(g_cons);
		if (g_conspairs) bh_conspairs_print_info(g_conspairs);      /* (a study of one sample: no pair, 1 x 1 matrices) */
		printf("Consensus written: %sconsensus.fa, %sconsensus.txt\n", cons_prefix, cons_prefix);
		if (g_conspairs) printf("Consensus pairs written: %sconsensus_pairs.txt, %sconsensus_identity.txt, %sconsensus_compared.txt\n", cons_prefix, cons_prefix, cons_prefix);
		PHASE("consensus");
		close_consensus();
	}
	if (g_vcf) {    /* OUT.vcf: written under a temporary name, renamed when it is whole (a failure leaves none) */
		if ((rc = bh_vcf_sample(g_vcf, hhs[0], output_FN, Q.codes, Q.qoff, Q.numEntries))) { if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; } DIE(rc); }
		bh_vcf_print_info(g_vcf);
		printf("VCF records written: %s.vcf\n", output_FN);
		PHASE("VCF");
		if (g_vcfstudy) {      /* a study of one sample */
			const int e = write_vcfstudy(hhs[0], vcf_study);
			if (e) { fflush(NULL); return e; }
			PHASE("study VCF");
			bh_vcfstudy_close(g_vcfstudy); g_vcfstudy = NULL;
		}
		bh_vcf_close(g_vcf); g_vcf = NULL;
	}
	if (cov) {      /* a study of one sample: the Dataset column and the sample's (rank 0's handle; the lines exist only here) */
		if ((shard_db && (rc = bh_cov_lengths_host(cov))) || (rc = bh_cov_sample(cov, hhs[0], output_FN, sink.lines, sink.n)) || (rc = bh_cov_write(cov))) DIE(rc);
		printf("Coverage tables written: %sshared.txt, %sunique.txt, %sshared_binary.txt, %sunique_binary.txt, %scounts.txt\n", cov_prefix, cov_prefix, cov_prefix, cov_prefix, cov_prefix);
		PHASE("coverage");
		bh_cov_print_info(cov);
	}
	if (em) {       /* likewise: one sample, so Dataset = its column */
		if ((rc = bh_em_sample(em, hhs[0], output_FN, sink.uq, sink.lines, sink.n)) || (rc = bh_em_write(em))) DIE(rc);
		bh_em_print_info(em);
		printf("Abundance table written: %sabundance.txt\n", em_prefix);
		PHASE("abundance");
	}
	if (taxa) {     /* likewise, from the same groups; the abundance's counts rolled up beside them */
		uint32_t nl = 0, nel = 0;
		if ((rc = bh_taxa_sample(taxa, hhs[0], output_FN, sink.uq, sink.lines, sink.n, em ? bh_em_last_column(em) : NULL)) || (rc = bh_taxa_write(taxa, &nl, &nel))) DIE(rc);
		bh_taxa_print_info(taxa);
		print_taxa_written(taxa_prefix, nl, nel);
		PHASE("taxa");
	}
	if (clu) {      /* the reads clustered from the lines just printed (rank 0's handle); a usage error -- two reads of one name -- writes no table */
		if ((rc = bh_cluster_sample(clu, hhs[0], &db, &Q, &sink)) || (rc = bh_cluster_write(clu))) { if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; } DIE(rc); }
		bh_cluster_print_info(clu);
		printf("Cluster tables written: %sclusters.txt, %scluster_sizes.txt\n", clu_prefix, clu_prefix);
		PHASE("clusters");
	}
	if (chi) {      /* the reads checked from the lines just printed and their paths (rank 0's handle) */
		if ((rc = bh_chimera_solve(chi, hhs[0])) || (rc = bh_chimera_write(chi))) { if (rc == BH_E_USAGE) { puts(bh_last_error()); fflush(NULL); return 1; } DIE(rc); }
		bh_chimera_print_info(chi);
		printf("Chimera table written: %schimeras.txt\n", chi_prefix);
		PHASE("chimera check");
	}
	if (sam) {      /* last: the run has succeeded, OUT.sam gets its name */
		if ((rc = bh_sam_end(g_sam))) DIE(rc);
		bh_sam_print_info(g_sam);
		printf("SAM records written: %s.sam\n", output_FN);
		PHASE("SAM records");
		bh_sam_close(g_sam); g_sam = NULL;
	}
	printf("\nAlignment time: %f seconds\n", wall() - start);
	fflush(NULL);
	/* The job is done and its output is on disk.  Unpinning and unmapping tens of gigabytes one table after the other took about a
	 * second for a 32 M-read job; the operating system releases a finished process's memory (host and device) far faster.
	 * BURST_HOST_TEARDOWN=1 walks through the orderly release instead (leak checks). */
	if (!getenv("BURST_HOST_TEARDOWN")) _exit(0);
	bh_cov_close(cov); bh_em_close(em); bh_taxa_close(taxa); bh_cluster_close(clu); bh_chimera_close(chi); free(sink.lines); free(sink.uq); free(sink.re); bh_paths_close(paths);
	if (comm) bhip_comm_destroy(comm);
	for (int r = 0; r < n_gpus; ++r) { bhip_destroy(hhs[r]); if (slices[r].numRclumps) bh_db_free(&slices[r]); }
	for (int r = 0; r < n_gpus; ++r) bh_run_free(&ranks[r].run);
	bh_run_free(&block); bh_run_free(&run); bh_queries_free(&Q); bh_db_free(&db); bh_tax_free(&taxonomy);
	return 0;
}
