/* bh_session.c -- a database that stays on the devices while a list of query files runs through it, each to its own .b6
 * (burst_hip --samples, host.Session, python -m burst_amd.run --samples).  No reference counterpart: the reference takes one -q and
 * one -o per process (burst.c:4918-4927), and on a CPU the search dwarfs the database load.  Here the database read, the upload and the
 * accelerator build are most of a run's wall time and depend on nothing in the query file.
 *
 *   resident (session)   the BhDb, the device handles (opened by the caller: bh_device_open_ex / _shared, slices for --shard db), the
 *                        devices' batch buffers (bhip_reserve_symbols: a reservation only ever grows), the ranks' record buffers
 *                        (BhRun; the one page-locked block of the multi-rank path), the buffer the ranks' records meet in
 *   per sample           the query tables (BhQueries) and their page-lockings, the ranks' query ranges, the output file; everything
 *                        the consolidation keeps (running minima, CAPITALIST's reference counts, duplicate flags) lives inside
 *                        bh_report_view and starts afresh with every call
 *   ingest ahead         one thread parses, sorts and de-duplicates sample i+1 while sample i is searched and reported
 *                        (bh_session_prefetch): at most one such thread, at most two samples' tables alive
 *
 * What one sample goes through is what burst_hip's single-sample path does once (main.c): ingest, bins, shear check, page-lock,
 * buffers, search (bh_align_ranges_reuse for one rank on a device, bh_search_multi_ex otherwise), report, release. */
#include "burst_host.h"
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <omp.h>

static double wall(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }

typedef struct SessIngest { struct BhSession *s; char *fn; BhQueries Q; int K, rc, threaded; char err[512]; double secs; } SessIngest;

struct BhSession {
	const BhDb *db; BhMultiRank *ranks; int n_local, n_ranks, i0; void *comm; BhNode *node;
	BhSessionOpts o; BhTaxOpts tax;
	uint64_t ru0[BH_MAX_RANKS], ru1[BH_MAX_RANKS];
	uint64_t resEntries[BH_MAX_RANKS], resSym[BH_MAX_RANKS]; uint32_t resMaxLen[BH_MAX_RANKS];      /* what every handle has reserved so far */
	BhRun block, all;
	SessIngest *cur, *ahead; pthread_t th; char *pending;
	FILE *out; char *out_path;
	char *cov_name;                 /* with a coverage or an abundance: the output the loaded sample was given (names its column, also when the sample fails) */
	int taxa_col;                   /* ... and its column in the taxon tables */
	int cov_col, em_col, pile_col, cons_col, vcf_col;  /* the loaded sample has its column in the coverage / the abundance, its block in the variants / the consensus already */
	BhPlaceSink sink;               /* the report's placements of the current sample (buffer kept across samples) */
	BhMates *mates;                 /* bh_session_run_mates: the joiner, made on first use */
	BhCluster *cluster;             /* bh_session_set_cluster: NULL, or the clustering every reported sample is given */
	BhChimera *chimera;             /* bh_session_set_chimera: NULL, or the chimera check every reported sample is given */
	BhSam *sam;                     /* bh_session_set_sam: NULL, or the SAM writer every reported sample is given */
	BhCons *cons;                   /* bh_session_set_consensus: NULL, or the consensus every reported sample feeds */
	BhVcf *vcf;                     /* bh_session_set_vcf: NULL, or the VCF writer every reported sample is given */
	BhTaxa *taxa;                   /* bh_session_set_taxa: NULL, or the taxon tables every reported sample feeds */
	BhPaths *paths;                 /* with o.cigar, o.pile, a consensus, a chimera check or a SAM writer: the tracer on the reporting rank's handle, opened by the first sample that reports */
	int dead, dbg, threads_ok;
	int alive;                      /* query tables alive (the current sample's and the prefetched one's) */
	pthread_mutex_t mu;             /* `alive` and its debug line */
	double tLoad;
};

static void tables_count(BhSession *s, int d, const char *fn) {
	pthread_mutex_lock(&s->mu);
	s->alive += d;
	if (s->dbg) fprintf(stderr, "[bh_session] query tables %s: %s (alive %d)\n", d > 0 ? "allocated" : "released", fn, s->alive);
	pthread_mutex_unlock(&s->mu);
}
static SessIngest *ingest_new(BhSession *s, const char *fn) {
	SessIngest *g = calloc(1, sizeof(*g));
	if (g && !(g->fn = strdup(fn))) { free(g); g = NULL; }
	if (!g) return NULL;
	g->s = s;
	/* K = 0 with an accelerator: the file says which K it was built with, the bins are made when the sample's turn comes */
	g->K = s->o.K ? s->o.K : (s->o.do_accel ? 0 : 12);
	tables_count(s, 1, fn);
	return g;
}
static void ingest_free(SessIngest *g) {
	if (!g) return;
	bh_queries_free(&g->Q);
	tables_count(g->s, -1, g->fn);
	free(g->fn); free(g);
}
static void *ingest_main(void *p) {
	SessIngest *g = p;
	const BhSessionOpts *o = &g->s->o;
	const double t0 = wall();
	g->rc = bh_queries_load(g->fn, o->thres, o->do_rc, o->incl_ws, o->do_accel, g->K, o->z, o->skip_ambig, &g->Q);
	if (g->rc) snprintf(g->err, sizeof g->err, "%s", bh_last_error());
	g->secs = wall() - t0;
	return NULL;
}
static void start_ahead(BhSession *s, const char *fn) {
	SessIngest *g = ingest_new(s, fn);
	if (!g) return;                                  /* (no memory for the job record: the sample is read when its turn comes) */
	g->threaded = 1;
	if (pthread_create(&s->th, NULL, ingest_main, g)) { ingest_free(g); return; }
	s->ahead = g;
}

int bh_session_open(const BhDb *db, BhMultiRank *ranks, int n_local, int n_ranks, void *comm, BhNode *node, const BhSessionOpts *o, BhSession **out) {
	if (!out) return bh_set_error(BH_E_USAGE, "bh_session_open: no place for the session");
	*out = NULL;
	if (!db || !ranks || !o || n_local < 1 || n_local > n_ranks || n_ranks > BH_MAX_RANKS) return bh_set_error(BH_E_USAGE, "bad rank layout (%d local of %d)", n_local, n_ranks);
	if (n_local != n_ranks && n_local != 1) return bh_set_error(BH_E_USAGE, "a session's ranks are the threads of one process, or one rank of a job of processes");
	const int S = o->shard_db > 1 ? o->shard_db : 1;
	if (n_ranks % S) return bh_set_error(BH_E_USAGE, "%d database shards do not divide %d ranks", S, n_ranks);
	BhSession *s = calloc(1, sizeof(*s));
	if (!s) return bh_set_error(BH_E_OOM, "OOM:session");
	s->db = db; s->ranks = ranks; s->n_local = n_local; s->n_ranks = n_ranks; s->comm = comm; s->node = node; s->o = *o;
	if (o->tax) { s->tax = *o->tax; s->o.tax = &s->tax; }
	s->i0 = -1;
	for (int i = 0; i < n_local; ++i) if (ranks[i].rank == 0) s->i0 = i;
	s->dbg = getenv("BURST_HOST_DEBUG") != NULL;
	s->threads_ok = o->ingest_ahead && !getenv("BURST_HOST_SERIAL_INGEST");
	pthread_mutex_init(&s->mu, NULL);
	*out = s;
	return BH_OK;
}

int bh_session_ended(const BhSession *s) { return s ? s->dead : 0; }
void bh_session_set_node(BhSession *s, BhNode *node) { if (s) s->node = node; }
void bh_session_set_coverage(BhSession *s, BhCov *cov) { if (s) s->o.cov = cov; }
void bh_session_set_abundance(BhSession *s, BhEm *em) { if (s) s->o.em = em; }
void bh_session_set_variants(BhSession *s, BhPile *pile) { if (s) s->o.pile = pile; }
int bh_session_set_cluster(BhSession *s, BhCluster *cl) {
	if (!s) return bh_set_error(BH_E_USAGE, "bh_session_set_cluster: no session");
	if (cl && s->o.mode != BH_FORAGE) return bh_set_error(BH_E_USAGE, "ERROR: clusters need every relationship under the identity cutoff: a session in mode FORAGE");
	if (cl && s->cons) return bh_set_error(BH_E_USAGE, "ERROR: clusters do not go with the consensus");
	if (cl && s->vcf) return bh_set_error(BH_E_USAGE, "ERROR: clusters do not go with the VCF output");
	if (cl && s->taxa) return bh_set_error(BH_E_USAGE, "ERROR: clusters do not go with the taxon tables");
	if (cl && (s->o.cov || s->o.em || s->o.pile || s->o.shard_db > 1)) return bh_set_error(BH_E_USAGE, "ERROR: clusters do not go with coverage, abundance, variants or database shards");
	s->cluster = cl;
	return BH_OK;
}
int bh_session_set_chimera(BhSession *s, BhChimera *ch) {
	if (!s) return bh_set_error(BH_E_USAGE, "bh_session_set_chimera: no session");
	if (ch && s->o.mode != BH_FORAGE) return bh_set_error(BH_E_USAGE, "ERROR: the chimera check needs every relationship under the identity cutoff: a session in mode FORAGE");
	if (ch && s->cons) return bh_set_error(BH_E_USAGE, "ERROR: the chimera check does not go with the consensus");
	if (ch && s->vcf) return bh_set_error(BH_E_USAGE, "ERROR: the chimera check does not go with the VCF output");
	if (ch && s->taxa) return bh_set_error(BH_E_USAGE, "ERROR: the chimera check does not go with the taxon tables");
	if (ch && (s->o.cov || s->o.em || s->o.pile || s->o.shard_db > 1)) return bh_set_error(BH_E_USAGE, "ERROR: the chimera check does not go with coverage, abundance, variants or database shards");
	s->chimera = ch;
	return BH_OK;
}
int bh_session_set_sam(BhSession *s, BhSam *sam) {
	if (!s) return bh_set_error(BH_E_USAGE, "bh_session_set_sam: no session");
	if (sam && s->o.shard_db > 1) return bh_set_error(BH_E_USAGE, "ERROR: --sam traces the paths on rank 0's handle, which must hold the whole database: it does not go with database shards");
	s->sam = sam;
	return BH_OK;
}
int bh_session_set_consensus(BhSession *s, BhCons *cons) {
	if (!s) return bh_set_error(BH_E_USAGE, "bh_session_set_consensus: no session");
	if (cons && s->o.shard_db > 1) return bh_set_error(BH_E_USAGE, "ERROR: --consensus traces the paths on rank 0's handle, which must hold the whole database: it does not go with database shards");
	if (cons && (s->cluster || s->chimera)) return bh_set_error(BH_E_USAGE, "ERROR: the consensus does not go with clusters or the chimera check");
	s->cons = cons;
	return BH_OK;
}

/* the end of a run whose consensus has a pairs collector, before the caller's bh_consensus_write: the one solver call on the reporting
 * rank's handle and the three files under their temporary names */
int bh_session_consensus_pairs(BhSession *s) {
	if (!s || !s->cons) return bh_set_error(BH_E_USAGE, "bh_session_consensus_pairs: no session with a consensus");
	if (s->dead) return bh_set_error(s->dead, "the session was ended by an earlier error (code %d): no file is written", s->dead);
	if (s->i0 < 0) return bh_set_error(BH_E_USAGE, "bh_session_consensus_pairs: this process holds no reporting rank");
	return bh_consensus_pairs(s->cons, s->ranks[s->i0].hh);
}
int bh_session_set_vcf(BhSession *s, BhVcf *vcf) {
	if (!s) return bh_set_error(BH_E_USAGE, "bh_session_set_vcf: no session");
	if (vcf && s->o.shard_db > 1) return bh_set_error(BH_E_USAGE, "ERROR: --vcf traces the paths on rank 0's handle, which must hold the whole database: it does not go with database shards");
	if (vcf && (s->cluster || s->chimera)) return bh_set_error(BH_E_USAGE, "ERROR: the VCF output does not go with clusters or the chimera check");
	s->vcf = vcf;
	return BH_OK;
}
int bh_session_set_taxa(BhSession *s, BhTaxa *tx) {
	if (!s) return bh_set_error(BH_E_USAGE, "bh_session_set_taxa: no session");
	if (tx && (s->cluster || s->chimera)) return bh_set_error(BH_E_USAGE, "ERROR: the taxon tables do not go with clusters or the chimera check: per-reference tables of a self-alignment are out of scope");
	s->taxa = tx;
	return BH_OK;
}
const BhQueries *bh_session_sample(const BhSession *s) { return s && s->cur ? &s->cur->Q : NULL; }

int bh_session_prefetch(BhSession *s, const char *queries) {
	if (!s || !queries) return bh_set_error(BH_E_USAGE, "bh_session_prefetch: no session / no file");
	if (s->dead || !s->threads_ok) return BH_OK;
	free(s->pending); s->pending = NULL;
	if (!s->ahead) { start_ahead(s, queries); return BH_OK; }
	/* one ingest is outstanding already (the sample whose turn is next): this one starts when that one has been taken */
	if (!(s->pending = strdup(queries))) return bh_set_error(BH_E_OOM, "OOM:session");
	return BH_OK;
}

static void close_output(BhSession *s, int keep) {
	if (s->out) { fclose(s->out); s->out = NULL; }
	if (s->out_path) { if (!keep) (void)unlink(s->out_path); free(s->out_path); s->out_path = NULL; }
}
static int sample_fail_ex(BhSession *s, BhSampleResult *res, int rc, const char *msg, int fatal) {
	res->rc = rc;
	snprintf(res->err, sizeof res->err, "%s", msg ? msg : bh_last_error());
	close_output(s, 0);
	if (s->cur) { ingest_free(s->cur); s->cur = NULL; }
	/* usage and I/O errors are the sample's own; anything else (memory, device, internal) ends the session: nothing more is
	 * started on a device after a device error */
	if (fatal || (rc != BH_E_USAGE && rc != BH_E_IO)) s->dead = rc;
	if (s->o.cov && s->i0 >= 0) {      /* a sample that fails alone is an all-zero column; a run that ends here writes no tables */
		if (s->dead) bh_cov_abort(s->o.cov);
		else if (s->cov_name && !s->cov_col) (void)bh_cov_sample_failed(s->o.cov, s->cov_name);
	}
	if (s->o.em && s->i0 >= 0) {
		if (s->dead) bh_em_abort(s->o.em);
		else if (s->cov_name && !s->em_col) (void)bh_em_sample_failed(s->o.em, s->cov_name);
	}
	if (s->taxa && s->i0 >= 0) {
		if (s->dead) bh_taxa_abort(s->taxa);
		else if (s->cov_name && !s->taxa_col) (void)bh_taxa_sample_failed(s->taxa, s->cov_name);
	}
	if (s->o.pile && s->i0 >= 0) {
		if (s->dead) bh_pile_abort(s->o.pile);
		else if (s->cov_name && !s->pile_col) (void)bh_pile_sample_failed(s->o.pile, s->cov_name);
	}
	if (s->cons && s->i0 >= 0) {
		if (s->dead) bh_consensus_abort(s->cons);
		else if (s->cov_name && !s->cons_col) (void)bh_consensus_sample_failed(s->cons, s->cov_name);
	}
	if (s->sam && s->i0 >= 0) { if (s->dead) bh_sam_abort(s->sam); else bh_sam_discard(s->sam); }      /* (no OUT.sam of a sample that failed) */
	if (s->vcf && s->i0 >= 0) {      /* (no OUT.vcf either; a study gives the sample its '.' column unless bh_vcf_sample has dealt with it) */
		if (s->dead) bh_vcf_abort(s->vcf);
		else { bh_vcf_sample_failed(s->vcf); if (s->cov_name && !s->vcf_col) (void)bh_vcf_study_sample_failed(s->vcf, s->cov_name); }
	}
	free(s->cov_name); s->cov_name = NULL;
	return bh_set_error(rc, "%s", res->err);
}
static int sample_fail(BhSession *s, BhSampleResult *res, int rc, const char *msg) { return sample_fail_ex(s, res, rc, msg, 0); }

int bh_session_load(BhSession *s, const char *queries, const char *out_path, BhSampleResult *res) {
	BhSampleResult tmp;
	if (!res) res = &tmp;
	memset(res, 0, sizeof *res);
	if (!s || !queries) return bh_set_error(BH_E_USAGE, "bh_session_load: no session / no file");
	if (s->dead) { res->rc = s->dead; snprintf(res->err, sizeof res->err, "the session was ended by an earlier error (code %d)", s->dead); return bh_set_error(s->dead, "%s", res->err); }
	if (s->cur) return bh_set_error(BH_E_USAGE, "bh_session_load: the previous sample has not been finished or dropped");
	s->tLoad = wall();
	free(s->cov_name); s->cov_name = NULL; s->cov_col = s->em_col = s->taxa_col = s->pile_col = s->cons_col = s->vcf_col = 0;
	if ((s->o.cov || s->o.em || s->o.pile || s->cons || s->vcf || s->taxa) && out_path && s->i0 >= 0 && !(s->cov_name = strdup(out_path))) return bh_set_error(BH_E_OOM, "OOM:session");
	SessIngest *g = NULL;
	/* the outstanding ingest is this sample's: take it.  If it is another one's (prefetched before this sample was named) it stays
	 * outstanding and this sample is read here */
	if (s->ahead && !strcmp(s->ahead->fn, queries)) { pthread_join(s->th, NULL); g = s->ahead; s->ahead = NULL; }
	if (!g && s->pending && !strcmp(s->pending, queries)) { free(s->pending); s->pending = NULL; }      /* (its turn has come before its ingest could start) */
	if (!g) {
		if (!(g = ingest_new(s, queries))) return sample_fail(s, res, BH_E_OOM, "OOM:session");
		ingest_main(g);
	}
	s->cur = g;
	res->secIngest = g->secs; res->secIngestWaited = wall() - s->tLoad;
	/* this sample's tables are in hand: the next one's ingest may start (two samples' tables alive, never three; an outstanding
	 * ingest nobody has asked for by now was prefetched for a turn that never came) */
	if (s->pending) {
		if (s->ahead) { pthread_join(s->th, NULL); ingest_free(s->ahead); s->ahead = NULL; }
		char *p = s->pending; s->pending = NULL; start_ahead(s, p); free(p);
	}
	if (g->rc) return sample_fail(s, res, g->rc, g->err);
	BhQueries *Q = &g->Q;
	if (s->o.do_accel && !g->K) bh_queries_bins(Q, s->o.do_accel, s->db->K, s->o.z);        /* K came with the accelerator file */
	res->totQ = Q->totQ; res->numUniq = Q->numUniq;
	if (s->o.verbose) printf("Parsed %lu queries, %lu unique [min %u, max %u, maxED %u]; clear %lu, ambiguous %lu, bad %lu\n", (unsigned long)Q->totQ,
	                         (unsigned long)Q->numUniq, Q->minLen, Q->maxLen, Q->maxED, (unsigned long)Q->nClear, (unsigned long)Q->nAmbig, (unsigned long)Q->nBad);
	if (s->db->shear && (uint32_t)(Q->maxLen / s->o.thres) > s->db->shear)                    /* burst.c:5152-5156 */
		return sample_fail(s, res, BH_E_USAGE, "ERROR: DB incompatible with selected queries/identity.");
	if (s->o.verbose) printf(" [%-28s %8.3f s%s; waited for %.3f s]\n", "queries parsed, sorted", g->secs, g->threaded ? ", on a thread ahead of its turn" : "", res->secIngestWaited);
	if (out_path && s->i0 >= 0) {      /* (in a job of processes only rank 0 writes) */
		if (!(s->out_path = strdup(out_path))) return sample_fail(s, res, BH_E_OOM, "OOM:session");
		if (!(s->out = fopen(out_path, "wb"))) {
			char msg[512]; snprintf(msg, sizeof msg, "ERROR: Cannot open output: %s", out_path);
			free(s->out_path); s->out_path = NULL;      /* (not ours to remove) */
			return sample_fail(s, res, BH_E_IO, msg);
		}
	}
	return BH_OK;
}

static void drop_sample(BhSession *s) {
	close_output(s, 0);
	if (s->sam) bh_sam_discard(s->sam);
	if (s->cur) { ingest_free(s->cur); s->cur = NULL; }
	free(s->cov_name); s->cov_name = NULL;
}
int bh_session_drop(BhSession *s) {
	if (!s) return BH_OK;
	/* a loaded sample that is given up (another rank could not have it) is a failed sample to the coverage: an all-zero column under
	 * its name, so that the later samples keep their columns */
	if (s->o.cov && s->cur && s->cov_name && !s->dead) (void)bh_cov_sample_failed(s->o.cov, s->cov_name);
	if (s->o.em && s->cur && s->cov_name && !s->dead) (void)bh_em_sample_failed(s->o.em, s->cov_name);
	if (s->taxa && s->cur && s->cov_name && !s->dead) (void)bh_taxa_sample_failed(s->taxa, s->cov_name);
	if (s->o.pile && s->cur && s->cov_name && !s->dead) (void)bh_pile_sample_failed(s->o.pile, s->cov_name);
	if (s->cons && s->cur && s->cov_name && !s->dead) (void)bh_consensus_sample_failed(s->cons, s->cov_name);
	if (s->vcf && s->cur) { bh_vcf_sample_failed(s->vcf); if (s->cov_name && !s->dead) (void)bh_vcf_study_sample_failed(s->vcf, s->cov_name); }
	drop_sample(s);
	return BH_OK;
}

static void sum_stats(BhipStats *t, const BhipStats *a) {
	t->n_queries += a->n_queries; t->n_pairs += a->n_pairs; t->n_columns += a->n_columns; t->n_raw_hits += a->n_raw_hits; t->n_hits += a->n_hits;
	t->acx_entries_read += a->acx_entries_read; t->n_windows += a->n_windows; t->n_window_columns += a->n_window_columns; t->n_lane_tasks += a->n_lane_tasks;
	t->n_task_columns += a->n_task_columns; t->n_seed_words += a->n_seed_words; t->myers_launches += a->myers_launches; t->prefilter_launches += a->prefilter_launches;
	t->ms_total += a->ms_total;
}

int bh_session_finish(BhSession *s, BhSampleResult *res) {
	BhSampleResult tmp;
	if (!res) { memset(&tmp, 0, sizeof tmp); res = &tmp; }
	if (!s || !s->cur) return bh_set_error(BH_E_USAGE, "bh_session_finish: no sample loaded");
	if (s->dead) return sample_fail(s, res, s->dead, "the session was ended by an earlier error");
	BhQueries *Q = &s->cur->Q;
	BhMultiRank *R = s->ranks;
	const BhSessionOpts *o = &s->o;
	const int n = s->n_local, S = o->shard_db > 1 ? o->shard_db : 1, n_groups = s->n_ranks / S;
	const uint64_t strands = Q->numEntries > Q->numUniq ? 2 : 1, batch = o->batch ? o->batch : (uint64_t)1 << 21;
	double tp = wall();
	#define PHASE(name) do { const double t_ = wall(); if (o->verbose) printf(" [%-28s %8.3f s]\n", name, t_ - tp); tp = t_; } while (0)
	int on_device = 0;
	for (int i = 0; i < n; ++i) on_device |= !R[i].align && R[i].hh;
	if (on_device) { bh_queries_pin(Q); PHASE("query arrays page-locked"); }
	for (int i = 0; i < n; ++i) {
		const int grp = R[i].rank / S;      /* the ranks of a replica group align the same queries, each against its shard */
		s->ru0[i] = Q->numUniq * (uint64_t)grp / (uint64_t)n_groups; s->ru1[i] = Q->numUniq * (uint64_t)(grp + 1) / (uint64_t)n_groups;
		R[i].r0 = &s->ru0[i]; R[i].r1 = &s->ru1[i]; R[i].n_ranges = 1;
		if (R[i].align) { R[i].run.nHits = 0; R[i].run.nBatches = 0; R[i].run.secAlign = 0; memset(&R[i].run.total, 0, sizeof R[i].run.total); }
	}
	s->all.nHits = 0; s->all.nBatches = 0; s->all.secAlign = 0; memset(&s->all.total, 0, sizeof s->all.total);
	const int multi = !(s->n_ranks == 1 && !R[0].align && !s->node);
	if (on_device && !s->node && n > 1 && !s->comm && S == 1) {
		/* the ranks' record buffers as slices of ONE page-locked block, so that what they deliver is read where it lies (a view over
		 * the block, bh_report_view); the block is kept across samples and grown when a sample needs more */
		uint64_t off[BH_MAX_RANKS + 1]; off[0] = 0;
		for (int i = 0; i < n; ++i) { const uint64_t k = s->ru1[i] - s->ru0[i]; off[i + 1] = off[i] + k * strands + k / 2 + (1u << 20); }
		const BhipHit *old = s->block.hits;
		if (!bh_run_reserve(&s->block, off[n])) for (int i = 0; i < n; ++i) {
			if (R[i].run.hits && R[i].run.hitsPinned != 2) bh_run_free(&R[i].run);      /* (a rank that outgrew its slice went on in a buffer of its own) */
			R[i].run.hits = s->block.hits + off[i]; R[i].run.capHits = off[i + 1] - off[i]; R[i].run.hitsPinned = 2;
		} else for (int i = 0; i < n; ++i) if (R[i].run.hitsPinned == 2 && old) memset(&R[i].run, 0, sizeof R[i].run);      /* (the old block is gone) */
	}
	if (on_device) {
		/* device and record buffers for the batches to come, sized from the batches that will really be staged (main.c).  The handle keeps
		 * what it has; bhip_reserve_symbols ends in a warm-up pass through the whole chain and every allocation synchronises the device,
		 * so it is called again only for a sample that exceeds what was reserved before */
		#pragma omp parallel for num_threads(n) schedule(static, 1)
		for (int i = 0; i < n; ++i) {
			if (!R[i].align && R[i].hh) {
				const uint64_t k = s->ru1[i] - s->ru0[i], B = k < batch ? k : batch;
				uint64_t sym = 0;
				for (uint64_t u = s->ru0[i]; u < s->ru1[i]; u += B ? B : 1) {
					const uint64_t e = u + B < s->ru1[i] ? u + B : s->ru1[i];
					uint64_t sy = Q->qoff[e] - Q->qoff[u];
					if (strands == 2) sy += Q->qoff[Q->numUniq + e] - Q->qoff[Q->numUniq + u];
					if (sy > sym) sym = sy;
				}
				if (!s->node && !R[i].run.hits) bh_run_reserve(&R[i].run, k * strands + k / 2 + (1u << 20));      /* (no slice of the block, no segment) */
				if (B && (B * strands > s->resEntries[i] || Q->maxLen > s->resMaxLen[i] || sym > s->resSym[i])) {
					const uint64_t e = B * strands > s->resEntries[i] ? B * strands : s->resEntries[i], sy = sym > s->resSym[i] ? sym : s->resSym[i];
					const uint32_t ml = Q->maxLen > s->resMaxLen[i] ? Q->maxLen : s->resMaxLen[i];
					if (bhip_reserve_symbols(R[i].hh, (uint32_t)e, ml, sy))
						fprintf(stderr, " --> WARNING: batch buffers not reserved for rank %d (%s); they are allocated batch by batch\n", R[i].rank, bhip_last_error());
					else { s->resEntries[i] = e; s->resMaxLen[i] = ml; s->resSym[i] = sy; }
				}
			}
		}
	}
	/* several ranks: the buffer their records meet in, made here and not inside the search (bh_search_multi_ex grows it if needed) */
	if (multi && s->i0 >= 0 && s->n_ranks > 1 && !s->block.hits && !s->node) bh_run_reserve_plain(&s->all, Q->numEntries + Q->numEntries / 2 + (1u << 20));
	if (on_device) PHASE("batch buffers");
	const double t0 = wall();
	BhRunView view; memset(&view, 0, sizeof view);
	uint64_t cnts[BH_MAX_RANKS]; memset(cnts, 0, sizeof cnts);
	int rc;
	uint64_t nHits = 0, nPairs = 0; uint32_t nBatches = 0;
	if (!multi) {
		rc = bh_align_ranges_reuse(R[0].hh, Q, &s->ru0[0], &s->ru1[0], 1, o->mode, batch, &R[0].run);
		view.base = R[0].run.hits; view.n_runs = 1; view.off[0] = 0; view.n[0] = R[0].run.nHits; view.total = R[0].run.nHits;
		nHits = R[0].run.nHits; nBatches = R[0].run.nBatches;
	} else {
		rc = bh_search_multi_ex(R, n, s->n_ranks, s->comm, s->node, Q, o->mode, batch, S > 1 ? S : 0, &s->all, cnts, &view);
		nHits = s->all.nHits; nBatches = s->all.nBatches;
		if (!rc && o->verbose && n == s->n_ranks && n > 1) {
			printf("host gather: %d rank(s)%s, records per rank:", n, S > 1 ? ", database-sharded" : "");
			for (int i = 0; i < n; ++i) printf(" %lu", (unsigned long)cnts[i]);
			printf("; align phase per rank [s]:");
			for (int i = 0; i < n; ++i) printf(" %.4f", R[i].secSearch);
			printf("\n");
		}
	}
	/* an error of the search is never the sample's own (the reference's "truncation within known good path" stop included): the
	 * devices' state is unknown from here on, the session ends */
	if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail_ex(s, res, rc, msg, 1); }
	for (int i = 0; i < n; ++i) { nPairs += R[i].run.total.n_pairs; sum_stats(&res->total, &R[i].run.total); }
	res->secSearch = wall() - t0; res->nHits = nHits; res->nBatches = nBatches;
	if (o->verbose) printf("Search complete [%f s, %u batches, %lu candidate (query, clump) pairs, %lu hits]. Consolidating results...\n", res->secSearch, nBatches, (unsigned long)nPairs, (unsigned long)nHits);
	PHASE("search (all batches)");
	if (s->i0 >= 0 && s->out) {
		const double tr = wall();
		uint64_t lines = 0;
		setvbuf(s->out, NULL, _IOFBF, 1 << 22);
		rc = (o->cigar || o->pile || s->cons || s->vcf || s->chimera || s->sam) && !s->paths ? bh_paths_open(R[s->i0].hh, &s->paths) : BH_OK;
		if (!rc && s->paths) bh_paths_set_pile(s->paths, o->pile, o->cigar);
		if (!rc && s->chimera && !(rc = bh_chimera_begin(s->chimera, s->db, Q))) bh_paths_set_chimera(s->paths, s->chimera, o->cigar);
		if (!rc && s->sam) rc = bh_sam_begin(s->sam, R[s->i0].hh, Q, s->out_path);
		if (!rc && s->paths) rc = bh_paths_set_sam(s->paths, s->sam, o->cigar);
		if (!rc && s->paths) rc = bh_paths_set_consensus(s->paths, s->cons, o->cigar);
		if (!rc && s->paths) rc = bh_paths_set_vcf(s->paths, s->vcf, o->cigar);
		s->sink.want_re = s->cluster != NULL;
		if (!rc) rc = bh_report_view_paths(s->out, s->db, Q, &view, o->mode, (o->do_accel ? 0 : BH_REP_MERGED_LIST) | o->rep_flags, o->tax ? o->tax : NULL, &lines, o->cov || o->em || s->cluster || s->taxa ? &s->sink : NULL, s->paths);
		if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail(s, res, rc, msg); }
		FILE *f = s->out; s->out = NULL;
		if (fclose(f)) { char msg[512]; snprintf(msg, sizeof msg, "ERROR: write failed: %s", s->out_path); return sample_fail(s, res, BH_E_IO, msg); }      /* (a full disk must not end in success) */
		close_output(s, 1);
		res->nLines = lines; res->secReport = wall() - tr;
		if (o->verbose) printf("Wrote %lu alignments\n", (unsigned long)lines);
		if (o->verbose && s->paths) bh_paths_print_info(s->paths, R[s->i0].hh);
		PHASE("consolidation, output");
		if (o->cov) {      /* the sample's column: its placements to rank 0's device (no collective: the lines exist only here) */
			rc = S > 1 ? bh_cov_lengths_host(o->cov) : BH_OK;      /* (database-sharded: rank 0's handle holds a slice, the default lengths come from host memory) */
			if (!rc) rc = bh_cov_sample(o->cov, R[s->i0].hh, s->cov_name, s->sink.lines, s->sink.n);
			s->cov_col = 1;      /* (the column exists: a failure below must not add another) */
			if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail_ex(s, res, rc, msg, 1); }
			PHASE("coverage of the sample");
		}
		if (o->em) {       /* the sample's abundance column, on rank 0's device as well */
			rc = bh_em_sample(o->em, R[s->i0].hh, s->cov_name, s->sink.uq, s->sink.lines, s->sink.n);
			s->em_col = 1;
			if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail_ex(s, res, rc, msg, 1); }
			if (o->verbose) bh_em_print_info(o->em);
			PHASE("abundance of the sample");
		}
		if (s->taxa) {     /* the sample's column of the taxon tables from the same groups, with the abundance's counts when there are any */
			rc = bh_taxa_sample(s->taxa, R[s->i0].hh, s->cov_name, s->sink.uq, s->sink.lines, s->sink.n, o->em ? bh_em_last_column(o->em) : NULL);
			s->taxa_col = 1;
			if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail_ex(s, res, rc, msg, 1); }
			if (o->verbose) bh_taxa_print_info(s->taxa);
			PHASE("taxa of the sample");
		}
		if (o->pile) {     /* the sample's variant sites: one call over the lines the tracer handed over, on rank 0's device as well */
			rc = bh_pile_sample(o->pile, R[s->i0].hh, s->cov_name, Q->codes, Q->qoff, Q->numEntries);
			s->pile_col = 1;
			if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail_ex(s, res, rc, msg, 1); }
			if (o->verbose) bh_pile_print_info(o->pile);
			PHASE("variant sites of the sample");
		}
		if (s->cons) {     /* the sample's consensus: one call over the lines the tracer handed over, on rank 0's device as well */
			rc = bh_consensus_sample(s->cons, R[s->i0].hh, s->cov_name, Q->codes, Q->qoff, Q->numEntries);
			s->cons_col = 1;
			if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail_ex(s, res, rc, msg, 1); }
			if (o->verbose) bh_consensus_print_info(s->cons);
			PHASE("consensus of the sample");
		}
		if (s->vcf) {      /* the sample's OUT.vcf: its sites and its alleles, one call each over the lines the tracer handed over */
			rc = bh_vcf_sample(s->vcf, R[s->i0].hh, s->cov_name, Q->codes, Q->qoff, Q->numEntries);
			s->vcf_col = 1;      /* (a study has the sample, or its '.' column) */
			if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail(s, res, rc, msg); }
			if (o->verbose) bh_vcf_print_info(s->vcf);
			PHASE("VCF of the sample");
		}
		if (s->cluster) {  /* the sample's reads clustered from its own lines, on rank 0's device as well; the tables at once */
			rc = bh_cluster_sample(s->cluster, R[s->i0].hh, s->db, Q, &s->sink);
			if (!rc) rc = bh_cluster_write(s->cluster);
			if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail_ex(s, res, rc, msg, 1); }
			if (o->verbose) bh_cluster_print_info(s->cluster);
			PHASE("clusters of the sample");
		}
		if (s->chimera) {  /* the sample's reads checked from its own lines and their paths, on rank 0's device as well; the table at once */
			rc = bh_chimera_solve(s->chimera, R[s->i0].hh);
			if (!rc) rc = bh_chimera_write(s->chimera);
			if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail_ex(s, res, rc, msg, 1); }
			if (o->verbose) bh_chimera_print_info(s->chimera);
			PHASE("chimera check of the sample");
		}
		if (s->sam) {      /* the sample has succeeded: the unmapped records, OUT.sam under its name */
			rc = bh_sam_end(s->sam);
			if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); return sample_fail(s, res, rc, msg); }
			if (o->verbose) bh_sam_print_info(s->sam);
			PHASE("SAM records of the sample");
		}
		free(s->cov_name); s->cov_name = NULL;
	}
	#undef PHASE
	ingest_free(s->cur); s->cur = NULL;      /* the sample's tables and page-lockings; the record buffers stay */
	return BH_OK;
}

int bh_session_run(BhSession *s, const char *queries, const char *out_path, BhSampleResult *res) {
	const int rc = bh_session_load(s, queries, out_path, res);
	return rc ? rc : bh_session_finish(s, res);
}

BhMates *bh_session_mates(BhSession *s) {
	if (s && !s->mates && bh_mates_open(NULL, &s->mates)) return NULL;
	return s ? s->mates : NULL;
}

static void add_result(BhSampleResult *t, const BhSampleResult *a) {
	t->totQ += a->totQ; t->numUniq += a->numUniq; t->nHits += a->nHits; t->nBatches += a->nBatches;
	t->secIngest += a->secIngest; t->secIngestWaited += a->secIngestWaited; t->secSearch += a->secSearch; t->secReport += a->secReport;
	sum_stats(&t->total, &a->total);
}
static int mates_fail(BhSession *s, BhSampleResult *res, int rc, const char *msg) {
	res->rc = rc;
	snprintf(res->err, sizeof res->err, "%s", msg);
	if (rc != BH_E_USAGE && rc != BH_E_IO) s->dead = rc;
	return bh_set_error(rc, "%s", res->err);
}

int bh_session_run_mates(BhSession *s, const char *queries1, const char *queries2, const char *out_path, BhSampleResult *res) {
	BhSampleResult tmp, one;
	if (!res) res = &tmp;
	memset(res, 0, sizeof *res);
	if (!s || !queries1 || !queries2) return bh_set_error(BH_E_USAGE, "bh_session_run_mates: no session / no files");
	if (s->o.mode != BH_ALLPATHS && s->o.mode != BH_FORAGE) return mates_fail(s, res, BH_E_USAGE, "ERROR: mates are joined from ALLPATHS or FORAGE placements (the other modes discard the ties the join needs)");
	if (!s->o.do_rc) return mates_fail(s, res, BH_E_USAGE, "ERROR: mates need both strands searched (-fr)");
	if (s->o.cov || s->o.cigar) return mates_fail(s, res, BH_E_USAGE, "ERROR: coverage and alignment paths of paired output are out of scope: mates go with neither");
	if (s->o.em) return mates_fail(s, res, BH_E_USAGE, "ERROR: the abundance of paired output is out of scope: mates do not go with it");
	if (s->taxa) return mates_fail(s, res, BH_E_USAGE, "ERROR: the taxon tables of paired output are out of scope: mates do not go with them");
	if (s->o.pile) return mates_fail(s, res, BH_E_USAGE, "ERROR: variants of paired output are out of scope: mates do not go with them");
	if (s->cons) return mates_fail(s, res, BH_E_USAGE, "ERROR: the consensus of paired output is out of scope: mates do not go with it");
	if (s->vcf) return mates_fail(s, res, BH_E_USAGE, "ERROR: the VCF output of paired output is out of scope: mates do not go with it");
	if (s->chimera) return mates_fail(s, res, BH_E_USAGE, "ERROR: the chimera check works from the lines of one query file against itself: mates do not go with it");
	if (s->sam) return mates_fail(s, res, BH_E_USAGE, "ERROR: paired flags, RNEXT and TLEN are out of scope: mates do not go with the SAM output");
	if (s->cluster) return mates_fail(s, res, BH_E_USAGE, "ERROR: clusters come from the lines of one query file against itself: mates do not go with them");
	if (s->o.mates.orientation > BHIP_MATES_FF || s->o.mates.report > BHIP_MATES_BEST || s->o.mates.ins_min > s->o.mates.ins_max)
		return mates_fail(s, res, BH_E_USAGE, "ERROR: mates: orientation fr|rf|ff, report all|best, insert-min <= insert-max");
	if (s->dead) { res->rc = s->dead; snprintf(res->err, sizeof res->err, "the session was ended by an earlier error (code %d)", s->dead); return bh_set_error(s->dead, "%s", res->err); }
	const int writes = out_path && s->i0 >= 0;      /* (in a job of processes only rank 0 holds lines) */
	char *t1 = NULL, *t2 = NULL, *to = NULL;
	if (writes) {
		const size_t n = strlen(out_path) + 16;
		t1 = malloc(n); t2 = malloc(n); to = malloc(n);
		if (!t1 || !t2 || !to) { free(t1); free(t2); free(to); return mates_fail(s, res, BH_E_OOM, "OOM:session"); }
		snprintf(t1, n, "%s.mate1.tmp", out_path); snprintf(t2, n, "%s.mate2.tmp", out_path); snprintf(to, n, "%s.tmp", out_path);
		if (!bh_session_mates(s)) { free(t1); free(t2); free(to); return mates_fail(s, res, BH_E_OOM, "OOM:mates"); }
	}
	int rc = BH_OK;
	const char *qs[2] = {queries1, queries2};
	for (int k = 0; k < 2 && !rc; ++k) {
		if (!k) bh_session_prefetch(s, queries2);      /* mate 2 is parsed while mate 1 is searched */
		if (s->o.verbose) printf("Mate %d: %s\n", k + 1, qs[k]);
		rc = bh_session_load(s, qs[k], writes ? (k ? t2 : t1) : NULL, &one);
		if (!rc && writes && (rc = bh_mates_names(s->mates, k, s->cur->Q.heads, s->cur->Q.totQ))) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); rc = sample_fail(s, &one, rc, msg); }
		if (!rc) rc = bh_session_finish(s, &one);
		add_result(res, &one);
		if (rc) { res->rc = rc; snprintf(res->err, sizeof res->err, "%s", one.err); }
	}
	if (!rc && writes) {
		const double tj = wall();
		FILE *f = fopen(to, "wb");
		if (!f) { char msg[512]; snprintf(msg, sizeof msg, "ERROR: Cannot open output: %s", to); rc = mates_fail(s, res, BH_E_IO, msg); }
		else {
			setvbuf(f, NULL, _IOFBF, 1 << 22);
			bh_mates_set_handle(s->mates, s->ranks[s->i0].hh);
			uint64_t lines = 0;
			rc = bh_mates_join_files(s->mates, t1, t2, f, &s->o.mates, &lines);
			if (rc) { char msg[512]; snprintf(msg, sizeof msg, "%s", bh_last_error()); fclose(f); rc = mates_fail(s, res, rc, msg); }
			else if (fclose(f) || rename(to, out_path)) { char msg[512]; snprintf(msg, sizeof msg, "ERROR: write failed: %s", out_path); rc = mates_fail(s, res, BH_E_IO, msg); }
			else {
				res->nLines = lines; res->secReport += wall() - tj;
				if (s->o.verbose) { printf("Wrote %lu lines of %lu concordant combinations\n", (unsigned long)lines, (unsigned long)(lines / 2)); bh_mates_print_info(s->mates); }
			}
		}
	}
	if (writes) { (void)unlink(t1); (void)unlink(t2); if (rc) (void)unlink(to); }
	free(t1); free(t2); free(to);
	return rc;
}

void bh_session_close(BhSession *s) {
	if (!s) return;
	if (s->ahead) { pthread_join(s->th, NULL); ingest_free(s->ahead); s->ahead = NULL; }
	drop_sample(s);      /* (not bh_session_drop: the coverage object may be gone by now) */
	free(s->pending);
	/* the ranks' runs belong to the caller (BhMultiRank.run); slices of the session's block must not outlive it */
	for (int i = 0; i < s->n_local; ++i) if (s->block.hits && s->ranks[i].run.hitsPinned == 2 && s->ranks[i].run.hits >= s->block.hits && s->ranks[i].run.hits < s->block.hits + s->block.capHits) memset(&s->ranks[i].run, 0, sizeof s->ranks[i].run);
	bh_run_free(&s->block); bh_run_free(&s->all);
	free(s->sink.lines); free(s->sink.uq); free(s->sink.re); free(s->cov_name); bh_paths_close(s->paths); bh_mates_close(s->mates);
	pthread_mutex_destroy(&s->mu);
	free(s);
}
