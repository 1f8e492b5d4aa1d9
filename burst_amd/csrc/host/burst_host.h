/* burst_amd/csrc/host/burst_host.h -- C host side of the alignment path (libburst_host.so + the burst_hip CLI).
 *
 * Mirrors, in plain C, the parts of the reference's single translation unit that sit either side of the
 * kernels: query pipeline (process_queries, burst.c:2980-3223), database readers (read_edb 2842-2975,
 * read_accelerator 3535-3594), direct-FASTA clumping (process_references QUICK path 1840-1858, 2109-2190,
 * 2687-2741), the batch scheduler that replaces the OpenMP loops of do_alignments (4018-4488) by calls into
 * libburst_hip.so, and the per-mode consolidation + .b6 writer (4490-4891).
 * Errors are return codes (<0) with bh_last_error(); nothing here calls exit().
 */
#ifndef BURST_HOST_H
#define BURST_HOST_H
#include <stdint.h>
#include <stdio.h>
#include "burst_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BH_OK        0
#define BH_E_USAGE  -1   /* reference exit(1): usage / format */
#define BH_E_IO     -2   /* reference exit(2): cannot open */
#define BH_E_OOM    -3   /* reference exit(3) */
#define BH_E_INTERNAL -4
#define BH_E_DEVICE -5
#define BH_E_CAPACITY -6   /* not an error of the job: the caller has to take the other path (bh_node_collect_view) */

typedef enum { BH_FORAGE = 0, BH_BEST, BH_ALLPATHS, BH_CAPITALIST, BH_ANY } BhMode;   /* burst.c:75-78 */

/* ---- tables (burst.c:164-192, 1237-1329) ---- */
void bh_score_lut(int z, uint8_t lut[256]);        /* SCOREFAST after setScore(): lut[16*q+r] in {0,1,255} */
void bh_char2code(uint8_t map[256]);               /* CHAR2NUM, bytes >= 128 map to 0 */
void bh_set_alphabet(const uint8_t map[256]);      /* -x: byte -> code 1..15 of a caller-made alphabet (NULL: back to CHAR2NUM); bh_score_lut is then the identity table */
int  bh_alphabet_is_set(void);
int  bh_alphabet_from_files(const char *ref_fa, const char *query_fa, uint8_t map[256], int *n_symbols);      /* BH_E_USAGE beyond 15 symbols */
uint8_t bh_rc_code(uint8_t c);                     /* RVT */
uint32_t bh_error_budget(float thres, uint32_t len);   /* burst.c:3069-3076 */

/* ---- database ---- */
typedef struct BhDb {
	/* .edx (burst.c:2842-2975) */
	int rebase, xalpha;
	uint32_t shear, totR, origTotR, numRclumps, maxLenR, numRefHeads;
	char *headDump;          /* NUL-separated unique headers */
	char **refHead;          /* [origTotR] header of each sheared reference (through RefMap) */
	uint32_t *refMap;        /* [origTotR] sheared ref -> unique header index */
	uint32_t *refStart;      /* [origTotR] or NULL */
	uint32_t *refDedupIx;    /* [totR+1] or NULL */
	uint32_t *tmpRIX;        /* [origTotR] */
	uint32_t *refIxSrt;      /* [totR] = TmpRIX[RefDedupIx[i]] or TmpRIX (burst.c:3688-3693) */
	uint32_t *clumpLen;      /* [numRclumps] */
	uint8_t  *packed;        /* clump area, 16-byte words */
	uint64_t packedWords;
	/* .acx (burst.c:3535-3594), optional */
	int hasAcx, K, acxFmt, acxZ;
	uint32_t *acxLens;       /* [4^K] */
	uint8_t  *acxLists; uint64_t acxListBytes;
	uint32_t *badList; uint32_t badSz;
	/* bookkeeping */
	int identityMap;         /* direct-FASTA runs: RefMap is the identity (burst.c:4545-4551) */
	void *owned[32]; int nOwned;
	void *mapBase; uint64_t mapLen;      /* the clump area of a large .edx is a read-only mapping of the file (bh_edx_read): the processes of a node share one copy */
	uint32_t *fragLen;       /* [origTotR] fragment lengths of a compressive (-d DNA) build, or NULL: what the accelerator builders index (bh_db_trim_lanes) */
} BhDb;

int  bh_is_edx(const char *path);                       /* burst.c:4894-4901: first byte has bit 7 set; <0 on IO error */
int  bh_edx_read(const char *path, BhDb *db);
int  bh_acx_read(const char *path, int K, int z, BhDb *db);
/* direct -r fasta (no DB): QUICK pipeline; shear_len = 0 disables shearing (burst.c:5046-5053) */
int  bh_db_from_fasta(const char *path, uint32_t maxLenQ, float thres, int do_shear, long shear_len, int dedupe, BhDb *db);
/* DB construction (tooling for tests/bench) */
int  bh_edx_write(const BhDb *db, const char *path, long db_qlen, float thres);
/* latency = clump formation tolerance, the reference's `-l` (LATENCY, burst.c:83): 16 in bh_db_from_fasta, 0 = input order */
int  bh_db_from_fasta_ex(const char *path, uint32_t maxLenQ, float thres, int do_shear, long shear_len, int dedupe, uint32_t latency, BhDb *db);
/* n .edx files laid end to end into one (every part but the last must fill its last clump; no duplicate-fragment tables): a
 * database too large to be built in one piece in the memory at hand, built part by part */
int  bh_edx_merge(const char *const *paths, int n, const char *out_path);
/* -d DNA / RNA with -s: the compressive build (process_references, DNA_16 branch, burst.c:1859-2108).  The sequences lie in one array,
 * a single 0 between consecutive ones (parse_tl_fasta_db, 541-605); duplicate marks per partition of ceil(n / partitions) references
 * (`-dp`, 0 = 1) on `device` (bhip_dna_marks) or, with device < 0 or none usable, by bh_dna_marks_host; the flag-guided shear; then
 * the stages of the QUICK build.  stats may be NULL. */
typedef struct BhDnaStats {
	int device;                 /* where the marks were computed: device number, or -1 = host */
	uint32_t W, shear, ov, partitions;
	uint64_t maxChain, maxSh, eligible, chunks, exactChunks, peakDeviceBytes, symbols, fragments;
	double secParse, secMarks, secShear, secStages;
	double secUpload, secSort, secClassify, secMark;      /* device marks, summed over partitions */
	char note[256];             /* why the host computed the marks on a machine asked to use a device */
} BhDnaStats;
int  bh_db_from_fasta_dna(const char *path, uint32_t maxLenQ, float thres, long shear_len, uint32_t partitions, int dedupe, uint32_t latency,
                          int device, BhDb *db, BhDnaStats *stats);
/* flags[p - ref_start[0]... ] for the positions [0, ref_start[n-1] + ref_len[n-1]) of one partition (ref_start relative to sym):
 * the OR of the two convs (low nibble); reads and updates *max_chain / *max_sh as the reference's state across partitions */
int  bh_dna_marks_host(const uint8_t *sym, const uint64_t *ref_start, const uint32_t *ref_len, uint64_t n_refs, uint32_t W,
                       uint64_t *max_chain, uint64_t *max_sh, uint8_t *flags);
int  bh_dna_shear(const uint8_t *flags, const uint64_t *ref_start, const uint32_t *ref_len, uint32_t n_refs, uint32_t shear, uint32_t ov,
                  uint32_t *frag_ref, uint32_t *frag_start, uint32_t *frag_len, uint64_t cap, uint64_t *n_frag);
int  bh_db_trim_lanes(BhDb *db, uint8_t **keep);      /* db->packed := copy with every lane zeroed from its fragment length on (no-op without fragLen) */
void bh_db_untrim_lanes(BhDb *db, uint8_t *keep);
int  bh_acx_build(BhDb *db, int K, int z);
/* skip_ambig = -sa: leave out every word that holds an ambiguous symbol (burst.c:3360-3366) */
int  bh_acx_build_ex(BhDb *db, int K, int z, int skip_ambig);
/* the accelerator tables of `db` from a device handle that holds this database's accelerator (bhip_acx_export), packed as the
 * reference writes them (burst.c:3501-3530): with a handle whose accelerator was built on the device this is make_accelerator
 * without the host pass */
int  bh_acx_from_device(BhDb *db, void *hip_handle, int K, int z);
/* the same tables written to an .acx file without being held on the host (the list area is streamed from the device run by run) */
int  bh_acx_write_from_device(const BhDb *db, void *hip_handle, int K, int z, const char *path);
/* view of the clumps [c0, c1) with the accelerator restricted to them (database sharding); `db` must outlive the view */
int  bh_db_slice(const BhDb *db, uint32_t c0, uint32_t c1, BhDb *out);
int  bh_acx_write(const BhDb *db, const char *path);
void bh_db_free(BhDb *db);

/* ---- queries (burst.c:2980-3223) ---- */
typedef struct BhQueries {
	uint64_t totQ, numUniq, numEntries;   /* entries = unique forward queries, then (with -fr) their reverse complements */
	char *dump;            /* file contents; heads point into it */
	char **heads;          /* [totQ] headers in sorted-sequence order (QHead after burst.c:3055-3060) */
	uint64_t *offset;      /* [numUniq+1] Offset: reads of unique query i are heads[offset[i]..offset[i+1]) */
	uint8_t *codes;        /* concatenated symbol codes of all entries */
	uint8_t *codes4;       /* the same, two symbols per byte (low nibble first): what the device batches are copied from */
	uint8_t *codes2;       /* the same, four symbols per byte (code - 1 in two bits; symbols beyond A/C/G/T read as A): batches without such symbols are copied from here */
	uint16_t *len16;       /* [numUniq] ShrBin.len again, as the 2-byte lengths the device batches carry instead of 8-byte offsets */
	uint32_t *ambBefore;   /* [numUniq+1] unique queries in front of i that hold a symbol beyond A/C/G/T (a batch [u, u+B) is clean iff the counts at its ends agree) */
	uint64_t *qoff;        /* [numEntries+1] */
	uint32_t *six;         /* [numEntries] shared slot = unique query index */
	uint8_t *rc;           /* [numEntries] */
	uint8_t *flags;        /* [numEntries] BHIP_Q_PREFILTER / BHIP_Q_EXHAUSTIVE (query binning, burst.c:3113-3141) */
	uint16_t *emac;        /* [numEntries] budget of the entry's shared slot */
	uint32_t *len;         /* [numUniq] ShrBin.len */
	uint16_t *ed;          /* [numUniq] ShrBin.ed (initial budget) */
	uint32_t maxLen, minLen, maxED;
	uint64_t nClear, nAmbig, nBad;
	int pinned;            /* codes / qoff are page-locked (bh_queries_pin) */
} BhQueries;

/* device that sorts and de-duplicates large query files (default 0; < 0 = always on the host) */
void bh_queries_sort_device(int device);
void bh_device_gate(int device, int take);
int  bh_device_gate_try(int device);      /* bh_align.c: serialises the set-up steps that size themselves from a device's free memory */
int  bh_queries_load(const char *fasta, float thres, int do_rc, int incl_whitespace, int do_accel, int K, int z,
                     int skip_ambig, BhQueries *q);
/* prefilter / exhaustive route per entry and the clear / ambiguous / bad counts; bh_queries_load does it itself unless it was
 * called with do_accel and K = 0 (queries read beside the database, K not known yet) */
void bh_queries_bins(BhQueries *q, int do_accel, int K, int z);
void bh_queries_free(BhQueries *q);
/* page-lock the arrays the device batches are copied from, so that the copies of batch k+1 run beside the kernels of batch k
 * (optional; needs a device) */
int  bh_queries_pin(BhQueries *q);

/* ---- alignment driver: batches of entries through bhip_align_batch ---- */
typedef struct BhRun {
	BhipHit *hits; uint64_t nHits;        /* all records, q = entry index, sorted by (q, refIx) */
	double secAlign;                      /* wall time inside the device calls */
	BhipStats total;                      /* summed over batches (times in ms) */
	uint32_t nBatches;
	int hitsPinned;                       /* hits is page-locked memory of the device library */
	uint64_t capHits;                     /* records the buffer holds */
	/* optional: called after every batch with the device handle (whose records of that batch are still resident) and the batch's place in
	 * `hits` -- the RCCL gather of bh_search_multi_ex stages the records device to device instead of uploading the host copy again */
	void (*onBatch)(void *ctx, void *hip_handle, uint64_t first_record, uint64_t n_records);
	void *onBatchCtx;
} BhRun;
/* entry range [e0, e1) of unique queries [u0, u1): forward entries u0..u1-1 and (if numEntries > numUniq) their RC twins
 * are always sent together because they share the running minimum (burst.c:277-280, 4218). */
int  bh_align(void *hip_handle, const BhQueries *q, uint64_t u0, uint64_t u1, BhMode mode, uint64_t batch_uniq, BhRun *run);
/* the same over several ranges of unique queries, in the order given (a range is cut into batches of at most batch_uniq);
 * bh_align is the one-range case */
int  bh_align_ranges(void *hip_handle, const BhQueries *q, const uint64_t *u0, const uint64_t *u1, uint32_t n_ranges, BhMode mode, uint64_t batch_uniq, BhRun *run);
/* into a BhRun used before (or zeroed): keeps its page-locked record buffer */
int  bh_align_ranges_reuse(void *hip_handle, const BhQueries *q, const uint64_t *u0, const uint64_t *u1, uint32_t n_ranges, BhMode mode, uint64_t batch_uniq, BhRun *run);
int  bh_run_reserve(BhRun *run, uint64_t cap_records);
int  bh_run_reserve_plain(BhRun *run, uint64_t cap_records);      /* pageable memory */
void bh_run_free(BhRun *run);
/* ---- multi-GPU search (bh_multi.c) ---- */
#define BH_MAX_RANKS 16
typedef struct BhMultiRank {
	int rank;                     /* rank of the node-wide job */
	void *hh;                     /* its device handle */
	const uint64_t *r0, *r1; uint32_t n_ranges;   /* ranges of unique queries it aligns (database-sharded: normally one range, everything) */
	uint32_t c0;                  /* database-sharded: first clump of its slice (added to the records' reference numbers) */
	BhRun run;                    /* its own records (the page-locked buffer is reused between calls) */
	double secSearch;             /* out: wall time of this rank's align phase (before the minima / the gather) */
	int gatherPath;               /* out: how this rank's records reached rank 0 -- 0 no collective (host memory), 1 RCCL gather fed from the device
	                               * (bhip_comm_gather_staged), 2 RCCL gather of the host copy uploaded again (bhip_comm_gather_hits) */
	/* Optional back ends (NULL = the device path).  `align`: in place of the device scheduler bh_align_ranges_reuse(hh, ...) -- it
	 * fills `run` (bh_run_put) with the records of the ranges, q = entry index, sorted by (q, refIx); the CPU tests of the multi-rank
	 * search put the oracle here.  `reduce_min`: the element-wise minimum of `buf` over all ranks, in place, for ranks in different
	 * processes that have no library communicator (a launcher's own collective: torch.distributed all_reduce MIN). */
	int (*align)(void *ctx, const BhQueries *q, const uint64_t *u0, const uint64_t *u1, uint32_t n_ranges, int mode, uint64_t batch_uniq, BhRun *run);
	int (*reduce_min)(void *ctx, uint8_t *buf, uint64_t n);
	void *ctx;
} BhMultiRank;
/* n records into a run's buffer (grown when the run owns it; a shared-memory segment must be large enough) */
int  bh_run_put(BhRun *run, const BhipHit *hits, uint64_t n);
/* clump range of rank `rank` of `n_ranks`: contiguous, about the same number of reference columns each */
void bh_clump_shard(const BhDb *db, int n_ranks, int rank, uint32_t *c0, uint32_t *c1);
/* The search of the n_local ranks that live in this process (listed in rank order; one host thread each) as part of a job of
 * n_ranks: align, [database-sharded: combine the per-query minimum, drop what lies above it], gather the records to rank 0.
 * shard_db = number of database shards (0 / 1 = none: query-sharded; n_ranks = every rank its own shard; a divisor S of n_ranks =
 * n_ranks / S replica groups of S shards, rank = group * S + shard, the caller passes each rank its group's ranges and its shard's c0).
 * comm = communicator over all n_ranks (bhip_comm_create / bhip_comm_create_rank), or NULL when all ranks are local: records
 * and minima then meet in host memory.  all = the gathered records where rank 0 lives (sorted by (query entry, reference));
 * counts[n_ranks] (optional, rank 0's process) = records per rank. */
int  bh_search_multi(BhMultiRank *ranks, int n_local, int n_ranks, void *comm, const BhQueries *q, BhMode mode, uint64_t batch_uniq, int shard_db, BhRun *all, uint64_t *counts);
/* pieces of the database-sharded search, exported for the tests: records in any order -> (query entry, reference) order in place
 * ((entry, reference) pairs must be unique); element-wise minimum of n tables of len bytes into best[0] (NULL tables are skipped) */
int  bh_order_records(BhipHit *hits, uint64_t n, uint64_t n_entries);
void bh_minima_merge(uint8_t *const *best, int n, uint64_t len);
/* n_shards database shards taking turns on ONE device (a database larger than the device): every shard is uploaded, searched with all
 * queries and released; minima over the shards, filter, (query entry, reference) order -- the records of a single device holding
 * everything.  secs / up (n_shards each, may be NULL): align phase and upload (+ accelerator build with build_K) of every shard */
int  bh_search_serial_shards(const BhDb *db, int device, int n_shards, int z, int build_K, const BhQueries *Q, BhMode mode, uint64_t batch, BhRun *all, double *secs, double *up);
/* ---- ranks of one node in different processes: the records meet in shared memory (bh_node.c) ---- */
typedef struct BhNode BhNode;
/* job: a name all ranks of the job share and no other job on the machine, before or after, uses again (a peer that opens early would
 * map the segment a dead job of the same name left behind: the launchers draw 48 random bits per job); cap_records: what the rank expects to deliver per
 * search (a search that brings up to four times as many still fits).  Every rank opens; rank 0 first or at the same time. */
int  bh_node_open(const char *job, int rank, int n_ranks, uint64_t cap_records, BhNode **node);
void bh_node_close(BhNode *node);
void bh_node_attach(BhNode *node, BhRun *run);                        /* the rank's record buffer = its segment */
int  bh_node_begin(BhNode *node);                                     /* a new search: rank 0 has read the previous one's records */
int  bh_node_publish(BhNode *node, const BhRun *run, int status);     /* this rank's records of the search are complete */
int  bh_node_collect(BhNode *node, BhRun *all, uint64_t *counts);     /* rank 0: everybody's records, rank order */
/* records as runs of one address range: run r = base[off[r] .. off[r] + n[r]); what lies between the runs is not records */
typedef struct BhRunView { const BhipHit *base; int n_runs; uint64_t off[BH_MAX_RANKS], n[BH_MAX_RANKS]; uint64_t total; } BhRunView;
int  bh_node_collect_view(BhNode *node, BhRunView *view, uint64_t *counts);   /* rank 0, no copy; BH_E_CAPACITY = use bh_node_collect */
/* bh_search_multi with the hand-over through `node` instead of the communicator's gather (one rank per process: n_local = 1;
 * comm is then only needed for the minima of a database-sharded search) */
int  bh_search_multi_ex(BhMultiRank *ranks, int n_local, int n_ranks, void *comm, BhNode *node, const BhQueries *q, BhMode mode, uint64_t batch_uniq, int shard_db, BhRun *all, uint64_t *counts,
                        BhRunView *view);
/* view (optional; rank 0's process): how to read the result -- with a node and a query-sharded search the ranks' records where they
 * lie, no copy (all->nHits is their number, all->hits is NOT their place); otherwise the one run all->hits[0 .. all->nHits).
 * Valid until this rank's next search.  bh_report_view consumes it. */
int  bh_device_open(const BhDb *db, int device, int z, void **hip_handle);
/* build_K > 0 and a database without accelerator tables: the device builds the accelerator itself (no .acx file) */
int  bh_device_open_ex(const BhDb *db, int device, int z, int build_K, void **hip_handle);
/* the same for one of n_parts handles of a replicated database that build the accelerator together (bhip_build_accelerator_shared) */
int  bh_device_open_shared(const BhDb *db, int device, int z, int build_K, int part, int n_parts, bhip_share_fn share, void *ctx, void **hip_handle);

/* ---- consolidation and .b6 output (burst.c:4553-4891); hits must be sorted by (q, refIx) ---- */
int  bh_report(FILE *out, const BhDb *db, const BhQueries *q, const BhipHit *hits, uint64_t nHits, BhMode mode, uint64_t *nLines);
/* flags: BH_REP_MERGED_LIST = rebuild each query's hit list the way the reference's exhaustive path does (one list per
 * unique query shared by both strands, burst.c:4368, instead of forward list + appended reverse list, 4218/4299-4312);
 * BH_REP_NO_DUPE_HUNT = print every (hit, reference) expansion (diagnostics / tests). */
#define BH_REP_MERGED_LIST  1
#define BH_REP_NO_DUPE_HUNT 2
uint64_t bh_report_format_identities(const float *score, uint64_t n, char *out, uint64_t cap);      /* test entry: "%f" of score * 100 as the report prints it */
int  bh_report_ex(FILE *out, const BhDb *db, const BhQueries *q, const BhipHit *hits, uint64_t nHits, BhMode mode, int flags, uint64_t *nLines);

/* ---- taxonomy (column 13; parse_taxonomy burst.c:447-479, taxa_lookup 409-440, CAPITALIST interpolation 4781-4829, -bs 4820-4828) ---- */
typedef struct { uint64_t n; char **pair; char *blob; } BhTax;        /* pair[2i] = header, pair[2i+1] = taxonomy, sorted by header */
typedef struct {
	const BhTax *tax;     /* NULL = no taxonomy column */
	int suppress;         /* -bs: cut the taxonomy at the level the identity supports */
	int strict;           /* -bs STRICT */
	uint32_t taxacut;     /* -bc (default 10): 1/taxacut of the placements may disagree at a level (CAPITALIST) */
	int ncbi;             /* -bn: headers are '>xxx|accession.version...' */
} BhTaxOpts;
int  bh_tax_load(const char *file, BhTax *T);
void bh_tax_free(BhTax *T);
const char *bh_tax_lookup(const BhTax *T, const char *ref_header, int ncbi);
int  bh_report_tax(FILE *out, const BhDb *db, const BhQueries *q, const BhipHit *hits, uint64_t nHits, BhMode mode, int flags, const BhTaxOpts *tx, uint64_t *nLines);
/* the same over records that lie in several runs (the records of an entry inside one run, contiguous) */
int  bh_report_view(FILE *out, const BhDb *db, const BhQueries *q, const BhRunView *view, BhMode mode, int flags, const BhTaxOpts *tx, uint64_t *nLines);

/* the same with a placement sink (bh_report.c): sink->lines (malloc'd, the caller's to free; may be handed in again) holds, in the order
 * of the file, one entry per (unique query, placement): header number (RefMap of the reference of column 2), columns 9 and 10, and
 * w = the number of lines the entry stands for (the reads of the unique query) | unique << 31 -- unique: each of those reads is on this one
 * line of the file only.  sink->uq holds, entry by entry, the number of the entry's unique query: the entries of one query, those of its
 * reverse complement included, are the placements of the same reads (the groups of bh_em.c).  sink = NULL: bh_report_view. */
typedef struct BhPlaceSink {
	BhipCovLine *lines; uint64_t n, cap; uint32_t *uq;      /* uq[k] (malloc'd like lines): the unique query number of entry k */
	int want_re; uint64_t *re;      /* want_re set by the caller: re[k] (malloc'd like lines) = reference index of the entry's line (db->refHead[re >> 32] is column 2) << 32 | column 11 */
} BhPlaceSink;
int  bh_report_view_sink(FILE *out, const BhDb *db, const BhQueries *q, const BhRunView *view, BhMode mode, int flags, const BhTaxOpts *tx, uint64_t *nLines, BhPlaceSink *sink);

/* ---- alignment paths of the printed lines (bh_paths.c; burst_hip --cigar) ----
 * Every line gets two further tab-separated columns behind everything it has (taxonomy included): the leftmost 1-based position of the
 * path on the ORIGINAL reference (refStart of the reference of column 2 + bhip_trace_paths' ref_first) and the CIGAR text in =XID.  The
 * path is that of the line's RECORD (query entry, refIx, finalPos, ed): a reverse-strand line carries the path of its reverse-complement
 * entry against the forward reference, a duplicate read its unique query's, and a record is traced once per group of report chunks
 * whatever the number of its lines.  What stands in front of the two columns is byte for byte what the report writes without them.
 *   bh_paths_open       the tracer is bhip_trace_paths on `hip_handle` (rank 0's: the records meet there)
 *   bh_paths_set_trace  another tracer (tests): same arguments and return codes in this file's terms, BH_E_CAPACITY = op_off[n] ops wanted
 *   bh_paths_push       the report's note of one printed line: index of its record in the report's record array, refStart of its reference
 *   bh_paths_emit       n_chunks rendered chunks (text[c], text_len[c]: whole lines) and their notes, in file order, to `out`
 *   bh_cigar_text       ops (length << 4 | code) as text; returns its length, 0 = does not fit `cap` or not an op */
typedef struct BhPaths BhPaths;
typedef int (*bh_paths_trace_fn)(void *ctx, const BhQueries *q, const BhipPathReq *req, uint64_t n, uint32_t *ops, uint64_t ops_cap, uint64_t *op_off,
                                 uint32_t *ref_first, uint32_t *gap_r);
typedef struct BhPathLine { uint64_t hit; uint32_t refOff, header, uniq; } BhPathLine;      /* header, uniq: what the placement sink notes (bh_paths_push: 0, 1) */
typedef struct BhPathBuf { BhPathLine *l; uint64_t n, cap; } BhPathBuf;
int  bh_paths_open(void *hip_handle, BhPaths **paths);
void bh_paths_set_trace(BhPaths *paths, bh_paths_trace_fn fn, void *ctx);
void bh_paths_totals(const BhPaths *paths, uint64_t *requests, uint64_t *ops, uint64_t *lines);
void bh_paths_print_info(BhPaths *paths, void *hip_handle);      /* one `Paths:` line on standard output: requests, ops, device milliseconds since the last one */
void bh_paths_close(BhPaths *paths);
int  bh_paths_push(BhPathBuf *b, uint64_t hit, uint32_t ref_off);
/* the same with the line's header number (RefMap of its reference) and whether its read is on this one line of the file only */
int  bh_paths_push_line(BhPathBuf *b, uint64_t hit, uint32_t ref_off, uint32_t header, int uniq);
/* every traced group -- its distinct records idx[0 .. n_records) (ascending) with their requests, first columns and ops, and the notes of
 * the lines printed from them -- also goes to fn (NULL: to nobody); columns = 0: the lines are written as they are rendered, without the
 * two columns.  bh_paths_set_pile (bh_pile.c): the collector is a variants object (--variants, with or without --cigar) */
typedef int (*bh_paths_collect_fn)(void *ctx, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t n_records,
                                   const BhPathBuf *bufs, uint64_t n_chunks);
void bh_paths_set_collector(BhPaths *paths, bh_paths_collect_fn fn, void *ctx, int columns);
/* BhPaths keeps a short list of collectors (at most BH_PATHS_MAX_COLLECTORS), called in the order they were added; nothing is traced
 * twice.  bh_paths_set_collector above sets or (fn = NULL) clears the one entry of the first kind.  bh_paths_add_collector adds an entry
 * of the second kind, which also gets the rendered text of the group's chunks (text[c], text_len[c]: whole lines, one per note of
 * bufs[c], without the two path columns): an entry with the same fn is replaced, ctx = NULL removes it; columns as above.  BH_E_USAGE
 * when the list is full. */
#define BH_PATHS_MAX_COLLECTORS 4
typedef int (*bh_paths_collect_text_fn)(void *ctx, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t n_records,
                                        const BhPathBuf *bufs, char *const *text, const size_t *text_len, uint64_t n_chunks);
int  bh_paths_add_collector(BhPaths *paths, bh_paths_collect_text_fn fn, void *ctx, int columns);
struct BhPile;
void bh_paths_set_pile(BhPaths *paths, struct BhPile *pile, int columns);
int  bh_paths_emit(BhPaths *paths, FILE *out, const BhQueries *q, const BhipHit *hits, char *const *text, const size_t *text_len, const BhPathBuf *bufs, uint64_t n_chunks);
size_t bh_cigar_text(const uint32_t *ops, uint64_t n, char *out, size_t cap);
int  bh_report_view_paths(FILE *out, const BhDb *db, const BhQueries *q, const BhRunView *view, BhMode mode, int flags, const BhTaxOpts *tx, uint64_t *nLines,
                          BhPlaceSink *sink, BhPaths *paths);

/* ---- paired-end reads: two mates' printed lines joined into concordant combinations (bh_mates.c; burst_hip --mates) ----
 * The definition is bhip_mates_join's (include/burst_hip.h) over the lines two single-end runs print; a reported combination is written as
 * mate 1's line and mate 2's line, each followed by two tab-separated columns: the fragment's 1-based leftmost position and its length.
 *   bh_mates_open        the joiner is bhip_mates_join on `hip_handle` (may be NULL until bh_mates_set_handle names it)
 *   bh_mates_set_join    another joiner (tests): same arguments and return codes in this file's terms, BH_E_CAPACITY = *n_out combinations
 *                        wanted (the call is repeated once with that room); fn = NULL: the device again
 *   bh_mates_names       the read names of mate file `side` (0, then 1) as column 1 prints them: a new pair of files starts with side 0
 *   bh_mates_join_files  the two single-end outputs (paths of their texts) -> the paired output on `out`; *n_lines = lines written
 *   bh_mates_stats       the figures of the last pair of files; bh_mates_print_info: the `Mates:` line on standard output */
typedef struct BhMates BhMates;
typedef struct BhMatesOpts { uint32_t orientation, ins_min, ins_max, report; } BhMatesOpts;      /* BHIP_MATES_FR / RF / FF, bounds of the fragment length, BHIP_MATES_ALL / BEST */
typedef struct BhMatesStats {
	uint64_t reads1, reads2;              /* reads in each file */
	uint64_t pairsNamed, pairsPlaced;     /* pair names in both files; of those, with a line on both sides */
	uint64_t lines1, lines2;              /* lines of the two single-end outputs */
	uint64_t examined, written;           /* combinations with equal pair and header; combinations reported (two lines each) */
	double deviceMs;                      /* device time of the join (0 with another joiner) */
} BhMatesStats;
typedef int (*bh_mates_join_fn)(void *ctx, const BhipMateLine *a, uint64_t na, const BhipMateLine *b, uint64_t nb, uint32_t orientation, uint32_t ins_min,
                                uint32_t ins_max, uint32_t report, uint32_t *out_a, uint32_t *out_b, uint64_t cap, uint64_t *n_out);
int  bh_mates_open(void *hip_handle, BhMates **mates);
void bh_mates_set_handle(BhMates *mates, void *hip_handle);
void bh_mates_set_join(BhMates *mates, bh_mates_join_fn fn, void *ctx);
int  bh_mates_names(BhMates *mates, int side, char *const *heads, uint64_t n);
int  bh_mates_join_files(BhMates *mates, const char *lines1, const char *lines2, FILE *out, const BhMatesOpts *o, uint64_t *n_lines);
void bh_mates_stats(const BhMates *mates, BhMatesStats *st);
void bh_mates_print_info(const BhMates *mates);
void bh_mates_close(BhMates *mates);

/* ---- coverage and count tables per reference header and sample (bh_cov.c; burst_hip --coverage) ----
 * What embalmlets/bcov.c and embalmulate.c compute from the .b6 text, from the report's own placements: PREFIXshared.txt, PREFIXunique.txt,
 * PREFIXshared_binary.txt, PREFIXunique_binary.txt (bcov's names and format) and PREFIXcounts.txt.  The statistics are the device's
 * (bhip_cov_*, exact 64-bit integers); the tables are written from them in double, to temporary names first and renamed together, so
 * that a failed run leaves no partial tables.
 *   bh_cov_open     lengths_file: bcov's table `name<TAB>length` per line (BH_E_USAGE naming the first header of the database it lacks),
 *                   or NULL: the database's own extent of every header (bh_cov_lengths_from_extents over bhip_lane_extents)
 *   bh_cov_sample   the next sample (column): its placements go to the device behind `hip_handle` (the same handle every time)
 *   bh_cov_sample_failed  the next column stays all zero (a sample that failed alone); named on standard output
 *   bh_cov_stats    columns x headers x {tot, cov, sq, lines}, column 0 = Dataset; either pointer may be NULL
 *   bh_cov_write    fetches the statistics and writes the five tables
 * Any device error is final: later calls return it and nothing is written. */
typedef struct BhCov BhCov;
typedef int (*bh_cov_tap_fn)(void *ctx, uint32_t sample, const BhipCovLine *lines, uint64_t n);
int  bh_cov_open(const BhDb *db, const char *prefix, const char *lengths_file, uint32_t pad, BhCov **cov);
/* test / diagnostic hook: called with every sample's placements before they go to the device; a return of 1 keeps them from it */
void bh_cov_set_tap(BhCov *cov, bh_cov_tap_fn fn, void *ctx);
int  bh_cov_sample(BhCov *cov, void *hip_handle, const char *out_path, const BhipCovLine *lines, uint64_t n);
int  bh_cov_sample_failed(BhCov *cov, const char *out_path);
void bh_cov_abort(BhCov *cov);                  /* the run ends on an error: nothing will be written */
void bh_cov_dims(const BhCov *cov, uint32_t *n_columns, uint32_t *n_headers);
const uint32_t *bh_cov_lengths(const BhCov *cov);      /* [n_headers]; NULL before the first sample of a run without a lengths file */
int  bh_cov_stats(BhCov *cov, uint64_t *shared, uint64_t *unique);
int  bh_cov_write(BhCov *cov);
void bh_cov_print_info(BhCov *cov);             /* one line on standard output: device time of the columns, peak of the event buffer, compactions */
void bh_cov_close(BhCov *cov);
/* extents[16 * clump + lane] -> length of every header: the largest refStart + extent of the lane over the header's fragments */
int  bh_cov_lengths_from_extents(const BhDb *db, const uint32_t *extents, uint32_t *lengths);
/* the lane extents from the packed references in host memory (where no one device holds the whole database) */
void bh_cov_extents_host(const BhDb *db, uint32_t *extents);
int  bh_cov_lengths_host(BhCov *cov);           /* no lengths table: take them from bh_cov_extents_host now */
/* the two sources of the lengths on their own (--sam-lengths takes them too): the table `name<TAB>length` looked up for heads[0 .. n_headers)
 * (`flag` names the option in the error texts), and the database's own extents from `hip_handle`'s lanes (NULL: from host memory) */
int  bh_cov_read_lengths(const char *file, const char *flag, uint32_t n_headers, const char *const *heads, uint32_t *lengths);
int  bh_cov_default_lengths(const BhDb *db, void *hip_handle, uint32_t *lengths);
/* the writer alone: stats = [n_columns][n_headers][4] (tot, cov, sq, lines), column 0 = Dataset, col_names[1 .. n_columns) the samples */
int  bh_cov_write_tables(const char *prefix, uint32_t n_headers, const char *const *headers, const uint32_t *lengths, uint32_t n_columns,
                         const char *const *col_names, const uint64_t *shared, const uint64_t *unique);

/* ---- abundance tables: the reads of multi-mapped lines split over their references (bh_em.c; burst_hip --abundance) ----
 * The definition is bhip_em_run's (include/burst_hip.h): per sample, group = a unique query of the report's sink (its number in sink->uq),
 * W = the reads of that query, candidates = the distinct headers of its entries.  PREFIXabundance.txt: `#OTU ID<TAB>Dataset[<TAB>sample...]`,
 * one row per header whose Dataset value is not zero, in strcmp order of the header, cells %.4f of count / 2^30; Dataset = the integer sum
 * of the sample columns (a pooled EM over the study is out of scope).  Written under a temporary name and renamed.
 *   bh_em_open           the headers are the database's unique-header numbers (RefMap), as the coverage's; bh_em_open_heads: any headers
 *   bh_em_sample         the next sample (column): reads[k] = the unique query number of placement lines[k]; solved on `hip_handle`
 *   bh_em_sample_failed  the next column stays all zero (a sample that failed alone); named on standard output
 *   bh_em_abort          the run ends on an error: nothing will be written
 *   bh_em_stats          columns x headers counts in units of 2^-30 read, column 0 = Dataset
 *   bh_em_print_info     the `Abundance:` line of the last sample on standard output; bh_em_last_info: the same figures (bhip_em_run's info)
 *   bh_em_set_solver     another solver (tests): bhip_em_run's arguments behind ctx, return codes in this file's terms; fn = NULL: the device
 *   bh_em_host           the definition in plain C, a solver (its first argument is ignored): the tests without a device, the yardstick
 * Any error of the solver is final: later calls return it and nothing is written. */
typedef struct BhEm BhEm;
typedef int (*bh_em_solver_fn)(void *ctx, uint32_t n_headers, uint32_t n_groups, const uint32_t *group_w, const BhipEmLine *lines, uint64_t n_lines,
                               uint32_t max_iters, uint64_t tol, uint64_t *counts, uint64_t info[8]);
int  bh_em_open(const BhDb *db, const char *prefix, uint32_t max_iters, uint64_t tol, BhEm **em);
int  bh_em_open_heads(const char *prefix, uint32_t n_headers, const char *const *heads, uint32_t max_iters, uint64_t tol, BhEm **em);
void bh_em_set_solver(BhEm *em, bh_em_solver_fn fn, void *ctx);
int  bh_em_sample(BhEm *em, void *hip_handle, const char *out_path, const uint32_t *reads, const BhipCovLine *lines, uint64_t n);
int  bh_em_sample_failed(BhEm *em, const char *out_path);
void bh_em_abort(BhEm *em);
void bh_em_dims(const BhEm *em, uint32_t *n_columns, uint32_t *n_headers);
int  bh_em_stats(BhEm *em, uint64_t *columns);
int  bh_em_write(BhEm *em);
void bh_em_print_info(BhEm *em);
void bh_em_last_info(const BhEm *em, uint64_t info[8], uint64_t *reads);
void bh_em_close(BhEm *em);
int  bh_em_host(void *unused, uint32_t n_headers, uint32_t n_groups, const uint32_t *group_w, const BhipEmLine *lines, uint64_t n_lines, uint32_t max_iters,
                uint64_t tol, uint64_t *counts, uint64_t info[8]);
const uint64_t *bh_em_last_column(const BhEm *em);      /* the counts [n_headers] of the last sample, NULL when it failed or none came (bh_taxa.c rolls them up) */

/* ---- taxon tables per sample: a read goes to the lowest common ancestor of its references' taxonomies (bh_taxa.c; burst_hip --taxa) ----
 * The definition is bhip_taxa_run's (include/burst_hip.h).  The taxonomy of a header is what bh_tax_lookup returns for it (the
 * string of column 13; ncbi as -bn), without trailing ';'; empty or exactly `Unassigned` is no taxonomy.  It splits at every ';' into levels,
 * bytes kept as they are (a leading blank stays, an empty inner level is a level); more than 64 levels is BH_E_USAGE that names the header.
 * The distinct level prefixes are the nodes, node 0 the root (depth 0, printed `Unassigned`), a node's name the string up to the end of its
 * last level; numbered in preorder (a subtree is a range of numbers), siblings in byte order with ';' below every other byte -- an order no
 * result depends on.  A header without taxonomy is at the root.  Groups, weights and candidates are the abundance's (bh_em.c).
 * Files, written under temporary names and renamed together, rows in strcmp order of the name, `#OTU ID<TAB>Dataset[<TAB>sample...]`,
 * Dataset = the integer sum of the sample columns, a failed sample an all-zero column:
 *   PREFIXtaxa.txt                  own counts, the nodes with a Dataset value other than zero (the root as `Unassigned`), integers
 *   PREFIXtaxa_L<k>.txt             k = 1 .. D, D the deepest level with a clade count: the nodes of depth k, clade counts, integers
 *   PREFIXtaxa_abundance_L<k>.txt   with an abundance beside it: the same rows, k = 1 .. D, from clade_em, %.4f of count / 2^30
 *   bh_taxa_tree          nodes, names, parents, depths and header -> node from headers and the map; bh_taxa_tree_free
 *   bh_taxa_open          the headers are the database's unique-header numbers (RefMap), as the abundance's; bh_taxa_open_heads: any headers
 *   bh_taxa_sample        the next sample (column), reduced on `hip_handle`; em_counts: NULL, or the sample's abundance counts per header
 *   bh_taxa_sample_failed the next column stays all zero; named on standard output
 *   bh_taxa_abort         the run ends on an error: nothing will be written
 *   bh_taxa_stats         [4][columns][nodes]: own, clade, own_em, clade_em; column 0 = Dataset
 *   bh_taxa_write         the files; n_levels / n_em_levels: how many level files of either kind
 *   bh_taxa_print_info    the `Taxa:` line of the last sample; bh_taxa_last_info: the same figures (bhip_taxa_run's info)
 *   bh_taxa_set_solver    other solvers (tests) for bhip_taxa_run and bhip_taxa_rollup, return codes in this file's terms; NULL: the device
 *   bh_taxa_host, bh_taxa_rollup_host   the definition in plain C (candidates counted below every ancestor), solvers whose first argument is ignored
 *   bh_taxa_check_opts    BH_E_USAGE with the command line's text: no map, or an agreement outside 501 .. 1000
 * Any error of a solver is final: later calls return it and nothing is written. */
typedef struct BhTaxa BhTaxa;
typedef struct BhTaxaTree { uint32_t n_nodes, n_headers; uint32_t *parent, *depth, *header_node; char **name; } BhTaxaTree;
typedef int (*bh_taxa_run_fn)(void *ctx, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, uint32_t n_groups,
                              const uint32_t *group_w, const BhipEmLine *lines, uint64_t n_lines, uint32_t agree, uint32_t *group_node, uint64_t *own, uint64_t *clade,
                              uint64_t info[8]);
typedef int (*bh_taxa_rollup_fn)(void *ctx, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, const uint64_t *header_count,
                                 uint64_t *own, uint64_t *clade);
int  bh_taxa_tree(uint32_t n_headers, const char *const *heads, const BhTax *map, int ncbi, BhTaxaTree *tree);
void bh_taxa_tree_free(BhTaxaTree *tree);
int  bh_taxa_check_opts(const char *tax_file, int agree_given, long long agree);
int  bh_taxa_open(const BhDb *db, const char *prefix, const BhTax *map, int ncbi, uint32_t agree, BhTaxa **tx);
int  bh_taxa_open_heads(const char *prefix, uint32_t n_headers, const char *const *heads, const BhTax *map, int ncbi, uint32_t agree, BhTaxa **tx);
void bh_taxa_set_solver(BhTaxa *tx, bh_taxa_run_fn run, bh_taxa_rollup_fn rollup, void *ctx);
int  bh_taxa_sample(BhTaxa *tx, void *hip_handle, const char *out_path, const uint32_t *reads, const BhipCovLine *lines, uint64_t n, const uint64_t *em_counts);
int  bh_taxa_sample_failed(BhTaxa *tx, const char *out_path);
void bh_taxa_abort(BhTaxa *tx);
const BhTaxaTree *bh_taxa_tree_of(const BhTaxa *tx);
void bh_taxa_dims(const BhTaxa *tx, uint32_t *n_columns, uint32_t *n_nodes);
int  bh_taxa_stats(BhTaxa *tx, uint64_t *columns);
int  bh_taxa_write(BhTaxa *tx, uint32_t *n_levels, uint32_t *n_em_levels);
void bh_taxa_print_info(BhTaxa *tx);
void bh_taxa_last_info(const BhTaxa *tx, uint64_t info[8]);
void bh_taxa_close(BhTaxa *tx);
int  bh_taxa_host(void *unused, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, uint32_t n_groups, const uint32_t *group_w,
                  const BhipEmLine *lines, uint64_t n_lines, uint32_t agree, uint32_t *group_node, uint64_t *own, uint64_t *clade, uint64_t info[8]);
int  bh_taxa_rollup_host(void *unused, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, const uint64_t *header_count,
                         uint64_t *own, uint64_t *clade);

/* ---- variant sites per sample from the alignment paths (bh_pile.c; burst_hip --variants) ----
 * The definition is bhip_pile_run's (include/burst_hip.h): per sample, every printed line is a line of the pile-up -- its record's path
 * (the tracer of the --cigar columns, traced once), the header of column 2, the position the --cigar column prints, weight = the reads it
 * stands for; with unique_only only the lines whose read is on exactly one line of the sample (the sink's bit 31).  PREFIXvariants.txt:
 * `#Reference<TAB>Position<TAB>Ref<TAB>Sample<TAB>Depth<TAB>A<TAB>C<TAB>G<TAB>T<TAB>Del<TAB>Other<TAB>Ins`, then one block per sample in
 * study order, rows in strcmp order of the header, then ascending position.  Written under a temporary name (opened by bh_pile_open,
 * a block appended per sample) and renamed by bh_pile_write; bh_pile_close removes a temporary file that was not renamed.  No Dataset
 * block: a pooled call over the samples is out of scope.
 *   bh_pile_open           the headers are the database's unique-header numbers (RefMap); bh_pile_open_heads: any headers
 *   bh_pile_collect        bh_paths_emit's hand-over of a traced group (records, paths, the notes of the printed lines)
 *   bh_pile_sample         the end of a sample: ONE solver call over its lines, its block appended; q_codes / q_off: the sample's entries
 *   bh_pile_sample_failed  the sample has no rows (it failed alone); named on standard output
 *   bh_pile_abort          the run ends on an error: nothing will be written
 *   bh_pile_rows           the rows so far (headers as unique-header numbers) and the sample of each; returns their number
 *   bh_pile_print_info     the `Variants:` line of the last sample on standard output; bh_pile_last_info: the same figures
 *   bh_pile_set_solver     another solver (tests): bhip_pile_run's arguments behind ctx, return codes in this file's terms
 *                          (BH_E_CAPACITY = *n_sites wanted); fn = NULL: the device
 *   bh_pile_host           the definition in plain C, a solver: ctx = a BhPileRefs (the packed references as bhip_init takes them); one record
 *                          per observed base, so its cost is lines x read length -- the tests without a device, the yardstick
 * Any error of the solver is final: later calls return it and nothing is written. */
typedef struct BhPile BhPile;
typedef struct BhPileRefs { const uint8_t *packed; const uint32_t *clump_len; uint32_t n_clumps, tot_refs; } BhPileRefs;
typedef int (*bh_pile_solver_fn)(void *ctx, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                                 const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, uint32_t min_alt, BhipPileSite *sites, uint64_t cap, uint64_t *n_sites, uint64_t info[8]);
int  bh_pile_open(const BhDb *db, const char *prefix, uint32_t min_depth, uint32_t min_alt, int unique_only, BhPile **pile);
int  bh_pile_open_heads(const char *prefix, uint32_t n_headers, const char *const *heads, uint32_t min_depth, uint32_t min_alt, int unique_only, BhPile **pile);
void bh_pile_set_solver(BhPile *pile, bh_pile_solver_fn fn, void *ctx);
int  bh_pile_collect(BhPile *pile, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t n_records,
                     const BhPathBuf *bufs, uint64_t n_chunks);
int  bh_pile_sample(BhPile *pile, void *hip_handle, const char *out_path, const uint8_t *q_codes, const uint64_t *q_off, uint64_t n_queries);
int  bh_pile_sample_failed(BhPile *pile, const char *out_path);
void bh_pile_abort(BhPile *pile);
uint64_t bh_pile_rows(const BhPile *pile, BhipPileSite *rows, uint32_t *samples, uint64_t cap);
int  bh_pile_write(BhPile *pile);
void bh_pile_print_info(BhPile *pile);
void bh_pile_last_info(const BhPile *pile, uint64_t info[8], uint64_t *lines);
void bh_pile_close(BhPile *pile);
/* what bh_vcf.c shares: the base name of an output without its last extension; a collector alone (no table, no file: bh_pile_collect fills
 * it, the lines keep the header numbers they come with; bh_pile_lines returns their number and the arrays, bh_pile_drop_lines empties it);
 * the checks of a solver's lines in plain C (`who` opens the texts; *n_obs: an upper bound of the records one walk writes) */
char *bh_pile_sample_name(const char *path);
int  bh_pile_open_lines(uint32_t n_headers, int unique_only, BhPile **pile);
uint64_t bh_pile_lines(const BhPile *pile, const BhipPileLine **lines, const uint32_t **ops, uint64_t *n_ops, uint64_t *n_printed);
void bh_pile_drop_lines(BhPile *pile);
int  bh_pile_check_lines(const char *who, const BhPileRefs *refs, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                         const uint32_t *ops, uint64_t n_ops, uint64_t *n_obs);
int  bh_pile_host(void *refs, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                  const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, uint32_t min_alt, BhipPileSite *sites, uint64_t cap, uint64_t *n_sites, uint64_t info[8]);

/* ---- consensus sequences per reference and sample from the alignment paths (bh_consensus.c; burst_hip --consensus) ----
 * The definition is bhip_consensus_run's (include/burst_hip.h): per sample, every printed line is a line of the pile-up, as for the variant
 * sites; every covered position gets a letter, and the segments of a header become one record in REFERENCE coordinates -- the header's
 * length L letters, N outside the segments, '-' for a deletion -- so that the records of one reference from all samples are the rows of
 * one alignment.  L: the table of --consensus-lengths (format and errors of --coverage-lengths) or the database's own extents; a segment
 * that ends beyond L is BH_E_USAGE that names the header.  Two files, written under temporary names (opened by bh_consensus_open, a block
 * per sample in study order, headers in strcmp order) and renamed together by bh_consensus_write; bh_consensus_close removes temporary
 * files that were not renamed:
 *   PREFIXconsensus.fa    `>SAMPLE|HEADER` and L letters, for every (sample, header) with Called >= 1 and 1000 * Called >= min_breadth * L
 *   PREFIXconsensus.txt   #Reference Sample Length Covered Called Same Subst Del Ambig InsMajor Record, a row per (sample, header) with Covered >= 1
 *   bh_consensus_open          the headers are the database's unique-header numbers (RefMap); bh_consensus_open_heads: any headers and lengths
 *   bh_consensus_collect       the tracer's hand-over of a traced group; bh_paths_set_consensus registers it beside the other collectors
 *   bh_consensus_sample        the end of a sample: ONE solver call over its lines (the room grows once), its block appended to both files
 *   bh_consensus_sample_failed the sample has no rows (it failed alone); named on standard output
 *   bh_consensus_abort         the run ends on an error: nothing will be written
 *   bh_consensus_rows          the rows of the table so far (headers as unique-header numbers); returns their number
 *   bh_consensus_print_info    the `Consensus:` line of the last sample on standard output; bh_consensus_last_info: the same figures
 *   bh_consensus_set_solver    another solver (tests): bhip_consensus_run's arguments behind ctx, return codes in this file's terms
 *   bh_consensus_host          the definition in plain C, a solver: ctx = a BhPileRefs; one record per observed base, sorted and counted */
typedef struct BhCons BhCons;
typedef struct BhConsRow { uint32_t header, sample, length, covered, called, same, subst, del, ambig, ins_major, record, pad; } BhConsRow;
typedef int (*bh_cons_solver_fn)(void *ctx, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                                 const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, BhipConsSeg *segs, uint64_t seg_cap, uint64_t *n_segs,
                                 char *letters, uint64_t letter_cap, uint64_t *n_letters, uint64_t info[8]);
int  bh_consensus_check_opts(uint32_t min_depth, uint32_t min_breadth);      /* BH_E_USAGE with the command line's text for a value outside its range */
int  bh_consensus_open(const BhDb *db, const char *prefix, const char *lengths_file, uint32_t min_depth, uint32_t min_breadth, int unique_only, BhCons **cons);
int  bh_consensus_open_heads(const char *prefix, uint32_t n_headers, const char *const *heads, const uint32_t *lengths, uint32_t min_depth, uint32_t min_breadth,
                             int unique_only, BhCons **cons);
void bh_consensus_set_solver(BhCons *cons, bh_cons_solver_fn fn, void *ctx);
int  bh_consensus_collect(BhCons *cons, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t n_records,
                          const BhPathBuf *bufs, uint64_t n_chunks);
int  bh_paths_set_consensus(BhPaths *paths, BhCons *cons, int columns);      /* BH_E_USAGE: the tracer's list of collectors is full */
int  bh_consensus_sample(BhCons *cons, void *hip_handle, const char *out_path, const uint8_t *q_codes, const uint64_t *q_off, uint64_t n_queries);
int  bh_consensus_sample_failed(BhCons *cons, const char *out_path);
void bh_consensus_abort(BhCons *cons);
uint64_t bh_consensus_rows(const BhCons *cons, BhConsRow *rows, uint64_t cap);
int  bh_consensus_write(BhCons *cons);
void bh_consensus_print_info(BhCons *cons);
void bh_consensus_last_info(const BhCons *cons, uint64_t info[8], uint64_t *lines, uint64_t *records);
void bh_consensus_close(BhCons *cons);
int  bh_consensus_host(void *refs, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                       const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, BhipConsSeg *segs, uint64_t seg_cap, uint64_t *n_segs,
                       char *letters, uint64_t letter_cap, uint64_t *n_letters, uint64_t info[8]);

/* ---- sample-to-sample identity of the consensus rows per reference (bh_conspairs.c; burst_hip --consensus PREFIX --consensus-pairs) ----
 * The definition is include/burst_hip.h "Consensus pairs" (DESIGN.md section 7l), a pure function of the written PREFIXconsensus.fa.  With a
 * collector attached (bh_conspairs_attach) bh_consensus_sample hands over the segments and letters of every (sample, header) whose record
 * it writes; the collector keeps them in host memory (24 bytes per segment, a byte per covered position; no spilling).  At the end of the
 * run bh_consensus_pairs makes ONE solver call on the reporting rank's handle and writes PREFIXconsensus_pairs.txt, _identity.txt and
 * _compared.txt under temporary names; bh_consensus_write, which refuses to run before it, renames all five files together.  A sample that
 * failed alone reads NA in its whole row and column of both matrices.  Two samples of one name are BH_E_USAGE that names both outputs
 * (bh_conspairs_check_names: the command line asks before a device is touched; names sorted, neighbours compared).  A record covered
 * through position 2^32 - 1 is BH_E_USAGE when it is handed over (the primitive's keys end one position earlier).  The matrices are
 * summed from the pair list (a sorted list of the cells that have a pair row), never as samples^2 sums.  Any error is final: no file is written, and
 * bh_conspairs_close removes the temporary files.
 *   bh_conspairs_check_min    BH_E_USAGE with the command line's text for --consensus-pairs-min outside 1 .. 2^31 - 1
 *   bh_conspairs_set_solver   another solver (tests): bhip_consensus_pairs' arguments behind ctx, return codes in this file's terms; NULL: the device
 *   bh_conspairs_print_info   the `ConsensusPairs:` line; bh_conspairs_last_info: [0] samples done [1] failed [2] participating records [3] headers
 *                             with two or more [4] union positions [5] pairs examined [6] pairs written [7] host bytes kept; the device microseconds
 *   bh_consensus_pairs_host   the primitive in plain sequential C, a solver (ctx unused): a dense row per (sample, header), a double loop over the samples
 * bh_consensus.c reaches the collector through BhConsPairsHooks alone, so that it links without this file. */
typedef struct BhConsPairs BhConsPairs;
typedef int (*bh_conspairs_solver_fn)(void *ctx, uint32_t n_samples, const BhipPairSeg *segs, uint64_t n_segs, const char *letters, uint64_t n_letters, uint32_t min_compared,
                                      BhipPair *pairs, uint64_t pair_cap, uint64_t *n_pairs, uint64_t info[8]);
typedef struct BhConsPairsHooks {
	int  (*add)(BhConsPairs *pairs, uint32_t sample, uint32_t header, const BhipConsSeg *segs, uint64_t n, const char *letters);
	int  (*write)(BhConsPairs *pairs, void *hip_handle, uint32_t n_samples, char *const *names, const uint8_t *failed, char *const *head, const uint32_t *by_rank,
	              const uint32_t *length, uint32_t n_headers);
	int  (*written)(const BhConsPairs *pairs);
	int  (*commit)(BhConsPairs *pairs);
	void (*abort)(BhConsPairs *pairs);
} BhConsPairsHooks;
int  bh_conspairs_check_min(uint64_t min_compared);
int  bh_conspairs_check_names(const char *const *out_paths, uint64_t n);
int  bh_conspairs_open(const char *prefix, uint32_t min_compared, BhConsPairs **pairs);
void bh_conspairs_set_solver(BhConsPairs *pairs, bh_conspairs_solver_fn fn, void *ctx);
void bh_conspairs_attach(BhConsPairs *pairs, BhCons *cons);
int  bh_conspairs_add(BhConsPairs *pairs, uint32_t sample, uint32_t header, const BhipConsSeg *segs, uint64_t n, const char *letters);
int  bh_conspairs_write(BhConsPairs *pairs, void *hip_handle, uint32_t n_samples, char *const *names, const uint8_t *failed, char *const *head, const uint32_t *by_rank,
                        const uint32_t *length, uint32_t n_headers);
int  bh_conspairs_written(const BhConsPairs *pairs);
int  bh_conspairs_commit(BhConsPairs *pairs);
void bh_conspairs_abort(BhConsPairs *pairs);
void bh_conspairs_print_info(BhConsPairs *pairs);
void bh_conspairs_last_info(const BhConsPairs *pairs, uint64_t info[8], uint64_t *device_us);
void bh_conspairs_close(BhConsPairs *pairs);
int  bh_consensus_pairs_host(void *unused, uint32_t n_samples, const BhipPairSeg *segs, uint64_t n_segs, const char *letters, uint64_t n_letters, uint32_t min_compared,
                             BhipPair *pairs, uint64_t pair_cap, uint64_t *n_pairs, uint64_t info[8]);
/* bh_consensus.c's side: the collector and its entry points (NULL: none; the caller opens and closes it); the end of the run, before
 * bh_consensus_write */
void bh_consensus_set_pairs(BhCons *cons, BhConsPairs *pairs, const BhConsPairsHooks *hooks);
int  bh_consensus_pairs(BhCons *cons, void *hip_handle);

/* ---- VCF output beside the .b6: SNVs and indel alleles per sample from the alignment paths (bh_vcf.c; burst_hip --vcf) ----
 * The alleles are bhip_alleles_run's (include/burst_hip.h "Indel alleles"), the SNVs a subset of bhip_pile_run's sites.  Per sample the
 * lines the tracer handed over (bh_pile.c's collector: the same lines, the same unique-read rule) go through ONE bhip_pile_run and ONE
 * bhip_alleles_run on the reporting rank's handle, and the two ordered lists are merged into the records of OUT.vcf, written under a
 * temporary name and renamed when the sample has succeeded; a sample that failed and a run that ended on an error leave none.  The file
 * holds no date and no command line.  Header lines: fileformat, source, a contig line per header in header-number order (SN and LN as
 * --sam's @SQ: bh_sam_names; LN from the table of --vcf-lengths or the database's own extents), INFO DP, FORMAT DP and AD, the column
 * line with the sample's name (bh_pile_sample_name).  Records in header-number order, then by POS; at one POS the SNV record first, then
 * the alleles in their order.  Letters: A C G T for the codes 1 .. 4, N for every other code.  ID, QUAL, FILTER `.`, INFO DP=Depth, FORMAT
 * DP:AD, no GT.
 *   SNV   a site whose Ref is A/C/G/T with Depth >= min_depth and a base b != Ref of A, C, G, T with n[b] >= min_alt: ALT those bases in the
 *         order A, C, G, T; sample field Depth:n[Ref],n[alt1],...
 *   Del   POS the anchor, REF the anchor's letter and the n deleted letters, ALT the anchor's letter; Depth:Depth-count,count
 *   Ins   POS the anchor, REF the anchor's letter, ALT the anchor's letter and the inserted letters; Depth:Depth-count,count
 *         (for both, AD's first number is the observing reads that do not carry this allele)
 *   bh_vcf_open          the headers are the database's unique-header numbers; two headers of one SN are BH_E_USAGE that names both
 *   bh_vcf_open_heads    any headers, with their lengths
 *   bh_vcf_set_solver    other solvers (tests): bhip_pile_run's and bhip_alleles_run's arguments behind a ctx each, return codes in this
 *                        file's terms (BH_E_CAPACITY = the numbers wanted); NULL: the device
 *   bh_vcf_sample        the end of a sample: the two calls (the room grows once), OUT.vcf; bh_vcf_sample_failed: its lines are dropped
 *   bh_vcf_print_info    the `Vcf:` line of the last sample; bh_vcf_last_info: [0] lines [1] allele events [2] distinct alleles [3] returned
 *                        alleles [4] SNV [5] Del [6] Ins records [7] END [8] ADJACENT [9] LONG skipped runs [10] device microseconds of both
 *                        calls [11] peak device bytes
 *   bh_alleles_host      the definition in plain sequential C, a solver: ctx = a BhPileRefs; one record per allele run, sorted and counted */
typedef struct BhVcf BhVcf;
typedef int (*bh_alleles_solver_fn)(void *ctx, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                                    const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, uint32_t min_alt, BhipAllele *alleles, uint64_t cap, uint64_t *n_alleles,
                                    uint8_t *codes, uint64_t code_cap, uint64_t *n_codes, uint64_t info[8]);
int  bh_sam_names(const char *flag, uint32_t n_headers, const char *const *heads, char ***sn);      /* (bh_sam.c) SN per header; a clash is BH_E_USAGE that opens with `flag` */
void bh_sam_names_free(char **sn, uint32_t n_headers);
int  bh_vcf_check_opts(uint32_t min_depth, uint32_t min_alt);      /* BH_E_USAGE with the command line's text for a value outside its range */
int  bh_vcf_open(const BhDb *db, const char *lengths_file, uint32_t min_depth, uint32_t min_alt, int unique_only, BhVcf **vcf);
int  bh_vcf_open_heads(uint32_t n_headers, const char *const *heads, const uint32_t *lengths, uint32_t min_depth, uint32_t min_alt, int unique_only, BhVcf **vcf);
void bh_vcf_set_solver(BhVcf *vcf, bh_pile_solver_fn pile_fn, void *pile_ctx, bh_alleles_solver_fn alleles_fn, void *alleles_ctx);
int  bh_vcf_collect(BhVcf *vcf, const uint64_t *idx, const BhipPathReq *req, const uint32_t *first, const uint64_t *off, const uint32_t *ops, uint64_t n_records,
                    const BhPathBuf *bufs, uint64_t n_chunks);
int  bh_paths_set_vcf(BhPaths *paths, BhVcf *vcf, int columns);      /* BH_E_USAGE: the tracer's list of collectors is full */
int  bh_vcf_sample(BhVcf *vcf, void *hip_handle, const char *out_path, const uint8_t *q_codes, const uint64_t *q_off, uint64_t n_queries);
void bh_vcf_sample_failed(BhVcf *vcf);
void bh_vcf_abort(BhVcf *vcf);
void bh_vcf_print_info(BhVcf *vcf);
void bh_vcf_last_info(const BhVcf *vcf, uint64_t info[12]);
void bh_vcf_close(BhVcf *vcf);
int  bh_alleles_host(void *refs, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPileLine *lines, uint64_t n_lines,
                     const uint32_t *ops, uint64_t n_ops, uint32_t min_depth, uint32_t min_alt, BhipAllele *alleles, uint64_t cap, uint64_t *n_alleles,
                     uint8_t *codes, uint64_t code_cap, uint64_t *n_codes, uint64_t info[8]);

/* ---- the study VCF: every sample's counts at every record any sample reports (bh_vcfstudy.c; burst_hip --vcf --vcf-study PREFIX) ----
 * The definition is include/burst_hip.h "Site counts" (DESIGN.md section 7k).  With a study attached (bh_vcf_set_study) bh_vcf_sample asks
 * its two solvers at thresholds (1, 1), applies --vcf-min-depth and --vcf-min-alt on the host -- OUT.vcf keeps its bytes -- and hands the
 * sample over (bh_vcfstudy_add): per sample the study keeps in host memory a range of 16 bytes per line, the (1, 1) sites and alleles and
 * the records the sample reports with the codes of its Dels; a failed sample keeps nothing.  bh_vcfstudy_write merges the reported records
 * in the order of OUT.vcf, makes ONE solver call per sample on the reporting rank's handle and writes PREFIXstudy.vcf under a temporary
 * name, renamed when it is whole: the header block of OUT.vcf by the same code (bh_vcf_write_header) with an NS line, a column per sample
 * in study order under the coverage tables' names (bh_pile_sample_name), INFO DP=<sum of the depths>;NS=<samples with depth >= 1>, FORMAT
 * DP:AD for every sample with no threshold applied, explicit zeros for a sample without a read there, `.` for a sample that failed alone.
 * Two samples of one name are BH_E_USAGE that names both (bh_vcfstudy_check_names: the command line asks before a device is touched).  A
 * list that comes back inconsistent (n[ref - 1] > depth, count > depth) is BH_E_INTERNAL.  Any error but a usage error is final: no file
 * is written and bh_vcfstudy_close removes the temporary file.
 *   bh_vcfstudy_set_solver   another solver (tests): bhip_site_counts' arguments behind ctx, return codes in this file's terms; NULL: the device
 *   bh_vcfstudy_print_info   the `VcfStudy:` line; bh_vcfstudy_last_info: [0] samples done [1] failed [2] SNV [3] Del [4] Ins records [5] cells
 *                            [6] host bytes kept [7] device microseconds
 *   bh_site_counts_host      the primitive in plain sequential C, a solver (ctx unused): a loop over all ranges per record */
typedef struct BhVcfStudy BhVcfStudy;
typedef int (*bh_sitecounts_solver_fn)(void *ctx, const BhipCountRange *ranges, uint64_t n_ranges, const BhipPileSite *sites, uint64_t n_sites, const BhipAllele *alleles, uint64_t n_alleles,
                                       const BhipCountRecord *records, uint64_t n_records, BhipCountCell *cells, uint64_t info[8]);
int  bh_vcfstudy_open(const char *prefix, BhVcfStudy **study);
void bh_vcfstudy_set_solver(BhVcfStudy *study, bh_sitecounts_solver_fn fn, void *ctx);
int  bh_vcfstudy_check_names(const char *const *out_paths, uint64_t n);
int  bh_vcfstudy_add(BhVcfStudy *study, const char *out_path, const BhipPileLine *lines, uint64_t n_lines, const uint32_t *ops, const BhipPileSite *sites, uint64_t n_sites,
                     const BhipAllele *alleles, uint64_t n_alleles, const uint8_t *codes, uint64_t n_codes, uint32_t min_depth, uint32_t min_alt);
int  bh_vcfstudy_sample_failed(BhVcfStudy *study, const char *out_path);
void bh_vcfstudy_abort(BhVcfStudy *study);
int  bh_vcfstudy_write(BhVcfStudy *study, BhVcf *vcf, void *hip_handle);
const char *bh_vcfstudy_path(const BhVcfStudy *study);
void bh_vcfstudy_print_info(BhVcfStudy *study);
void bh_vcfstudy_last_info(const BhVcfStudy *study, uint64_t info[8]);
void bh_vcfstudy_close(BhVcfStudy *study);
int  bh_site_counts_host(void *unused, const BhipCountRange *ranges, uint64_t n_ranges, const BhipPileSite *sites, uint64_t n_sites, const BhipAllele *alleles, uint64_t n_alleles,
                         const BhipCountRecord *records, uint64_t n_records, BhipCountCell *cells, uint64_t info[8]);
/* bh_vcf.c's side: the study every sample is handed to (NULL: none; the caller opens and closes it); a sample that failed before its
 * bh_vcf_sample gets its `.` column; what the study file shares with OUT.vcf */
void bh_vcf_set_study(BhVcf *vcf, BhVcfStudy *study);
int  bh_vcf_study_sample_failed(BhVcf *vcf, const char *out_path);
uint32_t bh_vcf_n_headers(const BhVcf *vcf);
const char *bh_vcf_contig(const BhVcf *vcf, uint32_t header);
int  bh_vcf_ensure_lengths(BhVcf *vcf, void *hip_handle);
void bh_vcf_write_header(const BhVcf *vcf, FILE *f, int study);

/* ---- greedy centroid clusters of the reads of a query file aligned against itself (bh_cluster.c; burst_hip --cluster) ----
 * The definition is bhip_cluster_run's (include/burst_hip.h): nodes = the reads in file order, named by column 1; weight 1, or with
 * use_sizes the N of a trailing `;size=N[;]`; an edge per printed line whose column 2 is the name of another read, its edits the smallest
 * column 11; a line whose column 2 names no read is foreign (counted), a self line is ignored.  PREFIXclusters.txt:
 * `#Read<TAB>Centroid<TAB>Role<TAB>Edits<TAB>Weight`, one row per read in file order, Role C or M; PREFIXcluster_sizes.txt:
 * `#OTU ID<TAB>Reads<TAB>Weight`, one row per centroid in priority order, Weight the 64-bit sum over its cluster.  Both are written under
 * temporary names and renamed together; neither is written when the run ends on an error.
 *   bh_cluster_names       the reads: resets the object; two byte-equal names are BH_E_USAGE with a text that names them
 *   bh_cluster_line        `count` printed lines of read q with this column 2 and column 11
 *   bh_cluster_add_b6      the lines of a .b6 file (columns 1, 2 and 11)
 *   bh_cluster_solve       one solver call over the edges collected, on `hip_handle`
 *   bh_cluster_sample      names + lines + solve for a finished run: the reads of Q, the lines of the report's sink (filled with want_re)
 *   bh_cluster_result      per read: its centroid's number, the edits that joined it, its weight (any may be NULL)
 *   bh_cluster_print_info  the `Clusters:` line on standard output; bh_cluster_last_info: the same figures (bhip_cluster_info's, lines, foreign lines)
 *   bh_cluster_set_solver  another solver (tests): bhip_cluster_run's arguments and bhip_cluster_info's array behind ctx, return codes in
 *                          this file's terms; fn = NULL: the device
 *   bh_cluster_host        the definition in plain sequential C, a solver (its first argument is ignored): the tests without a device, the yardstick
 * Any error is final: later calls return it and nothing is written. */
typedef struct BhCluster BhCluster;
typedef int (*bh_cluster_solver_fn)(void *ctx, uint32_t n_nodes, const uint32_t *weights, const BhipClusterEdge *edges, uint64_t n_edges, uint32_t *centroid,
                                    uint32_t *edits, uint64_t info[8]);
int  bh_cluster_open(const char *prefix, int use_sizes, BhCluster **cl);
void bh_cluster_set_solver(BhCluster *cl, bh_cluster_solver_fn fn, void *ctx);
int  bh_cluster_names(BhCluster *cl, const char *const *names, uint32_t n);
int  bh_cluster_line(BhCluster *cl, uint32_t q, const char *ref_name, size_t ref_len, uint32_t edits, uint64_t count);
int  bh_cluster_add_b6(BhCluster *cl, const char *path);
int  bh_cluster_solve(BhCluster *cl, void *hip_handle);
int  bh_cluster_sample(BhCluster *cl, void *hip_handle, const BhDb *db, const BhQueries *q, const BhPlaceSink *sink);
uint32_t bh_cluster_reads(const BhCluster *cl);
int  bh_cluster_result(const BhCluster *cl, uint32_t *centroid, uint32_t *edits, uint32_t *weights);
void bh_cluster_last_info(const BhCluster *cl, uint64_t info[8], uint64_t *lines, uint64_t *foreign);
int  bh_cluster_write(BhCluster *cl);
void bh_cluster_print_info(BhCluster *cl);
void bh_cluster_abort(BhCluster *cl);
void bh_cluster_close(BhCluster *cl);
int  bh_cluster_host(void *unused, uint32_t n_nodes, const uint32_t *weights, const BhipClusterEdge *edges, uint64_t n_edges, uint32_t *centroid, uint32_t *edits,
                     uint64_t info[8]);
/* the table of read names on its own (bh_chimera.c keeps its reads in one): bh_cluster_names with the flags its two usage errors name;
 * the node of a name (0xFFFFFFFF: none), a node's name, the weights (valid until the next names call); the reads of Q in file order */
int  bh_cluster_names_as(BhCluster *cl, const char *const *names, uint32_t n, const char *flag, const char *sizes_flag);
uint32_t bh_cluster_find(const BhCluster *cl, const char *s, size_t len);
const char *bh_cluster_name(const BhCluster *cl, uint32_t node);
const uint32_t *bh_cluster_weights(const BhCluster *cl);
int  bh_cluster_file_order(const BhQueries *q, const char **names, uint32_t *node_of);

/* ---- de-novo two-parent chimera check of the reads of a query file aligned against itself (bh_chimera.c; burst_hip --chimeras) ----
 * The definition is bhip_chimera_run's (include/burst_hip.h): nodes, names and weights as in the clustering (the same name table);
 * candidate parents weigh at least skew times the read; per (read, parent) the printed line with the fewest edits counts; the edit
 * positions of its alignment path, in read orientation, give for every cut the edits left and right of it; the best two-parent model
 * over all cuts is set against the best single parent.  PREFIXchimeras.txt:
 * `#Read<TAB>Role<TAB>Single<TAB>Model<TAB>Cut<TAB>ParentA<TAB>EditsA<TAB>ParentB<TAB>EditsB<TAB>Weight`, one row per read in file order, Role
 * Y (chimeric), N, or - (not evaluated: 0 for the numbers, * for the parents); written under a temporary name and renamed, never when the
 * run ends on an error.
 *   bh_chimera_open        skew, min_seg, min_gain outside 1 .. 2^31 - 1 are BH_E_USAGE
 *   bh_chimera_names       the reads and their lengths: resets the object; two byte-equal names are BH_E_USAGE with a text that names them
 *   bh_chimera_line        one printed line of read q: column 2, strand (reverse: column 9 > column 10), its path's op words
 *   bh_chimera_add_b6      the lines of a .b6 file written with --cigar (columns 1, 2, 9, 10 and the last)
 *   bh_chimera_begin       before a run's report: the reads of Q (names, lengths) and the headers of db
 *   bh_paths_set_chimera   the collector of the path tracer is this object (columns: whether the lines get the --cigar columns): every
 *                          traced group and the notes of its printed lines become lines here -- the read from the line's unique query
 *                          (duplicate reads carry its path, one line per read), the parent from the header's name, the strand from the entry
 *   bh_chimera_solve       one solver call over the lines collected, on `hip_handle`
 *   bh_chimera_result      per read: its BhipChimera, its weight (either may be NULL)
 *   bh_chimera_print_info  the `Chimeras:` line on standard output; bh_chimera_last_info: the same figures (bhip_chimera_info's, lines, foreign lines)
 *   bh_chimera_set_solver  another solver (tests): bhip_chimera_run's arguments and bhip_chimera_info's array behind ctx, return codes in
 *                          this file's terms; fn = NULL: the device
 *   bh_chimera_host        the definition in plain sequential C, a solver (its first argument is ignored): it materialises L[c] for every
 *                          line and cut; the tests without a device and the yardstick.  It checks what bhip_chimera_run checks
 *                          (BH_E_USAGE) and that a chimeric read has two different parents (BH_E_INTERNAL otherwise)
 * Any error is final: later calls return it and nothing is written. */
typedef struct BhChimera BhChimera;
typedef int (*bh_chimera_solver_fn)(void *ctx, uint32_t n_nodes, const uint32_t *weights, const uint32_t *len, const BhipChimLine *lines, uint64_t n_lines,
                                    const uint32_t *ops, uint64_t n_ops, uint32_t skew, uint32_t min_seg, uint32_t min_gain, BhipChimera *out, uint64_t info[8]);
int  bh_chimera_open(const char *prefix, int use_sizes, uint32_t skew, uint32_t min_seg, uint32_t min_gain, BhChimera **ch);
void bh_chimera_set_solver(BhChimera *ch, bh_chimera_solver_fn fn, void *ctx);
int  bh_chimera_names(BhChimera *ch, const char *const *names, const uint32_t *lens, uint32_t n);
int  bh_chimera_line(BhChimera *ch, uint32_t q, const char *ref_name, size_t ref_len, int reverse, const uint32_t *ops, uint32_t n_ops);
int  bh_chimera_add_b6(BhChimera *ch, const char *path);
int  bh_chimera_begin(BhChimera *ch, const BhDb *db, const BhQueries *q);
void bh_paths_set_chimera(BhPaths *paths, BhChimera *ch, int columns);
int  bh_chimera_solve(BhChimera *ch, void *hip_handle);
uint32_t bh_chimera_reads(const BhChimera *ch);
int  bh_chimera_result(const BhChimera *ch, BhipChimera *out, uint32_t *weights);
void bh_chimera_last_info(const BhChimera *ch, uint64_t info[8], uint64_t *lines, uint64_t *foreign);
int  bh_chimera_write(BhChimera *ch);
void bh_chimera_print_info(BhChimera *ch);
void bh_chimera_abort(BhChimera *ch);
void bh_chimera_close(BhChimera *ch);
int  bh_chimera_host(void *unused, uint32_t n_nodes, const uint32_t *weights, const uint32_t *len, const BhipChimLine *lines, uint64_t n_lines,
                     const uint32_t *ops, uint64_t n_ops, uint32_t skew, uint32_t min_seg, uint32_t min_gain, BhipChimera *out, uint64_t info[8]);

/* ---- SAM output beside the .b6, with NM and MD tags (bh_sam.c; burst_hip --sam) ----
 * For every .b6 output OUT the file OUT.sam: `@HD VN:1.6 SO:unknown GO:query`, one `@SQ SN LN` per database header in the order of the
 * unique-header numbers (RefMap: the numbers of the placement sink), `@PG ID:burst_hip PN:burst_hip` (no command line, so that a --samples
 * sample's file equals a separate invocation's), then one record per printed line in .b6 order: QNAME = column 1 up to its first white
 * space; FLAG = 0x10 when column 9 > column 10, | 0x100 on every line of a read but the first printed for it (a duplicate read is a read of
 * its own); RNAME = the header's SN (the header up to its first white space); POS and CIGAR = the two --cigar columns; MAPQ 255; RNEXT,
 * PNEXT, TLEN = * 0 0; SEQ = the codes of the query entry the path belongs to as .ACGTNKMRYSWBVHD (a reverse line: the reverse-complement
 * entry); QUAL *; NM:i: then MD:Z: (bhip_md_tags, include/burst_hip.h).  With `unmapped`, behind them one record per read without a
 * line, in query-file order: FLAG 4, * 0 0 * * 0 0, the forward SEQ, QUAL *, no tags.  The file is written under a temporary name and
 * renamed by bh_sam_end; a sample that failed alone (bh_sam_discard) and a run that ended on an error leave none.
 *   bh_sam_open        the headers are the database's unique-header numbers; two different headers with one SN are BH_E_USAGE with a text
 *                      that names both; lengths_file: the table of --coverage-lengths (same format, same errors, bh_cov_read_lengths), or
 *                      NULL: the database's own extents (bh_cov_default_lengths, taken when the first sample begins)
 *   bh_sam_open_heads  any headers, with their lengths
 *   bh_sam_set_md      another MD function (tests): bhip_md_tags' arguments behind ctx, return codes in this file's terms (BH_E_CAPACITY =
 *                      md_off[n] bytes wanted; the call is repeated once with that room); fn = NULL: the device
 *   bh_sam_begin       a sample: the handle its paths are traced on, its queries, its .b6 output's name; writes the header
 *   bh_paths_set_sam   a collector of the path tracer is this object (columns: whether the lines get the --cigar columns): ONE MD call per
 *                      traced group
 *   bh_sam_end         the unmapped records, the rename; bh_sam_print_info: the `Sam:` line (records, unmapped records, MD bytes, device
 *                      milliseconds); bh_sam_last_info: the same figures ([3] in microseconds)
 *   bh_sam_abort       the run ends on an error: nothing more will be written
 *   bh_md_host         the MD string and NM of ONE path in plain sequential C over a lane given as an array of codes (lane[0] = column 1):
 *                      the yardstick.  BH_E_USAGE for what bhip_md_tags refuses, BH_E_CAPACITY with *md_len = the bytes wanted */
typedef struct BhSam BhSam;
typedef int (*bh_md_fn)(void *ctx, const BhipPathReq *req, const uint32_t *ref_first, const uint64_t *op_off, const uint32_t *ops, uint64_t n_requests, char *md, uint64_t md_cap,
                        uint64_t *md_off, uint32_t *nm, uint64_t info[8]);
int  bh_sam_open(const BhDb *db, const char *lengths_file, int unmapped, BhSam **sam);
int  bh_sam_open_heads(uint32_t n_headers, const char *const *heads, const uint32_t *lengths, int unmapped, BhSam **sam);
void bh_sam_set_md(BhSam *sam, bh_md_fn fn, void *ctx);
int  bh_sam_begin(BhSam *sam, void *hip_handle, const BhQueries *q, const char *out_path);
int  bh_paths_set_sam(BhPaths *paths, BhSam *sam, int columns);      /* BH_E_USAGE: the tracer's list of collectors is full */
int  bh_sam_end(BhSam *sam);
void bh_sam_discard(BhSam *sam);
void bh_sam_abort(BhSam *sam);
void bh_sam_print_info(BhSam *sam);
void bh_sam_last_info(const BhSam *sam, uint64_t info[4]);
void bh_sam_close(BhSam *sam);
int  bh_md_host(const uint8_t *lane, uint32_t lane_len, uint32_t ref_first, const uint32_t *ops, uint64_t n_ops, char *md, uint64_t md_cap, uint64_t *md_len, uint32_t *nm);

/* ---- a session: the database stays on the devices, a list of query files runs through it (bh_session.c) ---- */
typedef struct BhSession BhSession;
typedef struct BhSessionOpts {            /* fixed for the whole session */
	BhMode mode; float thres; int do_rc, incl_ws, z, do_accel, K, skip_ambig, rep_flags;      /* K = 0 with do_accel: the accelerator file's (db->K when a sample's turn comes) */
	uint64_t batch;
	int shard_db;                         /* number of database shards (0 / 1 = query-sharded), as for bh_search_multi_ex */
	const BhTaxOpts *tax;                 /* NULL = no taxonomy column (copied; the BhTax it points to must outlive the session) */
	int ingest_ahead;                     /* 1 = bh_session_prefetch parses a sample on a thread while the current one is searched and reported */
	int verbose;                          /* 1 = the command line's per-sample lines on standard output */
	BhCov *cov;                           /* NULL, or the coverage every reported sample feeds (rank 0's process; the caller opens it, writes the tables and closes it) */
	int cigar;                            /* 1 = every line carries its path's position and CIGAR (bh_paths.c), traced on the handle of the rank that reports */
	BhMatesOpts mates;                    /* bh_session_run_mates: orientation, bounds of the fragment length, report (all zero: fr, [0, 0], all -- set the bounds) */
	BhEm *em;                             /* NULL, or the abundance every reported sample feeds (as cov: rank 0's process; the caller opens it, writes the table and closes it) */
	BhPile *pile;                         /* NULL, or the variant sites every reported sample feeds (as em); opens the path tracer even without cigar */
} BhSessionOpts;
typedef struct BhSampleResult {
	int rc; char err[512];
	uint64_t totQ, numUniq, nHits, nLines; uint32_t nBatches;
	double secIngest, secIngestWaited, secSearch, secReport;
	BhipStats total;                      /* counters of the sample's batches, summed over this process's ranks */
} BhSampleResult;
/* ranks / n_local / n_ranks / comm / node: as for bh_search_multi_ex (the threads of this process: n_local = n_ranks; or one rank of a
 * job of processes: n_local = 1).  The session keeps the pointers: `db`, `ranks` (whose handles may still be opened after this call,
 * before the first sample is finished) and their runs belong to the caller and must outlive it.  BhMultiRank.align back ends work as
 * in bh_search_multi_ex; they are handed the BhQueries of the sample being searched.  c0 is the caller's, the query ranges are the
 * session's (set per sample). */
int  bh_session_open(const BhDb *db, BhMultiRank *ranks, int n_local, int n_ranks, void *comm, BhNode *node, const BhSessionOpts *o, BhSession **s);
/* start the ingest of the sample whose turn comes after the next bh_session_load / _run.  One ingest thread at a time: called while
 * one is outstanding, the name is kept and its ingest starts as soon as that one has been taken.  Without ingest_ahead, or with
 * BURST_HOST_SERIAL_INGEST set, it does nothing and every sample is read when its turn comes. */
int  bh_session_prefetch(BhSession *s, const char *queries);
/* one sample: bh_session_run = bh_session_load (ingest or take the prefetched tables, bins, shear check, create the output) +
 * bh_session_finish (page-lock, buffers, search, report, release).  Between the two a launcher of several processes sees the sample
 * (bh_session_sample), agrees on its status with the other ranks and sizes their hand-over (bh_session_set_node); bh_session_drop
 * gives the loaded sample up.  BH_E_USAGE / BH_E_IO of a sample are recorded in `res` and leave the session usable (no output file is
 * left behind); every error of the search, BH_E_OOM, BH_E_DEVICE and BH_E_INTERNAL end it: later calls return that code at once.
 * In a job of processes only rank 0 writes; the other ranks pass through the search and return the sample's status. */
int  bh_session_load(BhSession *s, const char *queries, const char *out_path, BhSampleResult *res);
int  bh_session_finish(BhSession *s, BhSampleResult *res);
int  bh_session_drop(BhSession *s);
int  bh_session_run(BhSession *s, const char *queries, const char *out_path, BhSampleResult *res);
/* a pair of mate files: queries1 and then queries2 through the per-sample path above (queries2's ingest ahead, beside queries1's
 * search), each into a temporary file beside out_path; the two outputs joined (bh_mates.c, on the handle of the rank that reports) into
 * out_path, written under a temporary name and renamed.  Needs mode ALLPATHS or FORAGE, do_rc, no coverage, no abundance and no cigar (BH_E_USAGE
 * otherwise, before anything runs).  `res`: the two mates' counts and times summed, nLines = lines of the paired output.  A mate file that
 * fails fails the pair under the rule above; no output and no temporary file stays.  bh_session_mates: the session's joiner object (made
 * on first use: bh_mates_set_join, bh_mates_stats). */
int  bh_session_run_mates(BhSession *s, const char *queries1, const char *queries2, const char *out_path, BhSampleResult *res);
BhMates *bh_session_mates(BhSession *s);
const BhQueries *bh_session_sample(const BhSession *s);
void bh_session_set_node(BhSession *s, BhNode *node);
void bh_session_set_coverage(BhSession *s, BhCov *cov);      /* BhSessionOpts.cov for a session opened before its database was read */
void bh_session_set_abundance(BhSession *s, BhEm *em);       /* BhSessionOpts.em likewise */
void bh_session_set_variants(BhSession *s, BhPile *pile);    /* BhSessionOpts.pile likewise */
/* NULL, or the clustering every reported sample is given (rank 0's process; the caller opens and closes it): the sample's reads clustered
 * from its own lines on the reporting rank's handle, the two tables written at once (a later sample writes them again).  Needs mode FORAGE
 * (BH_E_USAGE otherwise) and is kept beside the options, not in BhSessionOpts */
int  bh_session_set_cluster(BhSession *s, BhCluster *cl);
/* likewise NULL, or the chimera check every reported sample is given: it opens the path tracer (without the --cigar columns unless the
 * session has them), collects the sample's lines from the traced groups, and writes its table at once.  Mode FORAGE only */
int  bh_session_set_chimera(BhSession *s, BhChimera *ch);
/* likewise NULL, or the SAM writer every reported sample is given (rank 0's process; the caller opens and closes it): OUT.sam beside every
 * output OUT.  It opens the path tracer (without the --cigar columns unless the session has them) and goes with variants and the chimera
 * check.  Not with database shards, not with bh_session_run_mates */
int  bh_session_set_sam(BhSession *s, BhSam *sam);
/* likewise NULL, or the taxon tables every reported sample feeds (rank 0's process; the caller opens it, writes the tables and closes it):
 * the report's sink is filled for it alone, and a session with an abundance hands each sample's counts over for the roll-up.  Not with
 * clusters or the chimera check, not with bh_session_run_mates */
int  bh_session_set_taxa(BhSession *s, BhTaxa *tx);
/* likewise NULL, or the consensus every reported sample feeds (rank 0's process; the caller opens it, writes the files and closes it): it
 * opens the path tracer (without the --cigar columns unless the session has them) and goes with coverage, abundance, variants and the SAM
 * writer.  Not with database shards, clusters, the chimera check or bh_session_run_mates */
int  bh_session_set_consensus(BhSession *s, BhCons *cons);
/* a consensus with a pairs collector (bh_conspairs_attach): when every sample has been reported and before the caller's
 * bh_consensus_write, the one bhip_consensus_pairs call on the reporting rank's handle and the three files under temporary names */
int  bh_session_consensus_pairs(BhSession *s);
/* likewise NULL, or the VCF writer every reported sample is given (rank 0's process; the caller opens and closes it): OUT.vcf beside the
 * output OUT.  Goes with coverage, abundance, variants, the consensus, cigar and the SAM writer.  Not with database shards, clusters, the
 * chimera check or bh_session_run_mates */
int  bh_session_set_vcf(BhSession *s, BhVcf *vcf);
int  bh_session_ended(const BhSession *s);      /* 0, or the code of the error that ended the session */
void bh_session_close(BhSession *s);

const char *bh_last_error(void);
int bh_set_error(int code, const char *fmt, ...);

/* ---- synthetic data (tests / bench tooling; behaviour modelled on embalmlets/LLsim.c:175-231) ---- */
int bh_synth_refs(const char *fasta_out, uint32_t n_base, uint32_t n_variants, uint32_t length, double variant_rate, uint64_t seed);
int  bh_synth_refs_range(const char *fasta_out, uint32_t first_base, uint32_t n_base, uint32_t n_variants, uint32_t length, double rate, uint64_t seed);
int bh_synth_reads(const char *refs_fasta, const char *fasta_out, uint64_t n_reads, uint32_t read_len, const uint32_t *edit_choices,
                   uint32_t n_choices, int rc, double iupac_rate, uint64_t seed);
int  bh_synth_reads_ex(const char *refs_fasta, const char *fasta_out, uint64_t n_reads, uint32_t read_len, const uint32_t *edit_choices,
                       uint32_t n_choices, int rc, double iupac_rate, uint64_t seed, uint64_t first_read, int append);

#ifdef __cplusplus
}
#endif
#endif
