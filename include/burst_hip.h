/* include/burst_hip.h -- C ABI of libburst_hip.so, the MI355X (gfx950) device side of the BURST
 * alignment hot path.  Plain pointers and sizes only; no C++ or torch types cross this line.
 *
 * The reference (knights-lab/BURST, burst.c @ 2024_08_07) has no plugin/FFI interface; what this
 * library replaces are the four kernel call sites inside do_alignments() and the k-mer scour block:
 *
 *   aded_mat16L(...)                burst.c:4215   \  banded edit distance of one query vs one 16-lane clump
 *   aded_mat16 / aded_xalpha(...)   burst.c:4423-4426 /  -> bhip_align_batch (kernel "myers"), bhip_align_pairs
 *   reScoreM_mat16 / _xalpha(...)   burst.c:4226, 4439-4442  -> bhip_align_batch (kernel "rescore")
 *   qsort + postScour + selection   burst.c:4096-4133, 3238-3282 -> bhip_align_batch (kernel "prefilter"),
 *                                                                   bhip_prefilter
 *   4-bit clump unpack              burst.c:4141-4150          -> folded into bhip_init (device layout)
 *
 * Conventions mirror those call sites: the caller owns every host buffer, the library owns device
 * memory, failures are return codes (never exit()), a handle is single-threaded, one handle per device.
 * Return values: 0 = ok, negative = BHIP_E_*; bhip_last_error() gives the text.
 */
#ifndef BURST_HIP_H
#define BURST_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* libburst_hip.so is built with -fvisibility=hidden: the entry points below are its whole dynamic symbol table */
#define BHIP_API __attribute__((visibility("default")))

#define BHIP_OK            0
#define BHIP_E_ARG        -1   /* invalid argument */
#define BHIP_E_DEVICE     -2   /* HIP runtime error (no device, OOM, launch failure) */
#define BHIP_E_CAPACITY   -3   /* caller's hit buffer too small: *n_hits holds the required count */
#define BHIP_E_QUERYLEN   -4   /* query longer than BHIP_MAX_QLEN */
#define BHIP_E_INTERNAL   -5
#define BHIP_E_RESCORE    -6   /* the re-scorer cannot reproduce a hit of the search: the state in which the reference prints "CRITICAL ERROR:
                                 Truncation within known good path" and exits (burst.c:812-816) -- a query whose FIRST symbol has code 0
                                 (row 1 of reScoreM takes the substitution cost alone, burst.c:722-739, while the search may gap it) */

#define BHIP_MAX_QLEN   4095   /* up to 1 024 symbols: register bit-vector kernels (2 .. 32 words); beyond: k_myers_long (vector in LDS, single-stage sweep) */

/* One alignment result = ResultPod (burst.c:3998-4004) minus the list pointer, plus the query index. */
typedef struct BhipHit {
	uint32_t q;         /* index of the query entry in the batch (forward or reverse-complement entry) */
	uint32_t refIx;     /* 16*clump + lane, burst.c:4234 */
	uint32_t finalPos;  /* MetaPack.finalPos, burst.c:862-883: 1-based end column in the sheared reference */
	float    score;     /* MetaPack.score, burst.c:844-860: 1 - ed/(len + numGapQ), IEEE f32 division */
	uint8_t  ed;        /* ResultPod.mismatches = MinA[lane], burst.c:4232 */
	uint8_t  gapR;      /* numGapR */
	uint8_t  gapQ;      /* numGapQ */
	uint8_t  rc;        /* strand of the query entry, burst.c:4238 */
} BhipHit;              /* 20 bytes */

/* Query flags (q_flags[i]) */
#define BHIP_Q_PREFILTER   0   /* candidate clumps come from the .acx prefilter + BadList (burst.c:4078-4284) */
#define BHIP_Q_EXHAUSTIVE  1   /* align against every clump (burst.c:4320-4488: no -a, or "bad"-bin queries) */

/* Counters and timings of the most recent bhip_align_batch / bhip_align_pairs call on a handle.
 * Times are HIP-event milliseconds measured on the library's own stream. */
typedef struct BhipStats {
	uint64_t n_queries;        /* query entries in the call */
	uint64_t n_pairs;          /* (query, clump) units of work aligned */
	uint64_t n_columns;        /* sum over clump-level pairs of ClumpLen: DP columns swept (x16 lanes x qlen rows of cells); lane tasks: n_task_columns */
	uint64_t n_raw_hits;       /* (query, ref) lanes with ed <= budget */
	uint64_t n_hits;           /* records returned */
	uint64_t acx_entries_read; /* list entries gathered by the prefilter */
	uint64_t bytes_algorithmic;/* per-launch algorithmic bytes of the myers kernel */
	uint64_t n_windows;        /* reference lanes that passed the prefix stage of the two-stage edit distance */
	uint64_t n_window_columns; /* columns swept by the full-length stage over those windows */
	uint64_t n_lane_tasks;     /* (query, reference lane) tasks emitted by the lane-resolved prefilter (0 = clump-level path) */
	uint64_t n_task_columns;   /* columns swept by the prefix stage over those tasks */
	uint64_t n_seed_words;     /* sampled query words looked up in the accelerator by the lane-resolved prefilter */
	float ms_h2d, ms_prefilter, ms_peq, ms_myers, ms_rescore, ms_d2h, ms_total;
	float ms_myers_prefix;     /* part of ms_myers spent in k_myers_prefix (the dominant kernel when the two-stage path runs) */
	float ms_myers_window;     /* part of ms_myers spent in k_myers_window */
	float ms_prefilter_hash;   /* part of ms_prefilter spent in k_prefilter_mask (HIP events around that kernel alone) */
	float ms_seed;             /* part of ms_prefilter spent in k_seed_ranges */
	float ms_stage_copy;       /* of ms_h2d (the staging of this batch, on the staging stream, two batches ahead): the copies over PCIe with the unpack kernels and offset scans between them */
	float ms_stage_route;      /* of ms_h2d: k_pack_queries, k_route and the radix sort of the entry lists behind the copies (kernels that share the CUs with the batch being aligned) */
	uint32_t myers_launches;   /* launches of the column-sweeping kernel (k_myers_prefix, or k_myers on the one-stage path) */
	uint32_t prefix_words;     /* NWP of the last launch, 0 = one-stage path */
	uint32_t prefilter_launches; /* launches of the lane-resolved prefilter kernel */
	uint32_t prefilter_algo;   /* kernel of the last such launch: 0 = k_prefilter_cf (counting filter), 1 = k_prefilter_mask (exact hash) */
} BhipStats;

/* Upload a database to device `device` and create a handle.
 *   edx_packed : the clump area of an .edx exactly as on disk (burst.c:2810-2824): for clump c,
 *                ceil(clump_len[c]/2) 16-byte words; byte k of a word = lane k; low nibble = even position.
 *   clump_len  : ClumpLen[n_clumps] (burst.c:2918);  tot_refs = totR (lanes >= tot_refs never hit, burst.c:4229)
 *   acx_lens   : Lens[4^K] of the .acx (burst.c:3558), or NULL: with K = 0 no accelerator is used, with K in 4..15 the accelerator
 *                is BUILT ON THE DEVICE from the references alone (what make_accelerator does, burst.c:3304-3532: same entries in
 *                the same order, same BadList; acx_lists / acx_fmt / badlist are then ignored) -- no .acx file, no upload
 *   acx_lists  : the packed list area (burst.c:3569); acx_fmt 0 = SMALL 20-bit pairs (3265-3274), 1 = LARGE 24-bit (3245-3248)
 *   badlist    : BadList[n_bad] (burst.c:3571): clumps every prefiltered query must be aligned against
 *   score_lut  : 16x16 cost table lut[16*q + r] in {0,1,255} = SCOREFAST after setScore() (burst.c:1310-1328)
 *   xalpha     : must be 0.  The alphabet-agnostic mode (-x; aded_xalpha / reScoreM_xalpha, burst.c:696-697, 894, 1099) needs no device
 *                switch: the host maps the run's alphabet (up to 15 symbols) onto the codes 1..15 and passes the IDENTITY cost table
 *                (0 iff equal, 1 otherwise, the padding code 0 included) as score_lut -- burst_hip -x, host/main.c
 */
BHIP_API int bhip_init(int device, const void *edx_packed, const uint32_t *clump_len, uint32_t n_clumps, uint32_t tot_refs,
              const uint32_t *acx_lens, const void *acx_lists, int acx_fmt, int K,
              const uint32_t *badlist, uint32_t n_bad,
              const uint8_t score_lut[256], int xalpha, void **handle);

/* Prefilter + banded edit distance + re-scoring for a batch of query entries (the body of the OpenMP
 * loops burst.c:4077-4289 and 4343-4484).
 *   q_codes : concatenated 1-byte symbol codes (0..15, burst.c:1288-1307), entry i = [q_off[i], q_off[i+1]); code 0 (a character
 *             outside the IUPAC nucleotide alphabet) costs 255 against everything, i.e. it can only face a gap
 *   q_emac  : per-entry error budget (ShrBin.ed, burst.c:3074-3076)
 *   q_six   : per-entry shared slot (UniBin.six, burst.c:3078, 3106): a forward entry and its reverse
 *             complement carry the same value in [0, n_shared) and share the running minimum (burst.c:4218-4220)
 *   q_rc    : per-entry strand flag copied into BhipHit.rc
 *   q_flags : BHIP_Q_PREFILTER / BHIP_Q_EXHAUSTIVE per entry (NULL = all exhaustive when the handle has no
 *             accelerator, all prefiltered otherwise)
 *   all_hits: 0 = BEST/ALLPATHS/CAPITALIST semantics (only lanes with ed == minimum over the shared slot),
 *             1 = FORAGE semantics (every lane with ed <= budget, burst.c:4224),
 *             2 = BHIP_HITS_BEST: the minimum-only semantics with BEST's choice made on the device -- per query ENTRY the one
 *                 record the reference's BEST scan keeps among that entry's records (burst.c:4847-4891: equal ed, then the higher
 *                 f32 score, then the lower RefIxSrt[refIx]; needs bhip_set_ref_order).  One record per entry with a hit crosses
 *                 PCIe instead of every equally good reference; the choice between a query's two strands stays with the caller.
 *   hits/cap: caller's buffer; on BHIP_E_CAPACITY *n_hits is the number required and nothing is returned.
 * Records are returned sorted by (q, refIx). */
BHIP_API int bhip_align_batch(void *handle, const uint8_t *q_codes, const uint64_t *q_off, const uint16_t *q_emac,
                     const uint32_t *q_six, const uint8_t *q_rc, const uint8_t *q_flags,
                     uint32_t n_q, uint32_t n_shared, int all_hits,
                     BhipHit *hits, uint64_t cap, uint64_t *n_hits);

/* The same in two steps.  bhip_stage_queries is synchronous (the caller's arrays are free again at return) and replaces any
 * batch that was waiting; bhip_align_staged may then run any number of times on the resident batch.
 * bhip_align_batch(...) == bhip_stage_queries(...) followed by bhip_align_staged(...). */
BHIP_API int bhip_stage_queries(void *handle, const uint8_t *q_codes, const uint64_t *q_off, const uint16_t *q_emac,
                       const uint32_t *q_six, const uint8_t *q_rc, const uint8_t *q_flags, uint32_t n_q, uint32_t n_shared);
BHIP_API int bhip_align_staged(void *handle, int all_hits, BhipHit *hits, uint64_t cap, uint64_t *n_hits);
#define BHIP_HITS_MIN   0
#define BHIP_HITS_ALL   1
#define BHIP_HITS_BEST  2
/* The tie-break table of all_hits = BHIP_HITS_BEST: order[refIx] = RefIxSrt[refIx] (burst.c:3688-3693; the reference's BEST prefers the
 * lower original reference number among equally good hits, burst.c:4865-4868), n = tot_refs.  Copied to the device.  order = NULL:
 * nothing is changed, the return value says whether the handle holds a table (1) or not (0). */
BHIP_API int bhip_set_ref_order(void *handle, const uint32_t *order, uint32_t n);

/* Pipelined staging for a batch scheduler (the replacement of the OpenMP loops burst.c:4050-4078 / 4326-4344 hands batch k+1
 * to the device while batch k is being aligned).  A batch is given as up to a few SPANS of consecutive entries of the caller's
 * own arrays (process_queries keeps all forward entries and then all reverse complements, burst.c:3087-3109: a batch of
 * unique queries [u, u+B) is two spans), so nothing is gathered on the host.  Entry j of EVERY span shares slot j (a forward
 * entry and its reverse complement: UniBin.six, burst.c:3106) and is reported as BhipHit.q = q_base + j.
 * The call only ENQUEUES the copies and the device-side routing (length classes, prefilter / exhaustive route, seed plans)
 * on the library's staging stream and returns; the arrays must stay valid until the batch has been aligned.  Three staging
 * slots: beside the batch being aligned, two more can be staged; bhip_align_staged always takes the oldest one that has
 * not been aligned yet (and, when none is waiting, runs the last one again).  With a batch staged AHEAD of the one being
 * aligned -- a caller that stages two batches ahead, as bh_align_ranges does -- the library runs that batch's seed lookups
 * and match profiles beside the current batch's sweeps (option "seed_ahead", default 1).  Page-locked arrays (bhip_alloc_host / bhip_host_register) make the copies
 * asynchronous; pageable ones work too.  max_len = an upper bound of the entry lengths (0 = computed from the offsets). */
typedef struct BhipQuerySpan {
	const uint8_t  *codes;   /* symbol codes; entry j = codes[off[j] .. off[j+1]) */
	const uint8_t  *codes4;  /* optional: the same array packed two symbols per byte (symbol i = (codes4[i >> 1] >> 4 * (i & 1)) & 15, i counted
	                            from the start of `codes`); when every span has it, this is what crosses PCIe (half the bytes) */
	const uint64_t *off;     /* n + 1 offsets into codes (off[0] need not be 0) */
	const uint16_t *emac;    /* n budgets */
	const uint8_t  *rc;      /* n strand flags, or NULL = 0 */
	const uint8_t  *flags;   /* n BHIP_Q_*, or NULL (all spans or none) */
	uint32_t n;
	uint32_t q_base;         /* BhipHit.q of the span's first entry */
	const uint8_t  *codes2;  /* optional, for spans whose every symbol is A, C, G or T (codes 1..4): the array packed four symbols per byte
	                            (symbol i = ((codes2[i >> 2] >> 2 * (i & 3)) & 3) + 1); when every span of a batch has it, it is what crosses
	                            PCIe (a quarter of the bytes) */
	const uint16_t *len;     /* optional: the n entry lengths off[j+1] - off[j]; when every span has it, the lengths cross PCIe instead of the
	                            8-byte offsets (prefix sum on the device).  `codes` and `off` are still required in full: the host pass that
	                            handles batches with symbols outside the alphabet reads them */
} BhipQuerySpan;
BHIP_API int bhip_stage_spans(void *handle, const BhipQuerySpan *spans, uint32_t n_spans, uint32_t n_shared, uint32_t max_len);

/* Optional: a function the library calls from inside bhip_align_staged once the whole chain of the batch (and the seed lookups of the
 * next staged one) has been ENQUEUED and before it waits for the device -- the moment a batch scheduler has for its own host work
 * (staging the batch after next: ~20 asynchronous copies and launches) without leaving the device idle between two batches.  The
 * hook may call bhip_stage_spans on the same handle; nothing else.  fn = NULL removes it.  No reference counterpart (the reference's
 * scheduler is the OpenMP loop burst.c:4077). */
BHIP_API int bhip_set_enqueued_hook(void *handle, void (*fn)(void *ctx), void *ctx);

/* Optional: allocate now what batches of up to n_entries entries of up to max_len symbols will need, so that no allocation
 * (each one synchronises the device) falls into the first batches. */
BHIP_API int bhip_reserve(void *handle, uint32_t n_entries, uint32_t max_len);
/* the same with the symbol count of the largest batch to come (sum of its entries' lengths; 0 = n_entries x max_len): what holds
 * symbols and match profiles is sized from it, so that one long read among millions of short ones does not multiply every buffer */
BHIP_API int bhip_reserve_symbols(void *handle, uint32_t n_entries, uint32_t max_len, uint64_t total_symbols);

/* Page-locked host memory (hipHostMalloc / hipHostRegister behind the C ABI, for callers that are plain C): copies from and to
 * it run asynchronously beside the kernels.  bhip_alloc_host returns NULL when no device is present. */
BHIP_API void *bhip_alloc_host(uint64_t bytes);
BHIP_API void  bhip_free_host(void *p);
BHIP_API int   bhip_host_register(void *p, uint64_t bytes);
BHIP_API int   bhip_host_unregister(void *p);

/* Multi-GPU (no reference counterpart).  Query-sharded: the unique queries are cut across the GPUs of a node -- one
 * handle per device, the database replicated.  The hit records are wanted in rank 0's HOST memory (the consolidation runs there):
 * inside one node the host library lets them meet there without a collective (every rank's records reach host memory over its own
 * PCIe link behind its batches; host/bh_multi.c, host/bh_node.c) -- these entry points are the exchange for ranks that cannot see
 * each other's memory, and the option --gather rccl: one variable-length gather over RCCL / xGMI to rank 0's device
 * (ncclAllGather of the counts + grouped ncclSend / ncclRecv of the 20-byte records) and one copy to its host.  Database-sharded (databases beyond one
 * device): every rank holds a range of clumps and aligns all queries; the hits of a query are the references at its GLOBAL minimum
 * edit distance (burst.c:4217-4277), so the ranks combine one byte per unique query with bhip_comm_allreduce_min (ncclAllReduce,
 * MIN) before the same gather.  The ranks are the threads of one process (bhip_comm_create: ncclCommInitAll over `devices`) or one
 * process each (bhip_comm_unique_id on one of them, the 128 bytes carried to the others by the launcher, bhip_comm_create_rank:
 * ncclCommInitRank); every rank's thread calls the collectives with its own rank, all ranks' calls in flight together.
 * bhip_comm_gather_hits: rank 0 gets all records in rank order, counts[n_ranks] the per-rank numbers; BHIP_E_CAPACITY: *n_total
 * needed.  A rank that cannot take part (out of memory ...) makes the call fail on EVERY rank instead of leaving them waiting. */
BHIP_API int  bhip_comm_create(int n_ranks, const int *devices, void **comm);
BHIP_API int  bhip_comm_unique_id(void *id128);
BHIP_API int  bhip_comm_create_rank(int n_ranks, int rank, int device, const void *id128, void **comm);
BHIP_API int  bhip_comm_gather_hits(void *comm, int rank, const BhipHit *hits, uint64_t n, BhipHit *out, uint64_t cap, uint64_t *n_total, uint64_t *counts);
/* The same gather fed from the DEVICE: bhip_comm_stage_device after every batch copies the records of the handle's last alignment call
 * (still resident there) into the rank's send buffer, device to device, behind the `first_record` records staged before;
 * bhip_comm_gather_staged then sends the n staged records without uploading the host copy again.  A rank whose staging failed makes
 * the gather fail on every rank (the caller falls back on bhip_comm_gather_hits); bhip_comm_stage_reset forgets what was staged. */
BHIP_API int  bhip_comm_stage_device(void *comm, int rank, void *handle, uint64_t first_record, uint64_t *n_records);
BHIP_API int  bhip_comm_gather_staged(void *comm, int rank, uint64_t n, BhipHit *out, uint64_t cap, uint64_t *n_total, uint64_t *counts);
BHIP_API void bhip_comm_stage_reset(void *comm, int rank);
BHIP_API int  bhip_comm_fetch_gathered(void *comm, BhipHit *out, uint64_t cap, uint64_t *n_total);      /* rank 0 after BHIP_E_CAPACITY: no collective, the records are still on its device */
BHIP_API int  bhip_comm_allreduce_min(void *comm, int rank, uint8_t *buf, uint64_t n);
BHIP_API void bhip_comm_destroy(void *comm);

/* Cooperative accelerator build (no reference counterpart: make_accelerator, burst.c:3304-3532, is one process).  With the database
 * replicated over n_parts devices every handle needs the whole accelerator, and building it is most of what a job waits for before its
 * first batch; so every handle -- initialised with K = 0, i.e. without one -- builds the lists of 1/n_parts of the WORD space (runs of
 * words with equal numbers of window tuples, cut alike by every rank from a histogram of the database), and the ranks complete each
 * other's tables in two exchanges: Lens (4^K x 4 bytes in all), then the 4-byte records.  The result on every handle is what bhip_init
 * with K would have built alone, bit for bit (tests/test_gpu_acx.py).
 *   bhip_share_fn: called by every rank at the same two points with ITS array (a device pointer) and the same byte offsets
 *     byte_off[0 .. n_parts]: region [byte_off[r], byte_off[r + 1]) is valid on rank r when the call is made and on every rank when it
 *     returns.  status != 0 announces that this rank could not do its part: the function then moves nothing and returns 1 on EVERY rank
 *     (all handles fall back to building alone); < 0 = the exchange itself failed.
 *   Ready-made exchanges: bhip_comm_share (ctx = BhipCommRank: ncclBroadcast of every region from its builder, one group, over xGMI),
 *   bhip_team_share (ctx = a team of the threads of ONE process: peer copies device to device behind a barrier; the ranks may share a
 *   device), or the caller's own (python -m burst_amd.run stages through torch.distributed where its ranks have no RCCL communicator:
 *   bhip_device_copy moves a region between a device array and host memory).
 * bhip_build_accelerator_shared with n_parts = 1 builds alone (share may be NULL).  All ranks must call it together. */
typedef int (*bhip_share_fn)(void *ctx, void *device_base, const uint64_t *byte_off, int part, int n_parts, int status);
typedef struct { void *comm; int rank; } BhipCommRank;
BHIP_API int  bhip_build_accelerator_shared(void *handle, int K, int part, int n_parts, bhip_share_fn share, void *ctx);
BHIP_API int  bhip_comm_share(void *comm_rank, void *device_base, const uint64_t *byte_off, int part, int n_parts, int status);
BHIP_API int  bhip_team_create(int n_ranks, void **team);
BHIP_API void bhip_team_destroy(void *team);
BHIP_API int  bhip_team_share(void *team, void *device_base, const uint64_t *byte_off, int part, int n_parts, int status);
BHIP_API int  bhip_device_copy(void *dst, const void *src, uint64_t bytes, int to_device);      /* (device addresses are unified: whichever device the calling thread is on) */

/* The accelerator of a handle in the file's terms (read_accelerator's tables, burst.c:3535-3594): Lens[4^K], the clump ids of all
 * lists in word order (ascending inside a list, as the reference writes them with one thread), their 16-bit lane masks (device
 * layout only: bit z = lane z of the clump MAY hold the word -- since the 4-byte records of ABI 5 the device keeps a lane-set CODE
 * per entry, and the mask returned here is decode(code): the exact set for one or two lanes, the smallest enclosing quad pattern
 * beyond (csrc/bhip_lanecode.h); a superset never loses a lane), the BadList.  For a handle whose accelerator was built on the device
 * this is what make_accelerator (burst.c:3304-3532) would have written.  Any output pointer may be NULL. */
BHIP_API int bhip_acx_export(void *handle, uint32_t *lens, uint32_t *clumps, uint16_t *masks, uint64_t cap_entries, uint64_t *n_entries,
                    uint32_t *badlist, uint32_t cap_bad, uint32_t *n_bad);
/* The same lists piece by piece: entries [first, first + n_entries) in word order (a RefSeq-scale accelerator has tens of billions of
 * entries: a caller that writes the .acx streams them instead of holding 4 bytes of each); masks may be NULL. */
BHIP_API int bhip_acx_export_entries(void *handle, uint64_t first, uint64_t n_entries, uint32_t *clumps, uint16_t *masks);

/* Kernel-level entry (what one aded_mat16 call returns, burst.c:1078-1094): for explicit (query, clump)
 * pairs, mins[16*p + z] = edit distance of lane z (255 when > budget of the pair's query). */
BHIP_API int bhip_align_pairs(void *handle, const uint8_t *q_codes, const uint64_t *q_off, const uint16_t *q_emac,
                     uint32_t n_q, const uint32_t *pair_q, const uint32_t *pair_clump, uint64_t n_pairs,
                     uint8_t *mins);

/* Kernel-level entry for the prefilter alone: candidate (query, clump, count) triples with
 * count > max(len-(E+1)K, 0) (burst.c:4091-4092, 4126), BadList clumps not included.
 * Output sorted by (q, clump).  On BHIP_E_CAPACITY *n_out is the number required. */
BHIP_API int bhip_prefilter(void *handle, const uint8_t *q_codes, const uint64_t *q_off, const uint16_t *q_emac,
                   uint32_t n_q, uint32_t *out_q, uint32_t *out_clump, uint32_t *out_count,
                   uint64_t cap, uint64_t *n_out);

/* The records of the last bhip_align_staged / bhip_align_batch call stay resident on the device (same order as the host
 * copy; `hits` may be NULL there to skip the host copy altogether).  This copies them into caller-owned DEVICE memory,
 * e.g. the send buffer of an RCCL gather (no reference counterpart: multi-GPU).  Synchronous. */
BHIP_API int bhip_copy_hits_device(void *handle, void *dst_device, uint64_t cap_records, uint64_t *n_records);

/* With option "async_d2h" = 1 the records of bhip_align_staged / bhip_align_batch reach the caller's buffer BEHIND the call:
 * *n_hits is final at return, the bytes are not until bhip_sync_hits() (or bhip_destroy).  The copy of call k then
 * overlaps the kernels of call k+1; callers alternate between two result buffers (the library page-locks them once).
 * No reference counterpart (the reference appends ResultPods in place, burst.c:4230-4238). */
BHIP_API int bhip_sync_hits(void *handle);

/* Query ingest: sort n records of symbol codes (record r = codes[start[r] .. start[r] + len[r]), codes 0..15) in the order
 * of the reference's query sort -- byte-wise over the common length, the shorter record first, equal records in input order
 * (burst.c:363-366, 636-690) -- and mark the first record of every run of identical ones (the uniqueness pass of
 * burst.c:3036-3053).  perm[i] = input number of the i-th record in sorted order, is_new[i] = 1 iff it differs from the
 * (i-1)-th.  A device-side LSD radix sort over 16-symbol keys; needs no handle (it runs before the database is uploaded) and
 * about codes_bytes + 40 n bytes of device memory for the duration of the call.  max_len >= every len[r]. */
BHIP_API int bhip_sort_queries(int device, const uint8_t *codes, uint64_t codes_bytes, const uint64_t *start, const uint32_t *len,
                      uint64_t n, uint32_t max_len, uint32_t *perm, uint8_t *is_new);

/* Duplicate marks of the compressive database build (-d DNA, the reference's process_references DNA_16 branch, burst.c:1899-2023)
 * for one partition, on the device; needs no handle.  sym = the partition's symbol codes (one byte each, 0..15), sym_len bytes from
 * the first reference's first symbol to the last one's end; reference r covers [ref_start[r], ref_start[r] + ref_len[r]) of it
 * (ascending).  W = shear + overlap >= 24.  Every position j < ref_len - W whose first 13 symbols are A/C/G/T is binned by that
 * 13-mer; classes of equal symbols [13, 24) and of equal windows [13, W) inside a bin give the two convs, and flags[p] (one byte
 * per position of [0, sym_len), written in full) = their OR.  *max_chain / *max_sh are the reference's state across partitions:
 * when both are 0 on entry this partition's tally sets them.  BHIP_E_ARG when a duplicate window meets max_chain == 0 (where the
 * reference divides by zero), BHIP_E_DEVICE when there is no usable device.  info (may be NULL): [0] eligible positions, [1]
 * chunks of bins, [2] chunks that a hash collision sent down the exact path, [3] peak device bytes, [4..7] microseconds of
 * upload, sort, classification and marking. */
BHIP_API int bhip_dna_marks(int device, const uint8_t *sym, uint64_t sym_len, const uint64_t *ref_start, const uint32_t *ref_len,
                            uint64_t n_refs, uint32_t W, uint64_t *max_chain, uint64_t *max_sh, uint8_t *flags, uint64_t *info);

/* Coverage of the printed placements per reference header and sample (burst_hip --coverage; no reference counterpart on the device: what
 * embalmlets/bcov.c and embalmulate.c compute from the .b6 text with two counters per reference POSITION).  A line covers the half-open
 * range [max(lo - 1 - pad, 0), min(hi - 1 + pad, length)) of its header, lo / hi = the smaller / larger of st and ed; the depth of a
 * position is the summed weight of the lines that cover it.  Per header and column the library returns four 64-bit integers:
 * tot = sum of the depths, cov = positions with depth != 0, sq = sum of the squared depths, lines = summed weight of the lines (those with
 * an empty range included).  Two columns each time: "shared" over all lines, "unique" over those with bit 31 of `w` set.  The device
 * works from two sorted events per line, never from per-position arrays (csrc/bhip_cov.hip): the cost follows the lines.
 *   bhip_cov_begin        n_headers lengths (copied) and the pad; replaces a coverage that was open on the handle
 *   bhip_cov_add          ONE WHOLE sample: its lines (header < n_headers).  A sample index can be added once; indices need not be dense
 *   bhip_cov_sample_stats shared / unique [n_headers][4] = tot, cov, sq, lines of that sample (either may be NULL); all zero for an index
 *                         that was never added
 *   bhip_cov_dataset_stats the same over the events of ALL samples added so far (the depths of the samples summed)
 *   bhip_cov_info         [0] events resident, [1] peak bytes of the event sets, [2] compactions so far, [3] the cap in bytes, [4] device
 *                         microseconds of the last bhip_cov_add's sorts, scans and statistics kernels (HIP events), [5] events per block of
 *                         the statistics kernel, [6] the sum of [4] over all calls, [7] samples added
 *   bhip_cov_end          releases everything (bhip_destroy does it too)
 * Option "cov_event_cap" (bytes, default 0 = a fifth of the device memory free at the first bhip_cov_add): beyond it the event sets are
 * compacted (equal keys summed, zeros dropped); BHIP_E_DEVICE only if the compacted sets still do not fit.
 * bhip_lane_extents: extents[16 * clump + lane] = index after the lane's last symbol that is not the pad code 0 (0 for an empty lane), for
 * all 16 * n_clumps lanes of the resident database -- the reference lengths a caller derives without walking the packed references. */
typedef struct BhipCovLine { uint32_t ref, st, ed, w; } BhipCovLine;      /* header, .b6 columns 9 and 10, weight (bits 0..30) | unique << 31 */
BHIP_API int bhip_cov_begin(void *handle, uint32_t n_headers, const uint32_t *lengths, uint32_t pad);
BHIP_API int bhip_cov_add(void *handle, uint32_t sample, const BhipCovLine *lines, uint64_t n);
BHIP_API int bhip_cov_sample_stats(void *handle, uint32_t sample, uint64_t *shared, uint64_t *unique);
BHIP_API int bhip_cov_dataset_stats(void *handle, uint64_t *shared, uint64_t *unique);
BHIP_API int bhip_cov_info(void *handle, uint64_t info[8]);
BHIP_API int bhip_cov_end(void *handle);
BHIP_API int bhip_lane_extents(void *handle, uint32_t *extents);

/* The alignment PATH of placements (burst_hip --cigar; no reference counterpart: the reference reports how many mismatches and gaps a
 * placement has, never where).  A request names a record of the search: query entry q of the caller's batch (q_codes / q_off as in
 * bhip_align_batch), refIx, finalPos and ed as in BhipHit.  The path is the one the re-scorer's own recurrence (reScoreM_mat16,
 * burst.c:713-886) decides: every cell of its matrix has a decision -- row 1: L if the cell's cost is 1 and the cell to its left scored 0
 * (burst.c:722-739), else D; column 0: U; elsewhere D if the diagonal is kept (burst.c:771-779), U if it is not, L if the second comparison
 * fails (789-795) -- and the path follows the decisions from cell (m, finalPos), which must score ed, back to row 0.  Read forwards:
 * D with cost 0 is '=', D with cost 1 is 'X', U is 'I' (a query symbol without a reference column), L is 'D' (a reference column without
 * a query symbol).  By construction '=' + X + I = the query's length, X + I + D = ed, D = the record's gapQ, and I = V of the FINAL cell --
 * which is the record's gapR whenever the best (score, H) of the last row is attained in one end column only, and may differ otherwise
 * (the reference takes gapR from the first such column and finalPos from the last, burst.c:824-885).
 *   ops       32-bit words length << 4 | code with BAM's codes (I = 1, D = 2, '=' = 7, X = 8), runs merged, in forward order; request i
 *             owns ops[op_off[i] .. op_off[i + 1]); op_off has n_requests + 1 entries
 *   ref_first [i] = the first reference column the path consumes, 1-based in the sheared lane (the column after the one where row 0 is reached)
 *   gap_r     [i] = the path's number of I
 * BHIP_E_ARG (before any device memory is touched) when a request names a query >= n_queries, a reference >= 16 n_clumps or >= tot_refs,
 * an end column outside 1 .. ClumpLen, a query of 0 or more than BHIP_MAX_QLEN symbols, or ed > 254; BHIP_E_CAPACITY when ops_cap is too small
 * (op_off is complete: op_off[n_requests] is the count needed; ref_first and gap_r are valid, ops is not); BHIP_E_RESCORE when cell
 * (m, finalPos) of a request does not score ed -- bhip_last_error names the first such request.  Query symbols are uploaded per call in
 * chunks of bounded size; the references are the resident ones.
 * bhip_paths_info: [0] device microseconds of the last bhip_trace_paths call (HIP events around its kernels), [1] of all calls, [2] requests
 * and [3] ops of all calls that returned BHIP_OK or BHIP_E_CAPACITY. */
typedef struct BhipPathReq { uint32_t q, refIx, finalPos, ed; } BhipPathReq;
#define BHIP_OP_I  1u
#define BHIP_OP_D  2u
#define BHIP_OP_EQ 7u
#define BHIP_OP_X  8u
BHIP_API int bhip_trace_paths(void *handle, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries, const BhipPathReq *requests, uint64_t n_requests,
                              uint32_t *ops, uint64_t ops_cap, uint64_t *op_off, uint32_t *ref_first, uint32_t *gap_r);
BHIP_API int bhip_paths_info(void *handle, uint64_t info[4]);

/* Paired-end reads: the join of two mates' printed placements into concordant combinations (burst_hip --mates; no reference counterpart:
 * the reference lists paired-end alignment as planned and names the recipe -- both mates in ALLPATHS mode, then the references both map to
 * with acceptable orientation and distance).  A line is one placement as the .b6 prints it: `pair` = the pair its read belongs to and `ref` =
 * its header, both DENSE numbers the caller assigns (equal numbers = equal names / byte-equal headers), st / ed = columns 9 and 10 as signed
 * numbers, edits = column 11.  A line is reverse when st > ed; lo / hi = the smaller / larger of st and ed.  A combination is a line of `a`
 * (mate 1) and a line of `b` (mate 2) with equal pair and ref; with U the upstream and D the downstream line --
 *   BHIP_MATES_FR  exactly one of the two is reverse, U = the forward one;   BHIP_MATES_RF  the same with U = the reverse one;
 *   BHIP_MATES_FF  both forward (U = the line of a) or both reverse (U = the line of b)
 * -- it is concordant when U.lo <= D.lo, U.hi <= D.hi and ins_min <= D.hi - U.lo + 1 <= ins_max.  BHIP_MATES_ALL reports every concordant
 * combination, BHIP_MATES_BEST one per pair: the smallest edits sum (saturating at 2^32 - 1), then the smallest index in a, then in b.
 * out_a[i], out_b[i] index the caller's arrays, in ascending (a, b) order; *n_out = their number.  BHIP_E_CAPACITY when cap is too small:
 * *n_out is the number wanted, nothing is written, the handle stays usable.  BHIP_E_ARG, before any device memory is touched, for an
 * orientation or report outside the values above, ins_min > ins_max, na or nb >= 2^32, and (BHIP_MATES_BEST, which keeps a table indexed
 * by pair) a pair number of `a` beyond 4 (na + nb) + 2^20.  na == 0 or nb == 0: no combinations, no launch.  Device side: csrc/bhip_mates.hip.
 * bhip_mates_info: [0] device microseconds of the last bhip_mates_join call that launched (HIP events around its kernels, sort and scan),
 * [1] of all calls, [2] lines taken in and [3] combinations returned by all calls that returned BHIP_OK. */
typedef struct BhipMateLine { uint32_t pair, ref; int32_t st, ed; uint32_t edits; } BhipMateLine;
#define BHIP_MATES_FR   0u
#define BHIP_MATES_RF   1u
#define BHIP_MATES_FF   2u
#define BHIP_MATES_ALL  0u
#define BHIP_MATES_BEST 1u
BHIP_API int bhip_mates_join(void *handle, const BhipMateLine *a, uint64_t na, const BhipMateLine *b, uint64_t nb,
                             uint32_t orientation, uint32_t ins_min, uint32_t ins_max, uint32_t report,
                             uint32_t *out_a, uint32_t *out_b, uint64_t cap, uint64_t *n_out);
BHIP_API int bhip_mates_info(void *handle, uint64_t info[4]);

/* Abundance: the reads of multi-mapped lines split over their references by expectation-maximisation (burst_hip --abundance; no reference
 * counterpart: its README leaves "EM interpolation" of ALLPATHS output to the user and its COMMUNIST mode is a stub).  The input is what a
 * sample prints: groups g (a group = the reads that print exactly these lines) of weight group_w[g] reads, and lines (group, ref).  The
 * candidate set S_g is the set of DISTINCT ref among the lines of g; a group without a line or of weight 0 takes no part.  With
 * ONE = 2^30, c0[h] = ONE for every header, and per iteration t >= 1, starting from ct[h] = 0, every participating group adds, with
 * d = the integer sum of c(t-1) over S_g and q_h = (uint64) floor(((double)c(t-1)[h] / (double)d) * 1073741824.0) (one IEEE division):
 * W_g q_h to ct[h] for each h of S_g, and W_g (ONE - sum of the q_h) to the candidate with the largest c(t-1), the lowest header among equals.
 * delta_t = the largest |ct[h] - c(t-1)[h]| over all headers; the loop ends after the first t with delta_t <= tol or after max_iters.
 * Everything but the division is 64-bit integer addition, which commutes: the result is bit-exact whatever the order.
 *   counts  [n_headers], units of 2^-30 read; their sum is ONE x the reads of the participating groups
 *   info    [0] iterations run, [1] distinct (group, ref) pairs of participating groups, [2] classes (groups of equal candidate set are
 *           merged into one class of summed weight: equal to the number of distinct sets, larger only under option "em_weak_hash"),
 *           [3] the last delta, [4] 1 if the loop ended on tol, [5] device microseconds (HIP events around everything launched), [6] peak
 *           device bytes, [7] 0
 * No participating group: all counts 0, 0 iterations, nothing is launched.  BHIP_E_ARG with a text, the handle staying usable, for a
 * ref >= n_headers, a group >= n_groups, summed weights beyond 2^31 - 1, n_lines >= 2^31 and max_iters = 0.  The call leaves nothing
 * resident but scratch buffers of the handle, which bhip_destroy frees.  Option "em_weak_hash": 1 = the candidate sets are hashed to two
 * bits, so that the element-by-element comparison decides which groups merge (tests); no count changes.  Device side: csrc/bhip_em.hip. */
typedef struct BhipEmLine { uint32_t group, ref; } BhipEmLine;
BHIP_API int bhip_em_run(void *handle, uint32_t n_headers, uint32_t n_groups, const uint32_t *group_w, const BhipEmLine *lines, uint64_t n_lines,
                         uint32_t max_iters, uint64_t tol, uint64_t *counts /* [n_headers], units of 2^-30 read */, uint64_t info[8]);

/* Taxon tables: every group of reads goes to the lowest common ancestor of the taxonomies of the references it was placed on (burst_hip
 * --taxa; the reference's embalmulate.c counts column 13 of BEST output, and its README leaves the tied references of ALLPATHS output to
 * the user).  Everything is in integers and bit-exact on any machine.
 *   tree        n_nodes nodes numbered in PREORDER: parent[0] = 0 is the root (depth 0); for v > 0, parent[v] < v and parent[v] is v - 1 or
 *               one of its ancestors, so that a subtree is a contiguous range of numbers.  The order of siblings is free and no result
 *               depends on it.  At most 64 levels below the root.  header_node[h] < n_nodes is the node of header h (0: no taxonomy).
 *   groups      as bhip_em_run: group g stands for group_w[g] reads, its candidates are the DISTINCT ref among its lines (both strands and
 *               all placements of one header are one candidate), n of them.  A group of weight 0 has a taxon and adds nothing.
 *   taxon       t = (agree * n + 999) / 1000, agree in 501 .. 1000 permille (1000: the strict lowest common ancestor).  The group's taxon is
 *               the deepest node whose subtree holds the nodes of at least t candidates.  It is unique: two nodes of one depth have
 *               disjoint subtrees and t > n / 2.  A candidate at the root sends the group to the root when agree = 1000.
 *   counts      own[v] = the sum of group_w over the groups whose taxon is v; clade[v] = the sum of own over the subtree of v (sums modulo
 *               2^64); a group without lines counts nowhere; clade[0] = the reads of the groups with lines.
 *   group_node  NULL, or [n_groups]: every group's taxon, 0xFFFFFFFF for a group without lines
 *   info        [0] distinct (group, ref) pairs, [1] groups with lines, [2] their reads, [3] reads at the root = own[0], [4] the deepest level
 *               of a group's taxon, [5] device microseconds (HIP events around everything launched), [6] peak device bytes, [7] 0
 * bhip_taxa_rollup sums counts given per header (the abundance's, units of 2^-30 read) the same way: own[v] = the sum of header_count over
 * the headers with header_node = v, clade = its subtree sums.
 * No line: zeros, nothing is launched.  BHIP_E_ARG with a text, never a device fault, the handle staying usable: parent[0] != 0, a parent
 * that breaks the preorder property, a node more than 64 levels deep, a header_node >= n_nodes, a line's ref >= n_headers or group >=
 * n_groups, agree outside 501 .. 1000, n_lines >= 2^31.  The calls leave nothing resident but scratch buffers of the handle, which
 * bhip_destroy frees.  Device side: csrc/bhip_taxa.hip. */
BHIP_API int bhip_taxa_run(void *handle, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node, uint32_t n_groups,
                           const uint32_t *group_w, const BhipEmLine *lines, uint64_t n_lines, uint32_t agree,
                           uint32_t *group_node /* may be NULL; 0xFFFFFFFF = no lines */, uint64_t *own, uint64_t *clade, uint64_t info[8]);
BHIP_API int bhip_taxa_rollup(void *handle, uint32_t n_nodes, const uint32_t *parent, uint32_t n_headers, const uint32_t *header_node,
                              const uint64_t *header_count, uint64_t *own, uint64_t *clade);

/* Variant sites: which bases one sample's reads show at a reference position, and where they differ from the reference (burst_hip
 * --variants; no reference counterpart).  The result is a function of the sample's printed lines.  A LINE is a path as bhip_trace_paths
 * returns it -- query entry q of q_codes / q_off, lane refIx, first lane column ref_first, ops[op_off .. op_off + n_ops) -- placed on the
 * reference the caller numbers `header`, at 1-based position `pos` (the position of lane column ref_first), standing for `w` reads.
 * Symbol codes .ACGTNKMRYSWBVHD = 0..15: codes 1..4 are the classes A, C, G, T, every other code is the class Other, Del is a class of its
 * own.  Walk the ops forwards with reference position p = pos and query index j = 0:
 *   '=' or X, per symbol   one OBSERVATION (header, p, class of query[j]); p++, j++
 *   D, per column          one observation (header, p, Del); p++
 *   I run of n             j += n, and one INSERTION MARK (header, p - 1) unless the run is the first or the last op of the path (a run at
 *                          an end is what a local aligner would clip)
 * A SITE is (header, position); observations and marks count w per line.  A, C, G, T, Del, Other = its observations per class, Depth = their
 * sum, Ins = its marks (not part of Depth), Ref = the code of the lane column the observing paths consumed there.  The lanes of a database
 * that share a position of a header are cuts of one original sequence and agree there; the smallest code is taken, so that no order matters
 * (the device takes it among the observations that are not plain, see below, and counts the plain ones as Ref: for lanes that agree the two
 * are the same).  A site is RETURNED when Ref is 1..4, Depth >= min_depth, and Depth - count[Ref] >= min_alt or Ins >= min_alt; sites come
 * back in ascending (header, pos) order, n[] = A, C, G, T, Del, Other.  No pooling over samples, no indel alleles, no genotypes.
 * The cost follows the lines and their edits, never lines x read length: an observation is PLAIN when its op is '=' and its query code is
 * 1..4; only the others and the marks become events, which are sorted and reduced to candidate sites; the depth of a candidate is the
 * weight of the lines whose range [pos, pos + ('=' + X + D) - 1] holds it, from two sorted arrays (starts, one-past-ends) with running
 * weight sums and two binary searches, and the plain observations are depth minus the others (csrc/bhip_pile.hip).
 * All sums are 64-bit integers: bit-exact whatever the order of threads or lines.
 * BHIP_E_CAPACITY when cap is too small: *n_sites is the number wanted, nothing is written, the handle stays usable.  n_lines == 0: no
 * sites, nothing is launched.  BHIP_E_ARG with a text, before any device memory is touched and with the handle staying usable, for a line
 * whose query is >= n_queries, whose lane is >= 16 n_clumps or >= tot_refs, whose ops leave `ops`, hold a word that is not a run of I / D /
 * '=' / X of length >= 1 or repeat the code of the op before (runs are merged), consume ('=' + X + I) another number of symbols than the
 * query has, or leave the columns 1 .. ClumpLen; for pos == 0 or pos + ('=' + X + D) > 2^32 - 1, w == 0, summed weights beyond 2^31 - 1,
 * and min_depth == 0 or min_alt == 0.
 * info (may be NULL): [0] events, [1] candidate sites, [2] sites returned, [3] device microseconds (HIP events around everything launched),
 * [4] peak device bytes of the call's scratch buffers (the handle keeps them; bhip_destroy frees them), [5..7] 0. */
typedef struct BhipPileLine { uint32_t q, refIx, ref_first, header, pos, w; uint32_t n_ops; uint64_t op_off; } BhipPileLine;
typedef struct BhipPileSite { uint32_t header, pos, ref, depth, n[6] /* A C G T Del Other */, ins; } BhipPileSite;
BHIP_API int bhip_pile_run(void *handle, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries,
                           const BhipPileLine *lines, uint64_t n_lines, const uint32_t *ops, uint64_t n_ops,
                           uint32_t min_depth, uint32_t min_alt, BhipPileSite *sites, uint64_t cap, uint64_t *n_sites, uint64_t info[8]);

/* Consensus: the sequence one sample's reads show on every reference position they cover (burst_hip --consensus; no reference counterpart:
 * the definition is this project's own).  A function of the sample's printed lines, all integer arithmetic, bit-exact on any machine.
 * Lines, observations, classes, Depth, the counts A C G T Del Other, Ins and Ref are exactly those of "Variant sites" above (a reverse line
 * carries the path of its reverse-complement entry, so letters are forward-strand; a duplicate read is a line of its own).
 *   COVERED   a position of a header with Depth >= 1.  A SEGMENT is a maximal run of consecutive covered positions of one header: a line
 *             that ends at p and one that starts at p + 1 are one segment, a gap of one position makes two.
 *   CALL      at a covered position, m = min_depth (policy, not a measurement):
 *             1. Depth < m: the letter is N (not called).
 *             2. else, Ref not A/C/G/T: the reference's own letter, "NACGTNKMRYSWBVHD"[Ref] (AMBIGUOUS; plain observations on such a
 *                column carry no class the device keeps, and the variants never report these sites either).
 *             3. else the largest of the five counts A, C, G, T, Del; among equal largest counts the class of Ref if it is one of them,
 *                otherwise the first in that order.  Other is part of Depth and never wins.  The letter is A/C/G/T, or '-' for Del.
 *   FIGURES   per segment: called = positions with Depth >= m; same, subst, del = rule-3 positions whose letter equals Ref, is another base,
 *             is '-'; ambig = rule-2 positions; ins_major = called positions with 2 * Ins > Depth (most reads insert behind the column,
 *             which a record in reference coordinates cannot show).  called = same + subst + del + ambig.
 * Segments come back in ascending (header, pos) order; segment s owns letters[off .. off + len), and the offsets are the running sum of
 * the lengths.  The cost follows lines + events + covered positions (csrc/bhip_consensus.hip): events and candidate
 * sites as the variants take them; the segments from a max-scan of the one-past-ends in start order; the depth of every covered position
 * as the stabbing count of two sorted arrays, with cursors that move forwards along a thread's run of positions; the reference code from
 * the lane column of one covering line (lanes that share a position agree there; the definition says the smallest code, the device takes
 * any covering lane's); the candidate sites then replace their letters.  The figures are integer sums: no order of threads matters.
 * The inputs and the BHIP_E_ARG checks are those of bhip_pile_run, before any device memory is touched and with the handle staying usable;
 * also for min_depth == 0 or > 2^31 - 1, and for more than 2^31 - 1 covered positions in one call (never a truncated result).
 * BHIP_E_CAPACITY when seg_cap or letter_cap is too small: *n_segs and *n_letters are the numbers wanted, nothing is written, the handle
 * stays usable.  n_lines == 0: no segments, nothing is launched.
 * info (may be NULL; bhip_consensus_info returns that of the last call on the handle): [0] events, [1] candidate sites, [2] segments, [3]
 * covered positions, [4] device microseconds (HIP events around everything launched), [5] peak device bytes of the scratch buffers (shared
 * with bhip_pile_run; the handle keeps them, bhip_destroy frees them), [6..7] 0. */
typedef struct BhipConsSeg { uint32_t header, pos, len, called, same, subst, del, ambig, ins_major, pad; uint64_t off; } BhipConsSeg;
BHIP_API int bhip_consensus_run(void *handle, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries,
                                const BhipPileLine *lines, uint64_t n_lines, const uint32_t *ops, uint64_t n_ops, uint32_t min_depth,
                                BhipConsSeg *segs, uint64_t seg_cap, uint64_t *n_segs, char *letters, uint64_t letter_cap, uint64_t *n_letters,
                                uint64_t info[8]);
BHIP_API int bhip_consensus_info(void *handle, uint64_t info[8]);

/* Consensus pairs: for every reference and every two samples, on how many positions both consensus rows show a call and on how many of
 * those they agree (burst_hip --consensus --consensus-pairs; no reference counterpart).  A pure function of the written
 * PREFIXconsensus.fa, all integer arithmetic, bit-exact on any machine.
 *   PARTICIPANT   a (sample, header) whose record --consensus writes (Called >= 1 and the --consensus-min-breadth test passes).  Its ROW
 *                 is the record's L letters: the letters bhip_consensus_run returned inside the segments, N everywhere else.
 *   COMPARABLE    a position of a row whose byte is one of A C G T - (rule 3 of the call).  N is not comparable, and neither are the
 *                 ambiguity letters of rule 2: both samples would show the reference's own letter there, which says nothing.
 *   FIGURES       for samples a < b (study order) that both take part on header h: Compared = the positions comparable in both rows, Same =
 *                 those of them with equal bytes ('-' against '-' is equal, '-' against a base is not), Differ = Compared - Same.
 *   PAIR ROW      exists when Compared >= M = --consensus-pairs-min (1 .. 2^31 - 1, default 1; policy, not a measurement).
 *   FILES         PREFIXconsensus_pairs.txt: `#Reference SampleA SampleB Length Compared Same Differ Identity` (tabs), rows in strcmp order
 *                 of the whole header, then a, then b; Identity = %.6f of (double)Same / (double)Compared.  PREFIXconsensus_identity.txt:
 *                 `#Identity` and the samples' names (those of the coverage tables), a row per sample; cell (a, b), a != b, = %.6f of
 *                 sum Same / sum Compared (64-bit sums) over the pair's rows in the pairs file, NA when it has none; the diagonal is
 *                 1.000000.  PREFIXconsensus_compared.txt: the same shape with the integer sum Compared (0 where the other has NA); its
 *                 diagonal is the number of comparable positions of the sample's records.  Both are symmetric.  A sample that failed alone
 *                 takes part nowhere: its whole row and column, the diagonal included, read NA in both matrices.
 * THE PRIMITIVE.  segs: strictly ascending by (sample, header, pos), within a (sample, header) pos >= the previous pos + len, pos >= 1,
 * len >= 1; segment s owns letters[off .. off + len); `header` is any number that orders the headers (the consensus's header numbers are
 * their places in strcmp order).  pairs: ascending (header, a, b), only those with compared >= min_compared.
 * The cost follows segments + covered positions + participating pairs x the words of their header's union, never a reference's length
 * (csrc/bhip_conspairs.hip): per header the union of all samples' segments gives a compressed axis; every (sample,
 * header) gets three code planes of 64-bit words over it; a workgroup owns a tile of sample pairs of one header, stages the tile's rows
 * through LDS and counts with popcounts; the selection is by key.  Integer sums only: no order of threads, and no budget, changes a byte.
 * Option "conspairs_bytes" (bhip_set_option; default 1 GiB, a stated policy) bounds the plane buffer: headers are processed in groups
 * that fit; a header too large alone goes in consecutive slabs of words while its pair cells stay resident (a value below one word of
 * every row of a header, 24 bytes x its samples, acts as that).  Copies of the input and the pair cells of a group are beside it.
 * BHIP_E_ARG with a text, before any device memory is touched and with the handle staying usable: segments out of order or overlapping,
 * pos == 0, len == 0, pos + len > 2^32 - 1, off + len beyond n_letters, sample >= n_samples, n_samples > 65535 (policy), min_compared == 0
 * or > 2^31 - 1, 2^32 or more segments.  (pos + len <= 2^32 - 1 is one position short of what --consensus itself takes: a record
 * called through position 2^32 - 1 is refused by the run with a usage message when it is handed over.)  n_samples < 2 or n_segs == 0: nothing is launched, no pairs.  BHIP_E_CAPACITY when pair_cap is
 * too small: *n_pairs is the number wanted, nothing is written, the handle stays usable (the sum of m (m - 1) / 2 over the headers with m
 * participants always suffices).
 * info (may be NULL; bhip_consensus_pairs_info returns that of the last call on the handle): [0] segments, [1] headers with at least two
 * samples, [2] union positions of those headers, [3] pairs examined, [4] pairs returned, [5] device microseconds (HIP events around
 * everything launched), [6] peak device bytes of the scratch buffers (the handle keeps them; bhip_destroy frees them), [7] 0. */
typedef struct BhipPairSeg { uint32_t sample, header, pos, len; uint64_t off; } BhipPairSeg;
typedef struct BhipPair    { uint32_t header, a, b, pad; uint32_t compared, same; } BhipPair;
BHIP_API int bhip_consensus_pairs(void *handle, uint32_t n_samples, const BhipPairSeg *segs, uint64_t n_segs, const char *letters,
                                  uint64_t n_letters, uint32_t min_compared, BhipPair *pairs, uint64_t pair_cap, uint64_t *n_pairs,
                                  uint64_t info[8]);
BHIP_API int bhip_consensus_pairs_info(void *handle, uint64_t info[8]);

/* Indel alleles: which bases one sample's reads insert behind a reference position, and which reference columns they delete there
 * (burst_hip --vcf; no reference counterpart: the definition is this project's own).  A function of the sample's printed lines, all
 * integer arithmetic, bit-exact on any machine.  Lines, the walk (reference position p, query index j), observations, Depth, Ref and the
 * meaning of the weights are exactly those of "Variant sites" above (a reverse line carries the path of its reverse-complement entry, so
 * alleles are forward-strand; a duplicate read is a line of its own).
 *   ALLELE RUN  an I or D run (ops are merged runs) whose directly preceding op is '=' or X and which is not the last op of its path.  Its
 *               ANCHOR is (header, p - 1), the column the preceding op consumed: every line that carries an allele observes its anchor, so
 *               count <= Depth(anchor) always.  A run that is the first or the last op (END) or stands directly behind the other indel kind
 *               (ADJACENT, ...3D2I...) is no allele; it still counts in the site's Ins / Del of the variant sites, and is counted as skipped,
 *               END before ADJACENT.
 *   Del(n)      a D allele run of n columns.
 *   Ins(c1..cn) an I allele run of n query symbols, 1 <= n <= 15: the stored query codes j .. j + n - 1, 0 .. 15 each.  A run of more than 15
 *               symbols is LONG: it gives no allele and is counted.  The limit is policy: an allele is then ONE 64-bit word (4 bits of
 *               length, 60 of codes) and stays an exact sort key, nothing is hashed.
 *   WORD        Del(n): n (top 4 bits 0).  Ins: n << 60 | c1 << 56 | c2 << 52 | ...  Plain integer order of the words is the order below.
 *   COUNT       of (anchor, allele): the sum of w over the lines that carry it.
 *   RETURNED    when Depth(anchor) >= min_depth and count >= min_alt, whatever the anchor's reference code; 1 .. 2^31 - 1 each.
 *   ORDER       ascending (header, pos), then Del before Ins, Del by n, Ins by n, then by c1..cn lexicographically.
 * A returned allele carries the anchor's reference code (ref) and Depth(anchor); a Del(n) also owns the n reference codes of the columns
 * p .. p + n - 1, codes[code_off .. code_off + n) (one byte per code; code_off is the running sum of the n of the returned Dels before it, for an
 * Ins as well, which owns no codes).  Lanes that share header positions agree there, so the codes are read from ONE carrying line (the one of the smallest index).
 * The cost follows lines + allele events (csrc/bhip_alleles.hip): the events are sorted by (anchor, word) in two
 * stable radix passes and reduced by key -- a pile-up of any depth on one allele is reduced in parallel --, Depth(anchor) is the stabbing
 * count of the variant sites.  All sums are 64-bit integers and every choice a minimum: no order of threads, and no order of the lines,
 * changes a byte.
 * The inputs and the BHIP_E_ARG checks are those of bhip_pile_run, before any device memory is touched and with the handle staying usable;
 * also for a threshold of 0 or above 2^31 - 1, and for more than 2^31 - 1 allele events in one call.  BHIP_E_CAPACITY when cap or code_cap
 * is too small: *n_alleles and *n_codes are the numbers wanted, nothing is written, the handle stays usable.  n_lines == 0: nothing is
 * launched.
 * info (may be NULL; bhip_alleles_info returns that of the last call on the handle): [0] allele events, [1] distinct alleles, [2] returned
 * alleles, [3] skipped END runs, [4] skipped ADJACENT runs, [5] skipped LONG runs, [6] device microseconds (HIP events around everything
 * launched), [7] peak device bytes of the scratch buffers (those of bhip_pile_run included; bhip_destroy frees them). */
typedef struct BhipAllele { uint32_t header, pos; uint64_t allele; uint32_t ref, depth, count, pad; uint64_t code_off; } BhipAllele;
BHIP_API int bhip_alleles_run(void *handle, const uint8_t *q_codes, const uint64_t *q_off, uint32_t n_queries,
                              const BhipPileLine *lines, uint64_t n_lines, const uint32_t *ops, uint64_t n_ops,
                              uint32_t min_depth, uint32_t min_alt, BhipAllele *alleles, uint64_t cap, uint64_t *n_alleles,
                              uint8_t *codes, uint64_t code_cap, uint64_t *n_codes, uint64_t info[8]);
BHIP_API int bhip_alleles_info(void *handle, uint64_t info[8]);

/* Site counts: one sample's counts at records the caller names, the primitive of the study VCF (burst_hip --vcf-study; no reference
 * counterpart).  All integer arithmetic, a pure function of the samples' printed lines, bit-exact on any machine.
 * STUDY VCF.  Lines, observations, classes, Depth, the counts A C G T Del Other, Ref, allele runs, allele words and all / unique are exactly
 * those of "Variant sites" and "Indel alleles" above.  For sample s write Depth_s(h,p), n_s[b](h,p) and count_s(h,p,word): all 0 where the
 * sample observes nothing.  D = --vcf-min-depth, A = --vcf-min-alt.
 *   SNV record at (h,p)         exists when Ref(h,p) is A/C/G/T and some sample has Depth_s >= D and, for a base b != Ref, n_s[b] >= A.  ALT is
 *                               the set of bases b != Ref for which some sample satisfies both, in the order A C G T.
 *   Allele record (h,p,word)    exists when some sample has Depth_s(h,p) >= D and count_s(h,p,word) >= A.  REF and ALT letters as in OUT.vcf;
 *                               a Del's deleted letters come from a reporting sample (all agree: the database is the same).
 *   The study file has a record exactly when at least one sample's OUT.vcf has it; an SNV's ALT is the union of the reporting samples' ALTs.
 *   SAMPLE FIELDS (FORMAT DP:AD) for every sample at every record, with no threshold applied: SNV Depth_s:n_s[Ref],n_s[alt1],... (a
 *                               sample's plain observations count as Ref); indel Depth_s(anchor):Depth_s-count_s,count_s; a sample with no
 *                               read at the record prints explicit zeros (0:0,0); a sample that failed alone prints `.`.
 *   INFO DP=<sum of Depth_s>;NS=<samples with Depth_s >= 1>.  Records in header-number order, then by POS; at one POS the SNV first, then the
 *   alleles by word: the order of OUT.vcf.  No pooled call (a record that passes only on counts summed over samples), no genotypes.
 * THE PRIMITIVE.  bhip_pile_run and bhip_alleles_run at thresholds (1, 1) return everything a sample observes that is not plain; what is
 * missing is the depth of a sample where it observed nothing unusual.  A RANGE is a line of the sample: it covers [pos, pos + span - 1] of
 * `header` and stands for w reads; span = the '=' + X + D of its path and may be 0 (it then contributes nothing).  A RECORD with allele 0 is
 * a site record (ref in 1..4), any other is an allele record with that word.  cells[i], each standing alone (records need not be sorted or
 * distinct):
 *   depth   the summed w of the ranges that hold (header, pos)
 *   site    n[0..3] = those of the entry of `sites` at (header, pos); without one n[ref - 1] = depth, the others 0; count = 0
 *   allele  count = that of the entry of `alleles` with (header, pos, allele), or 0; n = 0
 * `sites`: the sample's bhip_pile_run(1, 1) result, ascending (header, pos); `alleles`: its bhip_alleles_run(1, 1) result in its order.
 * The cost follows ranges + records (csrc/bhip_sitecounts.hip): starts and one-past-ends sorted with running weight
 * sums, per record two binary searches for the depth (the stabbing count of the variant sites) and one into `sites` or, by the 128-bit key
 * (header << 32 | pos, allele), into `alleles`.  64-bit integer sums and exact look-ups: no order of threads or ranges changes a byte.
 * n_records == 0: nothing is launched.  n_ranges == 0: every depth is 0 and nothing is launched.  BHIP_E_ARG with a text, before any device
 * memory is touched and with the handle staying usable, for a range with pos == 0, w == 0 or pos + span > 2^32 - 1, summed weights beyond
 * 2^31 - 1, `sites` not strictly ascending, `alleles` not strictly ascending by (header, pos, allele), a record with pos == 0, a site
 * record with ref outside 1..4, and any count of 2^32 or more.
 * info (may be NULL; bhip_site_counts_info returns that of the last call on the handle): [0] ranges, [1] records, [2] device microseconds
 * (HIP events around everything launched), [3] peak device bytes of the scratch buffers (the handle keeps them; bhip_destroy frees them),
 * [4..7] 0. */
typedef struct BhipCountRange  { uint32_t header, pos, span, w; } BhipCountRange;
typedef struct BhipCountRecord { uint32_t header, pos; uint64_t allele; uint32_t ref, pad; } BhipCountRecord;
typedef struct BhipCountCell   { uint32_t depth, n[4], count; } BhipCountCell;
BHIP_API int bhip_site_counts(void *handle, const BhipCountRange *ranges, uint64_t n_ranges, const BhipPileSite *sites, uint64_t n_sites,
                              const BhipAllele *alleles, uint64_t n_alleles, const BhipCountRecord *records, uint64_t n_records,
                              BhipCountCell *cells, uint64_t info[8]);
BHIP_API int bhip_site_counts_info(void *handle, uint64_t info[8]);

/* Clustering: greedy centroid clusters of the reads of a query file from the lines it prints against itself (burst_hip --cluster; no
 * reference counterpart: its README lists clustering "as an output mode" as planned and names the recipe -- the queries as their own
 * references in FORAGE, then clusters picked from that hit graph).  All of it is integer arithmetic, bit-exact on any machine.
 *   NODES     0 .. n_nodes - 1: the reads of the -q file in file order; a node's name is column 1 as printed.
 *   WEIGHT    weights[node]: 1, or with --cluster-sizes the N of a trailing `;size=N` or `;size=N;` of the name (1 .. 2^32 - 1; a name
 *             without that suffix weighs 1).  Two reads with byte-equal names are a usage error that names them.
 *   EDGE      q -> r with `edits`: a printed line whose column 1 is read q and whose column 2 is byte-equal to the name of a read r != q;
 *             edits = the smallest column 11 over all such lines (both strands, several placements, several shears).  A line whose
 *             column 2 names no read is FOREIGN: ignored and counted.  A self line is ignored.  Edges are directed -- the aligner places
 *             the query end to end inside the reference, so q -> r does not imply r -> q: an edge reads "r can represent q".
 *   PRIORITY  q is before r when its weight is larger, or the weights are equal and its number is smaller.
 *   CLUSTERS  the reads in priority order: a read with an edge to a centroid that came before it is a MEMBER of the one with the smallest
 *             edits among those, the one that came first among equals; any other read is a CENTROID.  Edges towards reads of lower
 *             priority never matter; a read without lines is a centroid of its own.
 * bhip_cluster_run takes the edges raw -- duplicates, self edges and edges towards lower priority included; the device cleans them -- and
 * returns per node centroid_out = its centroid's node (itself for a centroid) and edits_out = the edits of the edge that joined it (0
 * for a centroid).  Fewer than 2^32 - 1 nodes and fewer than 2^32 edges.  BHIP_E_ARG with a text, before any device memory is touched
 * and with the handle staying usable, for an edge that names a node >= n_nodes.  n_edges == 0 launches nothing: every read is a centroid.
 * The greedy order is resolved in rounds over a sorted adjacency (csrc/bhip_cluster.hip): a node decides once
 * every earlier neighbour it depends on has decided, so a chain i -> i - 1 takes one round per node -- correct and slow, and not capped.
 * A round that decides nothing is BHIP_E_INTERNAL.  The call leaves nothing resident but scratch buffers of the handle.
 * bhip_cluster_info, of the last bhip_cluster_run on the handle: [0] rounds, [1] edges kept (distinct, towards higher priority), [2]
 * centroids, [3] device microseconds (HIP events around everything launched), [4] device bytes of the scratch buffers, [5] raw edges,
 * [6] nodes, [7] 0. */
typedef struct BhipClusterEdge { uint32_t q, r, edits; } BhipClusterEdge;
BHIP_API int bhip_cluster_run(void *handle, uint32_t n_nodes, const uint32_t *weights, const BhipClusterEdge *edges, uint64_t n_edges,
                              uint32_t *centroid_out, uint32_t *edits_out);
BHIP_API int bhip_cluster_info(void *handle, uint64_t info[8]);

/* Chimera check: a de-novo two-parent test of the reads of a query file from the lines it prints against itself and their alignment
 * paths (burst_hip --chimeras; no reference counterpart: the definition is this project's own).  All of it is integer arithmetic,
 * bit-exact on any machine.  S, G and D below are policy, not measurements.
 *   NODES     as in the clustering: the reads of the -q file in file order, weight 1 or (--chimera-sizes) the N of a trailing `;size=N[;]`;
 *             len[q] = the read's number of symbols.  PRIORITY as there: the larger weight first, then the smaller number; rank[r] = r's place.
 *   PARENT    r is a CANDIDATE PARENT of q when r != q and weight[r] >= S * weight[q] (64-bit product; S = skew, --chimera-skew, default 2).
 *   LINE      of q towards r: a printed line whose column 1 is read q and whose column 2 is byte-equal to the name of a candidate parent
 *             r.  Per (q, r) one line counts: the one with the smallest column 11, the one printed first among equals.  A line whose
 *             column 2 names no read is FOREIGN (ignored, counted); self lines and lines towards non-candidates are ignored.
 *   EDITS     of a line, in read orientation and DOUBLED coordinates: walk the line's path (the ops --cigar prints), j = query symbols
 *             consumed so far: a symbol of an X or I gives position 2j + 1, then j++; a column of a D gives position 2j; '=' advances
 *             j.  The path of a reverse line (column 9 > column 10) is that of the reverse-complement entry: each position p becomes
 *             2 len[q] - p.  E = the number of positions = column 11.
 *   CUT       c splits the read into [0, c) and [c, len): L[c] = the positions <= 2c, R[c] = E - L[c] (a D exactly at the cut is left, in
 *             both orientations).  The cuts of q are c in [G, len[q] - G] (G = min_seg, --chimera-min-seg, default 16).
 *   ROLE      q is NOT EVALUATED (role 0, `-`) with fewer than two candidate parents with a line, or without a cut.  Otherwise
 *             single = the smallest E over its lines; bestL[c], bestR[c] = the smallest packed keys L[c] << 32 | rank[r] and
 *             R[c] << 32 | rank[r] over its lines; Model[c] = the sum of their two edit parts; cut = the smallest c with the smallest
 *             Model[c], model = that value; parent a and ea from bestL[cut], parent b and eb from bestR[cut].  Role 2 (`Y`, chimeric)
 *             when single - model >= D (D = min_gain, --chimera-min-gain, default 3), else role 1 (`N`).  With one line per (q, r) and
 *             D >= 1 a `Y` always has a != b (a == b would make model = that line's E >= single).
 * Out of scope: parents that are flagged themselves are not excluded; three-way chimeras; segments are not aligned afresh (the profile is
 * that of the end-to-end paths printed).
 * bhip_chimera_run takes the lines raw -- self lines, lines towards non-candidates and repeated (q, r) included; the device drops them --
 * with their paths as bhip_trace_paths writes them (ops[op_off .. op_off + n_ops), words length << 4 | code).  BHIP_E_ARG with a text, before
 * any device memory is touched and with the handle staying usable: a line that names a node >= n_nodes, ops that leave `ops`, a word that
 * is not a run of I/D/=/X of length >= 1, ops that consume ('=' + X + I) another number of symbols than len[q], len[q] of 0 or above
 * BHIP_MAX_QLEN, more than 254 edits, n_lines >= 2^32, n_nodes = 2^32 - 1, skew, min_seg or min_gain of 0.  n_lines == 0 launches
 * nothing: every role is 0.  out[q] of a role 0 is all zeros.  The call leaves nothing resident but scratch buffers of the handle
 * (csrc/bhip_chimera.hip, DESIGN.md section 7f: one wave per read).
 * bhip_chimera_info, of the last bhip_chimera_run on the handle: [0] (q, r) pairs kept, [1] reads evaluated, [2] chimeric reads, [3]
 * device microseconds (HIP events around everything launched), [4] device bytes of the scratch buffers, [5] raw lines, [6] nodes, [7] 0. */
typedef struct BhipChimLine { uint32_t q, r, flags /* bit 0: reverse */, n_ops; uint64_t op_off; } BhipChimLine;
typedef struct BhipChimera  { uint32_t role /* 0 '-', 1 'N', 2 'Y' */, single, model, cut, a, ea, b, eb; } BhipChimera;
BHIP_API int bhip_chimera_run(void *handle, uint32_t n_nodes, const uint32_t *weights, const uint32_t *len, const BhipChimLine *lines, uint64_t n_lines,
                              const uint32_t *ops, uint64_t n_ops, uint32_t skew, uint32_t min_seg, uint32_t min_gain, BhipChimera *out /* [n_nodes] */);
BHIP_API int bhip_chimera_info(void *handle, uint64_t info[8]);

/* MD tags: the SAM `MD:Z:` string and the `NM:i:` count of alignment paths (burst_hip --sam; no reference counterpart).  The inputs are
 * exactly what bhip_trace_paths returns for the same requests -- the lane refIx of the request, its first lane column ref_first (1-based,
 * as the tracer writes it) and its op words length << 4 | code, request i owning ops[op_off[i] .. op_off[i + 1]); the query symbols are
 * not needed.  The string is what `samtools calmd` computes, over these ops, where a MATCH is an '=' op: cost 0 under the run's scoring,
 * so an ambiguity code the matrix scores 0 is a match.  With a counter u = 0 and the lane column col = ref_first - 1 (0-based):
 *   '=' of length n   u += n; col += n
 *   X of length n     per column: u in decimal, then the reference letter at col; u = 0; col++
 *   D of length n     u in decimal, then '^', then the n reference letters; u = 0; col += n
 *   I                 nothing: the counter runs on across it
 *   at the end        u in decimal, also when it is 0
 * Letters are "NACGTNKMRYSWBVHD"[code]: the pad code 0 prints N (a valid path never consumes a pad column).  nm[i] = the X + I + D symbols.
 * Examples: 100= gives `100`; 1X gives `0A0`; 2X gives `0A0C0`; 3=2D1X4= gives `3^AC0T4`; 5=2I5= gives `10`; 1X1D gives `0A0^C0`.
 * The strings are not terminated: request i owns md[md_off[i] .. md_off[i + 1]), md_off has n_requests + 1 entries.
 * BHIP_E_CAPACITY when md_off[n_requests] exceeds md_cap: md_off and nm are complete, md is not valid, the handle stays usable.  BHIP_E_ARG
 * with a text, before any device memory is touched and with the handle staying usable, for null arguments, a word that is not a run of
 * I / D / '=' / X of length >= 1, op_off that is not ascending, a refIx >= 16 n_clumps or >= tot_refs, and a path whose '=' + X + D columns
 * leave the columns 1 .. ClumpLen of its lane.  n_requests == 0 launches nothing (md_off[0] = 0).
 * info (may be NULL): [0] device microseconds of the call (HIP events around its kernels and scan), [1] requests, [2] MD bytes, [3] peak
 * bytes of the call's scratch buffers (the handle keeps them; bhip_destroy frees them), [4..7] 0.
 * One thread per request: a counting walk, a 64-bit exclusive sum, the writing walk; an '=' run costs one addition and the lane is read
 * under X and D only (csrc/bhip_md.hip). */
BHIP_API int bhip_md_tags(void *handle, const BhipPathReq *requests, const uint32_t *ref_first, const uint64_t *op_off, const uint32_t *ops, uint64_t n_requests,
                          char *md, uint64_t md_cap, uint64_t *md_off /* [n_requests + 1] */, uint32_t *nm /* [n_requests] */, uint64_t info[8]);

/* Tuning knobs.  "prefilter_stride": 0 (default) = automatic sparse seeds -- per query the largest stride s <= K for
 * which an alignment within budget still keeps >= 3 of the words starting at 0, s, 2s, ... (one edit destroys at most
 * ceil(K/s) of them), fewest .acx look-ups with the same no-false-negative guarantee; s >= 1 forces every s-th word,
 * 1 = every word = the reference's own threshold count > len-(E+1)K (burst.c:4091-4092, 4126).
 * "two_stage": 1 (default) = prefix filter + windowed full-length edit distance, 0 = one full-length sweep.
 * "lanes": 1..15 (default 1) sub-pipelines a staged batch is cut into; their prefilter / sweep / window+re-score stages
 * run as a software pipeline on three HIP streams; "lane_min_entries" (default 32768) = fewest entries worth a lane.
 * "sweep_blocks": 1..8 workgroups per CU of the sweep kernels.  "lane_masks": 1 (default) = lane-resolved prefilter.
 * "prefilter_table": 0 (default, chosen from the accelerator's list lengths) or 9/10/11 = log2 slots of the per-query
 * tables; "prefilter_algo": -1 (default) = counting-filter kernel, switching to the exact-hash kernel for workloads where
 * more than 20 % of the list records survive the filter, 0 / 1 = force one of them; "prefilter_waves": 0 (default, as many as fit) .. 16 single-wave prefilter blocks per CU.
 * "prune": 1 (default) = when only the minimum per shared slot is wanted, lanes whose seed count bounds their edit distance
 * above the query's best bound are swept only if the first sweep leaves room for them (exact: the bound is a lower bound).
 * "async_d2h": 0 (default) / 1 = asynchronous hand-over of the records, see bhip_sync_hits.
 * "rescore_reg": 1 (default) = register-band re-scorer for narrow bands, 0 = LDS band only.
 * "fetch_once": 1 (default) = the register-band re-scorer copies a hit's packed query once into LDS, or takes it 16 bytes at a time where
 * the length class is too long for that, each only where it costs no resident wave; 0 = a dword of the query per 8 rows.  Same records.
 * "band": 1 (default) = windows whose flagged diagonals fit two to four words of the bit-vector column are swept by the banded kernel
 * (only those words are stepped; exact), 0 = every window through the full column.  "oversub": 1..16 (default 2) = blocks launched per
 * resident block slot of the per-item kernels (prefix tasks, windows, re-scoring); "band_blocks": 0 (default, as many as fit) or the
 * 64-thread blocks per CU of the banded kernel.
 * "host_routing": 0 (default) = batches are routed (length classes, seed plans, lists) by a device kernel, 1 = by the host pass
 * that otherwise only handles batches with query symbols outside the alphabet.  "discard_staged": forget batches that were
 * staged and not aligned (after an error).  "seed_ahead": 1 (default) = the seed lookups and match profiles of the next staged
 * batch run while the current one is swept, 0 = in place; "seed_ahead_blocks" (default 2, 0 = unlimited) / "peq_ahead_blocks"
 * (default 16) = 256-thread blocks per CU those kernels get while they share the device with the sweeps.
 * "seed_min_need": -1 (default) / 0 / n -- of a query's sampled words the ones with the LONGEST accelerator lists are left out while the
 * number of words an alignment within budget is guaranteed to keep stays >= n (any subset of the sampled words gives the same
 * no-false-negative guarantee with a correspondingly smaller count); 0 = every list is walked; -1 = n = 3 when the expected record
 * stream is long enough to matter and short enough for the counting filter to stay selective (bhip_align.hip seed_min_need_for).
 * "seed_drop_len" (default 8): lists shorter than this are never left out.  "prefilter_rb": 0 (default, from the expected stream) or
 * 2 / 3 / 4 = blocks of 64 list records per query the counting-filter kernel fetches one quad ahead and keeps in registers.
 * "prefilter_group": 0 (default) / 8 / 16 = lanes per query in the first pass of the four-queries-per-wave counting filter: 8 puts eight
 * queries into a wave (rows of at most 8 words only; wider rows run 16 whatever the value), 0 chooses by the expected record stream and the
 * survivors of the lane's previous batch (bhip_pf_select.h: bhip_pf_group).
 * "prefilter_bytes": 1 (default) = a query whose record stream is at most 255 records counts in bytes (twice the counters in the same LDS).
 * None of these changes a result.  BHIP_OPTS="name=value,..." in the environment sets options at bhip_init. */
BHIP_API int bhip_set_option(void *handle, const char *name, long long value);

/* Stats of the last call; device properties (name, CU count) for reports. */
BHIP_API int bhip_get_stats(void *handle, BhipStats *out);
BHIP_API int bhip_device_info(void *handle, char *name, int name_cap, int *n_cu, uint64_t *hbm_bytes);

BHIP_API void bhip_destroy(void *handle);
BHIP_API const char *bhip_last_error(void);
/* ABI version of this header */
BHIP_API int bhip_abi_version(void);
#define BHIP_ABI_VERSION 8

#ifdef __cplusplus
}
#endif
#endif
