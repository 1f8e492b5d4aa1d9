// burst_amd/csrc/bhip_pf_select.h -- which lane-resolved prefilter kernel a (lane, class) list runs, as data, decided once: bhip_align.hip
// launches from it (launch_prefilter_mask), sizes the seed plan from it (launch_seed) and enables the lower-bound pruning from it
// (enqueue_lane).  No HIP in here: tests/csrc/pf_select_host.cpp compiles it with the host compiler and pins every row.
#ifndef BHIP_PF_SELECT_H
#define BHIP_PF_SELECT_H
#include <stdint.h>

// kind: the numbers BhipStats::prefilter_algo reports
enum { BHIP_PF_CF = 0,       // k_prefilter_cf<htb, rb>: counting filter, four queries per wave, 16 lanes each (superseded: test-only library)
       BHIP_PF_MASK = 1,     // k_prefilter_mask<htb>: exact clump hash table
       BHIP_PF_CW = 2,       // k_prefilter_cw<cw_mode, BIG>: counting filter, one query per wave (cw_mode 0 / 1 superseded: test-only library)
       BHIP_PF_CQ = 3 };     // k_prefilter_cq<cw_mode, BIG, GW>: counting filter, four (GW = 16) or eight (GW = 8, bhip_pf_group) queries per wave, streams walked by the whole wave
struct BhipPfChoice {
	int kind;
	int htb;                 // log2 of the per-query table (k_prefilter_cf: approximate counters; k_prefilter_mask: hash slots)
	int rb;                  // k_prefilter_cf: 64-record blocks per query kept in registers
	int cw_mode;             // slot layout of k_prefilter_cw / k_prefilter_cq from the lists a query can have: 0 up to 8, 1 up to 16, 2 any number
	bool legacy;             // the kernel lives in libburst_hip_legacy.so
	bool two_pass;           // a second pass with the largest tables (BIG / <11, 4>) takes the queries that overflowed the first
};

// the algorithm of a lane's next prefilter launch: option prefilter_algo, or (-1) what the lane adapted to
static inline int bhip_pf_algo(int opt_pf_algo, int lane_algo) { return opt_pf_algo >= 0 ? opt_pf_algo : lane_algo; }

// per-query counters of the counting filter (algo 0) / slots of the exact table (algo 1) for an expected record stream (sampled words x
// occurrence-weighted mean list length): 512 slots keep 12 single-wave blocks on a CU, 1024 -> 7, 2048 -> 4.
// (the touched list holds half the slots; a query that exceeds it is re-done by the dense fallback, so the estimate -- an upper bound,
// every repeated clump counted once per word -- may be cut close; the approximate counters tolerate a load around 1 -- false survivors
// only cost work)
static inline int bhip_pf_table_bits(int opt_pf_table, int algo, double expect) {
	return opt_pf_table ? opt_pf_table : algo == 0 ? (expect <= 600.0 ? 9 : expect <= 1200.0 ? 10 : 11) : (expect <= 230.0 ? 9 : expect <= 470.0 ? 10 : 11);
}

// algo: bhip_pf_algo(); W16: words per query row of the range table (seed_row_words); expect: mean records per query of the list (mean, not
// max: outliers use the fallback)
static inline BhipPfChoice bhip_pf_choose(int algo, int opt_pf_cw, int opt_pf_table, int opt_pf_rb, uint32_t W16, double expect) {
	BhipPfChoice c;
	c.htb = bhip_pf_table_bits(opt_pf_table, algo, expect);
	// the expected stream of a query after the longest lists have been left out (expect counts them all: an upper bound), 2 .. 4; the wider
	// tables only come with 2 or 4
	c.rb = opt_pf_rb ? opt_pf_rb : (expect <= 110.0 ? 2 : expect <= 230.0 ? 3 : 4);
	if (c.htb != 9 && c.rb == 3) c.rb = 4;
	c.cw_mode = W16 <= 8 ? 0 : W16 <= 16 ? 1 : 2;
	const bool cw = algo == 0 && opt_pf_cw;
	const bool cq = cw && opt_pf_cw == 2 && c.cw_mode < 2;      // (up to 16 lists per query; plans beyond: one query per wave)
	c.kind = cq ? BHIP_PF_CQ : cw ? BHIP_PF_CW : algo;
	c.legacy = algo == 0 && !cq && !(cw && c.cw_mode == 2);
	c.two_pass = algo == 0 && (cw || c.htb != 11);
	return c;
}

// Lanes per query of k_prefilter_cq's FIRST pass: 16 (four queries per wave) or 8 (eight).  The kernel's per-quad half -- list scan, survivor
// rounds, emit, clears -- costs the same instructions whatever the number of queries in the wave, so eight queries halve it per query; the
// price is half of everything a query owns: 512 approximate slots, a 16-slot exact table, 8 survivors per round, two resident rows of 64
// records.  That pays for short streams with few survivors and nowhere else:
//  * only BHIP_PF_CQ in slot mode 0 (a query's lists are the lanes of its group: at most 8; a wider row runs 16 lanes whatever the option);
//  * expect <= BHIP_PF_GROUP8_MAX_EXPECT records per query (beyond two rows the records are loaded twice, and 512 slots fill up);
//  * the lane's previous chain left at most BHIP_PF_GROUP8_MAX_SURV survivors per query (a strain-rich lane: its queries fill the 16-slot
//    table and would all go through the BIG pass; surv_last < 0: no chain yet, the lane's first batch goes by expect alone).
// opt_group: 0 = by this rule, 8 / 16 = that width wherever the kernel has it.  Both limits are measurements (profiles/prefilter_group8.md,
// ms per launch at 16 / 8 lanes, 2 M 100-bp reads per batch on one MI355X):
//  * expect 37 (2.77 GB database): 0.78 / 0.69; 64 (5.5 GB): 0.83 / 0.73; 117 (11 GB, 88 records read per query): 0.96 / 0.88 -- 8 lanes win by
//    more than three times the leg-to-leg difference (at 117 in one run of two; every leg of the other has the same sign); 223 (22 GB, 173 records read): 1.14 / 1.83 -- they lose.  The limit sits at the two
//    resident rows, between the last win and the first loss.
//  * survivors per query: 6.3 - 6.9 on those databases; 34 - 52 on the strain-rich profile at 2.6 GB, where 8 lanes take 10.2 ms against 7.2.
//    The limit sits where a round of 8 no longer holds the mean query's survivors with some room; nothing between 7 and 34 was measured.
#define BHIP_PF_GROUP8_MAX_EXPECT 128.0
#define BHIP_PF_GROUP8_MAX_SURV 12.0
static inline int bhip_pf_group(int opt_group, const BhipPfChoice &c, uint32_t W16, double expect, double surv_last) {
	if (c.kind != BHIP_PF_CQ || c.cw_mode != 0 || W16 > 8 || opt_group == 16) return 16;
	if (opt_group == 8) return 8;
	return expect <= BHIP_PF_GROUP8_MAX_EXPECT && surv_last <= BHIP_PF_GROUP8_MAX_SURV ? 8 : 16;
}

// Leaving out a query's longest list (k_seed_ranges: its guaranteed count drops from 4 to 3 for a 100-bp read at 98 %) walks ~21 % fewer
// records -- and lets more of them through the counting filter: a record survives when its counter holds need - 1 OTHER records, and a
// survivor costs about eight records' worth of work (exact-table insertion).  Measured at three database sizes:
// it pays while the remaining stream loads the counters below ~0.35 per counter (19 GB database: 152 records on 512 counters, +6 %) and
// costs at the metric's size (246 records: 8 % survivors instead of 2.5 %, -6 %); on small databases the kernel's time does not depend on
// the records at all and the extra candidates only cost sweeps.  opt_seed_min_need: -1 = by that rule, 0 = never, n = whenever the count
// stays >= n.  (The counters are those of the kernel the OPTIONS name: neither the lane's adapted algorithm nor slot mode 2 is looked at.)
static inline uint32_t bhip_seed_min_need(int opt_seed_min_need, int opt_pf_cw, int opt_pf_table, int opt_pf_bytes, double acx_wmean, double mean_words, uint32_t W16) {
	if (opt_seed_min_need >= 0) return (uint32_t)opt_seed_min_need;
	const double t_all = mean_words * acx_wmean;
	const double t_less = t_all * (mean_words > 1.0 ? (mean_words - 1.0) / mean_words : 1.0) * 0.93;
	// (k_prefilter_cf: a stream of at most 255 records counts in bytes: twice the counters; the streams of a batch scatter around their mean.
	// k_prefilter_cw / k_prefilter_cq: 1 024 byte slots of list masks for up to 8 lists whatever the stream's length, 512 halfword slots beyond)
	const double counters = opt_pf_cw ? (W16 <= 8 ? 1024.0 : 512.0) : (double)(1u << bhip_pf_table_bits(opt_pf_table, 0, t_all)) * (opt_pf_bytes && t_less <= 200.0 ? 2.0 : 1.0);
	return (t_all >= 100.0 && t_less / counters <= 0.35) ? 3u : 0u;
}
#endif
