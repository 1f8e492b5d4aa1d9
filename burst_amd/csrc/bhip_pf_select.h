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
       BHIP_PF_CQ = 3 };     // k_prefilter_cq<cw_mode, BIG>: counting filter, four queries per wave, streams walked by the whole wave
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
