// The planning rules of the word-sliced accelerator build (burst_amd/csrc/bhip_acx_plan.h) on the host: answers one question per line of
// standard input, so that tests/test_host_cpu.py can hold the expected rows.  Records are 4 bytes, the range's chunks 1 GiB.
//   buf <n>                                                          -> bytes of the sort's part of the range for n tuples
//   runs <n_parts> <hist ...>                                        -> rb[0 .. n_parts]
//   range <available bytes> <total> <total_own>                      -> bytes to reserve (0: not even the records fit)
//   target <own0> <own1> <max_b> <range bytes> <target> <hist ...>   -> cuts | tuples per slice   ("-" when the build cannot run the plan)
//   room <own0> <own1> <max_b> <range bytes> <hist ...>              -> the same for the plan by room
//   plan <own0> <own1> <shift> <range bytes> <forced> <hist ...>     -> the same for the plan the build takes (forced: BHIP_MASK_SLICE)
// Test infrastructure: g++, no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "bhip_acx_plan.h"

static void print_plan(const BhipAcxPlan &p) {
	if (!bhip_acx_plan_ok(p)) { printf("-\n"); return; }
	std::string s;
	for (uint32_t c : p.cuts) s += std::to_string(c) + " ";
	s += "|";
	for (uint64_t n : p.items) s += " " + std::to_string(n);
	printf("%s\n", s.c_str());
}

int main() {
	char line[4096];
	while (fgets(line, sizeof line, stdin)) {
		char *tok = strtok(line, " \n");
		if (!tok) continue;
		const std::string what = tok;
		std::vector<double> a;
		while ((tok = strtok(nullptr, " \n"))) a.push_back(strtod(tok, nullptr));
		const size_t fixed = what == "buf" || what == "runs" ? 1 : what == "range" ? 3 : what == "target" || what == "plan" ? 5 : what == "room" ? 4 : 0;
		if (!fixed || a.size() < fixed) { fprintf(stderr, "cannot read: %s\n", what.c_str()); return 2; }
		std::vector<unsigned long long> hist;
		for (size_t i = fixed; i < a.size(); ++i) hist.push_back((unsigned long long)a[i]);
		BhipAcxPlan p;
		if (what == "buf") printf("%zu\n", bhip_acx_buf_bytes((uint64_t)a[0]));
		else if (what == "runs") {
			std::string s;
			for (uint32_t b : bhip_acx_rank_runs(hist, (int)a[0])) s += (s.empty() ? "" : " ") + std::to_string(b);
			printf("%s\n", s.c_str());
		} else if (what == "range") printf("%zu\n", bhip_acx_range_bytes(a[0], (uint64_t)a[1], (uint64_t)a[2], 4, (size_t)1 << 30));
		else if (what == "target") { bhip_acx_plan_by_target(hist, (uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (size_t)a[3], (uint64_t)a[4], 4, &p); print_plan(p); }
		else if (what == "room") { bhip_acx_plan_by_room(hist, (uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (size_t)a[3], 4, &p); print_plan(p); }
		else { bhip_acx_plan_run(hist, (uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (size_t)a[3], (long long)a[4], 4, &p); print_plan(p); }
	}
	return 0;
}
