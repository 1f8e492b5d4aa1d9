// The rules of option "fetch_once" (burst_amd/csrc/bhip_fetch_plan.h) on the host: answers one question per line of standard input, so that
// tests/test_fetch_plan_cpu.py can check them for every class word count and register set.  A kernel is given as <registers> <static LDS bytes>.
//   blocks <threads> <kernel> <dynamic LDS bytes>                 -> resident blocks per CU
//   query <qw> <fetch_once> <kernel dword> <kernel lds> <kernel chunk>   -> form (0 dword, 1 lds, 2 chunk), dynamic LDS bytes, blocks per CU, tail flag
// Test infrastructure: g++, no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "bhip_fetch_plan.h"

int main() {
	char line[4096];
	while (fgets(line, sizeof line, stdin)) {
		char *tok = strtok(line, " \n");
		if (!tok) continue;
		const std::string what = tok;
		std::vector<long long> a;
		while ((tok = strtok(nullptr, " \n"))) a.push_back(strtoll(tok, nullptr, 10));
		const size_t need = what == "blocks" ? 4 : what == "query" ? 8 : 0;
		if (!need || a.size() != need) { fprintf(stderr, "cannot read: %s\n", what.c_str()); return 2; }
		auto kernel = [&](size_t i) { return BhipKernelRes{(int)a[i], (size_t)a[i + 1]}; };
		if (what == "blocks") printf("%u\n", bhip_resident_blocks((uint32_t)a[0], kernel(1), (size_t)a[3]));
		else {
			const BhipKernelRes res[BHIP_QF_COUNT] = {kernel(2), kernel(4), kernel(6)};
			const BhipQueryFetch f = bhip_plan_query_fetch((uint32_t)a[0], (int)a[1], res);
			printf("%d %u %u %d\n", f.form, f.lds_bytes, f.blocks, f.tail ? 1 : 0);
		}
	}
	return 0;
}
