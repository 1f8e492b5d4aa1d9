// The prefilter's variant table (burst_amd/csrc/bhip_pf_select.h) on the host: answers one question per line of standard input, so that
// tests/test_host_cpu.py can hold the expected rows.
//   choose <algo> <prefilter_cw> <prefilter_table> <prefilter_rb> <W16> <expect>      -> kind htb rb cw_mode legacy two_pass
//   need <seed_min_need> <prefilter_cw> <prefilter_table> <prefilter_bytes> <acx_wmean> <mean_words> <W16>      -> 0 or 3 (or the explicit value)
// Test infrastructure: g++, no device.
#include <cstdio>
#include <cstring>
#include "bhip_pf_select.h"

int main() {
	char line[256], what[16];
	while (fgets(line, sizeof line, stdin)) {
		int a, b, c, d; unsigned w; double x, y;
		if (sscanf(line, "%15s", what) != 1) continue;
		if (!strcmp(what, "choose") && sscanf(line, "%*s %d %d %d %d %u %lf", &a, &b, &c, &d, &w, &x) == 6) {
			const BhipPfChoice ch = bhip_pf_choose(a, b, c, d, w, x);
			printf("%d %d %d %d %d %d\n", ch.kind, ch.htb, ch.rb, ch.cw_mode, (int)ch.legacy, (int)ch.two_pass);
		} else if (!strcmp(what, "need") && sscanf(line, "%*s %d %d %d %d %lf %lf %u", &a, &b, &c, &d, &x, &y, &w) == 7) {
			printf("%u\n", bhip_seed_min_need(a, b, c, d, x, y, w));
		} else { fprintf(stderr, "cannot read: %s", line); return 2; }
	}
	return 0;
}
