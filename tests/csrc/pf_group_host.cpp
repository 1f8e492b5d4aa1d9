// The group width of k_prefilter_cq's first pass (burst_amd/csrc/bhip_pf_select.h: bhip_pf_group) on the host: one question per line of
// standard input, so that tests/test_pf_group_cpu.py can hold the expected rows.
//   group <prefilter_group> <algo> <prefilter_cw> <W16> <expect> <survivors per query of the lane's last chain, -1 = none yet>      -> 8 or 16
//   limits      -> BHIP_PF_GROUP8_MAX_EXPECT BHIP_PF_GROUP8_MAX_SURV
// Test infrastructure: g++, no device.
#include <cstdio>
#include <cstring>
#include "bhip_pf_select.h"

int main() {
	char line[256], what[16];
	while (fgets(line, sizeof line, stdin)) {
		int grp, algo, cw; unsigned w; double x, s;
		if (sscanf(line, "%15s", what) != 1) continue;
		if (!strcmp(what, "group") && sscanf(line, "%*s %d %d %d %u %lf %lf", &grp, &algo, &cw, &w, &x, &s) == 6) {
			const BhipPfChoice ch = bhip_pf_choose(algo, cw, 0, 0, w, x);
			printf("%d\n", bhip_pf_group(grp, ch, w, x, s));
		} else if (!strcmp(what, "limits")) {
			printf("%.17g %.17g\n", (double)BHIP_PF_GROUP8_MAX_EXPECT, (double)BHIP_PF_GROUP8_MAX_SURV);
		} else { fprintf(stderr, "cannot read: %s", line); return 2; }
	}
	return 0;
}
