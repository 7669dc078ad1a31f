// bridge_ratios_plan_check.cpp -- csrc/bridge_plan.hpp run alone under mi_bridge_create_ratios' rules, without a GPU or the
// library (tests/test_bridge_ratios_cpu.py builds this with the address and undefined-behaviour sanitizers and reads its one
// line).  bridge_plan_check.cpp's arguments, with a seventh family and the plan's filters:
//   bridge_ratios_plan_check RULES CONF_RATE MEMBERS PLC RATE:IN:OUT...
// RULES: rational or ratios.  Prints `rc text` of a refusal, or `0 family=... tick_bytes=IN,OUT lds=... ...`;
//   bridge_ratios_plan_check rule NUM DEN
// prints `filt_len direct` of filter_rule for in : out = NUM : DEN.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../mediastreamer2_amd/csrc/bridge_plan.hpp"

static char g_error[1024];
void mi::set_error(const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_error, sizeof(g_error), fmt, ap);
	va_end(ap);
}
// plc.hip's, which is not linked here: the concealer's own refusals are its tests' to check
int mi_plc_check_rate(const char *, const char *, int, int) { return MI_OK; }

int main(int argc, char **argv) {
	if (argc == 4 && !strcmp(argv[1], "rule")) {
		const FilterRule f = filter_rule(atoi(argv[2]), atoi(argv[3]));
		return printf("%d %d\n", f.filt_len, (int)f.direct) < 0;
	}
	if (argc < 6) return 2;
	const Rules *rules = !strcmp(argv[1], "ratios") ? &RULES_RATIOS : !strcmp(argv[1], "rational") ? &RULES_RATIONAL : nullptr;
	if (!rules) return 2;
	std::vector<mi_bridge_leg> legs;
	for (int i = 5; i < argc; ++i) {
		mi_bridge_leg l;
		if (sscanf(argv[i], "%d:%d:%d", &l.rate, &l.in_codec, &l.out_codec) != 3) return 2;
		legs.push_back(l);
	}
	mi_bridge_config cfg = {};
	cfg.nstreams = (int32_t)legs.size(), cfg.rate = atoi(argv[2]), cfg.members_per_conference = atoi(argv[3]), cfg.plc = atoi(argv[4]);
	cfg.in_codec = legs[0].in_codec, cfg.out_codec = legs[0].out_codec;
	Plan p;
	const int rc = plan_legs(*rules, &cfg, legs.data(), &p);
	if (rc != MI_OK) return printf("%d %s\n", rc, g_error) < 0;
	static const char *const FAMILY[] = {"TICK", "RATED", "LEGS", "LEGS_RATED", "UPDOWN", "RATIONAL", "RATIOS"};
	printf("0 family=%s tick_bytes=%zu,%zu lds=%zu wide=%d row_w=%d sum_off=%d nslice=%d scratch=%d+4x%d pitch=%d hist=%d,%d leg_plc=%d "
	       "ratios=%zu codecs=%zu generic=%zu bytes=",
	       FAMILY[p.family], p.in_bytes, p.out_bytes, p.lds, p.wide, p.row_w, p.sum_off, p.nslice, p.scratch_off, p.scratch_per_wave, p.pitch,
	       p.hin_stride, p.hout_stride, (int)p.leg_plc, p.ratio.size(), p.leg_codec.size(), p.generic.size());
	for (size_t s = 0; s < p.ratio.size(); ++s) printf("%s%02x", s ? "," : "", p.ratio[s]);
	printf("\n");
	return 0;
}
