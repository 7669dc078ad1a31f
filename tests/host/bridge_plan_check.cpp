// bridge_plan_check.cpp -- csrc/bridge_plan.hpp run alone, without a GPU or the library (tests/test_bridge_plan_cpu.py builds
// this with the address and undefined-behaviour sanitizers and reads its one line):
//   bridge_plan_check RULES CONF_RATE MEMBERS PLC RATE:IN:OUT...
// RULES: create (no legs' rates: RATE must be CONF_RATE), rated (IN:OUT are leg 0's on every leg), legs, endpoints, concealed,
// rational.  Prints `rc text` of a refusal, or `0 family=... tick_bytes=IN,OUT lds=... ...`.
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
	if (argc < 6) return 2;
	static const struct { const char *name; const Rules *rules; } RULES[] = {
	    {"create", &RULES_RATED},         {"rated", &RULES_RATED},         {"legs", &RULES_LEGS},
	    {"endpoints", &RULES_ENDPOINTS}, {"concealed", &RULES_CONCEALED}, {"rational", &RULES_RATIONAL}};
	const Rules *rules = nullptr;
	for (const auto &r : RULES)
		if (!strcmp(argv[1], r.name)) rules = r.rules;
	if (!rules) return 2;
	std::vector<mi_bridge_leg> legs;
	std::vector<int32_t> rates;
	for (int i = 5; i < argc; ++i) {
		mi_bridge_leg l;
		if (sscanf(argv[i], "%d:%d:%d", &l.rate, &l.in_codec, &l.out_codec) != 3) return 2;
		legs.push_back(l);
		rates.push_back(l.rate);
	}
	mi_bridge_config cfg = {};
	cfg.nstreams = (int32_t)legs.size(), cfg.rate = atoi(argv[2]), cfg.members_per_conference = atoi(argv[3]), cfg.plc = atoi(argv[4]);
	cfg.in_codec = legs[0].in_codec, cfg.out_codec = legs[0].out_codec;
	Plan p;
	const bool by_rate = !strcmp(argv[1], "create") || !strcmp(argv[1], "rated");
	const int rc = by_rate ? plan_bridge(*rules, &cfg, strcmp(argv[1], "create") ? rates.data() : nullptr, nullptr, &p)
	                       : plan_legs(*rules, &cfg, legs.data(), &p);
	if (rc != MI_OK) return printf("%d %s\n", rc, g_error) < 0;
	static const char *const FAMILY[] = {"TICK", "RATED", "LEGS", "LEGS_RATED", "UPDOWN", "RATIONAL"};
	printf("0 family=%s tick_bytes=%zu,%zu lds=%zu wide=%d row_w=%d sum_off=%d nslice=%d scratch=%d+4x%d pitch=%d hist=%d,%d leg_plc=%d "
	       "ratios=%zu codecs=%zu\n",
	       FAMILY[p.family], p.in_bytes, p.out_bytes, p.lds, p.wide, p.row_w, p.sum_off, p.nslice, p.scratch_off, p.scratch_per_wave, p.pitch,
	       p.hin_stride, p.hout_stride, (int)p.leg_plc, p.ratio.size(), p.leg_codec.size());
	return 0;
}
