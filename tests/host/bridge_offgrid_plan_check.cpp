// bridge_offgrid_plan_check.cpp -- csrc/bridge_plan.hpp run alone under mi_bridge_create_offgrid's rules, without a GPU or the
// library (tests/test_bridge_offgrid_cpu.py builds this with the address and undefined-behaviour sanitizers and reads its one
// line).  bridge_ratios_plan_check.cpp's arguments with the admitted kinds of an open bridge behind the legs:
//   bridge_offgrid_plan_check RULES CONF_RATE MEMBERS PLC NADMIT RATE:IN:OUT...
// RULES: open (mi_bridge_create_open's) or offgrid; the last NADMIT triples are the admitted kinds, those before them the legs.
// Prints `rc text` of a refusal, or `0 family=... tick_bytes=IN,OUT lds=... ...`: every field of the plan.
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
	if (argc < 7) return 2;
	const Rules *rules = !strcmp(argv[1], "offgrid") ? &RULES_OFFGRID : !strcmp(argv[1], "open") ? &RULES_RATIOS : nullptr;
	const int nadmit = atoi(argv[5]);
	if (!rules || nadmit < 0 || nadmit > argc - 7) return 2;
	std::vector<mi_bridge_leg> legs;
	for (int i = 6; i < argc; ++i) {
		mi_bridge_leg l;
		if (sscanf(argv[i], "%d:%d:%d", &l.rate, &l.in_codec, &l.out_codec) != 3) return 2;
		legs.push_back(l);
	}
	const size_t n = legs.size() - (size_t)nadmit;
	mi_bridge_config cfg = {};
	cfg.nstreams = (int32_t)n, cfg.rate = atoi(argv[2]), cfg.members_per_conference = atoi(argv[3]), cfg.plc = atoi(argv[4]);
	cfg.in_codec = legs[0].in_codec, cfg.out_codec = legs[0].out_codec;
	Plan p;
	const int rc = plan_open(*rules, &cfg, legs.data(), legs.data() + n, nadmit, &p);
	if (rc != MI_OK) return printf("%d %s\n", rc, g_error) < 0;
	static const char *const FAMILY[] = {"TICK", "RATED", "LEGS", "LEGS_RATED", "UPDOWN", "RATIONAL", "RATIOS", "OFFGRID"};
	printf("0 family=%s tick_bytes=%zu,%zu lds=%zu wide=%d row_w=%d sum_off=%d nslice=%d scratch=%d+4x%d pitch=%d pcm_pitch=%d hist=%d,%d "
	       "leg_plc=%d rated=%d updown=%d rational=%d ratios=%d data=%d open=%d common=%d max_ratio=%d n=%d nconf=%d len=%d codecs=%zu generic=%zu "
	       "kinds=%zu offgrid=%d off=%d:%d taps=%d,%d bytes=",
	       FAMILY[p.family], p.in_bytes, p.out_bytes, p.lds, p.wide, p.row_w, p.sum_off, p.nslice, p.scratch_off, p.scratch_per_wave, p.pitch,
	       p.pcm_pitch(), p.hin_stride, p.hout_stride, (int)p.leg_plc, (int)p.rated, (int)p.updown, (int)p.rational, (int)p.ratios, (int)p.data,
	       (int)p.open, p.common, p.max_ratio, p.n, p.nconf, p.len, p.leg_codec.size(), p.generic.size(), p.kinds.size(), (int)p.offgrid, p.off_num,
	       p.off_den, p.off_fin, p.off_fout);
	for (size_t s = 0; s < p.ratio.size(); ++s) printf("%s%02x", s ? "," : "", p.ratio[s]);
	printf(" kind_bytes=");
	for (size_t s = 0; s < p.kind_ratio.size(); ++s) printf("%s%02x", s ? "," : "", p.kind_ratio[s]);
	printf(" rates=");
	for (size_t s = 0; s < p.leg_rate.size(); ++s) printf("%s%d", s ? "," : "", p.leg_rate[s]);
	printf("\n");
	return 0;
}
