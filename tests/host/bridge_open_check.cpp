// bridge_open_check.cpp -- csrc/bridge_plan.hpp's plan for seats that change hands and its validation of a change list, run
// alone, without a GPU or the library (tests/test_bridge_open_cpu.py builds this with the address and undefined-behaviour
// sanitizers and reads its one line):
//   bridge_open_check open   CONF_RATE MEMBERS PLC  RATE:IN:OUT... / RATE:IN:OUT...                 plan_open: legs / admitted kinds
//   bridge_open_check closed CONF_RATE MEMBERS PLC  RATE:IN:OUT...                                  plan_legs(RULES_RATIOS)
//   bridge_open_check change CONF_RATE MEMBERS PLC  RATE:IN:OUT... / RATE:IN:OUT... / SEAT... / STREAM:OP:RATE:IN:OUT...
//       check_changes on plan_open's plan (on plan_legs' where the second section is the word `closed`), the SEATs no members
// Prints `rc text` of a refusal, `0 name=value ...` of a plan, `0 ratio=b,b,...` of an accepted change list.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../mediastreamer2_amd/csrc/bridge_plan.hpp"

static char g_error[1024];
void mi::set_error(const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_error, sizeof(g_error), fmt, ap);
	va_end(ap);
}
// plc.hip's, which is not linked here, restated in its first rule: enough to see WHAT the plan puts to it and under which name
int mi_plc_check_rate(const char *fn, const char *what, int index, int rate) {
	if (rate >= 8000 && rate <= 48000) return MI_OK;
	mi::set_error("%s: %s %d at %d Hz: the concealer serves 8000 to 48000 Hz", fn, what, index, rate);
	return MI_ENOTSUP;
}

static std::string bools(const bool *v, int n) {
	std::string s;
	for (int i = 0; i < n; ++i) s += v[i] ? '1' : '0';
	return s;
}

template <class T>
static std::string list(const std::vector<T> &v) {
	std::string s = "[";
	for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string((long long)v[i]);
	return s + "]";
}

int main(int argc, char **argv) {
	if (argc < 6) return 2;
	const std::string mode = argv[1];
	std::vector<std::vector<std::string>> sec(1);
	for (int i = 5; i < argc; ++i) {
		if (!strcmp(argv[i], "/")) sec.emplace_back();
		else sec.back().push_back(argv[i]);
	}
	sec.resize(4);
	auto legs_of = [](const std::vector<std::string> &v, std::vector<mi_bridge_leg> *out) {
		for (const std::string &a : v) {
			mi_bridge_leg l;
			if (sscanf(a.c_str(), "%d:%d:%d", &l.rate, &l.in_codec, &l.out_codec) != 3) return false;
			out->push_back(l);
		}
		return true;
	};
	std::vector<mi_bridge_leg> legs, admit;
	const bool closed = mode == "closed" || (sec[1].size() == 1 && sec[1][0] == "closed");
	if (!legs_of(sec[0], &legs) || legs.empty() || (!closed && !legs_of(sec[1], &admit))) return 2;
	mi_bridge_config cfg = {};
	cfg.nstreams = (int32_t)legs.size(), cfg.rate = atoi(argv[2]), cfg.members_per_conference = atoi(argv[3]), cfg.plc = atoi(argv[4]);
	Plan p;
	// (an empty vector's data() may be null: nadmit == 0 must take either)
	const int rc = closed ? plan_legs(RULES_RATIOS, &cfg, legs.data(), &p) : plan_open(RULES_RATIOS, &cfg, legs.data(), admit.data(), (int)admit.size(), &p);
	if (rc != MI_OK) return printf("%d %s\n", rc, g_error) < 0;
	if (mode == "change") {
		std::vector<uint8_t> flags(legs.size(), MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT), ratio;
		for (const std::string &a : sec[2]) flags.at((size_t)atoi(a.c_str())) = 0;
		std::vector<mi_bridge_change> ch;
		for (const std::string &a : sec[3]) {
			mi_bridge_change c;
			if (sscanf(a.c_str(), "%d:%d:%d:%d:%d", &c.stream, &c.op, &c.leg.rate, &c.leg.in_codec, &c.leg.out_codec) != 5) return 2;
			ch.push_back(c);
		}
		const int cr = check_changes(p, flags.data(), ch.data(), (int)ch.size(), &ratio);
		if (cr != MI_OK) return printf("%d %s\n", cr, g_error) < 0;
		return printf("0 ratio=%s\n", list(ratio).c_str()) < 0;
	}
	static const char *const FAMILY[] = {"TICK", "RATED", "LEGS", "LEGS_RATED", "UPDOWN", "RATIONAL", "RATIOS"};
	std::vector<uint8_t> generic = p.generic;
	std::sort(generic.begin(), generic.end());
	printf("0 family=%s wide=%d row_w=%d lds=%zu scratch_off=%d scratch_per_wave=%d hin_stride=%d hout_stride=%d in_bytes=%zu out_bytes=%zu "
	       "pitch=%d used=%s above=%s r32=%d%d generic=%s leg_plc=%d data=%d sum_off=%d nslice=%d max_ratio=%d in_codec=%d out_codec=%d n=%d nconf=%d open=%d "
	       "kinds=%zu leg_rate=%s leg_codec=%s ratio=%s\n",
	       FAMILY[p.family], p.wide, p.row_w, p.lds, p.scratch_off, p.scratch_per_wave, p.hin_stride, p.hout_stride, p.in_bytes, p.out_bytes, p.pitch,
	       bools(p.used, 7).c_str(), bools(p.above, 7).c_str(), (int)p.r32_above, (int)p.r32_below, list(generic).c_str(), (int)p.leg_plc, (int)p.data,
	       p.sum_off, p.nslice, p.max_ratio, p.cfg.in_codec, p.cfg.out_codec, p.n, p.nconf, (int)p.open, p.kinds.size(), list(p.leg_rate).c_str(),
	       list(p.leg_codec).c_str(), list(p.ratio).c_str());
	return 0;
}
