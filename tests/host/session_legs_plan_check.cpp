// session_legs_plan_check.cpp -- csrc/session_plan.hpp run alone, without a GPU or the library (tests/test_session_legs_cpu.py
// builds this with the address and undefined-behaviour sanitizers and reads its one line):
//   session_legs_plan_check RATE MEMBERS PLC RATE:MIC:OUT...
// Prints `rc text` of a refusal, or `0 uniform=... tick_bytes=MIC,OUT ...` with the per-leg lists comma-separated.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../mediastreamer2_amd/csrc/session_plan.hpp"

static char g_error[1024];
void mi::set_error(const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_error, sizeof(g_error), fmt, ap);
	va_end(ap);
}
// plc.hip's, which is not linked here: the concealer's refusals are reached through the library
// (tests/test_session_legs_cpu.py::test_the_library_refuses_before_it_asks_for_a_device)
int mi_plc_check_rate(const char *, const char *, int, int) { return MI_OK; }

template <class F>
static void list(const char *name, int n, F value) {
	printf(" %s=", name);
	for (int s = 0; s < n; ++s) printf("%s%d", s ? "," : "", (int)value(s));
}

int main(int argc, char **argv) {
	if (argc < 5) return 2;
	std::vector<mi_session_leg> legs;
	for (int i = 4; i < argc; ++i) {
		mi_session_leg l;
		if (sscanf(argv[i], "%d:%d:%d", &l.rate, &l.mic_codec, &l.out_codec) != 3) return 2;
		legs.push_back(l);
	}
	mi_session_config cfg = {};
	cfg.nstreams = (int32_t)legs.size(), cfg.rate = atoi(argv[1]), cfg.members_per_conference = atoi(argv[2]), cfg.plc = atoi(argv[3]);
	cfg.tail_ms = 32;
	cfg.in_rate = 11025, cfg.out_rate = 22050, cfg.mic_codec = 7, cfg.out_codec = 9; // not read when the legs are given
	SessionPlan p;
	const int rc = plan_session_legs(&cfg, legs.data(), &p);
	if (rc != MI_OK) return printf("%d %s\n", rc, g_error) < 0;
	if (p.uniform)
		return printf("0 uniform=1 in_rate=%d out_rate=%d mic_codec=%d out_codec=%d rate=%d\n", p.cfg.in_rate, p.cfg.out_rate, p.cfg.mic_codec,
		              p.cfg.out_codec, p.cfg.rate) < 0;
	printf("0 uniform=0 tick_bytes=%zu,%zu pcm_pitch=%d hist_stride=%d,%d lds=%zu,%zu wave=%d,%d,%d max_ratio=%d", p.mic_pitch, p.out_pitch, p.pcm_pitch,
	       p.hin_stride, p.hout_stride, p.ingress_lds, p.egress_lds, p.in_row, p.in_scratch, p.out_scratch, p.max_ratio);
	list("ratio", p.n, [&](int s) { return p.ratio[(size_t)s]; });
	list("codec", p.n, [&](int s) { return p.codec[(size_t)s]; });
	list("mic_bytes", p.n, [&](int s) { return p.mic_bytes(s); });
	list("out_bytes", p.n, [&](int s) { return p.out_bytes(s); });
	list("up_hist", p.n, [&](int) { return session_up_hist(); });
	list("down_hist", p.n, [&](int s) { return session_down_hist(p.ratio[(size_t)s]); });
	printf("\n");
	return 0;
}
