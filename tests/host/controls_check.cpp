// controls_check.cpp -- mi::ConferenceBook (csrc/conference_book.hpp), the host's bookkeeping under mi_bridge and mi_session,
// driven through its controls half (csrc/control_changes.hpp) and what it shares with membership (mi::Roster of
// csrc/conference.hpp, mi::SeatChanges of csrc/seat_changes.hpp) by the very calls the entry points make, without a GPU or the
// library (tests/test_controls_cpu.py builds this with the address and undefined-behaviour sanitizers and reads its lines):
//   controls_check bridge|session NSEATS MEMBERS STEP...
//     c/STREAM:WHAT:FLAGS:GAIN[:STATIC[:PEER]],...  a call, as mi_*_change_controls makes it: checked, then applied to the
//                                 mirrors (c/ alone: count 0); STATIC, PEER: the params' static_gain and peer (MI_CTL_VOLUME)
//     n/COUNT                     a call with `count` COUNT and a null list
//     m/STREAM:OP,...             mi_session_change_members (1 JOIN, 2 LEAVE)
//     r/STREAM  a/STREAM          the waiting remove_member / add_member's part in the roster
//     f/STREAM:FLAGS  g/STREAM:GAIN  v/STREAM:STATIC   the waiting set_controls (flags, gains) / set_volume_params' part
//     R/WHAT                      set_reports: with reports on a JOIN's place in the joining order rides in the control row
//     s                           a submit: both rows staged, then the tick on its way
//     thr                         the election's threshold, held against 10 * log10f > -30 for every float within 64 ulp, and 0
// Prints one line per step: `call RC [text]`, `seat STREAM:OP:FLAGS ...` and `ctl STREAM:WHAT:FLAGS:GAIN:JOINED:STATIC ...`,
// `thr HEXBITS ok|FAILED`; and at the end `state` with every seat's flags, gain, static gain and the pending fields.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../mediastreamer2_amd/csrc/conference_book.hpp"

static char g_error[1024];
void mi::set_error(const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_error, sizeof(g_error), fmt, ap);
	va_end(ap);
}

struct Control { // mi_bridge_control's layout
	int32_t stream;
	uint32_t what, flags;
	float gain;
	mi_volume_params params;
};
struct Change { int32_t stream, op; };

static mi_volume_params default_params() { // mi_volume_default_params'
	mi_volume_params p;
	memset(&p, 0, sizeof(p));
	p.static_gain = 1, p.vol_upramp = 0.4f, p.vol_fast_upramp = 1.2f, p.vol_downramp = 0.4f, p.ea_thres = 0.1f, p.ea_transmit_thres = 4;
	p.force = 4.0f, p.sustain_time = 200, p.ng_cut_time = 400, p.ng_threshold = 0.1f, p.ng_floorgain = 0.005f, p.peer = -1;
	return p;
}

int main(int argc, char **argv) {
	if (argc < 4) return 2;
	const bool bridge = !strcmp(argv[1], "bridge");
	const int n = atoi(argv[2]), mm = atoi(argv[3]);
	if (n <= 0 || mm <= 0 || n % mm) return 2;
	const char *fn = bridge ? "mi_bridge_change_controls" : "mi_session_change_controls";
	const mi_volume_params dp = default_params();
	mi::ConferenceBook book; // a bridge's serves MI_CTL_VOLUME: it is given initial parameters
	book.init(n, mm, 3, bridge ? &dp : nullptr);
	const mi::Roster &roster = book.roster;
	const mi::SeatChanges &seats = book.seats;
	const mi::ControlChanges &ctl = book.controls;
	std::vector<mi_seat_cmd> seat_row((size_t)n);
	std::vector<mi_ctl_cmd> ctl_row((size_t)n);
	for (int i = 4; i < argc; ++i) {
		const std::string step = argv[i];
		const char *arg = step.c_str() + (step.size() > 1 ? 2 : 0);
		g_error[0] = 0;
		if (step == "s") {
			int ks = -1, kc = -1;
			book.stage(seat_row.data(), ctl_row.data(), &ks, &kc);
			if (ks < 0 || ks > n || kc < 0 || kc > n) return 3;
			book.submitted();
			printf("seat");
			for (int j = 0; j < ks; ++j) printf(" %d:%d:%d", seat_row[(size_t)j].stream, seat_row[(size_t)j].op, seat_row[(size_t)j].flags);
			printf("\nctl");
			for (int j = 0; j < kc; ++j) {
				const mi_ctl_cmd &c = ctl_row[(size_t)j];
				printf(" %d:%d:%d:%g:%u:%g", c.stream, c.what, c.flags, c.gain, c.joined, c.params.static_gain);
			}
			printf("\n");
		} else if (step == "thr") {
			const float thr = mi::report_threshold();
			uint32_t bits;
			memcpy(&bits, &thr, 4);
			bool ok = !(10 * log10f(0.f) > -30.0f);
			for (int d = -64; d <= 64; ++d) {
				const uint32_t b = bits + (uint32_t)d;
				float x;
				memcpy(&x, &b, 4);
				ok = ok && ((10 * log10f(x) > -30.0f) == (x >= thr));
			}
			printf("thr %08x %s\n", bits, ok ? "ok" : "FAILED");
		} else if (step.rfind("R/", 0) == 0) {
			book.reports = (unsigned)atoi(arg); // (mi::ConferencePlane::set_reports, behind its checks)
		} else if (step.rfind("r/", 0) == 0 || step.rfind("a/", 0) == 0) {
			const int s = atoi(arg);
			if (s < 0 || s >= n) return 2;
			printf("roster %d\n", step[0] == 'r' ? book.remove_member("remove_member", s) : book.add_member("add_member", s));
		} else if (step.rfind("f/", 0) == 0 || step.rfind("g/", 0) == 0 || step.rfind("v/", 0) == 0) {
			int s = 0;
			float v = 0;
			if (sscanf(arg, "%d:%f", &s, &v) != 2 || s < 0 || s >= n) return 2;
			if (step[0] == 'f') { // mi_*_set_controls(h_flags): the whole array
				std::vector<uint8_t> f = roster.flags;
				f[(size_t)s] = (uint8_t)v;
				book.set_controls(f.data(), nullptr);
			} else if (step[0] == 'g') { // mi_*_set_controls(h_gain)
				std::vector<float> g = ctl.gain;
				g[(size_t)s] = v;
				book.set_controls(nullptr, g.data());
			} else { // mi_bridge_set_volume_params
				mi_volume_params p = dp;
				p.static_gain = v;
				book.set_params(s, 1, &p);
			}
		} else if (step.rfind("m/", 0) == 0) {
			std::vector<Change> list;
			for (const char *p = arg; *p;) {
				Change c;
				int used = 0;
				if (sscanf(p, "%d:%d%n", &c.stream, &c.op, &used) != 2) return 2;
				list.push_back(c);
				p += used;
				if (*p == ',') ++p;
			}
			const int rc = book.change_uniform_members("mi_session_change_members", "JOIN or LEAVE", list.data(), (int)list.size(), 160);
			printf("call %d %s\n", rc, g_error);
		} else if (step.rfind("c/", 0) == 0 || step.rfind("n/", 0) == 0) {
			std::vector<Control> list;
			int count = 0;
			if (step[0] == 'n') count = atoi(arg);
			else {
				for (const char *p = arg; *p;) {
					Control c;
					memset(&c, 0, sizeof(c));
					c.params = dp;
					int used = 0;
					if (sscanf(p, "%d:%u:%u:%f%n", &c.stream, &c.what, &c.flags, &c.gain, &used) != 4) return 2;
					p += used;
					if (*p == ':' && sscanf(p, ":%f%n", &c.params.static_gain, &used) == 1) p += used;
					if (*p == ':' && sscanf(p, ":%d%n", &c.params.peer, &used) == 1) p += used;
					list.push_back(c);
					if (*p == ',') ++p;
				}
				count = (int)list.size();
			}
			const int rc = book.change_controls(fn, list.empty() ? nullptr : list.data(), count);
			printf("call %d %s\n", rc, g_error);
		} else {
			return 2;
		}
	}
	printf("state flags=");
	for (int s = 0; s < n; ++s) printf("%d", roster.flags[(size_t)s]);
	printf(" gain=");
	for (int s = 0; s < n; ++s) printf("%g,", ctl.gain[(size_t)s]);
	printf(" static=");
	for (size_t s = 0; s < ctl.params.size(); ++s) printf("%g,", ctl.params[s].static_gain);
	printf(" pending=");
	for (const int32_t s : ctl.changed) printf("%d:%d,", s, ctl.what[(size_t)s]);
	printf(" members=");
	for (const int32_t s : seats.changed) printf("%d:%d,", s, seats.pending[(size_t)s].op);
	printf("\n");
	return 0;
}
