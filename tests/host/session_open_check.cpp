// session_open_check.cpp -- csrc/seat_changes.hpp, the host's bookkeeping of membership changes that mi_bridge_change_members and
// mi_session_change_members share, run alone with mi::Roster (csrc/conference.hpp), without a GPU or the library
// (tests/test_session_open_cpu.py builds this with the address and undefined-behaviour sanitizers and reads its lines):
//   session_open_check NSEATS MEMBERS SLOTS STEP...
//     c/STREAM:OP,STREAM:OP,...   a call, as mi_session_change_members makes it: checked, then merged per seat (c/ alone: count 0)
//     n/COUNT                     a call with `count` COUNT and a null list
//     r/STREAM  a/STREAM          the waiting mi_session_remove_member / _add_member's part in the roster
//     s                           a submit: the command row staged, then the tick on its way
// Prints one line per step: `call RC [text]`, `row STREAM:OP:FLAGS ...`, `roster RC`; and at the end `state` with the members,
// the seats with a change pending, those still to be cleared and how often.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../mediastreamer2_amd/csrc/conference.hpp"
#include "../../mediastreamer2_amd/csrc/seat_changes.hpp"

static char g_error[1024];
void mi::set_error(const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_error, sizeof(g_error), fmt, ap);
	va_end(ap);
}

struct Change { int32_t stream, op; }; // mi_session_change's layout

int main(int argc, char **argv) {
	if (argc < 4) return 2;
	const int n = atoi(argv[1]), mm = atoi(argv[2]), slots = atoi(argv[3]);
	if (n <= 0 || mm <= 0 || n % mm || slots < 1) return 2;
	mi::Roster roster;
	roster.init(n, mm);
	mi::SeatChanges changes;
	changes.init(n, slots);
	std::vector<mi_seat_cmd> row((size_t)n);
	for (int i = 4; i < argc; ++i) {
		const std::string step = argv[i];
		g_error[0] = 0;
		if (step == "s") {
			const int k = changes.stage(row.data(), roster.flags.data());
			if (k < 0 || k > n) return 3;
			changes.submitted();
			printf("row");
			for (int j = 0; j < k; ++j) printf(" %d:%d:%d", row[(size_t)j].stream, row[(size_t)j].op, row[(size_t)j].flags);
			printf("\n");
		} else if (step.rfind("r/", 0) == 0 || step.rfind("a/", 0) == 0) {
			const int s = atoi(step.c_str() + 2);
			if (s < 0 || s >= n) return 2;
			printf("roster %d\n", (step[0] == 'r' ? roster.leave(s) : roster.join(s)) ? 0 : (int)MI_EINVAL);
		} else if (step.rfind("c/", 0) == 0 || step.rfind("n/", 0) == 0) {
			std::vector<Change> list;
			int count = 0;
			if (step[0] == 'n') count = atoi(step.c_str() + 2);
			else {
				const char *p = step.c_str() + 2;
				while (*p) {
					Change c;
					int used = 0;
					if (sscanf(p, "%d:%d%n", &c.stream, &c.op, &used) != 2) return 2;
					list.push_back(c);
					p += used;
					if (*p == ',') ++p;
				}
				count = (int)list.size();
			}
			const int rc = mi::check_uniform_changes("mi_session_change_members", "MI_SESSION_JOIN (1) or MI_SESSION_LEAVE (2)", n,
			                                         roster.flags.data(), list.empty() ? nullptr : list.data(), count);
			for (int j = 0; rc == MI_OK && j < count; ++j) { // session.hip's loop
				const bool was = roster.leave(list[(size_t)j].stream);
				changes.note(list[(size_t)j].stream, (uint8_t)list[(size_t)j].op, was);
				if (list[(size_t)j].op == MI_SEAT_JOIN) roster.join(list[(size_t)j].stream);
			}
			printf("call %d %s\n", rc, g_error);
		} else {
			return 2;
		}
	}
	printf("state members=");
	for (int s = 0; s < n; ++s) printf("%d", roster.is_member(s) ? 1 : 0);
	printf(" pending=");
	for (const int32_t s : changes.changed) printf("%d:%d,", s, changes.pending[(size_t)s].op);
	printf(" clearing=");
	for (const int32_t s : changes.clearing) printf("%d:%d,", s, changes.clear_left[(size_t)s]);
	printf(" joined=");
	for (int s = 0; s < n; ++s) printf("%u,", roster.joined[(size_t)s]);
	printf("\n");
	return 0;
}
