// session_open_check.cpp -- mi::ConferenceBook (csrc/conference_book.hpp), the host's bookkeeping under mi_bridge and mi_session,
// driven through its membership half (csrc/seat_changes.hpp, mi::Roster of csrc/conference.hpp) by the very calls
// mi_session's entry points make, without a GPU or the library
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

#include "../../mediastreamer2_amd/csrc/conference_book.hpp"

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
	mi::ConferenceBook book;
	book.init(n, mm, slots, nullptr);
	const mi::Roster &roster = book.roster;
	const mi::SeatChanges &changes = book.seats;
	std::vector<mi_seat_cmd> row((size_t)n);
	std::vector<mi_ctl_cmd> ctl_row((size_t)n);
	for (int i = 4; i < argc; ++i) {
		const std::string step = argv[i];
		g_error[0] = 0;
		if (step == "s") {
			int k = -1, kc = -1;
			book.stage(row.data(), ctl_row.data(), &k, &kc);
			if (k < 0 || k > n || kc != 0) return 3;
			book.submitted();
			printf("row");
			for (int j = 0; j < k; ++j) printf(" %d:%d:%d", row[(size_t)j].stream, row[(size_t)j].op, row[(size_t)j].flags);
			printf("\n");
		} else if (step.rfind("r/", 0) == 0 || step.rfind("a/", 0) == 0) {
			const int s = atoi(step.c_str() + 2);
			if (s < 0 || s >= n) return 2;
			printf("roster %d\n", step[0] == 'r' ? book.remove_member("mi_session_remove_member", s) : book.add_member("mi_session_add_member", s));
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
			const int rc = book.change_uniform_members("mi_session_change_members", "MI_SESSION_JOIN (1) or MI_SESSION_LEAVE (2)",
			                                           list.empty() ? nullptr : list.data(), count, 160);
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
