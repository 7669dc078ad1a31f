// roster_check.cpp -- TEST INFRASTRUCTURE: mi::Roster (mediastreamer2_amd/csrc/conference.hpp), the membership and election
// book mi_session and mi_bridge keep, driven next to the oracle's MSAudioConference (oracle/conference.c, restated from
// src/voip/audioconference.c) -- two conferences of four pins, every expected winner and size is the ORACLE's.  A program of
// its own, built by `make san` with -fsanitize=address,undefined; prints "ok roster <checks>" and exits 0, or says what differs.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mediastreamer2_amd/csrc/conference.hpp"
#include "../../oracle/ms2_oracle.h"

namespace {

constexpr int NCONF = 2, MM = 4, N = NCONF * MM;
constexpr uint8_t ON = MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT;
int checks = 0;

#define EXPECT(cond)                                                   \
	do {                                                               \
		++checks;                                                      \
		if (!(cond)) {                                                 \
			fprintf(stderr, "roster_check:%d: %s\n", __LINE__, #cond); \
			exit(1);                                                   \
		}                                                              \
	} while (0)

// the oracle's side: a conference and its member list in joining order (bctbx_list_append, audioconference.c:328)
struct Book {
	OrcConference c;
	std::vector<int> order;
	Book() {
		orc_conference_init(&c);
		for (int m = 0; m < MM; ++m) EXPECT(add() == m);
	}
	int add() {
		const int pin = orc_conference_add_member(&c, 0);
		order.push_back(pin);
		return pin;
	}
	void remove(int pin) {
		orc_conference_remove_member(&c, pin);
		for (size_t i = 0; i < order.size(); ++i)
			if (order[i] == pin) {
				order.erase(order.begin() + (long)i);
				break;
			}
	}
};

struct Rig {
	mi::Roster r;
	Book book[NCONF];
	std::vector<uint8_t> flags = std::vector<uint8_t>(N, ON);
	int32_t win[NCONF];
	float db[NCONF];

	Rig() { r.init(N, MM); }
	void mute(int s, bool muted) {
		flags[(size_t)s] = muted ? (uint8_t)(ON & ~MI_MIX_ACTIVE) : ON;
		r.set_flags(flags.data());
		orc_conference_mute_member(&book[s / MM].c, s % MM, muted);
	}
	void leave(int s) {
		EXPECT(r.leave(s));
		flags[(size_t)s] = 0;
		book[s / MM].remove(s % MM);
	}
	void join(int s) {
		EXPECT(r.join(s));
		flags[(size_t)s] = ON;
		EXPECT(book[s / MM].add() == s % MM); // the lowest free pin (audioconference.c:198-207) is the one given up
	}
	// one poll: the roster's winners and maxima are the oracle's (audioconference.c:436-452); sizes too (:390-392)
	void poll(const float (&lin)[N]) {
		r.elect(lin, win, db);
		for (int c = 0; c < NCONF; ++c) {
			float max_db[ORC_MIXER_MAX_CHANNELS];
			for (int m = 0; m < ORC_MIXER_MAX_CHANNELS; ++m) max_db[m] = m < MM ? orc_volume_linear_to_dbm0(lin[c * MM + m]) : ORC_VOLUME_DB_LOWEST;
			int pin;
			float wdb;
			orc_conference_process_events(&book[c].c, book[c].order.data(), max_db, &pin, &wdb);
			EXPECT(win[c] == (pin < 0 ? -1 : c * MM + pin));
			EXPECT(db[c] == wdb);
			EXPECT(r.count(c) == orc_conference_get_size(&book[c].c));
		}
	}
};

} // namespace

int main() {
	Rig g;
	// created full, joined in pin order
	for (int s = 0; s < N; ++s) EXPECT(g.r.is_member(s));
	EXPECT(g.r.count(0) == MM && g.r.count(1) == MM);
	// conference 0: pins 1 and 2 equally loud -- the earlier joiner; conference 1: its own loudest, whatever conference 0 does
	const float tie[N] = {0.01f, 0.2f, 0.2f, 0.05f, 0.02f, 0.03f, 0.3f, 0.04f};
	g.poll(tie);
	EXPECT(g.win[0] == 1 && g.win[1] == MM + 2); // audioconference.c:449 compares strictly: the first of equals stays
	// leave, then count: the other conference keeps its four
	g.leave(1);
	EXPECT(g.r.count(0) == MM - 1 && g.r.count(1) == MM && !g.r.is_member(1));
	g.poll(tie);
	EXPECT(g.win[0] == 2 && g.win[1] == MM + 2);
	// leave of a non-member and join of a member are reported and change nothing
	EXPECT(!g.r.leave(1));
	EXPECT(!g.r.join(2));
	g.poll(tie);
	EXPECT(g.win[0] == 2);
	// rejoin: the member goes to the end of the joining order (:328) and loses the tie it used to win
	g.join(1);
	EXPECT(g.r.count(0) == MM);
	g.poll(tie);
	EXPECT(g.win[0] == 2 && g.win[1] == MM + 2);
	const float louder[N] = {0.01f, 0.25f, 0.2f, 0.05f, 0.02f, 0.03f, 0.3f, 0.04f};
	g.poll(louder); // strictly louder, it wins from the end of the list too
	EXPECT(g.win[0] == 1);
	// a muted member is skipped (:445), and heard again when un-muted
	g.mute(1, true);
	g.poll(louder);
	EXPECT(g.win[0] == 2 && g.win[1] == MM + 2);
	g.mute(1, false);
	g.poll(louder);
	EXPECT(g.win[0] == 1);
	// a loudest member at or below -30 dB (:31; 0.001 = -30 dB, 0.0005 = -33 dB) elects nobody; conference 1 still has its speaker
	const float quiet[N] = {0.0002f, 0.0005f, 0.0001f, 0.f, 0.02f, 0.03f, 0.3f, 0.04f};
	g.poll(quiet);
	EXPECT(g.win[0] == -1 && g.db[0] == -120.f && g.win[1] == MM + 2);
	const float at[N] = {0.0002f, 0.001f, 0.0001f, 0.f, 0.f, 0.f, 0.f, 0.f};
	EXPECT(orc_volume_linear_to_dbm0(0.001f) == -30.f); // exactly at the threshold, which :449's `>` leaves out
	g.poll(at);
	EXPECT(g.win[0] == -1 && g.win[1] == -1);
	// the two conferences are independent: emptying one leaves the other's members, order and election alone
	for (int m = 0; m < MM; ++m) g.leave(m);
	EXPECT(g.r.count(0) == 0 && g.r.count(1) == MM);
	const float both[N] = {0.5f, 0.5f, 0.5f, 0.5f, 0.1f, 0.1f, 0.02f, 0.1f};
	g.poll(both);
	EXPECT(g.win[0] == -1 && g.win[1] == MM + 0);
	g.join(0), g.join(1); // a conference filled again elects again: the first joiner of the equally loud
	g.poll(both);
	EXPECT(g.win[0] == 0 && g.win[1] == MM + 0);
	printf("ok roster %d\n", checks);
	return 0;
}
