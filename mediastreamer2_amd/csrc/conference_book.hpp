// conference_book.hpp -- mi::ConferenceBook: what the host keeps about a running batch of conferences between two submits, with
// one method for each thing an entry point of mi_bridge (bridge.hip) or mi_session (session.hip) does to it.  Plain C++, no HIP:
// tests/host/session_open_check.cpp and controls_check.cpp drive this very struct.  mi::ConferencePlane (controls.hpp) owns it.
#pragma once
#include "conference.hpp"
#include "control_changes.hpp"

namespace mi {

struct ConferenceBook {
	Roster roster;           // who is a member, in which order they joined (conference.hpp)
	SeatChanges seats;       // membership changes on their way to the device (seat_changes.hpp)
	ControlChanges controls; // control changes likewise, and the mirrors (control_changes.hpp)
	unsigned reports = 0;    // MI_REPORT_* of the ticks to come (controls.hpp); here only: any at all
	unsigned allowed = 0;    // the MI_CTL_* bits a change_controls entry may carry

	// initial: every seat's MSVolume parameters at creation -- the book then serves MI_CTL_VOLUME --, or null: it does not
	void init(int n, int members, int pipe_slots, const mi_volume_params *initial) {
		roster.init(n, members), seats.init(n, pipe_slots), controls.init(n, initial);
		allowed = MI_CTL_FLAGS | MI_CTL_GAIN | (initial ? MI_CTL_VOLUME : 0u);
	}
	int n() const { return (int)roster.flags.size(); }

	// ---- the calls that do not wait: the mirrors answer at once, the device follows with the next tick submitted
	// one entry of a membership list that has been checked.  A seat that is taken is replaced: leave + join, the NEW endpoint the
	// last of its conference's list.  The caller fills in its JOIN's kind
	SeatChanges::Pending &change_member(int32_t stream, uint8_t op) {
		const bool was = roster.leave(stream);
		SeatChanges::Pending &p = seats.note(stream, op, was);
		if (op & MI_SEAT_JOIN) roster.join(stream);
		return p;
	}
	// mi_session_change_members whole: uniform seats, a JOIN brings a tick of `len` samples (the concealer's batch: class 0)
	template <class Change>
	int change_uniform_members(const char *fn, const char *names, const Change *ch, int count, int32_t len) {
		const int rc = check_uniform_changes(fn, names, n(), roster.flags.data(), ch, count, &controls.scratch);
		for (int i = 0; rc == MI_OK && i < count; ++i) {
			SeatChanges::Pending &p = change_member(ch[i].stream, (uint8_t)ch[i].op);
			if (ch[i].op == MI_SEAT_JOIN) p.len = len;
		}
		return rc;
	}
	// mi_*_change_controls whole
	template <class Control>
	int change_controls(const char *fn, const Control *ch, int count) {
		const bool vol = (allowed & MI_CTL_VOLUME) != 0;
		int rc = check_controls(fn, n(), roster.flags.data(), allowed, ch, count, controls.scratch);
		if (rc != MI_OK || (vol && (rc = check_control_params(fn, ch, count)) != MI_OK)) return rc;
		for (int i = 0; i < count; ++i) {
			controls.apply(ch[i], roster.flags.data());
			if (vol) controls.apply_params(ch[i]);
		}
		return MI_OK;
	}

	// ---- the waiting calls' part in the mirrors: the device is written by their own blocking copies
	void set_controls(const uint8_t *h_flags, const float *h_gain) { // either may be null
		if (h_flags) roster.set_flags(h_flags);
		if (h_gain) controls.set_gains(h_gain);
	}
	void set_params(int first, int count, const mi_volume_params *h) { controls.set_params(first, count, h); }
	int add_member(const char *fn, int stream) { return roster.join(stream) ? (int)MI_OK : (set_error("%s: stream %d is a member already", fn, stream), (int)MI_EINVAL); }
	int remove_member(const char *fn, int stream) { return roster.leave(stream) ? (int)MI_OK : (set_error("%s: stream %d is no member", fn, stream), (int)MI_EINVAL); }

	// ---- submit: both command rows of the tick about to go, each with room for n, in this order: the seats' row with the pins'
	// flags as the roster has them now; with reports on, every JOIN's place in the joining order noted; the control row
	void stage(mi_seat_cmd *seat_row, mi_ctl_cmd *ctl_row, int *nseat, int *nctl) {
		*nseat = seats.stage(seat_row, roster.flags.data());
		if (reports)
			for (const int32_t s : seats.changed)
				if (seats.pending[(size_t)s].op & MI_SEAT_JOIN) controls.note(s, MI_CTL_JOINED);
		*nctl = controls.stage(ctl_row, roster.flags.data(), roster.joined.data());
	}
	void submitted() { seats.submitted(), controls.submitted(); } // the tick is on its way

	// ---- read-outs (the election is the roster's: mi::active_speakers, conference.hpp)
	std::vector<int32_t> joining() const { return seats.joining(); }
	int member_count(int conference) const { return conference < 0 || conference >= roster.nconf ? (int)MI_EINVAL : roster.count(conference); }
};

} // namespace mi
