// conference.hpp -- MSAudioConference's bookkeeping that mi_session (session.hip) and mi_bridge (bridge.hip) share: host
// code only.  mi::Roster (who is a member, in which order they joined, who is elected) is plain C++ and calls nothing in
// the library; the helpers below it are the halves of the owners' read-outs and resets that go through an mi_volume.
// mi::ConferenceBook (conference_book.hpp) holds the roster next to the changes on their way to the device.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/msmi355x.h"

namespace mi {

// ms_audio_conference_process_events' election in mixer mode (src/voip/audioconference.c:436-452): per conference the
// unmuted member whose MS_VOLUME_GET_MAX -- the maximum of the smoothed energy over a one-second window
// (msvolume.c:143-148,:402-406), in dBm0 -- is the largest and above -30 dB (audioconference.c:31).  max_lin, flags and
// joined are [nconf * mm]; joined = the order in which the members joined (the conference's member LIST is in joining
// order, bctbx_list_append :328).
inline void elect_active_speakers(const float *max_lin, const uint8_t *flags, const uint32_t *joined, int nconf, int mm, int32_t *h_winner,
                                  float *h_max_db) {
	for (int c = 0; c < nconf; ++c) {
		float best = -120.f; // MS_VOLUME_DB_LOWEST
		int win = -1;
		uint32_t win_joined = 0;
		for (int m = 0; m < mm; ++m) {
			const size_t i = (size_t)c * mm + m;
			const uint8_t f = flags[i];
			if (!(f & MI_MIX_LINKED) || !(f & MI_MIX_ACTIVE)) continue; // not plumbed / muted (:445)
			const float lin = max_lin[i];
			const float db = lin == 0 ? -120.f : 10 * log10f(lin); // ms_volume_linear_to_dbm0 msvolume.c:565-568
			if (db <= -30.0f) continue;
			// the list is walked in joining order and a later member must be strictly louder (:449): of equals, the earliest joiner
			if (db > best || (db == best && win >= 0 && joined[i] < win_joined)) best = db, win = (int)i, win_joined = joined[i];
		}
		h_winner[c] = win;
		if (h_max_db) h_max_db[c] = best;
	}
}

// Conference membership and the active-speaker election (MSAudioConference, src/voip/audioconference.c) of nconf
// conferences of mm mixer pins each; stream = conference * mm + pin.
struct Roster {
	std::vector<uint8_t> flags;   // MI_MIX_* per stream as last set (default: every pin linked, active, output on)
	std::vector<uint32_t> joined; // the conference's member LIST is in joining order (bctbx_list_append, audioconference.c:328): of two
	uint32_t join_seq = 0;        // equally loud members the election takes the one that joined first (:449 compares strictly)
	int nconf = 0, mm = 0;

	void init(int n, int members) { // created full: joined in pin order
		nconf = n / members, mm = members;
		flags.assign((size_t)n, (uint8_t)(MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT));
		joined.resize((size_t)n);
		for (int i = 0; i < n; ++i) joined[(size_t)i] = ++join_seq;
	}
	void set_flags(const uint8_t *h_flags) { flags.assign(h_flags, h_flags + flags.size()); }
	bool is_member(int stream) const { return (flags[(size_t)stream] & MI_MIX_LINKED) != 0; }
	// ms_audio_conference_add_member (:322-345): the pin becomes linked / active / output enabled, the member is appended
	// to the list.  false: is a member already
	bool join(int stream) {
		if (is_member(stream)) return false;
		flags[(size_t)stream] = MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT;
		joined[(size_t)stream] = ++join_seq;
		return true;
	}
	// ms_audio_conference_remove_member (:366-374): the pin is unplumbed -- it neither contributes nor receives.  false: is no member
	bool leave(int stream) {
		if (!is_member(stream)) return false;
		flags[(size_t)stream] = 0;
		return true;
	}
	int count(int conference) const { // plumbed pins (ms_audio_conference_get_size :390-392)
		int c = 0;
		for (int m = 0; m < mm; ++m) c += is_member(conference * mm + m);
		return c;
	}
	// max_lin [nconf * mm]: every stream's MS_VOLUME_GET_MAX, linear -> winner [nconf] (stream or -1), max_db [nconf] or null
	void elect(const float *max_lin, int32_t *winner, float *max_db) const {
		elect_active_speakers(max_lin, flags.data(), joined.data(), nconf, mm, winner, max_db);
	}
};

// a leg's meter as a NEW MSVolume has it: fresh state, the one-second maximum window not started
inline int reset_meters(mi_volume *vol, int first, int count) {
	mi_volume_state st;
	memset(&st, 0, sizeof(st));
	st.gain = st.target_gain = 1; // volume_init msvolume.c:92
	st.ng_gain = 1;               // :112
	std::vector<mi_volume_state> all((size_t)count, st);
	const int rc = mi_volume_set_state(vol, first, count, all.data());
	return rc != MI_OK ? rc : mi_volume_reset_max(vol, first, count);
}

// the level meter read-out (MS_VOLUME_GET_LINEAR) an active-speaker detector polls.  fresh: the seats a NEW endpoint has
// taken whose meter the device has not been handed yet (mi_session_change_members: it travels with the next tick) -- a new
// MSVolume has metered nothing
inline int get_levels(mi_volume *vol, int n, float *h_linear, const std::vector<int32_t> *fresh = nullptr) {
	std::vector<mi_volume_state> st((size_t)n);
	const int rc = mi_volume_get_state(vol, 0, n, st.data());
	if (rc != MI_OK) return rc;
	for (int i = 0; i < n; ++i) h_linear[i] = st[(size_t)i].energy; // volume_get_linear msvolume.c:129-134
	if (fresh)
		for (const int32_t s : *fresh) h_linear[(size_t)s] = 0.f;
	return MI_OK;
}

// ms_audio_conference_process_events' election in mixer mode (:436-452) on the meters' one-second maxima.  The windows run
// on the device, one record per tick (msvolume.c:404): the caller's clock is not needed
// (fresh: as get_levels' -- ortp_extremum_init: 0 before the first record)
inline int active_speakers(mi_volume *vol, const Roster &r, int32_t *h_winner, float *h_max_db, const std::vector<int32_t> *fresh = nullptr) {
	std::vector<float> mx(r.flags.size());
	const int rc = mi_volume_get_max(vol, 0, (int)mx.size(), mx.data());
	if (rc != MI_OK) return rc;
	if (fresh)
		for (const int32_t s : *fresh) mx[(size_t)s] = 0.f;
	r.elect(mx.data(), h_winner, h_max_db);
	return MI_OK;
}

} // namespace mi
