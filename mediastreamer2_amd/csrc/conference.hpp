// conference.hpp -- MSAudioConference's bookkeeping that mi_session (session.hip) and mi_bridge (bridge.hip) share: host
// code only.
#pragma once
#include <cmath>
#include <cstdint>

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

} // namespace mi
