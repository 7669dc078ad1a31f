/* msmi355x_session_controls.h -- mi_session's mute, gain, levels and speaker election without a drain (libmsmi355x.so,
 * MI355X / gfx950).
 *
 * mi_session's control plane in msmi355x.h -- mi_session_set_controls, mi_session_get_levels, mi_session_active_speakers --
 * waits for every tick submitted and copies whole [nstreams] arrays: a mute toggle or a level poll empties the three-tick
 * pipeline that mi_session_change_members (msmi355x_session.h) leaves alone.  A conference server toggles mutes in most 10 ms
 * ticks and polls the levels for every RTP packet it sends (the mixer-to-client audio-level extension).  The entry points here
 * steer and observe a running session without ever waiting for the device, as their twins in msmi355x_bridge.h do for
 * mi_bridge.  The waiting calls keep their semantics and their waits.
 *
 * The symbols live in libmsmi355x.so beside those of msmi355x.h; mi_abi_version() covers this header too.  The calling
 * conventions are msmi355x.h's: MI_OK or a negative MI_E* code, mi_last_error() for the message, one thread at a time per
 * context. */
#ifndef MSMI355X_SESSION_CONTROLS_H
#define MSMI355X_SESSION_CONTROLS_H

#include "msmi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ms_audio_conference_mute_member (audioconference.c:377-388), MS_AUDIO_MIXER_SET_ACTIVE / _ENABLE_OUTPUT / _SET_INPUT_GAIN
 * (audiomixer.c:372-414), per seat.  The calling contract is mi_session_change_members': the changes travel with the NEXT tick
 * submitted -- the tick being filled, if one is acquired -- and the device applies them in stream order ahead of that tick's
 * kernels (controls_kernel, csrc/controls.hip; with cfg.use_graphs ahead of the slot's graph); ticks submitted earlier are
 * untouched, collected or not.  The call contains no stream, event or device synchronise, no blocking copy and no allocation.
 * Several calls before one submit merge per seat AND per field, the last one wins.
 *   MI_CTL_FLAGS: the pin's MI_MIX_ACTIVE and MI_MIX_OUTPUT bits are taken from `flags` (mute: ACTIVE clear; listen-only off:
 *     OUTPUT clear).  MI_MIX_LINKED is membership's: any bit outside ACTIVE | OUTPUT is MI_EINVAL.  The seat must be a member
 *     when the call is made; earlier mi_session_change_members calls not yet submitted count.  Clearing MI_MIX_OUTPUT does not
 *     clear what the seat last heard, as mi_session_set_controls does not.
 *   MI_CTL_GAIN:  the pin's input gain, on any seat; it survives joins.
 *   (The session has no public setter for mi_volume_params, so there is no MI_CTL_VOLUME here: bit 4 is an unknown `what`.)
 * Inside a tick membership changes are applied first, then controls: MI_SESSION_JOIN plus MI_CTL_FLAGS with ACTIVE clear
 * before one submit gives a member that arrives muted.  What a tick carries is staged at submit from the host's own mirrors
 * of flags and gains, which the waiting calls (mi_session_set_controls, _add_member, _remove_member) update too: a waiting
 * call made between a change and its submit has the last word on the fields it sets, and device and host agree after that
 * tick.  A LEAVE after an MI_CTL_FLAGS on the same seat leaves the seat unplumbed.
 * Nothing of a refused call is applied, and the message names the entry.  MI_EINVAL: a NULL session; count < 0, or count > 0
 * with a NULL h_changes; a stream out of range; an empty or unknown `what`; one stream twice in one call; the two rules of
 * MI_CTL_FLAGS.  count == 0 is MI_OK and does nothing. */
#define MI_CTL_FLAGS 1u
#define MI_CTL_GAIN 2u
typedef struct mi_session_control {
	int32_t stream;
	uint32_t what;  /* MI_CTL_* */
	uint32_t flags; /* MI_CTL_FLAGS: MI_MIX_ACTIVE | MI_MIX_OUTPUT */
	float gain;     /* MI_CTL_GAIN */
} mi_session_control;
int mi_session_change_controls(mi_session *s, const mi_session_control *h_changes, int count);

/* Levels and the election come back WITH the tick.  mi_session_set_reports(s, MI_REPORT_SPEAKERS | MI_REPORT_LEVELS) -- 0: off,
 * the default -- is a configuration call: it may wait once and allocate; nothing per tick does.  From the next submit on one
 * kernel (report_kernel, csrc/controls.hip; with cfg.use_graphs behind the slot's graph) runs behind the tick's kernels, reads
 * what the tick left and writes a report block that is downloaded with the tick's output.  mi_session_collected_report hands
 * out the block of the tick LAST COLLECTED: pointers into pinned memory, valid for as long as that tick's output is; it never
 * waits.  MI_EINVAL: nothing collected yet, reports were off for that tick, or its slot has been submitted again.  At most 64
 * members per conference (MI_ENOTSUP).
 *   MI_REPORT_LEVELS:   levels [nstreams], every stream's MS_VOLUME_GET_LINEAR: bit for bit what mi_session_get_levels returns
 *     when that tick is the last one submitted (the raw meter, muted members included).
 *   MI_REPORT_SPEAKERS: per conference ms_audio_conference_process_events' election (audioconference.c:436-452): winner
 *     [nconf] (stream or -1), max_lin [nconf] (the winner's one-second maximum, linear, or 0) and max_db [nconf], worked out
 *     on the host in this call from max_lin with the waiting call's own expression, so the float is the one
 *     mi_session_active_speakers gives.  Eligible are the plumbed, unmuted members whose maximum is above -30 dBm0 -- exactly
 *     the waiting call's set: the kernel compares with the smallest float whose dBm0 value is above -30.0f, derived once with
 *     the host's libm.  Of the eligible the largest maximum wins, of equal maxima the member that joined first.
 *   A VISIBLE, DELIBERATE DIFFERENCE (in the manner of SURVEY Appendix A): the kernel compares LINEAR maxima, the reference dBm0
 *   floats.  Where two eligible members' maxima are different floats whose dBm0 values round to the same float -- a band of
 *   about four ulp near -30 dBm0 -- the reference takes the earlier joiner and the report the louder.
 *   mi_session_active_speakers stays the reference-exact call. */
#define MI_REPORT_SPEAKERS 1u
#define MI_REPORT_LEVELS 2u
typedef struct mi_session_report {
	uint64_t seq;  /* the tick's sequence number: 0 for the first tick the session was submitted */
	uint32_t what; /* MI_REPORT_* as they were set when the tick was submitted */
	int32_t nstreams, nconf;
	const float *levels;   /* [nstreams], NULL without MI_REPORT_LEVELS */
	const int32_t *winner; /* [nconf], NULL without MI_REPORT_SPEAKERS, as are the next two */
	const float *max_lin;  /* [nconf] */
	const float *max_db;   /* [nconf]; -120 (MS_VOLUME_DB_LOWEST) where nobody was elected */
} mi_session_report;
int mi_session_set_reports(mi_session *s, uint32_t what);
int mi_session_collected_report(mi_session *s, mi_session_report *out);

#ifdef __cplusplus
}
#endif
#endif
