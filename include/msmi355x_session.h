/* msmi355x_session.h -- mi_session's membership without a drain (libmsmi355x.so, MI355X / gfx950).
 *
 * mi_session (msmi355x.h) is the chained path of a batch of call legs: MSResample -> MSSpeexEC (+ post-filter) -> MSVolume
 * -> MSAudioMixer, three ticks in flight.  Its membership calls there -- mi_session_add_member, _remove_member,
 * _reset_streams -- wait for every tick submitted: a fresh canceller alone is about 150 KB of state per leg at 48 kHz with a
 * 128 ms tail, written with blocking copies.  A server with tens of thousands of legs sees joins and leaves in every 10 ms
 * tick; the entry point here applies them on the device instead (session_roster_kernel, csrc/session_roster.hip), as
 * mi_bridge_change_members (msmi355x_bridge.h) does for the bridge.
 *
 * The symbol lives in libmsmi355x.so beside those of msmi355x.h; mi_abi_version() covers both headers.  The calling
 * conventions are msmi355x.h's: MI_OK or a negative MI_E* code, mi_last_error() for the message, one thread at a time per
 * context. */
#ifndef MSMI355X_SESSION_H
#define MSMI355X_SESSION_H

#include "msmi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MSAudioConference membership (audioconference.c:322-374) WITHOUT waiting for the device.  The changes travel with the NEXT
 * tick submitted -- the tick being filled, if one is acquired -- and the device applies them in stream order ahead of that
 * tick's kernels: ticks submitted earlier are untouched, collected or not.  The call contains no stream, event or device
 * synchronise, no blocking copy and no allocation.  Several calls before one submit merge per seat, the last one wins.
 * mi_session_member_count and the joining order of mi_session_active_speakers answer for the new roster as soon as the call
 * returns.  A session's legs are uniform, so a change names a seat and an op and nothing else.
 *   MI_SESSION_JOIN: a new endpoint brings everything mi_session_add_member -> mi_session_reset_streams gives the stream: the
 *     up-sampler's and down-sampler's history and position, a fresh canceller, a fresh meter (state, one-second window), a
 *     fresh concealer (cfg.plc), the three FIFOs empty and then, as at creation, the reference FIFO's ref_delay_ms of silence
 *     and the stream's stagger lead (cfg.stagger) in the microphone and reference FIFOs; nothing has been sent to the new leg
 *     yet (cfg.ref_loopback: its far end starts silent); the pin's flags MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT.  The
 *     pin's input gain and the seat's mi_volume_params stay as they are, as with mi_session_add_member.
 *   MI_SESSION_LEAVE: the pin's flags 0: the seat neither contributes nor receives, and what it last heard is cleared as
 *     mi_session_remove_member clears it -- the mix its row held is zero from that tick on.
 * Nothing of a refused call is applied, and the message names the entry.  MI_EINVAL: a NULL session; count < 0, or count > 0
 * with a NULL h_changes; a LEAVE of a seat that is no member; a stream out of range; an op outside the two; one stream twice
 * in one call.  count == 0 is MI_OK and does nothing.
 * mi_session_add_member, _remove_member, _reset_streams and _set_controls keep their behaviour and their waits.  One of those
 * calls made between a change and the submit that carries it has the last word on the pin's flags -- the change writes the
 * flags the roster holds when the tick is submitted --, so device and roster agree after that tick: a JOIN followed by
 * mi_session_remove_member leaves the seat unplumbed (with fresh filters), a LEAVE followed by mi_session_add_member leaves
 * it plumbed.
 * Out of scope: mi_volume_params and input gain per change (the waiting setters'); growing nstreams; legs of differing rate
 * or codec in one session (mi_bridge has those); the plugin's fused legs and server legs. */
#define MI_SESSION_JOIN 1  /* a NEW endpoint takes the seat; a seat that is taken is replaced (leave + join) */
#define MI_SESSION_LEAVE 2 /* the seat is unplumbed */
typedef struct mi_session_change {
	int32_t stream, op;
} mi_session_change;
int mi_session_change_members(mi_session *s, const mi_session_change *h_changes, int count);

#ifdef __cplusplus
}
#endif
#endif
