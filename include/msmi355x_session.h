/* msmi355x_session.h -- mi_session's membership without a drain, and legs at their own rate and codec (libmsmi355x.so,
 * MI355X / gfx950).
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
 * Out of scope: mi_volume_params and input gain per change (the waiting setters'); growing nstreams; a seat changing its kind
 * at a JOIN (mi_session_create_legs below: a JOIN re-seats the seat's own kind); the plugin's fused legs and server legs. */
#define MI_SESSION_JOIN 1  /* a NEW endpoint takes the seat; a seat that is taken is replaced (leave + join) */
#define MI_SESSION_LEAVE 2 /* the seat is unplumbed */
typedef struct mi_session_change {
	int32_t stream, op;
} mi_session_change;
int mi_session_change_members(mi_session *s, const mi_session_change *h_changes, int count);

/* Legs at their own rate and codec around ONE canceller rate: what plumb_to_conf hangs on every endpoint's pin -- its own
 * decoder, encoder and two resamplers (audioconference.c:226-251) -- for a batch whose legs differ: 8 kHz mu-law and A-law
 * trunks beside 16 kHz wideband and 48 kHz members in one conference, each with its echo canceller.
 * cfg->rate is the canceller's, the meter's and the mixer's rate; h_legs [cfg->nstreams] names every leg's rate in Hz -- one
 * rate in and out, as an endpoint has -- and its codecs, MI_SESSION_PCM16 | _PCMA | _PCMU.  cfg->in_rate, out_rate, mic_codec and
 * out_codec are not read; every other field keeps its meaning (tail_ms, agc, ref_loopback, ref_delay_ms, plc, stagger,
 * use_graphs -- except that with legs that differ AND plc the tick's kernels are launched directly, use_graphs or not: the
 * per-leg concealer is not captured into the slots' graphs).  h_legs == NULL is mi_session_create exactly.  Legs that all name one kind give exactly the session
 * mi_session_create builds with in_rate = out_rate = that rate and those codecs: its kernels, its tick bytes, its rows.
 * Supported: cfg->rate / leg rate in {1, 2, 3, 6}, the leg's rate a multiple of 800 -- 8, 16, 24 and 48 kHz legs in a 48 kHz
 * session, 8 and 16 kHz in a 16 kHz one.  MI_ENOTSUP, before anything is allocated, the message naming the leg, both rates
 * and the reason: a leg above cfg->rate; any other ratio (4, 3/2, a : b, 44.1 kHz); a codec outside the three; with cfg->plc
 * a rate the concealer does not serve.
 * With legs that differ, `mic` and `out` are BYTE rows at one pitch each, the widest leg's tick in bytes rounded up to 16:
 * mi_session_tick_bytes returns the pitches, a leg fills or receives the first mi_session_leg_bytes of its row; bytes of a mic
 * row past that are never used (a load of 16 bytes may fetch up to 8 of them inside the pitch and discards them), bytes of an
 * out row past that never written.  The reference rows stay [nstreams][rate / 100]
 * int16; with ref_loopback the reference is the kept mix at `rate`.  mi_session_events, mi_session_change_members, the
 * controls and reports of msmi355x_session_controls.h and the waiting calls all work on such a session: a JOIN (and
 * mi_session_add_member, mi_session_reset_streams) re-seats the seat's OWN kind and also zeroes both of that leg's resampler
 * histories -- 47 samples in front of the canceller, ratio x 48 - 1 behind the mix -- and with cfg->plc starts its concealer
 * over.  Every leg's out row is written every tick, member or not, as the uniform session's encoder does.
 * mi_session_leg_rate / _codec / _bytes answer for any session (mi_session_create's: its one kind, in_rate and the tick
 * bytes); MI_EINVAL for a null session or a stream out of range.
 * Out of scope: legs above the canceller's rate; ratios 4, 3/2, 2/3, a : b and 44.1 kHz (mi_bridge's later constructors show
 * how); a seat changing kind at a JOIN (mi_bridge_create_open shows how); tail_ms or a canceller rate per leg; codecs other
 * than G.711 and 16-bit PCM; the plugin's fused legs. */
typedef struct mi_session_leg {
	int32_t rate, mic_codec, out_codec; /* Hz; MI_SESSION_PCM16 | _PCMA | _PCMU */
} mi_session_leg;
/* The library's symbols behind the four calls.  Every exported mi_session_* symbol belongs to one of the lists the older entry
 * points were frozen with, so these carry a prefix of their own and the documented names are the inline functions below. */
int mi_legs_session_create(mi_ctx *ctx, const mi_session_config *cfg, const mi_session_leg *h_legs /* [nstreams] */, mi_session **out);
int mi_legs_session_rate(const mi_session *s, int stream);
int mi_legs_session_codec(const mi_session *s, int stream, int *mic_codec, int *out_codec);
int mi_legs_session_bytes(const mi_session *s, int stream, int *mic_bytes, int *out_bytes);

static inline int mi_session_create_legs(mi_ctx *ctx, const mi_session_config *cfg, const mi_session_leg *h_legs /* [nstreams] */, mi_session **out) {
	return mi_legs_session_create(ctx, cfg, h_legs, out);
}
static inline int mi_session_leg_rate(const mi_session *s, int stream) { return mi_legs_session_rate(s, stream); }
static inline int mi_session_leg_codec(const mi_session *s, int stream, int *mic_codec, int *out_codec) {
	return mi_legs_session_codec(s, stream, mic_codec, out_codec);
}
static inline int mi_session_leg_bytes(const mi_session *s, int stream, int *mic_bytes, int *out_bytes) {
	return mi_legs_session_bytes(s, stream, mic_bytes, out_bytes);
}

#ifdef __cplusplus
}
#endif
#endif
