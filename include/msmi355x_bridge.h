/* msmi355x_bridge.h -- server-side conference bridge sessions of libmsmi355x.so (MI355X / gfx950).
 *
 * What a conference server runs per member (src/voip/audioconference.c:209-257, audiostream.c:1812-1832):
 *     decoder -> MSVolume (level / meter) -> MSAudioMixer pin -> encoder
 * for a batch of conferences, fed from host buffers, one 10 ms tick per submit.  No echo canceller: that is the
 * endpoint's job (mi_session, msmi355x.h, is the chain WITH one).  The whole tick of a conference is ONE kernel launch
 * (bridge_tick_kernel, csrc/bridge.hip): G.711 code words or 16-bit PCM in, every member's mix out as code words or PCM;
 * the decoded and levelled audio never leaves the chip.  An 8 kHz G.711 leg costs 160 bytes of HBM traffic per tick
 * (80 code bytes in, 80 out) plus its meter state.  Results equal mi_g711_decode -> mi_volume_process ->
 * mi_mixer_process -> mi_g711_encode called one by one, bit for bit (tests/test_gpu_bridge.py).
 *
 * The symbols live in libmsmi355x.so beside those of msmi355x.h; mi_abi_version() covers both headers.  The calling
 * conventions are msmi355x.h's: MI_OK or a negative MI_E* code, mi_last_error() for the message, one thread at a time
 * per context.
 *
 * Out of scope, on purpose:
 *   - members at another rate than their conference (resamplers): mi_session and the MSFilter plugin do that;
 *   - jitter buffering and flow control: the host's, as with mi_session -- a leg whose packet is missing at the tick is
 *     flagged absent (or concealed, cfg.plc);
 *   - the plugin's server legs (MSMI355XServer*) keep their own launches: the plugin is built against the same ABI
 *     as its host double, which knows msmi355x.h only.
 */
#ifndef MSMI355X_BRIDGE_H
#define MSMI355X_BRIDGE_H

#include "msmi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_bridge mi_bridge;
typedef struct mi_bridge_config {
	int32_t nstreams;               /* legs in all; a multiple of members_per_conference (stream = conference * members + member) */
	int32_t members_per_conference; /* <= MI_MIXER_MAX_CHANNELS */
	int32_t rate;                   /* of every leg and of the mix; a multiple of 800: a tick is rate / 100 samples, whole 16-byte groups of PCM */
	int32_t in_codec;               /* MI_SESSION_PCM16 | MI_SESSION_PCMA | MI_SESSION_PCMU: what arrives (code words are samples at `rate`) */
	int32_t out_codec;              /* the same for what leaves */
	int32_t plc;                    /* 1: MSGenericPLC behind the decoder (msgenericplc.c): an absent leg is concealed and then counts as present */
} mi_bridge_config;

void mi_bridge_default_config(mi_bridge_config *c); /* 32 x 32 legs, 8 kHz, mu-law in and out, no plc */
/* MI_ENOTSUP: rate % 800 != 0, or a conference's tick that does not fit 64 KB of LDS (50 members up to 64 kHz) */
int mi_bridge_create(mi_ctx *ctx, const mi_bridge_config *cfg, mi_bridge **out);
void mi_bridge_destroy(mi_bridge *b);
/* bytes per stream and tick of the two host buffers */
int mi_bridge_tick_bytes(const mi_bridge *b, int *in_bytes, int *out_bytes);

/* pinned staging of the NEXT tick, to be filled in place: h_in [nstreams][rate/100] uint8 code words or int16 PCM;
 * h_present [nstreams] uint8, preset to 1 -- clear a leg's byte when nothing arrived from it for this tick: its row
 * is ignored, MSVolume gets no chunk (meter state, gain ramp and one-second window stay as they are, msvolume.c:480-486)
 * and the mixer reads silence for the pin (audiomixer.c:88).  With cfg.plc the leg is concealed instead (MI_PLC_CONCEAL)
 * and metered on what the concealer made. */
int mi_bridge_acquire(mi_bridge *b, void **h_in, uint8_t **h_present);
int mi_bridge_submit(mi_bridge *b);
/* the OLDEST tick in flight: waits for its download, returns the pinned output [nstreams][rate/100] (uint8 code words
 * or int16 PCM; valid until three more ticks have been submitted).  Rows of pins without MI_MIX_OUTPUT are not written. */
int mi_bridge_collect(mi_bridge *b, const void **h_out);
int mi_bridge_in_flight(const mi_bridge *b); /* up to three */

/* Control plane, as mi_session's: per-stream mixer flags (MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT) and input
 * gains, either may be NULL, arrays of [nstreams]; in effect for the ticks submitted afterwards. */
int mi_bridge_set_controls(mi_bridge *b, const uint8_t *h_flags, const float *h_gain);
/* MSVolume of streams [first, first + count): static gain, AGC, noise gate, DC removal.  Default:
 * mi_volume_default_params (a meter at unity gain).  An echo-limiter peer (params.peer != -1) is MI_ENOTSUP: a bridge
 * has no far end to limit against. */
int mi_bridge_set_volume_params(mi_bridge *b, int first, int count, const mi_volume_params *h_params);
/* a leg was replaced: the meter (and concealer) of streams [first, first + count) start over as new filters would */
int mi_bridge_reset_streams(mi_bridge *b, int first, int count);
/* MSAudioConference membership (audioconference.c:322-374), as mi_session_add_member / _remove_member: a bridge is
 * created full; remove unplumbs the pin and clears its output row, add plumbs it for a NEW endpoint (fresh meter) */
int mi_bridge_add_member(mi_bridge *b, int stream);
int mi_bridge_remove_member(mi_bridge *b, int stream);
int mi_bridge_member_count(const mi_bridge *b, int conference); /* plumbed pins, or MI_EINVAL */
int mi_bridge_get_levels(mi_bridge *b, float *h_linear);        /* MS_VOLUME_GET_LINEAR of every stream */
/* the election of audioconference.c:436-452, as mi_session_active_speakers (now_ms ignored: the ticks are the clock) */
int mi_bridge_active_speakers(mi_bridge *b, uint64_t now_ms, int32_t *h_winner, float *h_max_db);
/* the meters' running state and MS_VOLUME_GET_MAX (linear), for tests and monitoring; both wait for the ticks submitted */
int mi_bridge_get_volume_state(mi_bridge *b, int first, int count, mi_volume_state *h_state);
int mi_bridge_get_volume_max(mi_bridge *b, int first, int count, float *h_max);

#ifdef __cplusplus
}
#endif
#endif
