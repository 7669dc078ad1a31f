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
 * Legs at their own rate (mi_bridge_create_rated): plumb_to_conf (audioconference.c:209-257) puts an in_resampler in front
 * of every mixer pin and an out_resampler behind it, configured from the endpoint's rate and the conference's.  A bridge
 * runs both inside the same launch (bridge_rated_kernel) for legs at the conference's rate / 2, / 3 or / 6 -- 8 and
 * 16 kHz legs in a 16, 24 or 48 kHz mix, the ratios of the resampler's tile-FIR kernels at quality 3 -- bit for bit
 * equal to mi_resampler_process_masked called in front of and behind mi_mixer_process (tests/test_gpu_bridge_rates.py).
 * MSVolume sits in front of the in_resampler: meter, one-second window and gain run on the leg's own samples at the
 * leg's rate.  An absent leg gives its in_resampler no block and a pin without MI_MIX_OUTPUT gives its out_resampler
 * none: their histories stay as they are.
 *
 * Legs with their own codec (mi_bridge_create_legs): plumb_to_conf hangs each endpoint's own decoder and encoder on its
 * mixer pin, so a leg's codec pair -- A-law, mu-law or 16-bit PCM in, and any of the three out -- is data as its rate is:
 * A-law and mu-law trunks in one narrowband mix, 8 kHz G.711 callers beside 16 kHz PCM members (whose codec the host
 * decodes) in one wideband conference.  Still one launch per tick (bridge_legs_kernel, with or without the resamplers) and
 * bit for bit the parts called one by one, mi_g711_decode / _encode once per law (tests/test_gpu_bridge_legs.py).  The
 * host rows are then BYTE rows: the pitch is the widest leg's tick in bytes rounded up to 16, a leg fills or receives the
 * first mi_bridge_leg_bytes of its row.  A bridge whose legs all name one pair is the one mi_bridge_create_rated builds:
 * the same kernels, pitch and tick bytes.
 *
 * Endpoints on either side of the mix (mi_bridge_create_endpoints): plumb_to_conf configures the two resamplers from the
 * endpoint's rate and the conference's whichever is larger (msconference.h:91-93), so a member ABOVE the mix -- a 48 kHz
 * PCM member, whose Opus decoder always hands out 48 kHz (msopus.c:88), in a 16 kHz room of G.711 trunks -- gets the
 * down-sampler in front of its pin and the up-sampler behind it.  Leg rate / conference rate may be 2, 3 or 6 as well;
 * legs below, at and above the mix share one conference and one launch per tick (bridge_updown_kernel, run only by a
 * bridge with a leg above its mix), bit for bit the parts called one by one (tests/test_gpu_bridge_endpoints.py).  The
 * rules are the rated bridge's: MSVolume in front of the in_resampler on the leg's rate / 100 samples at the leg's rate,
 * no block for the in_resampler of an absent leg nor for the out_resampler of a pin without MI_MIX_OUTPUT.  Byte rows at
 * one pitch as with mi_bridge_create_legs; the pitch, the widest leg's tick, may now exceed the conference's own.
 *
 * Loss concealment for legs of any rate and codec (mi_bridge_create_concealed): in the reference every G.711 and L16 leg has
 * MSGenericPLC behind its own decoder.  The constructor takes mi_bridge_create_endpoints' arguments and rules and lets
 * cfg.plc hold whatever the legs: where they differ in rate or codec the concealer is a batch PER LEG in front of the
 * bridge's unchanged kernel -- its streams grouped into rate classes, at most the seven rates one bridge can hold, the
 * decoders inside its RECEIVED pass (plc_legs_received_kernel, plc_legs_conceal_kernel, csrc/plc.hip) --: three launches and
 * the bridge's one per tick, bit for bit mi_g711_decode per law -> mi_plc_process per rate -> the plc-less bridge
 * (tests/test_gpu_bridge_concealed.py).  An absent leg (h_present[s] == 0) is concealed at its own rate / 100 samples, then
 * counts as present and is metered on what the concealer made, at its rate, in front of its in_resampler.
 *
 * Legs at 3/2 and 2/3 of the mix's rate (mi_bridge_create_rational): Speex ultra-wideband and AAC-ELD run at 32 kHz
 * (msspeex.c:133, aac-eld.c:69), SILK and Opus with a capped playback rate hand out 12 and 24 kHz (msopus.c:434-436), and
 * plumb_to_conf resamples such a member without asking.  The constructor takes mi_bridge_create_concealed's arguments and
 * rules, and leg rate : conference rate may also be 3 : 2 or 2 : 3 -- a 32 kHz member of a 48 kHz room, a 24 kHz member of a
 * 16 kHz one, 12 kHz in 8 kHz.  Legs at 1, 2, 3 or 6 below or above the mix and at 3/2 or 2/3 share one conference and one
 * launch per tick (bridge_rational_kernel, run only by a bridge with such a leg): the resampler's 3/2 and 2/3 tile-FIR
 * kernels at quality 3 inside the tick, bit for bit mi_resampler_process_masked in front of and behind mi_mixer_process
 * (tests/test_gpu_bridge_rational.py).  Rows, MSVolume, absent legs and pins without MI_MIX_OUTPUT as with
 * mi_bridge_create_endpoints; cfg.plc as with mi_bridge_create_concealed.
 *
 * Every pair of the VoIP rates 8 - 48 kHz (mi_bridge_create_ratios): the codecs mediastreamer2 plumbs into conferences run
 * at 8, 12, 16, 24, 32 and 48 kHz, and on that grid 8 : 32 and 12 : 48 (ratio 4), 12 : 16 and 24 : 32 (3/4 and 4/3) and
 * 12 : 32 (3/8 and 8/3) were left.  The constructor takes mi_bridge_create_rational's arguments and rules, and a leg may also
 * be at 4 or 1/4 of the mix -- the ratio-4 tile kernels of the resampler, bit for bit mi_resampler_process_masked where that
 * runs them: ticks of at most 576 samples on the wider side -- or stand a : b to it, leg rate : conference rate in lowest
 * terms, wherever both its resamplers have a direct table of at most 128 taps by the resampler's own design rule: a, b <= 8
 * and a ratio of at most 8/3 -- 4 : 3, 5 : 4, 5 : 3, 5 : 2, 6 : 5, 7 : 3 ... 8 : 3 and their inverses.  Such a leg runs the
 * resampler's generic-order arithmetic (one fused multiply-add chain per output over the taps of its polyphase row) inside
 * the tick, bit for bit mi_resampler_process_masked at every shape.  All of it shares one conference and one launch per tick
 * with the older forms (bridge_ratios_kernel, csrc/bridge_ratios.hip, run only by a bridge with such a leg;
 * tests/test_gpu_bridge_ratios.py).  Rows, MSVolume, absent legs and pins without MI_MIX_OUTPUT as with
 * mi_bridge_create_endpoints; cfg.plc as with mi_bridge_create_concealed.
 *
 * Seats that change hands (mi_bridge_create_open, mi_bridge_change_members): a conference server is defined by its churn --
 * callers arrive with whatever codec they negotiated, and they leave; ms_audio_conference_add_member -> plumb_to_conf hangs the
 * new endpoint's own decoder, encoder and two fresh resamplers on whichever pin find_free_pin returns
 * (audioconference.c:198-257, :322-345).  mi_bridge_create_open takes mi_bridge_create_ratios' arguments and rules plus the
 * KINDS that may ever take a seat and plans the bridge once for all of them; mi_bridge_change_members then lets members join,
 * leave and change kind without waiting for the device: the changes travel with the next tick submitted and are applied in
 * stream order ahead of that tick's kernels (bridge_roster_kernel, csrc/bridge_roster.hip; the concealer's part in
 * csrc/plc.hip), ticks in flight untouched, no other member's meter, resampler histories or concealer disturbed.  On a bridge
 * from any older constructor the call is mi_bridge_add_member / _remove_member without the drain.  Bit for bit the parts called
 * one by one with batches for every admitted rate (tests/test_gpu_bridge_open.py).
 *
 * Legs at 44.1 kHz (mi_bridge_create_offgrid): the static RTP payload types 10 and 11 are L16 at 44 100 Hz (l16.c), AAC-ELD runs
 * there (aac-eld.c), and so does a local sound-card endpoint; plumb_to_conf resamples such a member without asking.  The
 * constructor takes mi_bridge_create_open's arguments and rules, and a leg or admitted kind may also be at 44 100 Hz -- the one
 * rate off the 800 Hz grid whose 10 ms tick is whole samples, 441 of them: 55 groups of eight and one sample, which the kernel
 * reads, levels and stores alone, no byte of a row touched past the leg's 882 (PCM) or 441 (code words).  Against a mix at 8,
 * 12, 16, 24, 32 or 48 kHz both its resamplers are interpolated designs of 48 to 264 taps whose per-phase tables (80 to 441
 * rows, 28 to 92 KB) mi_resampler blends once; the tick runs mi_resampler's generic-order arithmetic on those tables, each lane
 * reading its output's row from memory, bit for bit mi_resampler_process_masked.  One conference holds such legs beside
 * legs of every older form, still one launch per tick (bridge_offgrid_kernel, csrc/bridge_offgrid.hip, run only by a bridge
 * with such a leg or admitted kind; tests/test_gpu_bridge_offgrid.py); cfg.plc is served through the per-leg concealer, whose
 * rate classes may include 44 100 Hz.  The host swaps an L16 member's bytes, as it decodes every codec but G.711.
 *
 * Out of scope, on purpose:
 *   - per membership change: mi_volume_params and the pin's input gain (mi_bridge_set_volume_params and mi_bridge_set_controls,
 *     which wait, set them); growing nstreams; kinds outside mi_bridge_create_ratios' rules; mi_session, whose membership calls
 *     keep their waits;
 *   - rates off the 800 Hz grid other than 44.1 kHz (22.05 and 11.025 kHz: 220.5 and 110.25 samples are no 10 ms tick), and a
 *     MIX at 44.1 kHz; whole ratios other than 2, 3, 4 and 6 (5, 7, 8 and up: a down-sampler of 240 taps or more); a : b on the
 *     grid with a or b above 8 or a ratio above 8/3 (7 : 2, 9 : 8: an interpolated table or more than 128 taps), in either
 *     direction: refused with MI_ENOTSUP -- mi_session and the MSFilter plugin resample those; 3/2 and 2/3 through the five
 *     oldest constructors, 4, 1/4 and a : b through the six older ones and 44.1 kHz through all eight before
 *     mi_bridge_create_offgrid, which keep refusing them;
 *   - jitter buffering and flow control: the host's, as with mi_session -- a leg whose packet is missing at the tick is
 *     flagged absent (or concealed, cfg.plc);
 *   - cfg.plc with legs that differ in rate or codec through the four older constructors: they keep refusing it with
 *     MI_ENOTSUP, mi_bridge_create_concealed serves it; and through any constructor a leg the concealer cannot serve -- a
 *     rate outside 8 - 48 kHz (a 96 kHz member of a 16 kHz room, legal without plc), or one whose 50 ms window has a prime
 *     factor above 17 (46.4 kHz), which kiss_fft itself refuses;
 *   - codecs other than G.711 and 16-bit PCM (G.722, Opus): the host's -- such a leg is a PCM leg of the bridge;
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
/* The same with every leg at a rate of its own: cfg->rate is the conference's, h_leg_rate [nstreams] the rate of each
 * leg's code words or PCM, in AND out (one endpoint has one rate, audioconference.c:226-230).  h_leg_rate == NULL, or
 * every entry == cfg->rate, is mi_bridge_create exactly.  Supported: cfg->rate / leg rate in {1, 2, 3, 6} with
 * leg rate % 800 == 0.  MI_ENOTSUP, the message naming the value, before anything is allocated: a leg above the
 * conference; a ratio that is no whole number, or another one; cfg->plc with legs of more than one rate (the concealer
 * batch has one: with one common leg rate it runs at that rate); a conference whose tick plus the resamplers' scratch
 * does not fit the 64 KB of LDS the kernel allows itself (48 kHz with 8 kHz legs: up to 41 members). */
int mi_bridge_create_rated(mi_ctx *ctx, const mi_bridge_config *cfg, const int32_t *h_leg_rate, mi_bridge **out);
/* The same with every leg's codec pair its own as well.  cfg->rate is the conference's; cfg->in_codec and cfg->out_codec
 * are not read.  Rates follow mi_bridge_create_rated's rules.  h_legs == NULL is mi_bridge_create exactly; legs that all
 * name one pair give mi_bridge_create_rated's bridge with that pair.  MI_ENOTSUP, the message naming the leg and the
 * value, before anything is allocated: a codec outside the three; cfg->plc with legs that do not all share one in_codec
 * and one out_codec. */
typedef struct mi_bridge_leg {
	int32_t rate;      /* Hz */
	int32_t in_codec;  /* MI_SESSION_PCM16 | MI_SESSION_PCMA | MI_SESSION_PCMU */
	int32_t out_codec;
} mi_bridge_leg;
int mi_bridge_create_legs(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs /* [nstreams] */, mi_bridge **out);
/* Every endpoint at the rate audioconference.c would plumb it with: below, at or ABOVE cfg->rate.  The arguments are
 * mi_bridge_create_legs'; h_legs == NULL is mi_bridge_create, and with no leg above cfg->rate the bridge is the one
 * mi_bridge_create_legs builds: the same kernels, pitch and tick bytes.  Supported: leg rate / cfg->rate or cfg->rate / leg
 * rate in {1, 2, 3, 6}, leg rate % 800 == 0; a G.711 leg above the mix is legal (code words are samples at the leg's rate).
 * With a leg above the mix the host rows are byte rows whether the codecs differ or not.  MI_ENOTSUP, the message naming
 * the leg and the value, before anything is allocated: a ratio that is no whole number in either direction, or another
 * one; a rate that is no multiple of 800; a codec outside the three; cfg->plc unless every leg shares one rate and one
 * codec pair; a conference whose rows -- as wide as the widest leg of the bridge --, sum row and resampler scratch do not
 * fit the 64 KB of LDS the kernel allows itself (48 kHz members in a 16 kHz conference: up to 45; in an 8 kHz one: 42). */
int mi_bridge_create_endpoints(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs /* [nstreams] */, mi_bridge **out);
/* The same with cfg->plc served for legs of any rate and codec.  The arguments and every rule are
 * mi_bridge_create_endpoints'.  cfg->plc == 0, or h_legs == NULL: that constructor's bridge exactly.  cfg->plc == 1 and every
 * leg naming one rate and one codec pair: the plc bridge the older constructors build, the same launches, pitch and tick
 * bytes.  cfg->plc == 1 with legs that differ in rate, codec or both: a concealer per leg behind the leg's own decoder, in
 * front of the bridge's kernel; byte rows as with mi_bridge_create_legs; the event bytes are the uniform plc bridge's
 * (h_present[s] == 0: MI_PLC_CONCEAL at the leg's own length).  mi_bridge_reset_streams and mi_bridge_add_member start the
 * leg's concealer over.  MI_ENOTSUP, the message naming the leg and the value, before anything is allocated: what
 * mi_bridge_create_endpoints refuses but for plc; with cfg->plc a leg outside 8 - 48 kHz or one whose concealer needs a
 * transform radix above 17. */
int mi_bridge_create_concealed(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs /* [nstreams] */, mi_bridge **out);
/* The same with legs at 3/2 or 2/3 of the mix's rate as well.  The arguments and every rule are mi_bridge_create_concealed's,
 * and a leg may also have 2 * leg rate == 3 * cfg->rate or 3 * leg rate == 2 * cfg->rate (both rates multiples of 800, as
 * ever).  h_legs == NULL, or no leg at 3/2 or 2/3: that constructor's bridge exactly, the same kernels, pitch and tick bytes.
 * With such a leg the host rows are byte rows whether the codecs differ or not, and mi_bridge_reset_streams and
 * mi_bridge_add_member zero both its resamplers' histories: the 71 samples of the one that runs x 2/3 and the 47 of the one
 * that runs x 3/2, on whichever side of the pin each sits.  MI_ENOTSUP, the message naming the leg and the value, before
 * anything is allocated: what mi_bridge_create_concealed refuses but for the two ratios; a ratio that is no whole number and
 * not 3/2 or 2/3 (44.1 kHz; 4/3); a whole ratio other than 2, 3 and 6; a conference whose rows, sum row and resampler scratch
 * do not fit the 64 KB of LDS the kernel allows itself (32 kHz legs in a 48 kHz conference: up to 43 members; 24 kHz legs in
 * a 16 kHz room that also holds 48 kHz members: up to 45). */
int mi_bridge_create_rational(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs /* [nstreams] */, mi_bridge **out);
/* The same with legs at 4 or 1/4 of the mix's rate and at a : b of it as well.  The arguments and every rule are
 * mi_bridge_create_rational's.  Write a : b for leg rate : cfg->rate in lowest terms (both rates multiples of 800, as ever): a
 * leg may also have a : b == 4 : 1 or 1 : 4, or any a : b that is no whole ratio with a <= 8, b <= 8 and
 * max(a, b) / min(a, b) <= 8/3 -- where the resampler's design rule gives both directions a direct polyphase table of at most
 * 128 taps.  h_legs == NULL, or no such leg: mi_bridge_create_rational's bridge exactly, the same kernels, pitch and tick
 * bytes.  With such a leg the host rows are byte rows whether the codecs differ or not, and mi_bridge_reset_streams and
 * mi_bridge_add_member zero both its resamplers' histories: 191 and 47 samples at ratio 4; at a : b the 47 of the one that
 * goes up and the filter length - 1 (up to 127 at 8 : 3) of the one that goes down, on whichever side of the pin each sits.
 * MI_ENOTSUP, the message naming the leg, both rates and the ratio, before anything is allocated: what
 * mi_bridge_create_rational refuses but for these ratios; a rate off the 800 Hz grid (44.1 kHz); whole ratios 5, 7, 8 and up;
 * a : b beyond the rule (7 : 2, 9 : 8); a conference whose rows, sum row and resampler scratch do not fit the 64 KB of LDS the
 * kernel allows itself (12 kHz legs in a 16 kHz room that also holds 48 kHz members: up to 45 members; 32 kHz legs in a
 * 24 kHz conference need 42 640 bytes at the mixer's own limit of 50 members, so there the limit is the mixer's). */
int mi_bridge_create_ratios(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs /* [nstreams] */, mi_bridge **out);
/* The same with seats that may change hands.  h_legs [nstreams]: who sits there at creation.  h_admit [nadmit]: the KINDS of
 * endpoint (rate, in_codec, out_codec) that may ever take a seat, besides the kinds of h_legs themselves.  The arguments and
 * every rule are mi_bridge_create_ratios', held for the union of the two: the bridge is planned ONCE -- kernel, LDS, row pitch,
 * history strides, resampler tables, the concealer's rate classes -- for every kind that may come, so that
 * mi_bridge_change_members never allocates.  It is the plan of the closed bridge that holds h_legs followed by a whole
 * conference of each admitted kind: mi_bridge_tick_bytes gives the union's pitch, wider than the initial legs' where a wider
 * kind is admitted.  nadmit == 0 (h_admit NULL or not): mi_bridge_create_ratios' bridge exactly, the same kernels, pitch and
 * tick bytes.  MI_ENOTSUP before anything is allocated: what mi_bridge_create_ratios refuses, the message saying
 * "admitted kind k" where h_admit[k] is the offender (a conference that does not fit the LDS with an admitted kind in it is
 * refused though the initial legs alone would fit); with cfg->plc every admitted rate must be one the concealer serves, and
 * the distinct rates of the union may be seven at most (the message names the count). */
int mi_bridge_create_open(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs /* [nstreams] */,
                          const mi_bridge_leg *h_admit /* [nadmit] */, int nadmit, mi_bridge **out);
/* The same with legs and admitted kinds at 44 100 Hz as well.  The arguments and every rule are mi_bridge_create_open's, and a
 * leg or an admitted kind may also be at 44 100 Hz wherever both its resamplers, by the resampler's own design rule at quality
 * 3, have a per-phase table (up to 256 KB) of at most 264 taps: with cfg->rate at 8, 12, 16, 24, 32 or 48 kHz (264, 176, 136,
 * 88, 72 and 48 taps leg -> mix; 48 taps mix -> leg, 56 from 48 kHz).  cfg->rate itself stays a multiple of 800.  Any codec of
 * the three is legal on such a leg (code words are samples at the leg's rate): its tick is 882 bytes of PCM or 441 code words,
 * and the rows' pitch is rounded up to 16 as ever (896 and 448).  With no such leg or kind: mi_bridge_create_open's bridge
 * exactly, the same kernels, pitch and tick bytes.  mi_bridge_reset_streams, mi_bridge_add_member and a JOIN zero both its
 * resamplers' histories (filter length - 1 samples, up to 263) and start its concealer over in the 44 100 Hz class; with
 * cfg->plc and such a leg the concealer is the per-leg one whether the legs differ or not.  MI_ENOTSUP, the message naming the
 * leg or admitted kind, both rates and the reason, before anything is allocated: what mi_bridge_create_open refuses on the grid
 * (whole ratios 5, 7, 8 and up; 7 : 2, 9 : 8); 22 050 and 11 025 Hz, or any other rate off the grid; a mix at 44 100 Hz, or one
 * against which the tables fail the rule (4 kHz: 536 taps); a conference whose rows -- 448 samples for a 441-sample tick --, sum
 * row and resampler scratch do not fit the 64 KB of LDS the kernel allows itself.  44.1 kHz legs alone fit at the mixer's own
 * limit of 50 members in every one of the six mixes (58 896 bytes in a 48 kHz one); in a 16 kHz room that also holds 48 kHz
 * members: up to 45 members. */
int mi_bridge_create_offgrid(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs /* [nstreams] */,
                             const mi_bridge_leg *h_admit /* [nadmit] */, int nadmit, mi_bridge **out);
void mi_bridge_destroy(mi_bridge *b);
int mi_bridge_leg_rate(const mi_bridge *b, int stream); /* the leg's rate in Hz, or MI_EINVAL */
/* the leg's codecs and its own tick in bytes (rate / 100 x 1 or 2), on any bridge; either pointer may be NULL.
 * MI_EINVAL for a bad stream or a NULL bridge */
int mi_bridge_leg_codec(const mi_bridge *b, int stream, int *in_codec, int *out_codec);
int mi_bridge_leg_bytes(const mi_bridge *b, int stream, int *in_bytes, int *out_bytes);
/* bytes per stream and tick of the two host buffers: the row pitch, which is the tick of the WIDEST leg of the bridge
 * (a bridge of 8 kHz G.711 legs in a 48 kHz conference moves 80-byte rows); where the legs' codecs differ, the widest
 * leg's tick in BYTES, in and out each, rounded up to 16 */
int mi_bridge_tick_bytes(const mi_bridge *b, int *in_bytes, int *out_bytes);

/* pinned staging of the NEXT tick, to be filled in place: h_in [nstreams][rate/100] uint8 code words or int16 PCM;
 * h_present [nstreams] uint8, preset to 1 -- clear a leg's byte when nothing arrived from it for this tick: its row
 * is ignored, MSVolume gets no chunk (meter state, gain ramp and one-second window stay as they are, msvolume.c:480-486)
 * and the mixer reads silence for the pin (audiomixer.c:88).  With cfg.plc the leg is concealed instead (MI_PLC_CONCEAL)
 * and metered on what the concealer made.
 * With legs at their own rate the row pitch is mi_bridge_tick_bytes' (the widest leg's tick); a narrower leg fills the
 * first leg rate / 100 samples of its row and the rest is ignored.  With legs of differing codecs: byte rows, a leg fills
 * the first mi_bridge_leg_bytes of its row. */
int mi_bridge_acquire(mi_bridge *b, void **h_in, uint8_t **h_present);
int mi_bridge_submit(mi_bridge *b);
/* the OLDEST tick in flight: waits for its download, returns the pinned output [nstreams][rate/100] (uint8 code words
 * or int16 PCM; valid until three more ticks have been submitted).  Rows of pins without MI_MIX_OUTPUT are not written.
 * With legs at their own rate: rows at mi_bridge_tick_bytes' pitch, a narrower leg's mix in the first leg rate / 100
 * samples of its row, the rest of the row left as it is.  With legs of differing codecs: byte rows, a leg's mix in the
 * first mi_bridge_leg_bytes of its row. */
int mi_bridge_collect(mi_bridge *b, const void **h_out);
int mi_bridge_in_flight(const mi_bridge *b); /* up to three */

/* Control plane, as mi_session's: per-stream mixer flags (MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT) and input
 * gains, either may be NULL, arrays of [nstreams]; in effect for the ticks submitted afterwards. */
int mi_bridge_set_controls(mi_bridge *b, const uint8_t *h_flags, const float *h_gain);
/* MSVolume of streams [first, first + count): static gain, AGC, noise gate, DC removal.  Default:
 * mi_volume_default_params (a meter at unity gain).  An echo-limiter peer (params.peer != -1) is MI_ENOTSUP: a bridge
 * has no far end to limit against. */
int mi_bridge_set_volume_params(mi_bridge *b, int first, int count, const mi_volume_params *h_params);
/* a leg was replaced: the meter (and concealer, and both resamplers' histories -- ratio x 48 - 1 samples on the wider side
 * of the pin, 47 on the other; 71 and 47 for a leg at 3/2 or 2/3 of the mix) of streams [first, first + count) start over as new filters would */
int mi_bridge_reset_streams(mi_bridge *b, int first, int count);
/* MSAudioConference membership (audioconference.c:322-374), as mi_session_add_member / _remove_member: a bridge is
 * created full; remove unplumbs the pin and clears its output row, add plumbs it for a NEW endpoint (fresh meter) */
int mi_bridge_add_member(mi_bridge *b, int stream);
int mi_bridge_remove_member(mi_bridge *b, int stream);
/* The same membership WITHOUT waiting for the device, and with the seat's kind its own: ms_audio_conference_add_member hangs
 * the new endpoint's own decoder, encoder and two fresh resamplers on whichever pin is free (audioconference.c:198-257,
 * :322-345).  The changes travel with the NEXT tick submitted -- the tick being filled, if one is acquired -- and the device
 * applies them in stream order ahead of that tick's kernels: that tick's rows are read with the new kinds, ticks submitted
 * earlier are untouched, collected or not.  The call contains no stream, event or device synchronise and no blocking copy.
 * Several calls before one submit merge per seat, the last one wins.  mi_bridge_leg_rate / _codec / _bytes,
 * mi_bridge_member_count and the election's joining order answer for the new roster as soon as the call returns.
 *   MI_BRIDGE_JOIN: a new endpoint brings a fresh meter (state, one-second window), both resamplers' histories zero, a fresh
 *     concealer (cfg.plc), the pin's flags MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT; the pin's input gain and the seat's
 *     mi_volume_params stay as they are, as with mi_bridge_add_member.
 *   MI_BRIDGE_LEAVE: the pin's flags 0, its output row zero from that tick on.
 * Admitted kinds: on a bridge from mi_bridge_create_open with nadmit > 0, the kinds of its initial legs and its admitted
 * kinds, on every seat; on any other bridge, for each seat that seat's own kind only -- there the call is
 * mi_bridge_add_member / _remove_member without the drain.
 * Nothing of a refused call is applied, and the message names the entry.  MI_ENOTSUP: a JOIN whose kind is not admitted (the
 * message names seat, rate and codecs and says how many kinds are admitted).  MI_EINVAL: a LEAVE of a seat that is no member,
 * a stream out of range, an op outside the two, one stream twice in one call.
 * mi_bridge_add_member, _remove_member, _reset_streams, _set_controls and _set_volume_params keep their behaviour and their
 * waits on every bridge; mi_bridge_add_member on an open bridge re-seats the seat's current kind, and a later
 * mi_bridge_set_controls(h_flags) overrides every pin's flags as ever.  One of those calls made between a change and the
 * submit that carries it has the last word on the pin's flags -- the change writes the flags the roster holds when the tick
 * is submitted --, so device and roster agree after that tick: a LEAVE followed by mi_bridge_add_member leaves the seat
 * plumbed (its row still cleared once), a JOIN followed by mi_bridge_remove_member leaves it unplumbed with the new kind.
 * Out of scope: mi_volume_params and input gain per membership change (mi_bridge_change_controls below sends them with the
 * same tick, the waiting setters keep working); growing nstreams; kinds outside
 * mi_bridge_create_ratios' rules; the plugin's server legs.  (mi_session has the call of its own: msmi355x_session.h.) */
#define MI_BRIDGE_JOIN 1  /* a NEW endpoint of kind `leg` takes the seat; a seat that is taken is replaced (leave + join) */
#define MI_BRIDGE_LEAVE 2 /* the seat is unplumbed; `leg` is not read */
typedef struct mi_bridge_change {
	int32_t stream, op;
	mi_bridge_leg leg;
} mi_bridge_change;
int mi_bridge_change_members(mi_bridge *b, const mi_bridge_change *h_changes, int count);
int mi_bridge_member_count(const mi_bridge *b, int conference); /* plumbed pins, or MI_EINVAL */
int mi_bridge_get_levels(mi_bridge *b, float *h_linear);        /* MS_VOLUME_GET_LINEAR of every stream */
/* the election of audioconference.c:436-452, as mi_session_active_speakers (now_ms ignored: the ticks are the clock) */
int mi_bridge_active_speakers(mi_bridge *b, uint64_t now_ms, int32_t *h_winner, float *h_max_db);
/* the meters' running state and MS_VOLUME_GET_MAX (linear), for tests and monitoring; both wait for the ticks submitted */
int mi_bridge_get_volume_state(mi_bridge *b, int first, int count, mi_volume_state *h_state);
int mi_bridge_get_volume_max(mi_bridge *b, int first, int count, float *h_max);

/* ---- The rest of the conference control plane WITHOUT waiting for the device.
 *
 * mi_bridge_set_controls, mi_bridge_set_volume_params, mi_bridge_get_levels and mi_bridge_active_speakers above each wait for
 * every tick submitted (and copy whole [nstreams] arrays): a mute toggle or a level poll empties the three-tick pipeline that
 * mi_bridge_change_members leaves alone.  The calls below steer and observe a running bridge without that.  The waiting calls
 * keep their semantics and their waits.
 *
 * mi_bridge_change_controls: ms_audio_conference_mute_member (audioconference.c:377-388), MS_AUDIO_MIXER_SET_ACTIVE /
 * _ENABLE_OUTPUT / _SET_INPUT_GAIN (audiomixer.c:372-414) and MSVolume's setters, per seat.  The calling contract is
 * mi_bridge_change_members': the changes travel with the NEXT tick submitted -- the tick being filled, if one is acquired --
 * and the device applies them in stream order ahead of that tick's kernels (controls_kernel, csrc/controls.hip); ticks
 * submitted earlier are untouched, collected or not.  The call contains no stream, event or device synchronise, no blocking
 * copy and no allocation.  Several calls before one submit merge per seat AND per field, the last one wins.
 *   MI_CTL_FLAGS:  the pin's MI_MIX_ACTIVE and MI_MIX_OUTPUT bits are taken from `flags` (mute: ACTIVE clear; listen-only off:
 *     OUTPUT clear).  MI_MIX_LINKED is membership's: any bit outside ACTIVE | OUTPUT is MI_EINVAL.  The seat must be a member
 *     when the call is made; earlier mi_bridge_change_members calls not yet submitted count.  Clearing MI_MIX_OUTPUT does not
 *     clear what the seat last heard, as mi_bridge_set_controls does not.
 *   MI_CTL_GAIN:   the pin's input gain, on any seat.
 *   MI_CTL_VOLUME: the seat's whole mi_volume_params, on any seat; params.peer != -1 is MI_ENOTSUP, as in
 *     mi_bridge_set_volume_params.  Gain and parameters survive joins.
 * Inside a tick membership changes are applied first, then controls: MI_BRIDGE_JOIN plus MI_CTL_FLAGS with ACTIVE clear before
 * one submit gives a member that arrives muted.  What a tick carries is staged at submit from the host's own mirrors of flags,
 * gains and parameters, which the waiting setters (mi_bridge_set_controls, _set_volume_params, _add_member, _remove_member)
 * update too: a waiting call made between a change and its submit has the last word on the fields it sets, and device and
 * host agree after that tick.  A LEAVE after an MI_CTL_FLAGS on the same seat leaves the seat unplumbed.
 * Nothing of a refused call is applied, and the message names the entry.  MI_EINVAL: a NULL bridge; count < 0, or count > 0
 * with a NULL h_changes; a stream out of range; an empty or unknown `what`; one stream twice in one call; the two rules of
 * MI_CTL_FLAGS.  count == 0 is MI_OK and does nothing.
 * Measured at 1024 conferences x 32 mu-law legs, three ticks in flight (profiles/bridge_controls.md): 1.0 us per call for one
 * seat, 1.4 us for 32, 29 us for 1024, against 48 us for one mi_bridge_set_controls; a poll of every level and speaker costs
 * 4 us through mi_bridge_collected_report against 425 us through mi_bridge_active_speakers + mi_bridge_get_levels, and a
 * server that polls after every tick sustains 9880 ticks a second instead of 1694; the report kernel adds about 4 us to a
 * 96 us tick. */
#define MI_CTL_FLAGS 1u
#define MI_CTL_GAIN 2u
#define MI_CTL_VOLUME 4u
typedef struct mi_bridge_control {
	int32_t stream;
	uint32_t what;  /* MI_CTL_* */
	uint32_t flags; /* MI_CTL_FLAGS: MI_MIX_ACTIVE | MI_MIX_OUTPUT */
	float gain;     /* MI_CTL_GAIN */
	mi_volume_params params; /* MI_CTL_VOLUME */
} mi_bridge_control;
int mi_bridge_change_controls(mi_bridge *b, const mi_bridge_control *h_changes, int count);

/* Levels and the election come back WITH the tick.  mi_bridge_set_reports(b, MI_REPORT_SPEAKERS | MI_REPORT_LEVELS) -- 0: off,
 * the default -- is a configuration call: it may wait once and allocate; nothing per tick does.  From the next submit on one
 * kernel (report_kernel, csrc/controls.hip) runs behind the tick's kernels, reads what the tick left and writes a report block
 * that is downloaded with the tick's output.  mi_bridge_collected_report hands out the block of the tick LAST COLLECTED:
 * pointers into pinned memory, valid for as long as that tick's output is; it never waits.  MI_EINVAL: nothing collected yet,
 * reports were off for that tick, or its slot has been submitted again.  At most 64 members per conference (MI_ENOTSUP).
 *   MI_REPORT_LEVELS:   levels [nstreams], every stream's MS_VOLUME_GET_LINEAR: bit for bit what mi_bridge_get_levels returns
 *     when that tick is the last one submitted (the raw meter, muted members included).
 *   MI_REPORT_SPEAKERS: per conference ms_audio_conference_process_events' election (audioconference.c:436-452): winner
 *     [nconf] (stream or -1), max_lin [nconf] (the winner's one-second maximum, linear, or 0) and max_db [nconf], worked out
 *     on the host in this call from max_lin with the waiting call's own expression, so the float is the one
 *     mi_bridge_active_speakers gives.  Eligible are the plumbed, unmuted members whose maximum is above -30 dBm0 -- exactly the
 *     waiting call's set: the kernel compares with the smallest float whose dBm0 value is above -30.0f, derived once with the
 *     host's libm.  Of the eligible the largest maximum wins, of equal maxima the member that joined first.
 *   A VISIBLE, DELIBERATE DIFFERENCE (in the manner of SURVEY Appendix A): the kernel compares LINEAR maxima, the reference dBm0
 *   floats.  Where two eligible members' maxima are different floats whose dBm0 values round to the same float -- a band of
 *   about four ulp near -30 dBm0 -- the reference takes the earlier joiner and the report the louder.  mi_bridge_active_speakers
 *   stays the reference-exact call. */
#define MI_REPORT_SPEAKERS 1u
#define MI_REPORT_LEVELS 2u
typedef struct mi_bridge_report {
	uint64_t seq;  /* the tick's sequence number: 0 for the first tick the bridge was submitted */
	uint32_t what; /* MI_REPORT_* as they were set when the tick was submitted */
	int32_t nstreams, nconf;
	const float *levels;   /* [nstreams], NULL without MI_REPORT_LEVELS */
	const int32_t *winner; /* [nconf], NULL without MI_REPORT_SPEAKERS, as are the next two */
	const float *max_lin;  /* [nconf] */
	const float *max_db;   /* [nconf]; -120 (MS_VOLUME_DB_LOWEST) where nobody was elected */
} mi_bridge_report;
int mi_bridge_set_reports(mi_bridge *b, uint32_t what);
int mi_bridge_collected_report(mi_bridge *b, mi_bridge_report *out);

#ifdef __cplusplus
}
#endif
#endif
