/*
 * examples/mixed_rate_room.c -- a conference server's 16 kHz rooms on mi_bridge (include/msmi355x_bridge.h): 8 kHz mu-law
 * trunks, 12 kHz PCM members (SILK and Opus with a capped playback rate, msopus.c:434-436) and 32 kHz PCM members (Speex
 * ultra-wideband, msspeex.c:133) in ONE 16 kHz conference.  A 12 kHz member stands 3 : 4 to the mix: it gets the x 4/3
 * resampler in front of its pin and the x 3/4 one behind it, as plumb_to_conf (src/voip/audioconference.c:209-257) would
 * hang them, next to the trunks' x 2 and the 32 kHz members' x 1/2, all of it in one kernel launch per 10 ms tick
 * (mi_bridge_create_ratios).  Plain C99; links against libmsmi355x.so only.
 *
 *   cc -std=c99 -Iinclude examples/mixed_rate_room.c -Lmediastreamer2_amd -lmsmi355x -Wl,-rpath,$PWD/mediastreamer2_amd
 *
 * The host rows are byte rows at one pitch (mi_bridge_tick_bytes: here 640, a 32 kHz PCM tick); a leg fills and receives
 * the first mi_bridge_leg_bytes of its row: 80 code bytes for a trunk, 240 and 640 bytes of PCM for a 12 and a 32 kHz
 * member.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msmi355x_bridge.h"

#define MEMBERS 12
#define CONFERENCES 32

static const int RATE[3] = {8000, 12000, 32000}; /* thirds: mu-law trunk, then PCM members */
static const int BYTES[3] = {80, 240, 640};

/* stand-ins for the RTP side of a real server: a leg's payload in its own codec, `bytes` long */
static int rtp_receive(int leg, int tick, int codec, uint8_t *payload, int bytes) {
	int i;
	if (codec == MI_SESSION_PCM16) { /* a square wave */
		int16_t *pcm = (int16_t *)payload;
		for (i = 0; i < bytes / 2; ++i) pcm[i] = (int16_t)((i & 8) ? -4000 : 4000);
	} else {
		memset(payload, codec == MI_SESSION_PCMA ? 0xD5 : 0xFF, (size_t)bytes); /* the law's silence */
	}
	return (leg + tick) % 50 != 7; /* one packet in fifty is late */
}
static void rtp_send(int leg, const uint8_t *payload, int bytes) {
	(void)leg;
	(void)payload;
	(void)bytes;
}

int main(void) {
	mi_ctx *ctx;
	mi_bridge *br;
	mi_bridge_config cfg;
	mi_bridge_leg *legs;
	const int nlegs = CONFERENCES * MEMBERS;
	int tick, leg, in_pitch, out_pitch, rc = 0;
	int *in_bytes, *out_bytes, *in_codec;

	if (mi_ctx_create(0, NULL, &ctx) != MI_OK) {
		fprintf(stderr, "no MI355X: %s\n", mi_last_error()); /* there is no CPU fallback */
		return 1;
	}
	mi_bridge_default_config(&cfg);
	cfg.nstreams = nlegs;
	cfg.members_per_conference = MEMBERS;
	cfg.rate = 16000; /* the conference's; in_codec and out_codec are every leg's own */
	legs = (mi_bridge_leg *)malloc(sizeof(*legs) * (size_t)nlegs);
	for (leg = 0; leg < nlegs; ++leg) {
		legs[leg].rate = RATE[leg % 3];
		legs[leg].in_codec = legs[leg].out_codec = leg % 3 == 0 ? MI_SESSION_PCMU : MI_SESSION_PCM16;
	}
	if (mi_bridge_create_rational(ctx, &cfg, legs, &br) != MI_ENOTSUP) { /* the older constructors keep refusing 12 kHz in 16 kHz */
		fprintf(stderr, "mi_bridge_create_rational took a 12 kHz leg in a 16 kHz conference\n");
		return 1;
	}
	if (mi_bridge_create_ratios(ctx, &cfg, legs, &br) != MI_OK) {
		fprintf(stderr, "mi_bridge_create_ratios: %s\n", mi_last_error());
		return 1;
	}
	free(legs);
	in_bytes = (int *)malloc(sizeof(int) * (size_t)nlegs * 3);
	out_bytes = in_bytes + nlegs, in_codec = out_bytes + nlegs;
	if (mi_bridge_tick_bytes(br, &in_pitch, &out_pitch) != MI_OK || in_pitch != 640 || out_pitch != 640) rc = 1;
	for (leg = 0; leg < nlegs; ++leg) {
		const int want = BYTES[leg % 3];
		if (mi_bridge_leg_bytes(br, leg, &in_bytes[leg], &out_bytes[leg]) != MI_OK || in_bytes[leg] != want || out_bytes[leg] != want) rc = 1;
		if (mi_bridge_leg_codec(br, leg, &in_codec[leg], NULL) != MI_OK) rc = 1;
		if (mi_bridge_leg_rate(br, leg) != RATE[leg % 3]) rc = 1;
	}
	if (mi_bridge_leg_bytes(br, nlegs, NULL, NULL) != MI_EINVAL) rc = 1;

	for (tick = 0; tick < 300 && !rc; ++tick) { /* a real server paces this loop at 10 ms */
		void *in;
		uint8_t *present;
		const void *out;
		if (mi_bridge_in_flight(br) == 3) { /* three ticks in flight: upload | kernel | download overlap */
			if (mi_bridge_collect(br, &out) != MI_OK) rc = 1;
			for (leg = 0; leg < nlegs && !rc; ++leg) rtp_send(leg, (const uint8_t *)out + (size_t)out_pitch * leg, out_bytes[leg]);
		}
		if (mi_bridge_acquire(br, &in, &present) != MI_OK) rc = 1;
		for (leg = 0; leg < nlegs && !rc; ++leg)
			if (!rtp_receive(leg, tick, in_codec[leg], (uint8_t *)in + (size_t)in_pitch * leg, in_bytes[leg])) present[leg] = 0;
		if (!rc && mi_bridge_submit(br) != MI_OK) rc = 1;
	}
	if (rc) fprintf(stderr, "mixed_rate_room: %s\n", mi_last_error());
	while (mi_bridge_in_flight(br)) {
		const void *out;
		if (mi_bridge_collect(br, &out) != MI_OK) break;
	}
	free(in_bytes);
	mi_bridge_destroy(br);
	mi_ctx_destroy(ctx);
	puts(rc ? "failed" : "ok");
	return rc;
}
