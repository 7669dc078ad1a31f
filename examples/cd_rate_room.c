/*
 * examples/cd_rate_room.c -- a conference server's 16 kHz rooms on mi_bridge (include/msmi355x_bridge.h) with members at the
 * CD rate: L16 / 44 100 Hz (the static RTP payload type 11, l16.c) beside 8 kHz mu-law and A-law trunks and 16 kHz PCM
 * members in ONE 16 kHz conference.  A 44.1 kHz member stands 441 : 160 to the mix: plumb_to_conf
 * (src/voip/audioconference.c:209-257) hangs a 136-tap down-sampler in front of its pin and a 48-tap up-sampler behind it, and
 * the bridge runs both inside its one kernel launch per 10 ms tick (mi_bridge_create_offgrid).  L16 is big-endian on the
 * wire and the bridge knows 16-bit PCM in host order only: the HOST swaps the bytes, as it decodes every codec but G.711.
 * Plain C99; links against libmsmi355x.so only.
 *
 *   cc -std=c99 -Iinclude examples/cd_rate_room.c -Lmediastreamer2_amd -lmsmi355x -Wl,-rpath,$PWD/mediastreamer2_amd
 *
 * The host rows are byte rows at one pitch (mi_bridge_tick_bytes: here 896, a 441-sample PCM tick's 882 bytes rounded up to
 * 16); a leg fills and receives the first mi_bridge_leg_bytes of its row: 80 code bytes for a trunk, 320 bytes of PCM for a
 * 16 kHz member, 882 for a 44.1 kHz one.  The bridge leaves the 14 bytes behind those alone.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msmi355x_bridge.h"

#define MEMBERS 12
#define CONFERENCES 32

static const int RATE[4] = {8000, 44100, 8000, 16000}; /* quarters: mu-law trunk, L16 member, A-law trunk, PCM member */
static const int CODEC[4] = {MI_SESSION_PCMU, MI_SESSION_PCM16, MI_SESSION_PCMA, MI_SESSION_PCM16};
static const int BYTES[4] = {80, 882, 80, 320};

/* L16 (RFC 3551 4.5.11) is network byte order; the bridge's PCM is the host's */
static void swap16(uint8_t *p, int bytes) {
	int i;
	for (i = 0; i + 1 < bytes; i += 2) {
		const uint8_t t = p[i];
		p[i] = p[i + 1], p[i + 1] = t;
	}
}

/* stand-ins for the RTP side of a real server: a leg's payload as it is on the wire, `bytes` long */
static int rtp_receive(int leg, int tick, int kind, uint8_t *payload, int bytes) {
	int i;
	if (kind == 1) { /* L16: a square wave, big-endian */
		for (i = 0; i < bytes / 2; ++i) {
			const int16_t v = (int16_t)((i & 16) ? -4000 : 4000);
			payload[2 * i] = (uint8_t)((uint16_t)v >> 8), payload[2 * i + 1] = (uint8_t)((uint16_t)v & 0xff);
		}
	} else if (kind == 3) { /* a wideband codec the host has decoded already */
		int16_t *pcm = (int16_t *)payload;
		for (i = 0; i < bytes / 2; ++i) pcm[i] = (int16_t)((i & 8) ? -3000 : 3000);
	} else {
		memset(payload, kind == 2 ? 0xD5 : 0xFF, (size_t)bytes); /* the law's silence */
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
	uint8_t wire[882];

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
		legs[leg].rate = RATE[leg % 4];
		legs[leg].in_codec = legs[leg].out_codec = CODEC[leg % 4];
	}
	if (mi_bridge_create_open(ctx, &cfg, legs, NULL, 0, &br) != MI_ENOTSUP) { /* the older constructors keep refusing 44.1 kHz */
		fprintf(stderr, "mi_bridge_create_open took a 44.1 kHz leg\n");
		return 1;
	}
	if (mi_bridge_create_offgrid(ctx, &cfg, legs, NULL, 0, &br) != MI_OK) {
		fprintf(stderr, "mi_bridge_create_offgrid: %s\n", mi_last_error());
		return 1;
	}
	free(legs);
	if (mi_bridge_tick_bytes(br, &in_pitch, &out_pitch) != MI_OK || in_pitch != 896 || out_pitch != 896) rc = 1;
	for (leg = 0; leg < nlegs; ++leg) {
		int in_bytes, out_bytes;
		if (mi_bridge_leg_bytes(br, leg, &in_bytes, &out_bytes) != MI_OK || in_bytes != BYTES[leg % 4] || out_bytes != BYTES[leg % 4]) rc = 1;
		if (mi_bridge_leg_rate(br, leg) != RATE[leg % 4]) rc = 1;
	}

	for (tick = 0; tick < 300 && !rc; ++tick) { /* a real server paces this loop at 10 ms */
		void *in;
		uint8_t *present;
		const void *out;
		if (mi_bridge_in_flight(br) == 3) { /* three ticks in flight: upload | kernel | download overlap */
			if (mi_bridge_collect(br, &out) != MI_OK) rc = 1;
			for (leg = 0; leg < nlegs && !rc; ++leg) {
				const uint8_t *row = (const uint8_t *)out + (size_t)out_pitch * leg;
				if (leg % 4 == 1) { /* back to network order, in a buffer of the host's: the staging row is the bridge's */
					memcpy(wire, row, 882);
					swap16(wire, 882);
					row = wire;
				}
				rtp_send(leg, row, BYTES[leg % 4]);
			}
		}
		if (mi_bridge_acquire(br, &in, &present) != MI_OK) rc = 1;
		for (leg = 0; leg < nlegs && !rc; ++leg) {
			uint8_t *row = (uint8_t *)in + (size_t)in_pitch * leg;
			if (!rtp_receive(leg, tick, leg % 4, row, BYTES[leg % 4])) present[leg] = 0;
			if (leg % 4 == 1) swap16(row, 882);
		}
		if (!rc && mi_bridge_submit(br) != MI_OK) rc = 1;
	}
	if (rc) fprintf(stderr, "cd_rate_room: %s\n", mi_last_error());
	while (mi_bridge_in_flight(br)) {
		const void *out;
		if (mi_bridge_collect(br, &out) != MI_OK) break;
	}
	mi_bridge_destroy(br);
	mi_ctx_destroy(ctx);
	puts(rc ? "failed" : "ok");
	return rc;
}
