/*
 * examples/mixed_rate_session.c -- one conference server's legs as they really come: 8 kHz mu-law and A-law trunks beside
 * 16 kHz wideband members, every one with its own echo canceller, in conferences mixed at 48 kHz.  plumb_to_conf hangs each
 * endpoint's own decoder, encoder and two resamplers on its pin (src/voip/audioconference.c:226-251);
 * mi_session_create_legs (include/msmi355x_session.h) does that for the whole batch around ONE canceller rate: the legs' rows
 * are byte rows at one pitch, a leg fills and receives the first mi_session_leg_bytes of its row.  The far end of every leg
 * is what it was sent one tick ago (ref_loopback).
 *
 * The program checks itself against nothing but its own exit conditions: no call fails, and a leg of each kind hears
 * something at the end.  Plain C99; links against libmsmi355x.so only.
 *
 *   cc -std=c99 -Iinclude examples/mixed_rate_session.c -Lmediastreamer2_amd -lmsmi355x -Wl,-rpath,$PWD/mediastreamer2_amd
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msmi355x_session.h"

#define MEMBERS 4
#define CONFERENCES 2
#define SEATS (MEMBERS * CONFERENCES)
#define TICKS 50

/* a stand-in for the trunk and the sound card: code words or samples of noise, a different stream per seat */
static uint32_t noise(uint32_t seat, uint32_t tick, uint32_t i) {
	uint32_t x = (seat * 2654435761u) ^ (tick * 40503u + i) * 2246822519u;
	x ^= x >> 15, x *= 2246822519u, x ^= x >> 13;
	return x;
}

int main(void) {
	/* per conference: a mu-law trunk, an A-law trunk, two wideband members */
	static const mi_session_leg KINDS[MEMBERS] = {
	    {8000, MI_SESSION_PCMU, MI_SESSION_PCMU}, {8000, MI_SESSION_PCMA, MI_SESSION_PCMA}, {16000, MI_SESSION_PCM16, MI_SESSION_PCM16},
	    {16000, MI_SESSION_PCM16, MI_SESSION_PCM16}};
	mi_ctx *ctx;
	mi_session *se;
	mi_session_config cfg;
	mi_session_leg legs[SEATS];
	int heard[SEATS];
	int mic_pitch = 0, out_pitch = 0, tick, seat, i, rc = 0, collected = 0;

	if (mi_ctx_create(0, NULL, &ctx) != MI_OK) {
		fprintf(stderr, "no MI355X, and there is no CPU fallback: %s\n", mi_last_error());
		return 1;
	}
	mi_session_default_config(&cfg);
	cfg.nstreams = SEATS;
	cfg.members_per_conference = MEMBERS;
	cfg.rate = 48000; /* the cancellers', the meters' and the mixers' */
	cfg.tail_ms = 32;
	cfg.ref_loopback = 1;
	for (seat = 0; seat < SEATS; ++seat) legs[seat] = KINDS[seat % MEMBERS], heard[seat] = 0;
	if (mi_session_create_legs(ctx, &cfg, legs, &se) != MI_OK) {
		fprintf(stderr, "mi_session_create_legs: %s\n", mi_last_error());
		mi_ctx_destroy(ctx);
		return 1;
	}
	if (mi_session_tick_bytes(se, &mic_pitch, NULL, &out_pitch) != MI_OK) rc = 1;
	printf("%d legs, rows of %d bytes in and %d out\n", SEATS, mic_pitch, out_pitch);

	for (tick = 0; tick < TICKS + 3 && !rc; ++tick) { /* a real server paces this loop at 10 ms */
		if (mi_session_in_flight(se) == 3 || tick >= TICKS) { /* three ticks in flight */
			const int16_t *out;
			if (mi_session_collect(se, &out) != MI_OK) rc = 1;
			for (seat = 0; seat < SEATS && !rc; ++seat) { /* the leg's own bytes of its row: does it hear the others? */
				const uint8_t *row = (const uint8_t *)out + (size_t)seat * (size_t)out_pitch;
				int mine = 0, out_bytes = 0, differ = 0;
				if (mi_session_leg_bytes(se, seat, &mine, &out_bytes) != MI_OK) rc = 1;
				for (i = 1; i < out_bytes; ++i) differ += row[i] != row[0];
				heard[seat] = differ > out_bytes / 4;
			}
			++collected;
		}
		if (tick < TICKS && !rc) {
			int16_t *mic, *ref; /* ref is NULL: the far end is looped back on the device */
			if (mi_session_acquire(se, &mic, &ref) != MI_OK) rc = 1;
			for (seat = 0; seat < SEATS && !rc; ++seat) {
				uint8_t *row = (uint8_t *)mic + (size_t)seat * (size_t)mic_pitch;
				const int len = legs[seat].rate / 100;
				if (legs[seat].mic_codec == MI_SESSION_PCM16)
					for (i = 0; i < len; ++i) ((int16_t *)row)[i] = (int16_t)((int)(noise((uint32_t)seat, (uint32_t)tick, (uint32_t)i) % 6001u) - 3000);
				else /* any byte is a code word */
					for (i = 0; i < len; ++i) row[i] = (uint8_t)(0x90u | (noise((uint32_t)seat, (uint32_t)tick, (uint32_t)i) & 0x6fu));
			}
			if (!rc && mi_session_submit(se) != MI_OK) rc = 1;
		}
	}
	if (rc) fprintf(stderr, "mixed_rate_session: %s\n", mi_last_error());
	for (seat = 0; seat < SEATS && !rc; ++seat) {
		printf("leg %d at %d Hz (codecs %d, %d): %s\n", seat, mi_session_leg_rate(se, seat), legs[seat].mic_codec, legs[seat].out_codec,
		       heard[seat] ? "hears the conference" : "SILENT");
		rc = !heard[seat];
	}
	mi_session_destroy(se);
	mi_ctx_destroy(ctx);
	rc = rc || collected != TICKS;
	puts(rc ? "failed" : "ok");
	return rc;
}
