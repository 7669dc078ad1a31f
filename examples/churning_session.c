/*
 * examples/churning_session.c -- call legs that come and go on mi_session, the chained path WITH the echo canceller
 * (MSResample 16k -> 48k, MSSpeexEC + post-filter, MSVolume with AGC, MSAudioMixer; include/msmi355x.h).  Every few ticks a
 * caller hangs up or a new one takes a seat -- ms_audio_conference_remove_member / _add_member
 * (src/voip/audioconference.c:322-374): the new endpoint brings its own filters, all fresh.  mi_session_change_members
 * (include/msmi355x_session.h) never waits for the device: the change travels with the next tick, three ticks stay in flight
 * throughout, and nobody else loses a sample of canceller state.
 *
 * The program checks itself: a second session is driven by the waiting calls -- collect everything, mi_session_remove_member,
 * mi_session_add_member -- and every tick of the two must be equal byte for byte.  Plain C99; links against libmsmi355x.so
 * only.
 *
 *   cc -std=c99 -Iinclude examples/churning_session.c -Lmediastreamer2_amd -lmsmi355x -Wl,-rpath,$PWD/mediastreamer2_amd
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msmi355x_session.h"

#define MEMBERS 8
#define CONFERENCES 8
#define SEATS (MEMBERS * CONFERENCES)
#define TICKS 60
#define IN_LEN 160  /* 16 kHz */
#define OUT_LEN 480 /* 48 kHz */

/* a stand-in for the sound card and the RTP side: noise with a square wave under it, the same for both sessions */
static int16_t sample(uint32_t seat, uint32_t tick, uint32_t i, uint32_t salt) {
	uint32_t x = (seat * 2654435761u) ^ (tick * 40503u + i) * 2246822519u ^ salt;
	x ^= x >> 15, x *= 2246822519u, x ^= x >> 13;
	return (int16_t)((int)(x % 6001u) - 3000 + ((i & 16) ? 1500 : -1500));
}

static int fill_and_submit(mi_session *se, int tick) {
	int16_t *mic, *ref;
	int seat, i;
	if (mi_session_acquire(se, &mic, &ref) != MI_OK) return 1;
	for (seat = 0; seat < SEATS; ++seat) {
		for (i = 0; i < IN_LEN; ++i) mic[seat * IN_LEN + i] = sample((uint32_t)seat, (uint32_t)tick, (uint32_t)i, 1u);
		for (i = 0; i < OUT_LEN; ++i) ref[seat * OUT_LEN + i] = sample((uint32_t)seat, (uint32_t)tick, (uint32_t)i, 2u);
	}
	return mi_session_submit(se) != MI_OK;
}

int main(void) {
	mi_ctx *ctx;
	mi_session *open_se, *twin;
	mi_session_config cfg;
	static int16_t want[TICKS][SEATS * OUT_LEN]; /* the twin's ticks, kept until the open session's come down */
	int seated[SEATS];
	int tick, seat, rc = 0, collected = 0, differ = 0;

	if (mi_ctx_create(0, NULL, &ctx) != MI_OK) {
		fprintf(stderr, "no MI355X: %s\n", mi_last_error()); /* there is no CPU fallback */
		return 1;
	}
	mi_session_default_config(&cfg);
	cfg.nstreams = SEATS;
	cfg.members_per_conference = MEMBERS;
	cfg.in_rate = 16000;
	cfg.rate = 48000;
	cfg.tail_ms = 32;
	if (mi_session_create(ctx, &cfg, &open_se) != MI_OK || mi_session_create(ctx, &cfg, &twin) != MI_OK) {
		fprintf(stderr, "mi_session_create: %s\n", mi_last_error());
		return 1;
	}
	for (seat = 0; seat < SEATS; ++seat) seated[seat] = 1;
	{ /* a refused call applies nothing: seat 1 stays seated although its entry was good */
		mi_session_change bad[2] = {{1, MI_SESSION_LEAVE}, {SEATS, MI_SESSION_JOIN}};
		if (mi_session_change_members(open_se, bad, 2) != MI_EINVAL || mi_session_member_count(open_se, 0) != MEMBERS) rc = 1;
	}

	for (tick = 0; tick < TICKS && !rc; ++tick) { /* a real server paces this loop at 10 ms */
		const int16_t *out;
		if (mi_session_in_flight(open_se) == 3) { /* three ticks in flight */
			if (mi_session_collect(open_se, &out) != MI_OK) rc = 1;
			else differ += memcmp(out, want[collected++], sizeof(want[0])) != 0;
		}
		if (!rc && tick % 3 == 1) { /* a seat changes hands; the tick about to be filled is the first the new roster holds for */
			mi_session_change ch;
			ch.stream = (tick * 7) % SEATS;
			ch.op = seated[ch.stream] && tick % 2 == 0 ? MI_SESSION_LEAVE : MI_SESSION_JOIN; /* a JOIN on a taken seat replaces the caller */
			if (mi_session_change_members(open_se, &ch, 1) != MI_OK) rc = 1;
			/* the twin: the waiting calls (nothing of it is in flight here) */
			if (!rc && seated[ch.stream] && mi_session_remove_member(twin, ch.stream) != MI_OK) rc = 1;
			if (!rc && ch.op == MI_SESSION_JOIN && mi_session_add_member(twin, ch.stream) != MI_OK) rc = 1;
			seated[ch.stream] = ch.op == MI_SESSION_JOIN;
			if (!rc && mi_session_member_count(open_se, ch.stream / MEMBERS) != mi_session_member_count(twin, ch.stream / MEMBERS)) rc = 1;
		}
		if (!rc && fill_and_submit(open_se, tick)) rc = 1;
		if (!rc && (fill_and_submit(twin, tick) || mi_session_collect(twin, &out) != MI_OK)) rc = 1;
		if (!rc) memcpy(want[tick], out, sizeof(want[0]));
	}
	while (!rc && mi_session_in_flight(open_se)) {
		const int16_t *out;
		if (mi_session_collect(open_se, &out) != MI_OK) rc = 1;
		else differ += memcmp(out, want[collected++], sizeof(want[0])) != 0;
	}
	if (rc) fprintf(stderr, "churning_session: %s\n", mi_last_error());
	else {
		int seats = 0;
		for (seat = 0; seat < CONFERENCES; ++seat) seats += mi_session_member_count(open_se, seat);
		printf("%d ticks, %d of %d seats taken at the end, %d ticks differ from the waiting calls' session\n", collected, seats, SEATS, differ);
	}
	mi_session_destroy(open_se);
	mi_session_destroy(twin);
	mi_ctx_destroy(ctx);
	rc = rc || differ || collected != TICKS;
	puts(rc ? "failed" : "ok");
	return rc;
}
