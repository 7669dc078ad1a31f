/*
 * examples/moderated_bridge.c -- a moderated conference server on mi_bridge (include/msmi355x_bridge.h): rooms of 8 kHz mu-law
 * trunks whose moderator mutes, un-mutes and re-levels members all the time while the server shows who is speaking --
 * ms_audio_conference_mute_member, MS_AUDIO_MIXER_SET_INPUT_GAIN and ms_audio_conference_process_events' election
 * (src/voip/audioconference.c:377-457).  The server loop keeps three ticks in flight and never waits for the device:
 * mi_bridge_change_controls sends the moderator's changes with the next tick, and every tick's elected speaker and levels come
 * back with its output (mi_bridge_set_reports, mi_bridge_collected_report).
 *
 * The program checks itself: a twin bridge is fed the same packets and driven by the waiting calls -- mi_bridge_set_controls,
 * mi_bridge_active_speakers, mi_bridge_get_levels, one tick at a time -- and every tick's output, winner, level in dBm0 and
 * meter read-out must be the twin's, bit for bit.  Plain C99; links against libmsmi355x.so only.
 *
 *   cc -std=c99 -Iinclude examples/moderated_bridge.c -Lmediastreamer2_amd -lmsmi355x -Wl,-rpath,$PWD/mediastreamer2_amd
 *   ./a.out [conferences [members [ticks]]]      (default 4 8 150)
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msmi355x_bridge.h"

#define TICK 80 /* bytes per leg and tick: 10 ms of G.711 at 8 kHz */

/* a stand-in for the RTP side: in every room one member talks for a quarter of a second, then the next one; each member has a
 * loudness of its own (a square wave between two mu-law code words), everybody else sends the law's silence */
static void rtp_receive(int tick, int member, int members, uint8_t *payload) {
	int i;
	if ((tick / 25) % members != member) {
		memset(payload, 0xFF, TICK);
		return;
	}
	for (i = 0; i < TICK; ++i) payload[i] = (uint8_t)(((i & 8) ? 0x2F : 0xAF) - member % 32); /* the later talker is the louder */
}

int main(int argc, char **argv) {
	const int nconf = argc > 1 ? atoi(argv[1]) : 4, members = argc > 2 ? atoi(argv[2]) : 8, ticks = argc > 3 ? atoi(argv[3]) : 150;
	const int seats = nconf * members;
	mi_ctx *ctx;
	mi_bridge *br, *twin;
	mi_bridge_config cfg;
	uint8_t *flags, *want_out;
	float *gain, *want_levels, *want_db;
	int32_t *want_winner;
	int tick, collected = 0, changes_of_speaker = 0, last_speaker = -2, rc = 0;

	if (nconf < 1 || members < 2 || members > 50 || ticks < 1) {
		fprintf(stderr, "usage: %s [conferences [members (2..50) [ticks]]]\n", argv[0]);
		return 2;
	}
	if (mi_ctx_create(0, NULL, &ctx) != MI_OK) {
		fprintf(stderr, "no MI355X: %s\n", mi_last_error()); /* there is no CPU fallback */
		return 1;
	}
	mi_bridge_default_config(&cfg);
	cfg.nstreams = seats;
	cfg.members_per_conference = members;
	if (mi_bridge_create(ctx, &cfg, &br) != MI_OK || mi_bridge_create(ctx, &cfg, &twin) != MI_OK) {
		fprintf(stderr, "mi_bridge_create: %s\n", mi_last_error());
		return 1;
	}
	if (mi_bridge_set_reports(br, MI_REPORT_SPEAKERS | MI_REPORT_LEVELS) != MI_OK) rc = 1; /* once: this call may wait */
	/* the twin's controls as whole arrays, and what the twin answered for every tick */
	flags = malloc((size_t)seats), gain = malloc((size_t)seats * sizeof(float));
	want_out = malloc((size_t)ticks * seats * TICK), want_levels = malloc((size_t)ticks * seats * sizeof(float));
	want_winner = malloc((size_t)ticks * nconf * sizeof(int32_t)), want_db = malloc((size_t)ticks * nconf * sizeof(float));
	if (!flags || !gain || !want_out || !want_levels || !want_winner || !want_db) return 1;
	memset(flags, MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT, (size_t)seats);
	for (tick = 0; tick < seats; ++tick) gain[tick] = 1.0f;

	for (tick = 0; tick < ticks && !rc; ++tick) { /* a real server paces this loop at 10 ms */
		void *in, *twin_in;
		uint8_t *present;
		const void *out;
		int seat;
		if (mi_bridge_in_flight(br) == 3) { /* the oldest tick's mix goes out to the members, with its speaker and levels */
			mi_bridge_report rep;
			if (mi_bridge_collect(br, &out) != MI_OK || mi_bridge_collected_report(br, &rep) != MI_OK) rc = 1;
			else if (rep.seq != (uint64_t)collected || memcmp(out, want_out + (size_t)collected * seats * TICK, (size_t)seats * TICK) ||
			         memcmp(rep.winner, want_winner + (size_t)collected * nconf, (size_t)nconf * sizeof(int32_t)) ||
			         memcmp(rep.max_db, want_db + (size_t)collected * nconf, (size_t)nconf * sizeof(float)) ||
			         memcmp(rep.levels, want_levels + (size_t)collected * seats, (size_t)seats * sizeof(float))) {
				fprintf(stderr, "tick %d differs from the twin's\n", collected);
				rc = 1;
			} else if (rep.winner[0] != last_speaker) {
				printf("tick %3d: room 0's speaker is %d (%.1f dBm0)\n", collected, (int)rep.winner[0], rep.max_db[0]);
				last_speaker = rep.winner[0], ++changes_of_speaker;
			}
			++collected;
		}
		if (!rc && (mi_bridge_acquire(br, &in, &present) != MI_OK || mi_bridge_acquire(twin, &twin_in, &present) != MI_OK)) rc = 1;
		if (!rc && tick % 3 == 1) { /* the moderator: the tick being filled is the first the change holds for */
			mi_bridge_control ch[2];
			const int a = (tick * 7) % seats, b = (tick * 7 + 3) % seats;
			memset(ch, 0, sizeof(ch));
			ch[0].stream = a, ch[0].what = MI_CTL_FLAGS; /* mute or un-mute; every sixth time listen-only off as well */
			ch[0].flags = (flags[a] & MI_MIX_ACTIVE ? 0 : MI_MIX_ACTIVE) | (tick % 6 == 1 ? 0 : MI_MIX_OUTPUT);
			ch[1].stream = b, ch[1].what = MI_CTL_GAIN, ch[1].gain = 0.5f + 0.25f * (float)(tick % 5);
			if (mi_bridge_change_controls(br, ch, 2) != MI_OK) rc = 1; /* no wait: three ticks stay in flight */
			if (mi_bridge_in_flight(br) != (tick < 3 ? tick : 2)) rc = 1;
			flags[a] = (uint8_t)(MI_MIX_LINKED | ch[0].flags), gain[b] = ch[1].gain;
			if (mi_bridge_set_controls(twin, flags, gain) != MI_OK) rc = 1; /* the twin's way: waits for the device */
		}
		for (seat = 0; seat < seats && !rc; ++seat) {
			rtp_receive(tick, seat % members, members, (uint8_t *)in + (size_t)seat * TICK);
			memcpy((uint8_t *)twin_in + (size_t)seat * TICK, (uint8_t *)in + (size_t)seat * TICK, TICK);
		}
		if (!rc && (mi_bridge_submit(br) != MI_OK || mi_bridge_submit(twin) != MI_OK)) rc = 1;
		/* the twin, one tick at a time: its output and the two polls that stop its pipeline */
		if (!rc && mi_bridge_collect(twin, &out) != MI_OK) rc = 1;
		if (!rc) memcpy(want_out + (size_t)tick * seats * TICK, out, (size_t)seats * TICK);
		if (!rc && (mi_bridge_active_speakers(twin, 0, want_winner + (size_t)tick * nconf, want_db + (size_t)tick * nconf) != MI_OK ||
		            mi_bridge_get_levels(twin, want_levels + (size_t)tick * seats) != MI_OK))
			rc = 1;
	}
	while (!rc && mi_bridge_in_flight(br)) { /* (the last ticks are checked like the others in a real shutdown; here they are let go) */
		const void *out;
		if (mi_bridge_collect(br, &out) != MI_OK) rc = 1;
	}
	if (!rc && ticks >= 60 && changes_of_speaker < 2) rc = 1, fprintf(stderr, "the speaker never changed\n");
	if (rc && mi_last_error()[0]) fprintf(stderr, "moderated_bridge: %s\n", mi_last_error());
	free(flags), free(gain), free(want_out), free(want_levels), free(want_winner), free(want_db);
	mi_bridge_destroy(br);
	mi_bridge_destroy(twin);
	mi_ctx_destroy(ctx);
	puts(rc ? "failed" : "ok");
	return rc;
}
