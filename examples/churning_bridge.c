/*
 * examples/churning_bridge.c -- a conference server whose members come and go, on mi_bridge (include/msmi355x_bridge.h): a
 * 16 kHz room of 8 kHz mu-law trunks that also admits A-law trunks, 16 kHz PCM and 48 kHz PCM members
 * (mi_bridge_create_open).  Every few ticks a caller hangs up and whoever dials in next takes the seat with whatever codec
 * it negotiated -- ms_audio_conference_remove_member / _add_member (src/voip/audioconference.c:322-374), where plumb_to_conf
 * hangs the new endpoint's own decoder, encoder and resamplers on the free pin.  mi_bridge_change_members never waits for the
 * device: the change travels with the next tick, three ticks stay in flight throughout, and nobody else in the room loses
 * its meter, its resamplers' histories or its concealer.  Plain C99; links against libmsmi355x.so only.
 *
 *   cc -std=c99 -Iinclude examples/churning_bridge.c -Lmediastreamer2_amd -lmsmi355x -Wl,-rpath,$PWD/mediastreamer2_amd
 *
 * The byte rows have one pitch for good (mi_bridge_tick_bytes: 960, a 48 kHz PCM tick, the widest kind admitted); a seat fills
 * and receives the first mi_bridge_leg_bytes of its row, which follow the seat's kind as soon as the call returns.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msmi355x_bridge.h"

#define MEMBERS 6
#define CONFERENCES 4
#define SEATS (MEMBERS * CONFERENCES)

static const mi_bridge_leg TRUNK = {8000, MI_SESSION_PCMU, MI_SESSION_PCMU};
static const mi_bridge_leg ADMIT[3] = {{8000, MI_SESSION_PCMA, MI_SESSION_PCMA}, {16000, MI_SESSION_PCM16, MI_SESSION_PCM16},
                                       {48000, MI_SESSION_PCM16, MI_SESSION_PCM16}};

/* a stand-in for the RTP side: the seat's payload in its own codec; seat `loud` of every room talks, the others are silent */
static void rtp_receive(int seat, int loud, int codec, uint8_t *payload, int bytes) {
	int i;
	if (codec == MI_SESSION_PCM16) {
		int16_t *pcm = (int16_t *)payload;
		for (i = 0; i < bytes / 2; ++i) pcm[i] = (int16_t)(seat % MEMBERS == loud ? ((i & 8) ? -9000 : 9000) : 0);
	} else if (seat % MEMBERS == loud) {
		for (i = 0; i < bytes; ++i) payload[i] = (uint8_t)((i & 8) ? 0x1C : 0x9C); /* a square wave in either law */
	} else {
		memset(payload, codec == MI_SESSION_PCMA ? 0xD5 : 0xFF, (size_t)bytes); /* the law's silence */
	}
}

static void print_roster(mi_bridge *br, int tick) {
	int32_t winner[CONFERENCES];
	int seat, c;
	if (mi_bridge_active_speakers(br, 0, winner, NULL) != MI_OK) return; /* (reads the meters: this one waits for the ticks submitted) */
	printf("tick %3d:", tick);
	for (c = 0; c < CONFERENCES; ++c) {
		printf("  room %d (%d seated, speaker %d) [", c, mi_bridge_member_count(br, c), (int)winner[c]);
		for (seat = c * MEMBERS; seat < (c + 1) * MEMBERS; ++seat) {
			int in = 0;
			mi_bridge_leg_codec(br, seat, &in, NULL);
			printf("%s%d%s", seat % MEMBERS ? " " : "", mi_bridge_leg_rate(br, seat) / 1000, in == MI_SESSION_PCMU ? "u" : in == MI_SESSION_PCMA ? "a" : "");
		}
		printf("]");
	}
	printf("\n");
}

int main(void) {
	mi_ctx *ctx;
	mi_bridge *br;
	mi_bridge_config cfg;
	mi_bridge_leg legs[SEATS];
	int seated[SEATS];
	int tick, seat, in_pitch, out_pitch, rc = 0, next_kind = 0;

	if (mi_ctx_create(0, NULL, &ctx) != MI_OK) {
		fprintf(stderr, "no MI355X: %s\n", mi_last_error()); /* there is no CPU fallback */
		return 1;
	}
	mi_bridge_default_config(&cfg);
	cfg.nstreams = SEATS;
	cfg.members_per_conference = MEMBERS;
	cfg.rate = 16000;
	for (seat = 0; seat < SEATS; ++seat) legs[seat] = TRUNK, seated[seat] = 1;
	if (mi_bridge_create_open(ctx, &cfg, legs, ADMIT, 3, &br) != MI_OK) {
		fprintf(stderr, "mi_bridge_create_open: %s\n", mi_last_error());
		return 1;
	}
	if (mi_bridge_tick_bytes(br, &in_pitch, &out_pitch) != MI_OK || in_pitch != 960 || out_pitch != 960) rc = 1;
	{ /* a kind that was not admitted is refused, and nothing changes */
		mi_bridge_change bad = {0, MI_BRIDGE_JOIN, {32000, MI_SESSION_PCM16, MI_SESSION_PCM16}};
		if (mi_bridge_change_members(br, &bad, 1) != MI_ENOTSUP || mi_bridge_leg_rate(br, 0) != 8000) rc = 1;
	}

	for (tick = 0; tick < 120 && !rc; ++tick) { /* a real server paces this loop at 10 ms */
		void *in;
		uint8_t *present;
		const void *out;
		if (mi_bridge_in_flight(br) == 3 && mi_bridge_collect(br, &out) != MI_OK) rc = 1; /* three ticks in flight */
		if (!rc && mi_bridge_acquire(br, &in, &present) != MI_OK) rc = 1;
		if (!rc && tick % 4 == 1) { /* a seat changes hands: the tick being filled is the first the new roster holds for */
			mi_bridge_change ch;
			ch.stream = (tick * 7) % SEATS, ch.op = seated[ch.stream] && tick % 3 == 0 ? MI_BRIDGE_LEAVE : MI_BRIDGE_JOIN;
			ch.leg = next_kind % 4 == 3 ? TRUNK : ADMIT[next_kind % 4];
			if (ch.op == MI_BRIDGE_JOIN) ++next_kind;
			if (mi_bridge_change_members(br, &ch, 1) != MI_OK) rc = 1;
			seated[ch.stream] = ch.op == MI_BRIDGE_JOIN;
		}
		for (seat = 0; seat < SEATS && !rc; ++seat) {
			int bytes, codec;
			if (!seated[seat]) continue; /* nobody sends on a pin that is not plumbed */
			if (mi_bridge_leg_bytes(br, seat, &bytes, NULL) != MI_OK || mi_bridge_leg_codec(br, seat, &codec, NULL) != MI_OK) rc = 1;
			else rtp_receive(seat, (tick / 40) % MEMBERS, codec, (uint8_t *)in + (size_t)in_pitch * seat, bytes);
		}
		if (!rc && mi_bridge_submit(br) != MI_OK) rc = 1;
		if (!rc && tick % 20 == 19) print_roster(br, tick);
	}
	if (rc) fprintf(stderr, "churning_bridge: %s\n", mi_last_error());
	while (mi_bridge_in_flight(br)) {
		const void *out;
		if (mi_bridge_collect(br, &out) != MI_OK) break;
	}
	mi_bridge_destroy(br);
	mi_ctx_destroy(ctx);
	puts(rc ? "failed" : "ok");
	return rc;
}
