/*
 * examples/g711_bridge.c -- the main loop of a G.711 conference server on mi_bridge (include/msmi355x_bridge.h): per
 * member decoder -> MSVolume (meter) -> MSAudioMixer pin -> encoder, what src/voip/audioconference.c builds per call
 * in the reference, for 64 conferences of 32 in one kernel launch per 10 ms tick.  No echo canceller: the endpoints'
 * job (examples/conference_bridge.c is the chain with one).  Plain C99; links against libmsmi355x.so only.
 *
 *   cc -std=c99 -Iinclude examples/g711_bridge.c -Lmediastreamer2_amd -lmsmi355x -Wl,-rpath,$PWD/mediastreamer2_amd
 *
 *   ./a.out            the mix at the legs' own 8 kHz
 *   ./a.out 16000      the same narrowband legs in a wideband conference (16000, 24000 or 48000): every pin gets the
 *                      in_resampler and out_resampler of plumb_to_conf (audioconference.c:209-257), inside the same launch
 *                      (mi_bridge_create_rated).  The rows stay 80 bytes: the pitch is the widest LEG's tick.
 *
 * Every 10 ms: the RTP side hands over one PCMU payload of 80 bytes per leg (or nothing: the leg is absent for the tick),
 * and takes back the 80 bytes to send to that leg: everybody else in its conference, mixed and encoded.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "msmi355x_bridge.h"

#define MEMBERS 32
#define CONFERENCES 64
#define TALKER 5 /* the pin that talks in every conference */

/* stand-ins for the RTP side of a real server */
static int rtp_receive(int leg, int tick, uint8_t payload[80]) {
	int i;
	if (leg % MEMBERS == TALKER) /* a 1 kHz square wave at about -9 dBm0; everybody else sends mu-law silence */
		for (i = 0; i < 80; ++i) payload[i] = (uint8_t)((i & 4) ? 0x1F : 0x9F);
	else
		memset(payload, 0xFF, 80);
	return (leg + tick) % 50 != 7; /* one packet in fifty is late */
}
static void rtp_send(int leg, const uint8_t payload[80]) {
	(void)leg;
	(void)payload;
}

int main(int argc, char **argv) {
	mi_ctx *ctx;
	mi_bridge *br;
	mi_bridge_config cfg;
	const int legs = CONFERENCES * MEMBERS;
	int tick, leg, rc = 0;
	uint8_t *flags;
	int32_t winner[CONFERENCES];
	float level[CONFERENCES];
	const int conference_rate = argc > 1 ? atoi(argv[1]) : 8000;

	if (mi_ctx_create(0, NULL, &ctx) != MI_OK) {
		fprintf(stderr, "no MI355X: %s\n", mi_last_error()); /* there is no CPU fallback */
		return 1;
	}
	mi_bridge_default_config(&cfg); /* 8 kHz, mu-law in, mu-law out */
	cfg.nstreams = legs;
	cfg.members_per_conference = MEMBERS;
	if (conference_rate == 8000) {
		rc = mi_bridge_create(ctx, &cfg, &br);
	} else { /* the legs stay 8 kHz G.711; cfg.rate is the conference's */
		int32_t *leg_rate = (int32_t *)malloc(sizeof(int32_t) * (size_t)legs);
		for (leg = 0; leg < legs; ++leg) leg_rate[leg] = 8000;
		cfg.rate = conference_rate;
		rc = mi_bridge_create_rated(ctx, &cfg, leg_rate, &br);
		free(leg_rate);
	}
	if (rc != MI_OK) {
		fprintf(stderr, "mi_bridge_create: %s\n", mi_last_error());
		return 1;
	}
	rc = 0;
	if (mi_bridge_leg_rate(br, 0) != 8000) return 1;
	/* pin 1 of every conference is muted (MS_AUDIO_MIXER_SET_ACTIVE 0: it hears, nobody hears it); pin 2 is a source that
	 * is only listened to -- an announcement player: nothing is sent back to it (MS_AUDIO_MIXER_ENABLE_OUTPUT 0) */
	flags = (uint8_t *)malloc((size_t)legs);
	memset(flags, MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT, (size_t)legs);
	for (leg = 0; leg < legs; leg += MEMBERS) {
		flags[leg + 1] = MI_MIX_LINKED | MI_MIX_OUTPUT;
		flags[leg + 2] = MI_MIX_LINKED | MI_MIX_ACTIVE;
	}
	mi_bridge_set_controls(br, flags, NULL);
	free(flags);

	for (tick = 0; tick < 300; ++tick) { /* a real server paces this loop at 10 ms */
		void *in;
		uint8_t *present, *codes;
		const void *out;
		if (mi_bridge_in_flight(br) == 3) { /* three ticks in flight: upload | kernel | download overlap */
			mi_bridge_collect(br, &out);
			for (leg = 0; leg < legs; ++leg) rtp_send(leg, (const uint8_t *)out + 80 * leg);
		}
		mi_bridge_acquire(br, &in, &present); /* pinned staging, filled in place; present[] arrives as all ones */
		codes = (uint8_t *)in;
		for (leg = 0; leg < legs; ++leg)
			if (!rtp_receive(leg, tick, codes + 80 * leg)) present[leg] = 0;
		if (mi_bridge_submit(br) != MI_OK) {
			fprintf(stderr, "mi_bridge_submit: %s\n", mi_last_error());
			return 1;
		}
		if (tick % 100 == 99) { /* ms_audio_conference_process_events: who is talking (waits for the ticks submitted) */
			mi_bridge_active_speakers(br, (uint64_t)tick * 10, winner, level);
			printf("tick %d: conference 0 hears member %d at %.1f dBm0\n", tick, (int)winner[0], (double)level[0]);
			for (leg = 0; leg < CONFERENCES; ++leg)
				if (winner[leg] != leg * MEMBERS + TALKER) rc = 1;
		}
	}
	while (mi_bridge_in_flight(br)) {
		const void *out;
		mi_bridge_collect(br, &out);
	}
	mi_bridge_destroy(br);
	mi_ctx_destroy(ctx);
	puts(rc ? "wrong speaker elected" : "ok");
	return rc;
}
