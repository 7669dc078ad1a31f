// bridge_roster.hpp -- what bridge_roster.hip's kernel is handed by bridge.hip: a tick's membership changes and every array of
// the bridge that a new endpoint on a seat rewrites.  What a bridge does not have (no resamplers, codecs at compile time) is
// null and is skipped.
#pragma once
#include "common.hpp"

struct RosterArgs {
	const mi_seat_cmd *cmd; // [count]
	int count, nstreams;
	uint8_t *ratio;     // [nstreams] the ratio bytes, or null
	uint8_t *codec;     // [nstreams] in_codec | out_codec << 2, or null
	uint8_t *codec_pcm; // the same behind the concealer ("PCM in"), or null
	VolumeEdit vol;
	uint8_t *flags;     // the pins' MI_MIX_*
	int16_t *hist_in, *hist_out; // both resamplers' histories at hin_stride / hout_stride samples per seat, or null
	int hin_stride, hout_stride;
	uint8_t *out; // this tick's slot: the output rows at out_bytes
	int out_bytes;
};

// bridge_roster_kernel, one wavefront per command, on `stream`
int mi_bridge_roster_launch(const RosterArgs &args, hipStream_t stream);
