// session_legs.hpp -- what session_legs.hip keeps on the device for a session whose legs differ in rate or codec
// (mi_session_create_legs, session.hip): every leg's ratio byte and codec pair, both resamplers' history rows and the shared
// tables, and the two launches around the canceller and the mixer -- session_ingress_kernel in front, session_egress_kernel
// behind.  The plan (session_plan.hpp, no HIP) has decided every size.
#pragma once
#include "common.hpp"

#include <vector>

struct SessionLegsSizes { // the plan's figures, handed over as plain numbers: session_plan.hpp lives in its includer's namespace
	int n, len, rate;                             // legs; the canceller's tick in samples and its rate
	int hin_stride, hout_stride;                  // samples per leg of the history rows, multiples of eight
	int in_row, in_scratch, out_scratch;          // a wavefront's LDS, bytes
	const bool *used;                             // [7] the ratios > 1 among the legs
	const uint8_t *ratio, *codec;                 // [n] on the host
};

struct SessionLegs {
	mi_ctx *ctx = nullptr;
	SessionLegsSizes z = {};
	uint8_t *d_ratio = nullptr;
	uint8_t *d_codec = nullptr; // [2][n]: mic_codec | out_codec << 2, and the same with PCM in (behind the concealer)
	int16_t *d_hist_in = nullptr, *d_hist_out = nullptr;
	float *d_tab = nullptr;
	int tab_up[7] = {}, tab_down[7] = {}; // float offsets of ratio r's tables in d_tab
};

int mi_session_legs_create(mi_ctx *ctx, const SessionLegsSizes &sizes, SessionLegs **out);
void mi_session_legs_destroy(SessionLegs *g);
// both histories of legs [first, first + count) zero, as speex_resampler_init leaves them; on the context's stream
int mi_session_legs_reset(SessionLegs *g, int first, int count);
// d_in: the legs' byte rows at in_pitch bytes, read through every leg's mic codec -- or, pcm: the concealer's int16 rows at
// in_pitch bytes; d_mic [n][mic_stride] the microphone tick at `rate` for the canceller, mic_stride a multiple of eight
int mi_session_legs_ingress(SessionLegs *g, const uint8_t *d_in, size_t in_pitch, bool pcm, int16_t *d_mic, int mic_stride);
// d_mix [n][len] the legs' mixes at `rate`; d_out: the legs' byte rows at out_pitch bytes, written through every leg's out codec
int mi_session_legs_egress(SessionLegs *g, const int16_t *d_mix, uint8_t *d_out, size_t out_pitch);
