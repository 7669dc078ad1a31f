// session_roster.hpp -- what session_roster.hip's kernel is handed by session.hip: a tick's membership changes and every array
// of the session that a new endpoint on a seat rewrites, as the edit records and views of common.hpp.  What a session does not
// have (no up-sampler, no down-sampler, no kept mix) is null and is skipped.
#pragma once
#include "common.hpp"

constexpr int SESSION_ROSTER_SLOTS = 3;

struct SessionRosterArgs {
	const mi_seat_cmd *cmd; // [count]
	int count, nstreams;
	AecEdit aec;
	ResamplerEdit rs_in, rs_out;
	bool leg_rows; // rs_in, rs_out are the per-leg history rows of session_legs.hip (mi_session_create_legs): no position word
	VolumeEdit vol;
	uint8_t *flags; // the pins' MI_MIX_*
	FifoView f_mic, f_ref, f_out;
	int ref_delay;               // samples of silence a fresh reference FIFO starts with (speexec.c:205-208)
	int lead_unit, lead_phases;  // mi_aec_stagger_info's; phases < 2: no lead
	int16_t *mix[SESSION_ROSTER_SLOTS]; // the kept mix of every slot ([nstreams][mix_len]), or null
	int mix_len;
	uint8_t *out; // this tick's slot: the output rows at out_bytes
	int out_bytes;
};

// session_roster_kernel, one workgroup per command, on `stream`
int mi_session_roster_launch(const SessionRosterArgs &args, hipStream_t stream);
