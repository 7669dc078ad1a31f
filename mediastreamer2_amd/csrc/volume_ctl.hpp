// volume_ctl.hpp -- MSVolume's per-chunk control chain on the device (msvolume.c:388-445), shared by the kernels of
// volume.hip and the bridge's fused tick (bridge.hip).  Every unit that includes this is built with -ffp-contract=off:
// the chain is float32 evaluated unfused in source order on the reference's x86-64 build, and the integer gain (hence
// every output sample) depends on it bit for bit.
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int sat16(int v) { return (v > 32767) ? 32767 : ((v < -32767) ? -32767 : v); }

// What update_energy leaves behind and everything volume_process derives from it for one chunk (msvolume.c:388-407,
// :172-260, :409-445's gain ramp): the smoothed energy, the echo limiter / AGC / noise gate targets, the ramped gain as the
// Q12 integer the samples are scaled with, the DC estimate, the one-second maximum.  acc = the float32 sum of the squares
// in sample order, pk / dcsum = integer peak and sum of the chunk.  One lane per stream; shared by volume_kernel, volmix_kernel
// (volume.hip) and bridge_tick_kernel (bridge.hip).
struct VolCtl {
	int intgain, dcoff, mode; // mode 0: samples untouched (gain exactly 1), 1: gain, 2: DC removal + gain
};
__device__ __forceinline__ VolCtl volume_control(const mi_volume_params &p, mi_volume_state &st, float peer_energy, float acc, int n, int pk,
                                                 int dcsum, int sample_rate, float2 &win) {
	const float max_e = (32768 * 0.7f);
	VolCtl o;
	const float en = (float)((sqrt((double)(acc / n)) + 1) / (double)max_e);
	st.energy = (en * 0.2f) + st.energy * (1.0f - 0.2f);
	st.level_pk = (float)pk / max_e;
	st.instant_energy = en;

	float target = p.static_gain;
	if (p.peer != -1) { // echo limiter
		const float peer_e = peer_energy, peer_pk = peer_e;
		if (peer_pk > st.lt_speaker_en) st.lt_speaker_en = peer_pk;
		else st.lt_speaker_en = (0.005f * peer_pk) + (0.995f * st.lt_speaker_en);
		const float ratio = (st.energy / (st.lt_speaker_en + p.ea_thres));
		if (peer_e > p.ea_thres) {
			if (ratio > p.ea_transmit_thres) {
				st.target_gain = p.static_gain;
				st.fast_upramp = 1;
			} else {
				st.target_gain = p.static_gain / (1 + (peer_e * p.force));
				st.sustain_dur = p.sustain_time;
			}
		} else {
			if (st.sustain_dur > 0) {
				st.sustain_dur -= (n * 1000) / sample_rate;
			} else {
				st.target_gain = p.static_gain;
				st.fast_upramp = 1;
			}
		}
		target = st.target_gain;
	}
	if (p.agc_enabled) target /= (0.5f + st.level_pk) / 1;
	if (p.noise_gate_enabled) {
		float tgain = p.ng_floorgain;
		if (st.instant_energy > p.ng_threshold) {
			st.ng_noise_dur = p.ng_cut_time;
			tgain = 1.0f;
		} else if (st.ng_noise_dur > 0) {
			st.ng_noise_dur -= (n * 1000) / sample_rate;
			tgain = 1.0f;
		}
		st.ng_gain = st.ng_gain * 0.75f + tgain * 0.25f;
	}
	// apply_gain: multiplicative ramp toward target
	if (st.gain < target) {
		if (st.gain < p.ng_floorgain) st.gain = p.ng_floorgain;
		st.gain *= 1 + (st.fast_upramp ? p.vol_fast_upramp : p.vol_upramp);
		if (st.gain > target) st.gain = target;
	} else if (st.gain > target) {
		st.gain *= 1 - p.vol_downramp;
		if (st.gain < target) st.gain = target;
		st.fast_upramp = 0;
	}
	const float gain = st.gain * st.ng_gain;
	o.intgain = (int32_t)(gain * 4096);
	o.dcoff = st.dc_offset;
	if (p.remove_dc) {
		o.mode = 2;
		st.dc_offset = (st.dc_offset * 7 + dcsum * 2 / (2 * n)) / 8;
	} else {
		o.mode = (gain != 1) ? 1 : 0;
	}
	{ // ortp_extremum_record_max(&v->max, curtime, v->energy), period 1000 ms
		float2 w = win;
		if (w.y >= 0) {
			w.y += (float)((n * 1000) / sample_rate);
			if (w.y > 1000.f) w.y = -1.f; // (int)(now - start) > period: the old maximum is dropped
		}
		if (w.y < 0) w = make_float2(st.energy, 0.f);
		if (st.energy > w.x) w.x = st.energy;
		win = w;
	}
	return o;
}

} // namespace
