// session_plan.hpp -- what mi_session_create_legs decides before anything is allocated, as plain C++ with no HIP in it, the way
// bridge_plan.hpp does for the bridge (whose ratio_byte, resampler lengths and LDS bound it reuses): the refusals, whether the
// legs are all one kind (then the session is mi_session_create's, and nothing below is used), the byte rows' pitches, every
// leg's ratio byte and codec pair, the history strides and the LDS of session_legs.hip's two kernels.
// tests/host/session_legs_plan_check.cpp runs the plan alone on the CPU.
#pragma once
#include "bridge_plan.hpp"

#include <cstdio>

#include "../../include/msmi355x_session.h"

namespace {

constexpr int SESSION_LEG_WAVES = 4; // one wavefront per leg, four legs per workgroup (session_ingress_kernel, session_egress_kernel)

// samples a leg's resamplers keep from tick to tick: the up-sampler's taps - 1 whatever the ratio, the down-sampler's
// ratio * 48 - 1 (none at ratio 1)
constexpr int session_up_hist() { return RS_FILT - 1; }
constexpr int session_down_hist(int ratio) { return ratio > 1 ? ratio * RS_FILT - 1 : 0; }

struct SessionPlan {
	// every leg names one kind: `cfg` is mi_session_create's configuration of that session (in_rate = out_rate = the legs' rate,
	// their codecs), and nothing else of the plan is read
	bool uniform = false;
	mi_session_config cfg = {};
	int n = 0, len = 0;         // legs; the canceller's tick in samples
	int max_ratio = 1;
	bool used[7] = {};          // the ratios rate / leg rate > 1 among the legs: a pair of tables each
	size_t mic_pitch = 0, out_pitch = 0; // bytes per row of `mic` and `out`: the widest leg's tick in bytes, rounded up to 16
	int pcm_pitch = 0;          // samples per row of the concealer's PCM (cfg.plc): the widest leg's tick, whole groups of eight
	int hin_stride = RS_FILT;   // samples per leg of the up-samplers' history rows (47 kept, one pad slot)
	int hout_stride = RS_FILT;  // and of the down-samplers': max_ratio * 48 (ratio * 48 - 1 kept)
	// a wavefront's share of the dynamic LDS, bytes: session_ingress_kernel's row of one tick at `rate` and its up-sampler's flat
	// window behind it; session_egress_kernel's phase arrays and partial sums
	int in_row = 0, in_scratch = 0, out_scratch = 0;
	size_t ingress_lds = 0, egress_lds = 0; // of a workgroup
	std::vector<int32_t> rate;  // [n]
	std::vector<uint8_t> ratio; // [n] rate / leg rate: 1, 2, 3 or 6
	std::vector<uint8_t> codec; // [n] mic_codec | out_codec << 2
	int leg_len(int s) const { return rate[(size_t)s] / 100; }
	int mic_bytes(int s) const { return leg_len(s) * ((codec[(size_t)s] & 3) ? 1 : 2); }
	int out_bytes(int s) const { return leg_len(s) * ((codec[(size_t)s] >> 2) ? 1 : 2); }
};

// MI_OK, or the refusal with its text set (MI_ENOTSUP: the leg, both rates and the reason); *p is whole only with MI_OK.
inline int plan_session_legs(const mi_session_config *cfg, const mi_session_leg *legs, SessionPlan *p) {
	const char *fn = "mi_session_create_legs";
	MI_PLAN_ARG(cfg && legs && p);
	MI_PLAN_ARG(cfg->nstreams > 0 && cfg->members_per_conference > 0 && cfg->nstreams % cfg->members_per_conference == 0);
	MI_PLAN_ARG(cfg->rate > 0 && cfg->rate % 100 == 0 && cfg->tail_ms > 0);
	MI_PLAN_ARG(cfg->ref_delay_ms >= 0 && cfg->ref_delay_ms <= 1000);
	*p = SessionPlan();
	const int n = p->n = cfg->nstreams, len = p->len = cfg->rate / 100;
	bool uniform = true;
	for (int s = 0; s < n; ++s) {
		const mi_session_leg &l = legs[s];
		for (int v : {l.mic_codec, l.out_codec})
			if (v < MI_SESSION_PCM16 || v > MI_SESSION_PCMU)
				MI_REFUSE("%s: leg %d at %d Hz in a %d Hz session names codec %d: not one of the codecs served, MI_SESSION_PCM16 (0), "
				          "MI_SESSION_PCMA (1), MI_SESSION_PCMU (2)", fn, s, l.rate, cfg->rate, v);
		MI_PLAN_ARG(l.rate > 0);
		if (l.rate > cfg->rate)
			MI_REFUSE("%s: leg %d at %d Hz is above the session's %d Hz, the canceller's rate: only legs at or below it are resampled", fn, s,
			          l.rate, cfg->rate);
		int rb = ratio_byte(l.rate, cfg->rate);
		if (rb >= 0 && (rb & (int)UD_R32)) rb = NO_WHOLE_RATIO; // (2/3 of the rate: the bridge's rational form, not the session's)
		if (rb == NO_WHOLE_RATIO)
			MI_REFUSE("%s: leg %d at %d Hz in a %d Hz session is no whole ratio (%.3f); supported: 1, 2, 3, 6", fn, s, l.rate, cfg->rate,
			          (double)cfg->rate / l.rate);
		if (rb == RATIO_NOT_SERVED)
			MI_REFUSE("%s: leg %d at %d Hz in a %d Hz session is ratio %d; supported: 1, 2, 3, 6", fn, s, l.rate, cfg->rate, cfg->rate / l.rate);
		if (l.rate % 800 != 0)
			MI_REFUSE("%s: leg %d at %d Hz in a %d Hz session: the rate is no multiple of 800 (a 10 ms tick must be whole groups of 8 samples)",
			          fn, s, l.rate, cfg->rate);
		uniform &= l.rate == legs[0].rate && l.mic_codec == legs[0].mic_codec && l.out_codec == legs[0].out_codec;
		p->rate.push_back(l.rate);
		p->ratio.push_back((uint8_t)rb);
		p->codec.push_back((uint8_t)(l.mic_codec | l.out_codec << 2));
		p->used[rb] |= rb > 1;
		p->max_ratio = std::max(p->max_ratio, rb);
	}
	if (cfg->plc) { // what the concealer cannot serve, in its own words behind the session's rate
		char where[96];
		snprintf(where, sizeof(where), "%s: plc in a %d Hz session", fn, cfg->rate);
		for (int s = 0; s < n; ++s)
			if (const int rc = mi_plc_check_rate(where, "leg", s, legs[s].rate)) return rc;
	}
	p->cfg = *cfg;
	if (uniform) { // mi_session_create's session: the up-sampler folded into the canceller's launch, its rows, its tick bytes
		p->uniform = true;
		p->cfg.in_rate = p->cfg.out_rate = legs[0].rate;
		p->cfg.mic_codec = legs[0].mic_codec, p->cfg.out_codec = legs[0].out_codec;
		return MI_OK;
	}
	// ---- the rows: the widest leg's tick in bytes, rounded up to the 16 bytes a lane loads
	int widest = 0;
	for (int s = 0; s < n; ++s) {
		p->mic_pitch = std::max(p->mic_pitch, (size_t)p->mic_bytes(s)), p->out_pitch = std::max(p->out_pitch, (size_t)p->out_bytes(s));
		widest = std::max(widest, p->leg_len(s));
	}
	p->mic_pitch = up16(p->mic_pitch), p->out_pitch = up16(p->out_pitch);
	p->pcm_pitch = (widest + 7) & ~7;
	p->hout_stride = p->max_ratio * RS_FILT;
	// ---- the LDS of the two launches, per wavefront the largest form a leg needs
	p->in_row = (int)up16((size_t)len * sizeof(int16_t));
	for (int r = 2; r < 7; ++r) {
		if (!p->used[r]) continue;
		p->in_scratch = std::max(p->in_scratch, (int)up16((size_t)rs_flat_len(len / r) * sizeof(float)));
		p->out_scratch = std::max(p->out_scratch, (int)up16(((size_t)r * rs_plen(RS_FILT, r, len) + (size_t)len) * sizeof(float)));
	}
	p->ingress_lds = (size_t)SESSION_LEG_WAVES * (p->in_row + p->in_scratch);
	p->egress_lds = (size_t)SESSION_LEG_WAVES * p->out_scratch;
	if (std::max(p->ingress_lds, p->egress_lds) > BRIDGE_LDS_MAX)
		MI_REFUSE("%s: a %d Hz session with legs down to ratio %d: %d wavefronts' resamplers must fit %zu bytes of LDS (%zu in front of the "
		          "canceller, %zu behind the mix)", fn, cfg->rate, p->max_ratio, SESSION_LEG_WAVES, BRIDGE_LDS_MAX, p->ingress_lds, p->egress_lds);
	return MI_OK;
}

} // namespace
