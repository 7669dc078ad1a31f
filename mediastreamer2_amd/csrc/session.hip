// session.hip -- the chained hot path for a batch of call legs, fed from host buffers, one 10 ms tick per call:
//   MSResample in_rate->rate -> FIFO (ticks -> canceller frames) -> MSSpeexEC (+post-filter) -> FIFO (frames -> ticks)
//   -> MSVolume (AGC) -> MSAudioMixer (conferences of `members`, conference mode)
// i.e. what BASELINE.json's north_star counts per stream, as ONE object for a media server that does not run the
// reference's per-filter ticker (a batch-aware runtime).  It owns nothing but plumbing: every
// stage is the C ABI object of its filter (mi_resampler, mi_aec, ...), so its output is by construction the output of
// tests/test_gpu_pipeline.py's chain.
//
// Three HIP streams: uploads, kernels (the context's stream), downloads.  A tick's inputs go up while the previous
// tick computes and the one before comes down; events order the three (mi::TickPipe, tick_pipe.hpp), hipGraphs (one per
// buffer slot) replay the kernel sequence.  Pinned host buffers belong to the session: the caller fills / reads them in place.
// Membership, controls and reports -- waiting or carried by the ticks -- are mi::ConferencePlane's (controls.hpp); here is what
// is the session's own: launch_seats, mi_session_reset_streams, the rows a departed leg leaves behind, two meter read-outs.
// mi_session_create_legs: legs at their own rate and codec -- the plan is session_plan.hpp's, the two launches around the
// canceller and the mixer session_legs.hip's (run_leg_tick).
#include "common.hpp"

#include "../../include/msmi355x_session.h"
#include "../../include/msmi355x_session_controls.h"
#include "controls.hpp"
#include "session_legs.hpp"
#include "session_plan.hpp"
#include "session_roster.hpp"

#include <cmath>

namespace {
constexpr int SLOTS = 3; // upload | compute | download can each hold a different tick
static_assert(SLOTS == SESSION_ROSTER_SLOTS, "the roster kernel clears the kept mix of every slot");
}

struct mi_session {
	mi_ctx *ctx = nullptr;
	mi_session_config cfg;
	int n = 0, in_len = 0, len = 0, frame = 0, up_stride = 0;
	int out_len = 0, down_stride = 0;               // samples per tick leaving, row pitch of the down-sampled mix
	size_t mic_bytes = 0, ref_bytes = 0, out_bytes = 0; // per stream and tick, on the host side
	mi_resampler *rs = nullptr, *rs_out = nullptr;
	mi_plc *plc = nullptr;
	uint8_t *h_ev[SLOTS] = {}, *d_ev[SLOTS] = {};
	int32_t *d_evlen = nullptr;
	int16_t *d_pcm = nullptr, *d_down = nullptr, *d_zero = nullptr;
	int16_t *d_mix[SLOTS] = {}; // the mix at `rate` per slot when it is not what leaves (out_rate / out_codec / loopback)
	mi_aec *aec = nullptr;
	mi_volume *vol = nullptr;
	mi_mixer *mix = nullptr;
	mi_fifo *f_mic = nullptr, *f_ref = nullptr, *f_out = nullptr;
	mi::TickPipe pipe;
	int16_t *h_mic[SLOTS] = {}, *h_ref[SLOTS] = {}, *h_out[SLOTS] = {};
	int16_t *d_mic[SLOTS] = {}, *d_ref[SLOTS] = {}, *d_out[SLOTS] = {};
	int16_t *d_up = nullptr, *d_tick = nullptr;
	bool fold_resampler = true; // the canceller's launch runs the up-sampler too (until it says it cannot)
	bool fuse_mix = true;       // volume + conference mix in one launch (likewise)
	int rounds = 0;                 // the canceller's frames of a tick, at most (max_frames of its call)
	uint8_t *d_reset_gate = nullptr; // [n] mi_session_reset_streams: 1 = the leg's reference FIFO gets its delay again
	mi_graph *graph[SLOTS] = {};
	// conference membership, controls and reports (MSAudioConference), the waiting calls' and what travels with the ticks: controls.hpp
	mi::ConferencePlane conf;
	int lead_unit = 0, lead_phases = 0; // cfg.stagger: mi_aec_stagger_info's, what a fresh seat's queues lead with
	// mi_session_create_legs: every leg's kind as it was given (empty: mi_session_create's session, cfg's one kind).  With legs
	// that differ, `plan` is whole and `legs` holds their ingress and egress (session_legs.hip): `mic` and `out` are byte rows at
	// mic_bytes / out_bytes, no mi_resampler and no encoder's launch, d_up the ingress' tick at `rate`, the mix always kept
	std::vector<mi_session_leg> kinds;
	SessionPlan plan;
	SessionLegs *legs = nullptr;
};

namespace {

// the mixer side of a tick, into `mix` [n][len]: what both kinds of session run behind the canceller
int level_and_mix(mi_session *s, int16_t *mix) {
	int rc;
	// MSVolume on the tick the mixer side reads: popped from the canceller's output FIFO inside the kernel where the sizes
	// allow 16-byte groups (every rate in use), else pop + process
	// MSVolume + MSAudioMixer: one launch (every leg's tick popped from the canceller's output FIFO, levelled, the conference
	// mixed from the levelled ticks on the chip) where the sizes allow 16-byte groups (every rate in use); else pop, level, mix
	rc = s->fuse_mix ? mi_mixer_process_volume_fifo(s->mix, s->vol, 0, s->f_out, mix) : MI_ENOTSUP;
	if (rc == MI_ENOTSUP) {
		s->fuse_mix = false;
		if ((s->len & 7) == 0) {
			if ((rc = mi_volume_process_fifo(s->vol, s->f_out, s->d_tick, s->len, s->len)) != MI_OK) return rc;
		} else {
			if ((rc = mi_fifo_pop(s->f_out, s->len, s->d_tick, s->len, nullptr, nullptr, 1)) != MI_OK) return rc;
			if ((rc = mi_volume_process(s->vol, s->d_tick, s->len, s->len, nullptr)) != MI_OK) return rc;
		}
		rc = mi_mixer_process(s->mix, s->d_tick, nullptr, 1, mix);
	}
	return rc;
}

// a tick of a session whose legs differ (mi_session_create_legs): the concealer with the decoders inside, the ingress, the
// canceller on the ingress' tick, volume + mix into the kept mix, the egress
int run_leg_tick(mi_session *s, int slot) {
	int rc;
	const uint8_t *in = reinterpret_cast<const uint8_t *>(s->d_mic[slot]);
	size_t in_pitch = s->mic_bytes;
	if (s->plc) { // every leg's decoder and MSGenericPLC at its own rate: byte rows in, PCM rows out
		if ((rc = mi_plc_process_legs(s->plc, in, s->mic_bytes, s->d_pcm, (size_t)s->plan.pcm_pitch, s->d_ev[slot])) != MI_OK) return rc;
		in = reinterpret_cast<const uint8_t *>(s->d_pcm), in_pitch = (size_t)s->plan.pcm_pitch * sizeof(int16_t);
	}
	if ((rc = mi_session_legs_ingress(s->legs, in, in_pitch, s->plc != nullptr, s->d_up, s->up_stride)) != MI_OK) return rc;
	const int16_t *ref = s->cfg.ref_loopback ? s->d_mix[(slot + SLOTS - 1) % SLOTS] : s->d_ref[slot];
	if ((rc = mi_aec_process_fifos(s->aec, s->f_mic, s->d_up, s->up_stride, s->f_ref, ref, s->len, nullptr, s->len, s->f_out, s->rounds,
	                               MI_AEC_POSTFILTER, nullptr)) != MI_OK)
		return rc;
	if ((rc = level_and_mix(s, s->d_mix[slot])) != MI_OK) return rc;
	return mi_session_legs_egress(s->legs, s->d_mix[slot], reinterpret_cast<uint8_t *>(s->d_out[slot]), s->out_bytes);
}

int run_tick_kernels(mi_session *s, int slot) { // everything on the context's stream
	if (s->legs) return run_leg_tick(s, slot);
	int rc;
	const mi_session_config &cf = s->cfg;
	const int16_t *mic = s->d_mic[slot];
	if (cf.mic_codec) { // MSAlawDec / MSUlawDec
		if ((rc = mi_g711_decode(s->ctx, cf.mic_codec == MI_SESSION_PCMA ? MI_LAW_PCMA : MI_LAW_PCMU, (const uint8_t *)s->d_mic[slot],
		                         (size_t)s->in_len, s->d_pcm, (size_t)s->in_len, nullptr, s->in_len, (size_t)s->n)) != MI_OK)
			return rc;
		mic = s->d_pcm;
	}
	if (s->plc) { // MSGenericPLC behind the decoder: lost legs are concealed, the others delayed by 5 ms (edits the rows in place)
		int16_t *rows = cf.mic_codec ? s->d_pcm : s->d_mic[slot];
		if ((rc = mi_plc_process(s->plc, rows, (size_t)s->in_len, s->d_evlen, s->d_ev[slot])) != MI_OK) return rc;
	}
	// far end: from the host, or what this leg was sent one tick ago
	const int16_t *ref = cf.ref_loopback ? s->d_mix[(slot + SLOTS - 1) % SLOTS] : s->d_ref[slot];
	// MSResample + MSSpeexEC for the tick, FIFOs included: the microphone block is up-sampled, both blocks are queued, the one
	// or two whole frames (480 / 256) a leg then holds are cancelled + post-filtered, the cleaned frames queued for the mixer
	// side -- ONE launch where the canceller's kernel can run the up-sampler itself (integer ratios: 16k -> 48k, 8k -> 48k,
	// 8k -> 16k), else the resampler's launch and then the canceller's
	rc = MI_ENOTSUP;
	if (s->rs && s->fold_resampler)
		rc = mi_aec_process_fifos_resampled(s->aec, s->rs, mic, s->in_len, s->in_len, s->f_mic, s->f_ref, ref, s->len, nullptr, s->f_out,
		                                    s->rounds, MI_AEC_POSTFILTER, nullptr);
	if (rc == MI_ENOTSUP) {
		s->fold_resampler = false; // decided once: the shapes do not change
		const int16_t *mic_tick = mic; // the microphone block at the processing rate
		int mic_stride = s->len;
		if (s->rs) {
			if ((rc = mi_resampler_process(s->rs, mic, s->in_len, s->in_len, s->d_up, s->up_stride, nullptr)) != MI_OK) return rc;
			mic_tick = s->d_up;
			mic_stride = s->up_stride;
		}
		rc = mi_aec_process_fifos(s->aec, s->f_mic, mic_tick, mic_stride, s->f_ref, ref, s->len, nullptr, s->len, s->f_out, s->rounds,
		                          MI_AEC_POSTFILTER, nullptr);
	}
	if (rc != MI_OK) return rc;
	int16_t *mix = s->d_mix[slot] ? s->d_mix[slot] : s->d_out[slot];
	if ((rc = level_and_mix(s, mix)) != MI_OK) return rc;
	const int16_t *leaving = mix;
	int pitch = s->len;
	if (s->rs_out) { // MSResample rate -> out_rate
		if ((rc = mi_resampler_process(s->rs_out, mix, s->len, s->len, s->d_down, s->down_stride, nullptr)) != MI_OK) return rc;
		leaving = s->d_down;
		pitch = s->down_stride;
	}
	if (cf.out_codec) // MSAlawEnc / MSUlawEnc
		return mi_g711_encode(s->ctx, cf.out_codec == MI_SESSION_PCMA ? MI_LAW_PCMA : MI_LAW_PCMU, leaving, (size_t)pitch,
		                      (uint8_t *)s->d_out[slot], (size_t)s->out_len, nullptr, s->out_len, (size_t)s->n);
	if (leaving != s->d_out[slot]) // 16-bit output that went through the down-sampler (or a kept mix): pack the rows
		MI_HIP(hipMemcpy2DAsync(s->d_out[slot], (size_t)s->out_len * 2, leaving, (size_t)pitch * 2, (size_t)s->out_len * 2, (size_t)s->n,
		                        hipMemcpyDeviceToDevice, s->ctx->stream));
	return MI_OK;
}

// a tick that carries membership changes: the session's own state in one launch (mi::ConferencePlane::apply's seat_launch)
int launch_seats(mi_session *s, int slot, const mi_seat_cmd *d_cmd, int count) {
	SessionRosterArgs ra = {};
	ra.cmd = d_cmd, ra.count = count, ra.nstreams = s->n;
	mi_aec_edit(s->aec, &ra.aec);
	mi_resampler_edit(s->rs, &ra.rs_in);
	mi_resampler_edit(s->rs_out, &ra.rs_out);
	if (s->legs) { // the two per-leg history rows: a tick is whole periods, so these resamplers keep no position
		ra.leg_rows = true;
		ra.rs_in.hist = s->legs->d_hist_in, ra.rs_in.hist_stride = s->plan.hin_stride;
		ra.rs_out.hist = s->legs->d_hist_out, ra.rs_out.hist_stride = s->plan.hout_stride;
	}
	mi_volume_edit(s->vol, &ra.vol);
	MixerEdit me;
	mi_mixer_edit(s->mix, &me);
	ra.flags = me.flags;
	ra.f_mic = fifo_view(s->f_mic), ra.f_ref = fifo_view(s->f_ref), ra.f_out = fifo_view(s->f_out);
	ra.ref_delay = s->cfg.ref_delay_ms * s->cfg.rate / 1000;
	ra.lead_unit = s->lead_unit, ra.lead_phases = s->lead_phases;
	for (int i = 0; i < SLOTS; ++i) ra.mix[i] = s->d_mix[i];
	ra.mix_len = s->len;
	ra.out = reinterpret_cast<uint8_t *>(s->d_out[slot]), ra.out_bytes = (int)s->out_bytes;
	return mi_session_roster_launch(ra, s->ctx->stream);
}

} // namespace

extern "C" {

void mi_session_default_config(mi_session_config *c) {
	if (!c) return;
	memset(c, 0, sizeof(*c));
	c->nstreams = 32;
	c->members_per_conference = 32;
	c->in_rate = 16000;
	c->rate = 48000;
	c->tail_ms = 128;
	c->agc = 1;
	c->stagger = 1;
	c->use_graphs = 0; // per-tick graphs cost more to launch than ~17 kernels do (0.99 vs 0.68 ms at 4096 streams); no gain at 65536
}

void mi_session_destroy(mi_session *s) {
	if (!s) return;
	mi_ctx *c = s->ctx;
	(void)c->activate();
	s->pipe.drain();
	for (int i = 0; i < SLOTS; ++i) {
		if (s->graph[i]) mi_graph_destroy(s->graph[i]);
		if (s->h_mic[i]) mi_host_free(c, s->h_mic[i]);
		if (s->h_ref[i]) mi_host_free(c, s->h_ref[i]);
		if (s->h_out[i]) mi_host_free(c, s->h_out[i]);
		if (s->d_mic[i]) mi_dev_free(c, s->d_mic[i]);
		if (s->d_ref[i]) mi_dev_free(c, s->d_ref[i]);
		if (s->d_out[i]) mi_dev_free(c, s->d_out[i]);
		if (s->d_mix[i]) mi_dev_free(c, s->d_mix[i]);
		if (s->h_ev[i]) mi_host_free(c, s->h_ev[i]);
		if (s->d_ev[i]) mi_dev_free(c, s->d_ev[i]);
	}
	s->conf.destroy();
	void *dv[] = {s->d_up, s->d_tick, s->d_pcm, s->d_down, s->d_zero, s->d_evlen, s->d_reset_gate};
	for (void *p : dv)
		if (p) mi_dev_free(c, p);
	if (s->rs) mi_resampler_destroy(s->rs);
	if (s->rs_out) mi_resampler_destroy(s->rs_out);
	if (s->plc) mi_plc_destroy(s->plc);
	if (s->legs) mi_session_legs_destroy(s->legs);
	if (s->aec) mi_aec_destroy(s->aec);
	if (s->vol) mi_volume_destroy(s->vol);
	if (s->mix) mi_mixer_destroy(s->mix);
	if (s->f_mic) mi_fifo_destroy(s->f_mic);
	if (s->f_ref) mi_fifo_destroy(s->f_ref);
	if (s->f_out) mi_fifo_destroy(s->f_out);
	s->pipe.destroy();
	delete s;
}

// lp: mi_session_create_legs' plan for legs that differ (cfg then names `rate` in and out and PCM, and the rows, the resamplers,
// the codecs and the concealer are the plan's), or null: mi_session_create's session
static int build_session(mi_ctx *ctx, const mi_session_config *cfg, const SessionPlan *lp, mi_session **out) {
	MI_CHECK_ARG(ctx && cfg && out);
	*out = nullptr;
	MI_CHECK_ARG(cfg->nstreams > 0 && cfg->members_per_conference > 0 && cfg->nstreams % cfg->members_per_conference == 0);
	MI_CHECK_ARG(cfg->rate > 0 && cfg->in_rate > 0 && cfg->rate % 100 == 0 && cfg->in_rate % 100 == 0 && cfg->tail_ms > 0);
	MI_CHECK_ARG(cfg->mic_codec >= MI_SESSION_PCM16 && cfg->mic_codec <= MI_SESSION_PCMU && cfg->out_codec >= MI_SESSION_PCM16 &&
	             cfg->out_codec <= MI_SESSION_PCMU);
	MI_CHECK_ARG(cfg->out_rate >= 0 && cfg->out_rate % 100 == 0 && cfg->ref_delay_ms >= 0 && cfg->ref_delay_ms <= 1000);
	if (ctx->activate() != MI_OK) return MI_ENODEV;
	mi_session *s = new mi_session();
	s->ctx = s->pipe.ctx = ctx;
	s->cfg = *cfg;
	s->n = cfg->nstreams;
	s->in_len = cfg->in_rate / 100;
	s->len = cfg->rate / 100;
	const bool down = cfg->out_rate != 0 && cfg->out_rate != cfg->rate;
	s->out_len = (down ? cfg->out_rate : cfg->rate) / 100;
	s->mic_bytes = (size_t)s->in_len * (cfg->mic_codec ? 1 : 2);
	s->ref_bytes = cfg->ref_loopback ? 0 : (size_t)s->len * 2;
	s->out_bytes = (size_t)s->out_len * (cfg->out_codec ? 1 : 2);
	if (lp) s->plan = *lp, s->mic_bytes = lp->mic_pitch, s->out_bytes = lp->out_pitch; // byte rows at one pitch
	s->frame = mi_aec_framesize(64, cfg->rate); // speexec.c:41,171-180
	int rc = MI_OK;
	auto fail = [&](int code) {
		mi_session_destroy(s);
		return code;
	};
	if (cfg->in_rate != cfg->rate) {
		if ((rc = mi_resampler_create(ctx, s->n, (uint32_t)cfg->in_rate, (uint32_t)cfg->rate, 3, &s->rs)) != MI_OK) return fail(rc);
		s->up_stride = (mi_resampler_out_capacity(s->rs, s->in_len) + 7) & ~7;
	}
	if (down) {
		if ((rc = mi_resampler_create(ctx, s->n, (uint32_t)cfg->rate, (uint32_t)cfg->out_rate, 3, &s->rs_out)) != MI_OK) return fail(rc);
		s->down_stride = (mi_resampler_out_capacity(s->rs_out, s->len) + 7) & ~7;
	}
	if ((rc = mi_aec_create(ctx, s->n, cfg->rate, s->frame, cfg->tail_ms * cfg->rate / 1000, &s->aec)) != MI_OK) return fail(rc);
	if ((rc = mi_volume_create(ctx, s->n, cfg->rate, &s->vol)) != MI_OK) return fail(rc);
	if (cfg->agc) {
		mi_volume_params p;
		mi_volume_default_params(&p);
		p.agc_enabled = 1;
		std::vector<mi_volume_params> all((size_t)s->n, p);
		if ((rc = mi_volume_set_params(s->vol, 0, s->n, all.data())) != MI_OK) return fail(rc);
	}
	if ((rc = mi_mixer_create(ctx, s->n / cfg->members_per_conference, cfg->members_per_conference, s->len, &s->mix)) != MI_OK) return fail(rc);
	// capacities: whole frames (the canceller reads / writes the rings frame-wise, mi_aec_process_fifos), two ticks + two
	// frames, + one frame for the lead of a staggered leg (its output queue stands one frame fuller)
	const int cap = (2 * s->len + (cfg->stagger ? 3 : 2) * s->frame + s->frame - 1) / s->frame * s->frame;
	const int delay = cfg->ref_delay_ms * cfg->rate / 1000;
	const int ref_cap = (cap + delay + s->frame - 1) / s->frame * s->frame;
	if ((rc = mi_fifo_create(ctx, s->n, cap, &s->f_mic)) != MI_OK || (rc = mi_fifo_create(ctx, s->n, ref_cap, &s->f_ref)) != MI_OK ||
	    (rc = mi_fifo_create(ctx, s->n, cap, &s->f_out)) != MI_OK)
		return fail(rc);
	if ((rc = s->pipe.create(ctx, SLOTS)) != MI_OK) return fail(rc);
	const size_t n = (size_t)s->n;
	for (int i = 0; i < SLOTS; ++i) {
		s->h_mic[i] = (int16_t *)mi_host_alloc(ctx, n * s->mic_bytes);
		s->h_out[i] = (int16_t *)mi_host_alloc(ctx, n * s->out_bytes);
		s->d_mic[i] = (int16_t *)mi_dev_alloc(ctx, n * s->mic_bytes);
		s->d_out[i] = (int16_t *)mi_dev_alloc(ctx, n * s->out_bytes);
		if (!s->h_mic[i] || !s->h_out[i] || !s->d_mic[i] || !s->d_out[i]) return fail(MI_ENOMEM);
		if (!cfg->ref_loopback) {
			s->h_ref[i] = (int16_t *)mi_host_alloc(ctx, n * s->ref_bytes);
			s->d_ref[i] = (int16_t *)mi_dev_alloc(ctx, n * s->ref_bytes);
			if (!s->h_ref[i] || !s->d_ref[i]) return fail(MI_ENOMEM);
		}
		if (lp) { // what lies in a row past its leg's bytes is never written: it reads as zeros
			MI_HIP(hipMemsetAsync(s->d_out[i], 0, n * s->out_bytes, ctx->stream));
			memset(s->h_out[i], 0, n * s->out_bytes);
		}
		if (cfg->ref_loopback || down || cfg->out_codec || lp) { // the mix at `rate` is kept: next tick's reference and / or the encoder's input
			s->d_mix[i] = (int16_t *)mi_dev_alloc(ctx, n * s->len * 2);
			if (!s->d_mix[i]) return fail(MI_ENOMEM);
			MI_HIP(hipMemsetAsync(s->d_mix[i], 0, n * s->len * 2, ctx->stream));
		}
	}
	if (lp) { // the ingress writes the microphone tick at `rate` here
		const SessionLegsSizes sizes = {s->n, s->len, cfg->rate, lp->hin_stride, lp->hout_stride, lp->in_row, lp->in_scratch, lp->out_scratch,
		                                lp->used, lp->ratio.data(), lp->codec.data()};
		if ((rc = mi_session_legs_create(ctx, sizes, &s->legs)) != MI_OK) return fail(rc);
		s->up_stride = s->len;
	}
	if (s->rs || lp) s->d_up = (int16_t *)mi_dev_alloc(ctx, n * s->up_stride * 2);
	s->rounds = (s->len + s->frame - 1) / s->frame;
	if (s->rounds > MI_AEC_MAX_TICK_FRAMES) return fail(MI_ENOTSUP);
	if (!(s->d_reset_gate = (uint8_t *)mi_dev_alloc(ctx, n))) return fail(MI_ENOMEM);
	s->d_tick = (int16_t *)mi_dev_alloc(ctx, n * s->len * 2);
	if (((s->rs || lp) && !s->d_up) || !s->d_tick) return fail(MI_ENOMEM);
	if (cfg->mic_codec && !(s->d_pcm = (int16_t *)mi_dev_alloc(ctx, n * s->in_len * 2))) return fail(MI_ENOMEM);
	if (s->rs_out && !(s->d_down = (int16_t *)mi_dev_alloc(ctx, n * s->down_stride * 2))) return fail(MI_ENOMEM);
	if (cfg->plc) {
		if (lp) { // at every leg's own rate behind its own decoder, into PCM rows of pcm_pitch samples
			std::vector<uint8_t> kind(n);
			for (size_t i = 0; i < n; ++i) kind[i] = lp->codec[i] & 3;
			if ((rc = mi_plc_create_legs(ctx, s->n, lp->rate.data(), kind.data(), lp->pcm_pitch, &s->plc)) != MI_OK) return fail(rc);
			if (!(s->d_pcm = (int16_t *)mi_dev_alloc(ctx, n * lp->pcm_pitch * 2))) return fail(MI_ENOMEM);
			MI_HIP(hipMemsetAsync(s->d_pcm, 0, n * lp->pcm_pitch * 2, ctx->stream));
		} else {
			if ((rc = mi_plc_create(ctx, s->n, cfg->in_rate, s->in_len, &s->plc)) != MI_OK) return fail(rc);
			std::vector<int32_t> lens(n, s->in_len);
			if (!(s->d_evlen = (int32_t *)mi_dev_alloc(ctx, n * 4))) return fail(MI_ENOMEM);
			MI_HIP(hipMemcpy(s->d_evlen, lens.data(), n * 4, hipMemcpyHostToDevice));
		}
		for (int i = 0; i < SLOTS; ++i) {
			s->h_ev[i] = (uint8_t *)mi_host_alloc(ctx, n);
			s->d_ev[i] = (uint8_t *)mi_dev_alloc(ctx, n);
			if (!s->h_ev[i] || !s->d_ev[i]) return fail(MI_ENOMEM);
		}
	}
	if (delay > 0) { // speexec.c:205-208: delay_ms of silence ahead of the reference
		if (!(s->d_zero = (int16_t *)mi_dev_alloc(ctx, n * (size_t)delay * 2))) return fail(MI_ENOMEM);
		MI_HIP(hipMemsetAsync(s->d_zero, 0, n * (size_t)delay * 2, ctx->stream));
		if ((rc = mi_fifo_push(s->f_ref, s->d_zero, delay, delay, nullptr)) != MI_OK) return fail(rc);
	}
	if (cfg->stagger && (rc = mi_aec_stagger_fifos(s->aec, s->f_mic, s->f_ref, s->len, 0, s->n)) != MI_OK) return fail(rc);
	if (cfg->stagger && (rc = mi_aec_stagger_info(s->aec, s->len, &s->lead_unit, &s->lead_phases)) != MI_OK) return fail(rc);
	// (no initial parameters: the session's meters have no setter, so its controls carry no MI_CTL_VOLUME)
	if ((rc = s->conf.create(ctx, s->n, cfg->members_per_conference, SLOTS, nullptr, s->vol, s->mix, s->plc)) != MI_OK) return fail(rc);
	MI_HIP(hipStreamSynchronize(ctx->stream));
	*out = s;
	return MI_OK;
}

int mi_session_create(mi_ctx *ctx, const mi_session_config *cfg, mi_session **out) { return build_session(ctx, cfg, nullptr, out); }

int mi_legs_session_create(mi_ctx *ctx, const mi_session_config *cfg, const mi_session_leg *h_legs, mi_session **out) {
	if (!h_legs) return mi_session_create(ctx, cfg, out);
	MI_CHECK_ARG(cfg && out);
	*out = nullptr;
	SessionPlan plan; // every refusal comes from here, before the device is asked for anything
	int rc = plan_session_legs(cfg, h_legs, &plan);
	if (rc != MI_OK) return rc;
	MI_CHECK_ARG(ctx != nullptr);
	if (plan.uniform) rc = build_session(ctx, &plan.cfg, nullptr, out);
	else { // the canceller's side of the session: `rate` in and out, 16-bit PCM; the legs' side is the plan's
		mi_session_config c = *cfg;
		c.in_rate = c.rate, c.out_rate = 0, c.mic_codec = c.out_codec = MI_SESSION_PCM16;
		rc = build_session(ctx, &c, &plan, out);
	}
	if (rc == MI_OK) (*out)->kinds.assign(h_legs, h_legs + cfg->nstreams);
	return rc;
}

// a leg's kind: as mi_session_create_legs was given it, else the one kind of mi_session_create's configuration (its in_rate)
static mi_session_leg leg_kind(const mi_session *s, int stream) {
	if (!s->kinds.empty()) return s->kinds[(size_t)stream];
	return {s->cfg.in_rate, s->cfg.mic_codec, s->cfg.out_codec};
}

int mi_legs_session_rate(const mi_session *s, int stream) {
	if (!s || stream < 0 || stream >= s->n) return mi::set_error("mi_session_leg_rate: %s", s ? "stream out of range" : "a null session"), (int)MI_EINVAL;
	return leg_kind(s, stream).rate;
}

int mi_legs_session_codec(const mi_session *s, int stream, int *mic_codec, int *out_codec) {
	if (!s || stream < 0 || stream >= s->n) return mi::set_error("mi_session_leg_codec: %s", s ? "stream out of range" : "a null session"), (int)MI_EINVAL;
	const mi_session_leg k = leg_kind(s, stream);
	if (mic_codec) *mic_codec = k.mic_codec;
	if (out_codec) *out_codec = k.out_codec;
	return MI_OK;
}

int mi_legs_session_bytes(const mi_session *s, int stream, int *mic_bytes, int *out_bytes) {
	if (!s || stream < 0 || stream >= s->n) return mi::set_error("mi_session_leg_bytes: %s", s ? "stream out of range" : "a null session"), (int)MI_EINVAL;
	if (mic_bytes) *mic_bytes = s->legs ? s->plan.mic_bytes(stream) : (int)s->mic_bytes;
	if (out_bytes) *out_bytes = s->legs ? s->plan.out_bytes(stream) : (int)s->out_bytes;
	return MI_OK;
}

int mi_session_tick_samples(const mi_session *s, int *in_samples, int *out_samples) {
	MI_CHECK_ARG(s != nullptr);
	if (in_samples) *in_samples = s->in_len;
	if (out_samples) *out_samples = s->len;
	return MI_OK;
}

int mi_session_tick_bytes(const mi_session *s, int *mic_bytes, int *ref_bytes, int *out_bytes) {
	MI_CHECK_ARG(s != nullptr);
	if (mic_bytes) *mic_bytes = (int)s->mic_bytes;
	if (ref_bytes) *ref_bytes = (int)s->ref_bytes;
	if (out_bytes) *out_bytes = (int)s->out_bytes;
	return MI_OK;
}

int mi_session_acquire(mi_session *s, int16_t **h_mic, int16_t **h_ref) {
	MI_CHECK_ARG(s && h_mic && h_ref);
	int slot;
	// the slot's previous upload must have been consumed by its kernels before the host overwrites the staging
	const int rc = s->pipe.acquire(mi::TickPipe::CONSUMED, &slot);
	if (rc == mi::TickPipe::FULL) mi::set_error("all %d ticks in flight: collect one first", SLOTS);
	if (rc != MI_OK) return rc;
	*h_mic = s->h_mic[slot];
	*h_ref = s->h_ref[slot];
	if (s->plc) memset(s->h_ev[slot], MI_PLC_RECEIVED, (size_t)s->n);
	return MI_OK;
}

int mi_session_events(mi_session *s, uint8_t **h_events) {
	MI_CHECK_ARG(s && h_events);
	if (!s->plc || !s->pipe.acquired) {
		mi::set_error(s->plc ? "mi_session_events outside acquire .. submit" : "the session was created without plc");
		return MI_EINVAL;
	}
	*h_events = s->h_ev[s->pipe.next_slot()];
	return MI_OK;
}

int mi_session_submit(mi_session *s) {
	MI_CHECK_ARG(s != nullptr);
	if (!s->pipe.acquired) {
		mi::set_error("mi_session_submit without mi_session_acquire");
		return MI_EINVAL;
	}
	mi_ctx *c = s->ctx;
	const size_t n = (size_t)s->n;
	s->conf.stage(s->pipe.next_slot(), s->pipe.submitted);
	const int rc = s->pipe.submit(
	    [&](int slot) {
		    if (s->conf.upload(slot, s->pipe.s_up) != MI_OK) return (int)MI_ENODEV;
		    MI_HIP(hipMemcpyAsync(s->d_mic[slot], s->h_mic[slot], n * s->mic_bytes, hipMemcpyHostToDevice, s->pipe.s_up));
		    if (s->ref_bytes) MI_HIP(hipMemcpyAsync(s->d_ref[slot], s->h_ref[slot], n * s->ref_bytes, hipMemcpyHostToDevice, s->pipe.s_up));
		    if (s->plc) MI_HIP(hipMemcpyAsync(s->d_ev[slot], s->h_ev[slot], n, hipMemcpyHostToDevice, s->pipe.s_up));
		    return MI_OK;
	    },
	    [&](int slot) {
		    int rc = s->conf.apply(slot, [&](const mi_seat_cmd *d_cmd, int count) { return launch_seats(s, slot, d_cmd, count); });
		    if (rc != MI_OK) return rc;
		    // the report's launch follows the tick's kernels -- behind the slot's graph, never inside it
		    // (legs that differ with plc: the per-leg concealer's launches are not captured -- the tick is launched directly)
		    if (!s->cfg.use_graphs || (s->legs && s->plc)) return (rc = run_tick_kernels(s, slot)) != MI_OK ? rc : s->conf.report(slot);
		    if (!s->graph[slot]) {
			    // first use of the slot: run eagerly once is not an option (state would advance twice), so capture directly
			    if ((rc = mi_ctx_capture_begin(c)) != MI_OK) return rc;
			    rc = run_tick_kernels(s, slot);
			    mi_graph *g = nullptr;
			    const int rc2 = mi_ctx_capture_end(c, &g);
			    if (rc != MI_OK) return rc;
			    if (rc2 != MI_OK) return rc2;
			    s->graph[slot] = g;
		    }
		    return (rc = mi_graph_launch(s->graph[slot])) != MI_OK ? rc : s->conf.report(slot);
	    },
	    [&](int slot) {
		    MI_HIP(hipMemcpyAsync(s->h_out[slot], s->d_out[slot], n * s->out_bytes, hipMemcpyDeviceToHost, s->pipe.s_down));
		    return s->conf.download(slot, s->pipe.s_down);
	    });
	if (rc == MI_OK) s->conf.submitted();
	return rc;
}

int mi_session_collect(mi_session *s, const int16_t **h_out) {
	MI_CHECK_ARG(s && h_out);
	int slot;
	const int rc = s->pipe.collect(&slot);
	if (rc == mi::TickPipe::EMPTY) mi::set_error("nothing in flight");
	if (rc != MI_OK) return rc;
	*h_out = s->h_out[slot];
	return MI_OK;
}

int mi_session_in_flight(const mi_session *s) { return s ? s->pipe.in_flight() : 0; }

// ---- conference control plane: every call's body is mi::ConferencePlane's (controls.hpp), the session brings what is its own
int mi_session_set_controls(mi_session *s, const uint8_t *h_flags, const float *h_gain) {
	MI_CHECK_ARG(s && (h_flags || h_gain));
	return s->conf.set_controls(h_flags, h_gain);
}

int mi_session_add_member(mi_session *s, int stream) {
	MI_CHECK_ARG(s && stream >= 0 && stream < s->n);
	return s->conf.add_member("mi_session_add_member", stream, [&](int seat) { return mi_session_reset_streams(s, seat, 1); });
}

// (what the departed leg last heard: its output rows and, where the mix at `rate` is kept, its rows there)
int mi_session_remove_member(mi_session *s, int stream) {
	MI_CHECK_ARG(s && stream >= 0 && stream < s->n);
	return s->conf.remove_member("mi_session_remove_member", stream, s->pipe, [&](int seat) -> int {
		for (int i = 0; i < SLOTS; ++i) {
			if (s->d_out[i]) MI_HIP(hipMemsetAsync((uint8_t *)s->d_out[i] + (size_t)seat * s->out_bytes, 0, s->out_bytes, s->ctx->stream));
			if (s->d_mix[i]) MI_HIP(hipMemsetAsync(s->d_mix[i] + (size_t)seat * s->len, 0, (size_t)s->len * 2, s->ctx->stream));
			if (s->h_out[i]) memset((uint8_t *)s->h_out[i] + (size_t)seat * s->out_bytes, 0, s->out_bytes);
		}
		return MI_OK;
	});
}

// no stream, event or device synchronise, no blocking copy and no allocation on these two paths: the book answers at once, the
// device follows with the next tick submitted (mi::ConferenceBook; mi::ConferencePlane::stage, ::apply)
int mi_session_change_members(mi_session *s, const mi_session_change *h_changes, int count) {
	static_assert(MI_SESSION_JOIN == MI_SEAT_JOIN && MI_SESSION_LEAVE == MI_SEAT_LEAVE, "the public ops are the command's");
	const char *fn = "mi_session_change_members";
	if (!s) return mi::set_error("%s: a null session", fn), (int)MI_EINVAL;
	const char *names = "MI_SESSION_JOIN (1) or MI_SESSION_LEAVE (2)";
	if (!s->legs) return s->conf.book.change_uniform_members(fn, names, h_changes, count, s->in_len);
	// legs that differ: a JOIN re-seats the seat's own kind -- its tick's length, its class and decoder in the concealer
	mi::ConferenceBook &book = s->conf.book;
	const int rc = mi::check_uniform_changes(fn, names, book.n(), book.roster.flags.data(), h_changes, count, &book.controls.scratch);
	for (int i = 0; rc == MI_OK && i < count; ++i) {
		const mi_session_change &c = h_changes[i];
		mi::SeatChanges::Pending &p = book.change_member(c.stream, (uint8_t)c.op);
		if (c.op != MI_SEAT_JOIN) continue;
		const mi_session_leg &k = s->kinds[(size_t)c.stream];
		p.len = k.rate / 100, p.codec = s->plan.codec[(size_t)c.stream], p.ratio = s->plan.ratio[(size_t)c.stream];
		if (s->plc) p.cls = (uint8_t)std::max(0, mi_plc_class_of(s->plc, c.stream, k.rate)), mi_plc_seat(s->plc, c.stream, p.cls, k.mic_codec);
	}
	return rc;
}

int mi_session_change_controls(mi_session *s, const mi_session_control *h_changes, int count) {
	const char *fn = "mi_session_change_controls";
	if (!s) return mi::set_error("%s: a null session", fn), (int)MI_EINVAL;
	return s->conf.book.change_controls(fn, h_changes, count);
}

int mi_session_set_reports(mi_session *s, uint32_t what) {
	if (!s) return mi::set_error("mi_session_set_reports: a null session"), (int)MI_EINVAL;
	return s->conf.set_reports("mi_session_set_reports", what);
}

int mi_session_collected_report(mi_session *s, mi_session_report *out) {
	if (!s || !out) return mi::set_error("mi_session_collected_report: a null %s", s ? "report" : "session"), (int)MI_EINVAL;
	return s->conf.collected("mi_session_collected_report", s->pipe.collected, out);
}

int mi_session_member_count(const mi_session *s, int conference) { return s ? s->conf.book.member_count(conference) : (int)MI_EINVAL; }

// ms_audio_conference_process_events' election in mixer mode (:436-452, mi::Roster::elect).  now_ms: the caller's clock; not
// read (mi::active_speakers).  A seat that has joined since the last submit reads as a fresh meter
int mi_session_active_speakers(mi_session *s, uint64_t now_ms, int32_t *h_winner, float *h_max_db) {
	MI_CHECK_ARG(s && h_winner);
	(void)now_ms;
	const std::vector<int32_t> fresh = s->conf.book.joining();
	return mi::active_speakers(s->vol, s->conf.book.roster, h_winner, h_max_db, &fresh);
}

// A call leg leaves and another takes its place: every per-stream state of the chain goes back to its initial value
// (what destroying and re-creating the leg's filters does in the reference), the other streams are not touched.
int mi_session_reset_streams(mi_session *s, int first, int count) {
	MI_CHECK_ARG(s && first >= 0 && count >= 0 && first + count <= s->n);
	if (count == 0) return MI_OK;
	int rc;
	if (s->ctx->activate() != MI_OK) return MI_ENODEV;
	if (s->rs && (rc = mi_resampler_reset(s->rs, first, count)) != MI_OK) return rc;
	if ((rc = mi_aec_reset(s->aec, first, count)) != MI_OK) return rc;
	if ((rc = mi::reset_meters(s->vol, first, count)) != MI_OK) return rc;
	if ((rc = mi_fifo_reset_range(s->f_mic, first, count)) != MI_OK || (rc = mi_fifo_reset_range(s->f_ref, first, count)) != MI_OK ||
	    (rc = mi_fifo_reset_range(s->f_out, first, count)) != MI_OK)
		return rc;
	if (s->rs_out && (rc = mi_resampler_reset(s->rs_out, first, count)) != MI_OK) return rc;
	if (s->legs && (rc = mi_session_legs_reset(s->legs, first, count)) != MI_OK) return rc;
	if (s->plc && (rc = mi_plc_reset(s->plc, first, count)) != MI_OK) return rc;
	if (s->cfg.ref_loopback) // the new leg was not sent anything yet
		for (int i = 0; i < SLOTS; ++i)
			MI_HIP(hipMemsetAsync(s->d_mix[i] + (size_t)first * s->len, 0, (size_t)count * s->len * 2, s->ctx->stream));
	if (s->d_zero) { // its reference FIFO starts with the configured delay again
		const int delay = s->cfg.ref_delay_ms * s->cfg.rate / 1000;
		std::vector<uint8_t> gate((size_t)s->n, 0);
		for (int i = 0; i < count; ++i) gate[(size_t)(first + i)] = 1;
		MI_HIP(hipMemcpyAsync(s->d_reset_gate, gate.data(), (size_t)s->n, hipMemcpyHostToDevice, s->ctx->stream));
		if ((rc = mi_fifo_push_gated(s->f_ref, s->d_zero, delay, delay, s->d_reset_gate)) != MI_OK) return rc;
		MI_HIP(hipStreamSynchronize(s->ctx->stream)); // gate is a stack-lifetime buffer
	}
	if (s->cfg.stagger && (rc = mi_aec_stagger_fifos(s->aec, s->f_mic, s->f_ref, s->len, first, count)) != MI_OK) return rc;
	return MI_OK;
}

int mi_session_get_levels(mi_session *s, float *h_linear) {
	MI_CHECK_ARG(s && h_linear);
	const std::vector<int32_t> fresh = s->conf.book.joining();
	return mi::get_levels(s->vol, s->n, h_linear, &fresh);
}

} // extern "C"
