// controls.hpp -- mi::ConferencePlane, the one object under mi_bridge (bridge.hip) and mi_session (session.hip) through which a
// running batch of conferences is steered and observed, and ahead of it what controls.hip's two kernels are handed: a tick's
// control changes with the arrays they are written to, and the arrays a tick leaves behind with their report block.
#pragma once
#include <cmath>

#include "common.hpp"
#include "conference_book.hpp"
#include "tick_pipe.hpp"

// the pins' gains and the meters' parameters as the waiting setters write them (mi_mixer_set_controls, mi_volume_set_params)
float *mi_mixer_gain_edit(mi_mixer *m);
mi_volume_params *mi_volume_params_edit(mi_volume *v);

struct ControlArgs {
	const mi_ctl_cmd *cmd; // [count]
	int count, nstreams;
	uint8_t *flags;           // [nstreams] the pins' MI_MIX_*
	float *gain;              // [nstreams] the pins' input gains
	mi_volume_params *params; // [nstreams], or null: the object takes no MI_CTL_VOLUME
	uint32_t *joined;         // [nstreams] the joining order the report kernel's election reads
};
// controls_kernel, one lane per command, on `stream`
int mi_controls_launch(const ControlArgs &args, hipStream_t stream);

#define MI_REPORT_SPEAKERS 1u
#define MI_REPORT_LEVELS 2u
struct ReportArgs {
	const mi_volume_state *state; // [nstreams] .energy: MS_VOLUME_GET_LINEAR
	const float2 *win;            // [nstreams] the one-second maximum windows (VolumeView::win)
	const uint8_t *flags;         // [nstreams]
	const uint32_t *joined;       // [nstreams]
	int nconf, mm;
	unsigned what; // MI_REPORT_*
	float thr;     // mi::report_threshold()
	float *levels;    // [nstreams]  (LEVELS)
	int32_t *winner;  // [nconf]     (SPEAKERS)
	float *max_lin;   // [nconf]     (SPEAKERS)
};
// the block's layout in a slot's buffer, device and pinned alike: levels, then winner, then max_lin
inline size_t report_bytes(int nstreams, int nconf) { return ((size_t)nstreams + 2 * (size_t)nconf) * 4; }
constexpr int REPORT_MAX_MEMBERS = 64; // a conference is one wavefront
// report_kernel, one wavefront per conference, on `stream`
int mi_report_launch(const ReportArgs &args, hipStream_t stream);

namespace mi {

// Owned once, held by both: the book (conference_book.hpp), per pipe slot both pinned command rows (seats, controls) with their
// device copies and lengths, the joining order on the device, and -- from the first mi_*_set_reports on -- per slot the report
// block, on the device and pinned.  The meters, the pins and the concealer are the owner's, borrowed.  What differs between the
// owners comes in as callables, as with mi::TickPipe.  The owner calls stage / upload / apply / report / download from the
// matching places of its submit, `submitted` behind it, and the rest from its entry points of the same names.
struct ConferencePlane {
	static constexpr int MAX_SLOTS = 8;
	ConferenceBook book;
	mi_ctx *ctx = nullptr;
	mi_volume *vol = nullptr;
	mi_mixer *mix = nullptr;
	mi_plc *plc = nullptr; // or null: no concealer
	int n = 0, nconf = 0, mm = 0, slots = 0;
	mi_seat_cmd *h_seat[MAX_SLOTS] = {}, *d_seat[MAX_SLOTS] = {};
	mi_ctl_cmd *h_ctl[MAX_SLOTS] = {}, *d_ctl[MAX_SLOTS] = {};
	int nseat[MAX_SLOTS] = {}, nctl[MAX_SLOTS] = {};
	uint32_t *d_joined = nullptr;
	unsigned rep_what[MAX_SLOTS] = {}; // MI_REPORT_* of the tick that last ran in the slot (book.reports: of the ticks to come),
	long long rep_seq[MAX_SLOTS] = {};  // and which tick that was
	uint8_t *h_rep[MAX_SLOTS] = {}, *d_rep[MAX_SLOTS] = {};
	std::vector<float> max_db; // [nconf] worked out by `collected`
	float thr = 0;

	int create(mi_ctx *c, int nstreams, int members, int pipe_slots, const mi_volume_params *initial, mi_volume *v, mi_mixer *m, mi_plc *p) {
		ctx = c, vol = v, mix = m, plc = p;
		n = nstreams, mm = members, nconf = n / mm, slots = pipe_slots;
		book.init(n, mm, slots, initial);
		max_db.assign((size_t)nconf, 0.f);
		thr = report_threshold();
		for (int i = 0; i < slots; ++i) { // every seat may change in one tick
			h_seat[i] = (mi_seat_cmd *)mi_host_alloc(c, (size_t)n * sizeof(mi_seat_cmd)), d_seat[i] = (mi_seat_cmd *)mi_dev_alloc(c, (size_t)n * sizeof(mi_seat_cmd));
			h_ctl[i] = (mi_ctl_cmd *)mi_host_alloc(c, (size_t)n * sizeof(mi_ctl_cmd)), d_ctl[i] = (mi_ctl_cmd *)mi_dev_alloc(c, (size_t)n * sizeof(mi_ctl_cmd));
			if (!h_seat[i] || !d_seat[i] || !h_ctl[i] || !d_ctl[i]) return MI_ENOMEM;
		}
		if (!(d_joined = (uint32_t *)mi_dev_alloc(c, (size_t)n * 4))) return MI_ENOMEM;
		MI_HIP(hipMemcpy(d_joined, book.roster.joined.data(), (size_t)n * 4, hipMemcpyHostToDevice));
		return MI_OK;
	}

	void destroy() {
		for (int i = 0; i < slots; ++i) {
			for (void *p : {(void *)h_seat[i], (void *)h_ctl[i], (void *)h_rep[i]})
				if (p) mi_host_free(ctx, p);
			for (void *p : {(void *)d_seat[i], (void *)d_ctl[i], (void *)d_rep[i]})
				if (p) mi_dev_free(ctx, p);
		}
		if (d_joined) mi_dev_free(ctx, d_joined);
	}

	// before the pipe's submit: both rows of the tick about to go (acquire has waited for the slot's last use)
	void stage(int slot, long long seq) {
		book.stage(h_seat[slot], h_ctl[slot], &nseat[slot], &nctl[slot]);
		rep_what[slot] = book.reports, rep_seq[slot] = seq;
	}
	int upload(int slot, hipStream_t s_up) {
		if (nseat[slot]) MI_HIP(hipMemcpyAsync(d_seat[slot], h_seat[slot], (size_t)nseat[slot] * sizeof(mi_seat_cmd), hipMemcpyHostToDevice, s_up));
		if (nctl[slot]) MI_HIP(hipMemcpyAsync(d_ctl[slot], h_ctl[slot], (size_t)nctl[slot] * sizeof(mi_ctl_cmd), hipMemcpyHostToDevice, s_up));
		return MI_OK;
	}
	// first thing in the pipe's kernels(slot): behind the wait for the download that last read this slot's output rows -- only
	// there is zeroing a row free of a race with it -- and ahead of the tick's kernels or the slot's graph, never inside it.  The
	// order is fixed here: membership (seat_launch(d_cmd, count): the owner's roster kernel; the concealer's), then the controls
	template <class SeatLaunch>
	int apply(int slot, SeatLaunch &&seat_launch) {
		int rc;
		if (nseat[slot]) {
			if ((rc = seat_launch(d_seat[slot], nseat[slot])) != MI_OK) return rc;
			if (plc && (rc = mi_plc_apply_seats(plc, d_seat[slot], nseat[slot])) != MI_OK) return rc;
		}
		if (!nctl[slot]) return MI_OK;
		ControlArgs a = {};
		MixerEdit me;
		mi_mixer_edit(mix, &me);
		a.cmd = d_ctl[slot], a.count = nctl[slot], a.nstreams = n;
		a.flags = me.flags, a.gain = mi_mixer_gain_edit(mix), a.joined = d_joined;
		a.params = (book.allowed & MI_CTL_VOLUME) ? mi_volume_params_edit(vol) : nullptr;
		return mi_controls_launch(a, ctx->stream);
	}
	// behind the tick's kernels, and behind the slot's graph where there is one
	int report(int slot) {
		if (!rep_what[slot]) return MI_OK;
		ReportArgs a = {};
		VolumeView vv;
		MixerView mv;
		mi_volume_view(vol, &vv);
		mi_mixer_view(mix, &mv);
		a.state = vv.state, a.win = vv.win, a.flags = mv.flags, a.joined = d_joined;
		a.nconf = nconf, a.mm = mm, a.what = rep_what[slot], a.thr = thr;
		a.levels = reinterpret_cast<float *>(d_rep[slot]);
		a.winner = reinterpret_cast<int32_t *>(d_rep[slot]) + n, a.max_lin = a.levels + n + nconf;
		return mi_report_launch(a, ctx->stream);
	}
	// with the tick's output, behind the same event
	int download(int slot, hipStream_t s_down) {
		if (rep_what[slot]) MI_HIP(hipMemcpyAsync(h_rep[slot], d_rep[slot], report_bytes(n, nconf), hipMemcpyDeviceToHost, s_down));
		return MI_OK;
	}
	void submitted() { book.submitted(); }

	// ---- the waiting calls (what MSAudioConference drives through the mixer's methods, src/voip/audioconference.c: mute =
	// MS_AUDIO_MIXER_SET_ACTIVE 0, listen-only = MS_AUDIO_MIXER_ENABLE_OUTPUT ..., per-member input gain): the mixer's setter
	// waits for the ticks submitted.  `stream` has been checked by the owner
	int set_controls(const uint8_t *h_flags, const float *h_gain) {
		book.set_controls(h_flags, h_gain);
		return mi_mixer_set_controls(mix, h_flags, h_gain); // [nconf][members] == [nstreams]
	}
	// ms_audio_conference_add_member (:322-345): a NEW endpoint joins -- its own filters are fresh (reset(stream): the owner's
	// mi_*_reset_streams), its mixer pin becomes linked / active / output enabled.  The other members' filters keep their state
	// (the graph is detached and re-attached around this, :325-327; their MSFilter objects survive)
	template <class Reset>
	int add_member(const char *fn, int stream, Reset &&reset) {
		int rc;
		if (book.roster.is_member(stream)) return book.add_member(fn, stream); // refused before anything is reset
		if ((rc = reset(stream)) != MI_OK || (rc = book.add_member(fn, stream)) != MI_OK) return rc;
		if (book.reports) MI_HIP(hipMemcpy(d_joined + stream, &book.roster.joined[(size_t)stream], 4, hipMemcpyHostToDevice));
		return mi_mixer_set_controls(mix, book.roster.flags.data(), nullptr);
	}
	// ms_audio_conference_remove_member (:366-374): the pin is unplumbed and the mixer leaves its row alone from now on: what the
	// departed leg last heard must not linger.  clear(stream): the owner zeroes the seat's rows of every slot behind the waits here
	template <class Clear>
	int remove_member(const char *fn, int stream, const TickPipe &pipe, Clear &&clear) {
		int rc = book.remove_member(fn, stream);
		if (rc != MI_OK || (rc = mi_mixer_set_controls(mix, book.roster.flags.data(), nullptr)) != MI_OK) return rc;
		if (ctx->activate() != MI_OK) return MI_ENODEV;
		MI_HIP(hipStreamSynchronize(ctx->stream));
		if (pipe.s_down) MI_HIP(hipStreamSynchronize(pipe.s_down));
		return clear(stream);
	}

	// mi_*_set_reports: a configuration call -- the only one here that allocates or waits.  The joining order goes up whole:
	// while reports are off no tick carries it
	int set_reports(const char *fn, unsigned what) {
		if (what & ~(MI_REPORT_SPEAKERS | MI_REPORT_LEVELS)) return set_error("%s: what 0x%x; MI_REPORT_SPEAKERS | MI_REPORT_LEVELS or 0", fn, what), (int)MI_EINVAL;
		if (what && mm > REPORT_MAX_MEMBERS) return set_error("%s: %d members per conference; the report kernel seats %d", fn, mm, REPORT_MAX_MEMBERS), (int)MI_ENOTSUP;
		if (what) {
			if (ctx->activate() != MI_OK) return MI_ENODEV;
			for (int i = 0; i < slots; ++i) {
				if (!h_rep[i]) h_rep[i] = (uint8_t *)mi_host_alloc(ctx, report_bytes(n, nconf));
				if (!d_rep[i]) d_rep[i] = (uint8_t *)mi_dev_alloc(ctx, report_bytes(n, nconf));
				if (!h_rep[i] || !d_rep[i]) return MI_ENOMEM;
			}
			MI_HIP(hipStreamSynchronize(ctx->stream)); // a report in flight reads the order it was submitted with
			MI_HIP(hipMemcpy(d_joined, book.roster.joined.data(), (size_t)n * 4, hipMemcpyHostToDevice));
		}
		book.reports = what;
		return MI_OK;
	}

	// mi_*_collected_report: the block of the tick last collected (`ncollected` ticks so far) into the owner's public record
	// (the same fields in both).  max_db: the waiting election's expression (elect_active_speakers) on the winner's maximum
	template <class Report>
	int collected(const char *fn, long long ncollected, Report *out) {
		out->nstreams = n, out->nconf = nconf;
		if (ncollected <= 0) return set_error("%s: no tick has been collected", fn), (int)MI_EINVAL;
		const int slot = (int)((ncollected - 1) % slots);
		if (rep_seq[slot] != ncollected - 1) return set_error("%s: tick %lld's slot has been submitted again", fn, ncollected - 1), (int)MI_EINVAL;
		if (!rep_what[slot]) return set_error("%s: reports were off for tick %lld", fn, ncollected - 1), (int)MI_EINVAL;
		const float *lv = reinterpret_cast<const float *>(h_rep[slot]);
		const bool speakers = (rep_what[slot] & MI_REPORT_SPEAKERS) != 0;
		out->seq = (uint64_t)(ncollected - 1), out->what = rep_what[slot];
		out->levels = (rep_what[slot] & MI_REPORT_LEVELS) ? lv : nullptr;
		out->winner = speakers ? reinterpret_cast<const int32_t *>(h_rep[slot]) + n : nullptr;
		out->max_lin = speakers ? lv + n + nconf : nullptr;
		out->max_db = speakers ? max_db.data() : nullptr;
		for (int c = 0; speakers && c < nconf; ++c) {
			const float lin = out->max_lin[c];
			max_db[(size_t)c] = lin == 0 ? -120.f : 10 * log10f(lin);
		}
		return MI_OK;
	}
};

} // namespace mi
