// controls.hpp -- what controls.hip's two kernels are handed by bridge.hip and session.hip: a tick's control changes with the
// arrays they are written to, and the arrays a tick leaves behind with the report block they are read into.
#pragma once
#include <cmath>

#include "common.hpp"
#include "conference.hpp"
#include "control_changes.hpp"

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

// What mi_bridge and mi_session each own of this, the same in both: the bookkeeping (control_changes.hpp), per pipe slot the
// pinned command row, its device copy and its length, the joining order on the device, and -- from the first mi_*_set_reports
// on -- per slot the report block, on the device and pinned.  The owner calls stage / upload / apply / report / download from
// the matching places of its submit, `collected` from its read-out.
struct ControlPlane {
	static constexpr int MAX_SLOTS = 8;
	mi_ctx *ctx = nullptr;
	int n = 0, nconf = 0, mm = 0, slots = 0;
	ControlChanges changes;
	mi_ctl_cmd *h_cmd[MAX_SLOTS] = {}, *d_cmd[MAX_SLOTS] = {};
	int ncmd[MAX_SLOTS] = {};
	uint32_t *d_joined = nullptr;
	unsigned reports = 0;              // MI_REPORT_* of the ticks to come
	unsigned rep_what[MAX_SLOTS] = {}; // ... of the tick that last ran in the slot,
	long long rep_seq[MAX_SLOTS] = {};  // and which tick that was
	uint8_t *h_rep[MAX_SLOTS] = {}, *d_rep[MAX_SLOTS] = {};
	std::vector<float> max_db; // [nconf] worked out by `collected`
	float thr = 0;

	int create(mi_ctx *c, const Roster &r, int pipe_slots, const mi_volume_params *initial) {
		ctx = c, n = (int)r.flags.size(), nconf = r.nconf, mm = r.mm, slots = pipe_slots;
		changes.init(n, initial);
		max_db.assign((size_t)nconf, 0.f);
		thr = report_threshold();
		for (int i = 0; i < slots; ++i) { // every seat may change in one tick
			h_cmd[i] = (mi_ctl_cmd *)mi_host_alloc(c, (size_t)n * sizeof(mi_ctl_cmd)), d_cmd[i] = (mi_ctl_cmd *)mi_dev_alloc(c, (size_t)n * sizeof(mi_ctl_cmd));
			if (!h_cmd[i] || !d_cmd[i]) return MI_ENOMEM;
		}
		if (!(d_joined = (uint32_t *)mi_dev_alloc(c, (size_t)n * 4))) return MI_ENOMEM;
		MI_HIP(hipMemcpy(d_joined, r.joined.data(), (size_t)n * 4, hipMemcpyHostToDevice));
		return MI_OK;
	}

	void destroy() {
		for (int i = 0; i < slots; ++i) {
			if (h_cmd[i]) mi_host_free(ctx, h_cmd[i]);
			if (d_cmd[i]) mi_dev_free(ctx, d_cmd[i]);
			if (h_rep[i]) mi_host_free(ctx, h_rep[i]);
			if (d_rep[i]) mi_dev_free(ctx, d_rep[i]);
		}
		if (d_joined) mi_dev_free(ctx, d_joined);
	}

	// mi_*_set_reports: a configuration call -- the only one here that allocates or waits.  The joining order goes up whole:
	// while reports are off no tick carries it
	int set_reports(const char *fn, unsigned what, const Roster &r) {
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
			MI_HIP(hipMemcpy(d_joined, r.joined.data(), (size_t)n * 4, hipMemcpyHostToDevice));
		}
		reports = what;
		return MI_OK;
	}

	// the waiting mi_*_add_member has appended `stream` to its conference's list (behind its own waits)
	int joined_waiting(int stream, const Roster &r) {
		if (!reports) return MI_OK;
		MI_HIP(hipMemcpy(d_joined + stream, &r.joined[(size_t)stream], 4, hipMemcpyHostToDevice));
		return MI_OK;
	}

	// submit, before the pipe's: the row of the tick about to go.  seats: the membership changes it carries -- with reports on,
	// every JOIN's place in the joining order rides along
	void stage(int slot, long long seq, const Roster &r, const SeatChanges &seats) {
		if (reports)
			for (const int32_t s : seats.changed)
				if (seats.pending[(size_t)s].op & MI_SEAT_JOIN) changes.note(s, MI_CTL_JOINED);
		ncmd[slot] = changes.stage(h_cmd[slot], r.flags.data(), r.joined.data());
		rep_what[slot] = reports, rep_seq[slot] = seq;
	}
	int upload(int slot, hipStream_t s_up) {
		if (ncmd[slot]) MI_HIP(hipMemcpyAsync(d_cmd[slot], h_cmd[slot], (size_t)ncmd[slot] * sizeof(mi_ctl_cmd), hipMemcpyHostToDevice, s_up));
		return MI_OK;
	}
	// ahead of the tick's kernels, behind the membership kernel
	int apply(int slot, mi_mixer *mix, mi_volume *vol, bool with_params) {
		if (!ncmd[slot]) return MI_OK;
		ControlArgs a = {};
		MixerEdit me;
		mi_mixer_edit(mix, &me);
		a.cmd = d_cmd[slot], a.count = ncmd[slot], a.nstreams = n;
		a.flags = me.flags, a.gain = mi_mixer_gain_edit(mix), a.params = with_params ? mi_volume_params_edit(vol) : nullptr, a.joined = d_joined;
		return mi_controls_launch(a, ctx->stream);
	}
	// behind the tick's kernels
	int report(int slot, mi_mixer *mix, mi_volume *vol) {
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
	void submitted() { changes.submitted(); }

	// mi_*_collected_report: the block of the tick last collected (`collected` ticks so far, `depth` slots).  max_db: the
	// expression of the waiting election (conference.hpp, elect_active_speakers), on the winner's linear maximum
	int collected(const char *fn, long long ncollected, uint64_t *seq, unsigned *what, const float **levels, const int32_t **winner,
	              const float **max_lin, const float **db) {
		if (ncollected <= 0) return set_error("%s: no tick has been collected", fn), (int)MI_EINVAL;
		const int slot = (int)((ncollected - 1) % slots);
		if (rep_seq[slot] != ncollected - 1) return set_error("%s: tick %lld's slot has been submitted again", fn, ncollected - 1), (int)MI_EINVAL;
		if (!rep_what[slot]) return set_error("%s: reports were off for tick %lld", fn, ncollected - 1), (int)MI_EINVAL;
		const float *lv = reinterpret_cast<const float *>(h_rep[slot]);
		const bool speakers = (rep_what[slot] & MI_REPORT_SPEAKERS) != 0;
		*seq = (uint64_t)(ncollected - 1), *what = rep_what[slot];
		*levels = (rep_what[slot] & MI_REPORT_LEVELS) ? lv : nullptr;
		*winner = speakers ? reinterpret_cast<const int32_t *>(h_rep[slot]) + n : nullptr;
		*max_lin = speakers ? lv + n + nconf : nullptr;
		*db = speakers ? max_db.data() : nullptr;
		for (int c = 0; speakers && c < nconf; ++c) {
			const float lin = (*max_lin)[c];
			max_db[(size_t)c] = lin == 0 ? -120.f : 10 * log10f(lin);
		}
		return MI_OK;
	}
};

} // namespace mi
