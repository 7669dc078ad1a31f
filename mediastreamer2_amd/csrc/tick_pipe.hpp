// tick_pipe.hpp -- the slot ring under mi_session (session.hip), mi_bridge (bridge.hip) and mi_scaler_pipe (scaler.hip):
// upload | kernels | download on three HIP streams -- the pipe's two and the context's --, ordered by three events per slot,
// up to `depth` ticks in flight.  Host code only.  The pipe owns streams, events and counters; the buffers stay with their
// owners (they differ in number, type, allocator and initialisation), who hand the pipe three callables per submit.
//
// What orders a slot's reuse:
//   acquire   the host is about to overwrite the slot's staging: it waits for the previous use's upload (UPLOADED) or for
//             the kernels that consumed it (CONSUMED), as the owner asks;
//   submit    the kernels wait for this tick's upload (ev_up) and for the download that last read the slot's output
//             (ev_down); the download waits for the kernels (ev_done);
//   collect   the host waits for the oldest tick's download (ev_down).
#pragma once
#include "common.hpp"

namespace mi {

struct TickPipe {
	static constexpr int MAX_DEPTH = 8;
	enum WaitFor { UPLOADED, CONSUMED };
	// acquire / collect could not be served.  Nothing else makes them return MI_EINVAL, and the owner words the error
	static constexpr int FULL = MI_EINVAL, EMPTY = MI_EINVAL;

	mi_ctx *ctx = nullptr;
	int depth = 0;
	hipStream_t s_up = nullptr, s_down = nullptr;
	hipEvent_t ev_up[MAX_DEPTH] = {}, ev_done[MAX_DEPTH] = {}, ev_down[MAX_DEPTH] = {};
	bool used[MAX_DEPTH] = {};
	long long submitted = 0, collected = 0;
	bool acquired = false; // between acquire and the submit that follows it

	int create(mi_ctx *c, int slots) {
		ctx = c, depth = slots;
		if (hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking) != hipSuccess ||
		    hipStreamCreateWithFlags(&s_down, hipStreamNonBlocking) != hipSuccess) {
			set_error("hipStreamCreate failed");
			return MI_ENODEV;
		}
		for (int i = 0; i < depth; ++i)
			if (hipEventCreateWithFlags(&ev_up[i], hipEventDisableTiming) != hipSuccess ||
			    hipEventCreateWithFlags(&ev_done[i], hipEventDisableTiming) != hipSuccess ||
			    hipEventCreateWithFlags(&ev_down[i], hipEventDisableTiming) != hipSuccess) {
				set_error("hipEventCreate failed");
				return MI_ENODEV;
			}
		return MI_OK;
	}

	// everything submitted has left the device (the owner has selected it).  Also what a half-created pipe is handed
	void drain() {
		if (ctx) (void)hipStreamSynchronize(ctx->stream);
		if (s_up) (void)hipStreamSynchronize(s_up);
		if (s_down) (void)hipStreamSynchronize(s_down);
	}

	void destroy() {
		for (int i = 0; i < depth; ++i)
			for (hipEvent_t e : {ev_up[i], ev_done[i], ev_down[i]})
				if (e) (void)hipEventDestroy(e);
		if (s_up) (void)hipStreamDestroy(s_up);
		if (s_down) (void)hipStreamDestroy(s_down);
	}

	int in_flight() const { return (int)(submitted - collected); }
	int next_slot() const { return (int)(submitted % depth); } // the slot acquire handed out / submit will use

	// the next slot's staging, once its previous use no longer needs it; FULL when `depth` ticks are in flight
	int acquire(WaitFor wait_for, int *slot) {
		if (in_flight() >= depth) return FULL;
		const int i = next_slot();
		if (ctx->activate() != MI_OK) return MI_ENODEV;
		if (used[i]) MI_HIP(hipEventSynchronize(wait_for == UPLOADED ? ev_up[i] : ev_done[i]));
		*slot = i;
		acquired = true;
		return MI_OK;
	}

	// upload(slot) enqueues on s_up, kernels(slot) on the context's stream, download(slot) on s_down; each returns MI_*.
	// A failure leaves the tick unsubmitted: `acquired` still set, `submitted` where it was.
	template <class Upload, class Kernels, class Download>
	int submit(Upload &&upload, Kernels &&kernels, Download &&download) {
		if (ctx->activate() != MI_OK) return MI_ENODEV;
		const int i = next_slot();
		int rc;
		if ((rc = upload(i)) != MI_OK) return rc;
		MI_HIP(hipEventRecord(ev_up[i], s_up));
		// kernels wait for this tick's upload and for the download that last read this slot's output buffer
		MI_HIP(hipStreamWaitEvent(ctx->stream, ev_up[i], 0));
		if (used[i]) MI_HIP(hipStreamWaitEvent(ctx->stream, ev_down[i], 0));
		if ((rc = kernels(i)) != MI_OK) return rc;
		MI_HIP(hipEventRecord(ev_done[i], ctx->stream));
		MI_HIP(hipStreamWaitEvent(s_down, ev_done[i], 0));
		if ((rc = download(i)) != MI_OK) return rc;
		MI_HIP(hipEventRecord(ev_down[i], s_down));
		used[i] = true;
		submitted++;
		acquired = false;
		return MI_OK;
	}

	// the oldest tick in flight, downloaded; EMPTY when there is none
	int collect(int *slot) {
		if (collected >= submitted) return EMPTY;
		if (ctx->activate() != MI_OK) return MI_ENODEV;
		const int i = (int)(collected % depth);
		MI_HIP(hipEventSynchronize(ev_down[i]));
		*slot = i;
		collected++;
		return MI_OK;
	}
};

} // namespace mi
