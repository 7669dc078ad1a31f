// session_roster.hip -- a tick's membership changes applied on the device, in stream order ahead of that tick's kernels
// (mi_session_change_members, session.hip): what ms_audio_conference_add_member brings to a seat of the chained path -- the
// endpoint's own filters, all fresh (resamplers, MSSpeexEC, MSVolume, the bufferizers between them: what
// mi_session_reset_streams' waiting calls write), its mixer pin linked -- and remove_member's unplumbing
// (audioconference.c:322-374).  The changes arrive as a row of mi_seat_cmd uploaded with the tick; one workgroup of 256 lanes
// takes one command.  Nearly all of a JOIN is the canceller: both filter halves and the X history, about 150 KB at 48 kHz with
// a 128 ms tail, zero in a fresh speex_echo_state -- 16-byte stores spread over the whole group -- and the few KB that are not
// (the `small` row, the scalar record), copied from the template the canceller built when it was created.  Which bytes those
// are is aec.hip's to say (AecEdit, common.hpp); nothing of the canceller's layout is known here.  A tick without changes
// does not launch this.  The concealer's part is plc.hip's own launch (mi_plc_apply_seats).
#include "session_roster.hpp"

namespace {

constexpr int RT = 256;

// `bytes` from p, both multiples of 16
__device__ __forceinline__ void zero_groups(void *p, size_t bytes, int t) {
	uint4 *q = static_cast<uint4 *>(p);
	const unsigned n = (unsigned)(bytes >> 4);
	for (unsigned i = (unsigned)t; i < n; i += RT) q[i] = make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ void copy_groups(void *dst, const void *src, int bytes, int t) {
	uint4 *q = static_cast<uint4 *>(dst);
	const uint4 *r = static_cast<const uint4 *>(src);
	for (int i = t; i < (bytes >> 4); i += RT) q[i] = r[i];
}

// rows whose pitch may be any even number of bytes: sample by sample (a tick's row, a FIFO's lead: a few hundred)
__device__ __forceinline__ void zero_samples(int16_t *p, int n, int t) {
	for (int i = t; i < n; i += RT) p[i] = 0;
}

// an MSBufferizer just created, then `silence` samples written into it: head 0, the ring's first samples zero
__device__ __forceinline__ void fresh_fifo(const FifoView &f, int s, int silence, int t) {
	if (silence < 0 || silence > f.cap) silence = 0; // (the host has checked the sizes: no store past the ring)
	zero_samples(f.ring + (size_t)s * f.cap, silence, t);
	if (t == 0) f.pos[s] = make_int2(0, silence);
}

__device__ __forceinline__ void fresh_resampler(const ResamplerEdit &r, int s, int t) { // speex_resampler_init
	if (!r.hist) return;
	zero_groups(r.hist + (size_t)s * r.hist_stride, (size_t)r.hist_stride * sizeof(int16_t), t);
	if (t == 0 && r.pos) r.pos[s] = make_int2(0, 0); // (a per-leg history row of mi_session_create_legs has no position word)
}

__global__ __launch_bounds__(RT) void session_roster_kernel(SessionRosterArgs a) {
	const int i = blockIdx.x, t = threadIdx.x;
	if (i >= a.count) return;
	const SeatFields c = load_seat(a.cmd, i);
	const int s = c.stream;
	const unsigned op = c.op;
	if (s < 0 || s >= a.nstreams) return; // (the host has checked every entry: no store without its seat)
	if (op & MI_SEAT_JOIN) {
		// speex_echo_state_init: the filters and the far end's history zero, the rest from the template
		zero_groups(reinterpret_cast<char *>(a.aec.WF) + (size_t)s * a.aec.wf_bytes, a.aec.wf_bytes, t);
		zero_groups(reinterpret_cast<char *>(a.aec.X) + (size_t)s * a.aec.x_bytes, a.aec.x_bytes, t);
		copy_groups(reinterpret_cast<char *>(a.aec.small) + (size_t)s * a.aec.small_bytes, a.aec.small_tpl, a.aec.small_bytes, t);
		copy_groups(static_cast<char *>(a.aec.scal) + (size_t)s * a.aec.scal_bytes, a.aec.scal_tpl, a.aec.scal_bytes, t);
		fresh_resampler(a.rs_in, s, t);
		fresh_resampler(a.rs_out, s, t);
		// the three queues empty at head 0; then the reference's delay line (speexec.c:205-208) and, in both queues the canceller
		// reads, the lead of this seat's re-framing phase (mi_aec_stagger_fifos)
		const int lead = a.lead_phases >= 2 ? a.lead_unit * (int)fifo_phase_of((unsigned)s, (unsigned)a.lead_phases) : 0;
		fresh_fifo(a.f_mic, s, lead, t);
		fresh_fifo(a.f_ref, s, a.ref_delay + lead, t);
		fresh_fifo(a.f_out, s, 0, t);
		if (t == 0) fresh_meter(a.vol, s);
	}
	if (op & (MI_SEAT_JOIN | MI_SEAT_LEAVE)) {
		// linked, active, output on / unplumbed -- unless a later mi_session_set_controls said otherwise
		if (t == 0) a.flags[s] = (uint8_t)c.flags;
		// the kept mix is the next tick's far end (ref_loopback) and the encoder's input: nothing was sent to a new leg yet, and
		// what a departed one last heard must not linger.  Only the context's stream touches these rows
		for (int k = 0; k < SESSION_ROSTER_SLOTS; ++k)
			if (a.mix[k]) zero_samples(a.mix[k] + (size_t)s * a.mix_len, a.mix_len, t);
	}
	// an unplumbed pin's row is left alone by the tick: this slot's, and no other's -- their downloads may be running
	if (op & MI_SEAT_CLEAR) {
		uint8_t *row = a.out + (size_t)s * a.out_bytes;
		if ((a.out_bytes & 1) == 0) zero_samples(reinterpret_cast<int16_t *>(row), a.out_bytes >> 1, t);
		else
			for (int j = t; j < a.out_bytes; j += RT) row[j] = 0;
	}
}

bool whole_groups(const AecEdit &e) {
	return e.X && e.WF && e.small && e.scal && e.small_tpl && e.scal_tpl && e.x_bytes % 16 == 0 && e.wf_bytes % 16 == 0 && e.small_bytes % 16 == 0 &&
	       e.scal_bytes % 16 == 0;
}

} // namespace

int mi_session_roster_launch(const SessionRosterArgs &a, hipStream_t stream) {
	MI_CHECK_ARG(a.cmd && a.count > 0 && a.count <= a.nstreams && whole_groups(a.aec) && a.vol.state && a.vol.win && a.vol.energy[0] &&
	             a.vol.energy[1] && a.flags && a.out && a.out_bytes > 0 && a.mix_len > 0);
	// an mi_resampler's history goes with its position word; the legs' own rows have none
	MI_CHECK_ARG((!a.rs_in.hist || ((a.leg_rows || a.rs_in.pos) && a.rs_in.hist_stride % 8 == 0)) &&
	             (!a.rs_out.hist || ((a.leg_rows || a.rs_out.pos) && a.rs_out.hist_stride % 8 == 0)));
	MI_CHECK_ARG(!a.leg_rows || (a.rs_in.hist && a.rs_out.hist && !a.rs_in.pos && !a.rs_out.pos));
	// every queue holds what a fresh seat is given
	const int lead = a.lead_phases >= 2 ? a.lead_unit * (a.lead_phases - 1) : 0;
	MI_CHECK_ARG(a.f_mic.ring && a.f_mic.pos && a.f_ref.ring && a.f_ref.pos && a.f_out.ring && a.f_out.pos && a.ref_delay >= 0 && a.lead_unit >= 0 &&
	             lead <= a.f_mic.cap && a.ref_delay + lead <= a.f_ref.cap);
	hipLaunchKernelGGL(session_roster_kernel, dim3((unsigned)a.count), dim3(RT), 0, stream, a);
	MI_LAUNCH_CHECK();
	return MI_OK;
}
