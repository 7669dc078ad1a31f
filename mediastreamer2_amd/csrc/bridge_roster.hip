// bridge_roster.hip -- a tick's membership changes applied on the device, in stream order ahead of that tick's kernels
// (mi_bridge_change_members, bridge.hip): what ms_audio_conference_add_member's plumb_to_conf brings to a mixer pin -- the
// endpoint's own decoder and encoder, two fresh resamplers, a fresh MSVolume (audioconference.c:209-257, :322-345) -- as data
// written where mi_bridge_add_member's waiting calls write it, and remove_member's unplumbing.  The changes arrive as a row
// of mi_seat_cmd uploaded with the tick; one wavefront takes one command, lane 0 the scalars, all 64 lanes the rows it
// zeroes.  A tick without changes does not launch this.  The concealer's part is plc.hip's own launch (mi_plc_apply_seats).
#include "bridge_roster.hpp"

namespace {

// `words` 32-bit words from p, which is 4-byte aligned
__device__ __forceinline__ void zero_words(void *p, int words, int lane) {
	uint32_t *w = static_cast<uint32_t *>(p);
	for (int i = lane; i < words; i += 64) w[i] = 0u;
}

__global__ __launch_bounds__(64) void bridge_roster_kernel(RosterArgs a) {
	const int i = blockIdx.x, lane = threadIdx.x;
	if (i >= a.count) return;
	const SeatFields c = load_seat(a.cmd, i);
	const int s = c.stream;
	const unsigned op = c.op;
	if (s < 0 || s >= a.nstreams) return; // (the host has checked every entry: no store without its seat)
	if (op & MI_SEAT_JOIN) {
		if (lane == 0) {
			if (a.ratio) a.ratio[s] = (uint8_t)c.ratio;
			if (a.codec) a.codec[s] = (uint8_t)c.codec;
			if (a.codec_pcm) a.codec_pcm[s] = (uint8_t)(c.codec & ~3u);
			fresh_meter(a.vol, s);
			a.flags[s] = (uint8_t)c.flags; // linked, active, output on -- unless a later mi_bridge_set_controls said otherwise
		}
		// speex_resampler_init: both histories zero, over the stride the plan keeps for the longest filter of any kind
		if (a.hist_in) zero_words(a.hist_in + (size_t)s * a.hin_stride, a.hin_stride >> 1, lane);
		if (a.hist_out) zero_words(a.hist_out + (size_t)s * a.hout_stride, a.hout_stride >> 1, lane);
	}
	if ((op & MI_SEAT_LEAVE) && lane == 0) a.flags[s] = (uint8_t)c.flags; // 0, with the same proviso
	// an unplumbed pin's row is left alone by the tick: what the departed leg last heard must not linger in this slot
	if (op & MI_SEAT_CLEAR) zero_words(a.out + (size_t)s * a.out_bytes, a.out_bytes >> 2, lane);
}

} // namespace

int mi_bridge_roster_launch(const RosterArgs &args, hipStream_t stream) {
	// every row is zeroed in whole words
	MI_CHECK_ARG(args.cmd && args.count > 0 && args.count <= args.nstreams && args.vol.state && args.vol.win && args.vol.energy[0] &&
	             args.vol.energy[1] && args.flags && args.out && args.out_bytes % 4 == 0 && args.hin_stride % 2 == 0 && args.hout_stride % 2 == 0);
	hipLaunchKernelGGL(bridge_roster_kernel, dim3((unsigned)args.count), dim3(64), 0, stream, args);
	MI_LAUNCH_CHECK();
	return MI_OK;
}
