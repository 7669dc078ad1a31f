// controls.hip -- the two launches that let a running mi_bridge or mi_session be steered and observed without a wait:
//
// controls_kernel: a tick's control changes (mi_bridge_change_controls, mi_session_change_controls) applied on the device, in
// stream order ahead of that tick's kernels and behind its membership kernel: what MS_AUDIO_MIXER_SET_ACTIVE / _ENABLE_OUTPUT /
// _SET_INPUT_GAIN (audiomixer.c:372-414) and MSVolume's setters do to one filter, as data written where the waiting setters
// write it -- the pin's flags and gain (mi_mixer_set_controls), the seat's mi_volume_params (mi_volume_set_params) -- and the
// seat's place in the joining order.  The changes arrive as a row of mi_ctl_cmd uploaded with the tick; one lane takes one
// command.  A tick without changes does not launch this.
//
// report_kernel: what a tick left, read behind its kernels into a block that comes down with the tick's output: every stream's
// MS_VOLUME_GET_LINEAR and per conference ms_audio_conference_process_events' election (audioconference.c:436-452).  A
// conference is one wavefront, lane m its member m; four conferences share a workgroup.  The maximum is a wave reduction on the
// linear one-second maxima, the tie-break -- the member that joined first -- a second one on the joining order among the lanes
// that hold the maximum, the winner's lane read off a ballot.  No LDS.  Launched only while reports are on.
#include "controls.hpp"

namespace {

__global__ __launch_bounds__(64) void controls_kernel(ControlArgs a) {
	const int i = blockIdx.x * 64 + threadIdx.x;
	if (i >= a.count) return;
	const CtlFields c = load_ctl(a.cmd, i);
	const int s = c.stream;
	const unsigned what = c.what;
	if (s < 0 || s >= a.nstreams) return; // (the host has checked every entry: no store without its seat)
	if (what & MI_CTL_FLAGS) a.flags[s] = (uint8_t)c.flags;
	if (what & MI_CTL_GAIN) a.gain[s] = c.gain;
	if (what & MI_CTL_JOINED) a.joined[s] = c.joined;
	if ((what & MI_CTL_VOLUME) && a.params) {
		const uint4 *src = reinterpret_cast<const uint4 *>(a.cmd + i); // the parameters: the four loads behind the head
		const uint4 p0 = src[1], p1 = src[2], p2 = src[3], p3 = src[4];
		uint32_t *dst = reinterpret_cast<uint32_t *>(a.params + s); // 60 bytes at a 60-byte pitch: words
		dst[0] = p0.x, dst[1] = p0.y, dst[2] = p0.z, dst[3] = p0.w;
		dst[4] = p1.x, dst[5] = p1.y, dst[6] = p1.z, dst[7] = p1.w;
		dst[8] = p2.x, dst[9] = p2.y, dst[10] = p2.z, dst[11] = p2.w;
		dst[12] = p3.x, dst[13] = p3.y, dst[14] = p3.z;
	}
}

constexpr int REPORT_BT = 256; // four conferences

__global__ __launch_bounds__(REPORT_BT) void report_kernel(ReportArgs a) {
	const int c = blockIdx.x * (REPORT_BT / 64) + (threadIdx.x >> 6), m = threadIdx.x & 63;
	if (c >= a.nconf) return; // (whole wavefronts)
	const bool seat = m < a.mm;
	const int s = c * a.mm + (seat ? m : 0);
	if ((a.what & MI_REPORT_LEVELS) && seat) a.levels[s] = a.state[s].energy; // volume_get_linear msvolume.c:129-134
	if (!(a.what & MI_REPORT_SPEAKERS)) return;
	const float2 w = a.win[s];
	const unsigned f = a.flags[s];
	const unsigned order = a.joined[s];
	const float lin = w.y < 0 ? 0.f : w.x; // ortp_extremum_init: 0 before the first record
	// plumbed, not muted (:445), above the threshold (:31)
	const bool eligible = seat && (f & MI_MIX_LINKED) && (f & MI_MIX_ACTIVE) && lin >= a.thr;
	float best = eligible ? lin : -1.f;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) best = fmaxf(best, __shfl_xor(best, off));
	// of equals, the earliest joiner: the list is walked in joining order and a later member must be strictly louder (:449)
	const bool top = eligible && lin == best;
	unsigned first = top ? order : 0xffffffffu;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) first = min(first, (unsigned)__shfl_xor((int)first, off));
	const unsigned long long who = __ballot(top && order == first);
	if (m == 0) {
		const int lane = who ? __ffsll((long long)who) - 1 : -1;
		a.winner[c] = lane < 0 ? -1 : c * a.mm + lane;
		a.max_lin[c] = lane < 0 ? 0.f : best;
	}
}

} // namespace

int mi_controls_launch(const ControlArgs &args, hipStream_t stream) {
	MI_CHECK_ARG(args.cmd && args.count > 0 && args.count <= args.nstreams && args.flags && args.gain && args.joined);
	hipLaunchKernelGGL(controls_kernel, dim3((unsigned)mi::ceil_div(args.count, 64)), dim3(64), 0, stream, args);
	MI_LAUNCH_CHECK();
	return MI_OK;
}

int mi_report_launch(const ReportArgs &args, hipStream_t stream) {
	MI_CHECK_ARG(args.state && args.win && args.flags && args.joined && args.nconf > 0 && args.mm > 0 && args.mm <= REPORT_MAX_MEMBERS);
	MI_CHECK_ARG(args.what && !(args.what & ~(MI_REPORT_SPEAKERS | MI_REPORT_LEVELS)));
	MI_CHECK_ARG((!(args.what & MI_REPORT_LEVELS) || args.levels) && (!(args.what & MI_REPORT_SPEAKERS) || (args.winner && args.max_lin)));
	hipLaunchKernelGGL(report_kernel, dim3((unsigned)mi::ceil_div(args.nconf, REPORT_BT / 64)), dim3(REPORT_BT), 0, stream, args);
	MI_LAUNCH_CHECK();
	return MI_OK;
}
