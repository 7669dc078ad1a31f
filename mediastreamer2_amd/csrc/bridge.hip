// bridge.hip -- mi_bridge (include/msmi355x_bridge.h): a conference server's member chain
//   decoder -> MSVolume (level / meter) -> MSAudioMixer pin -> encoder      (src/voip/audioconference.c:209-257)
// for a batch of conferences, a conference's whole 10 ms tick in ONE launch, fed from host buffers like mi_session
// (session.hip): three slots of pinned staging, upload / kernel / download on three HIP streams (mi::TickPipe,
// tick_pipe.hpp), up to three ticks in flight.  No echo canceller -- that is the endpoint's.  Built with
// -ffp-contract=off like volume.hip: MSVolume's control chain is float32 evaluated unfused in source order, and every
// output sample depends on it bit for bit.
//
// One workgroup of 256 lanes = one conference; the members' ticks live in LDS as packed int16 rows whose pitch is an odd
// number of 8-byte words (volmix_kernel's layout, volume.hip), so the lanes that walk one row each in the serial meter read
// disjoint banks.  A tick is these phases, each written once in bridge_phases.hpp, a barrier between any two:
//   (0) lane m < members: its MSVolume parameters, state and window, its mixer controls, its `present` byte (load_member);
//   (A) eight lanes per member (32 members a round): the rows into LDS -- 16 bytes of PCM, or 8 code words decoded with
//       codec.hip's arithmetic (g711.hpp), per lane and group, four groups in flight --, integer peak and DC sum reduced
//       over the eight lanes in registers.  An absent member's row is zeros (audiomixer.c:88) (stage_rows);
//   (B) lane m: the float32 sum of squares IN SAMPLE ORDER (the order is part of the reference's result) and the control
//       chain (volume_control, volume_ctl.hpp) on the leg's own samples at the leg's rate: MSVolume sits in front of the
//       in_resampler.  An absent member is skipped whole: MSVolume got no chunk (msvolume.c:480-486) (meter);
//   (G) with resamplers only: the Q12 gain (apply_gain) on the leg-rate samples, in the row (level_legs);
//   (U) with resamplers only, one wavefront per member: the in_resampler of a present, plumbed leg (resample_in);
//   (C) lane = (member slice, four columns): the Q12 gain where there was no (G), then the pin's contribution as
//       channel_process_in leaves it (0 unless linked and active; input gain) back into the row, and the int32 sum over
//       the slice's members added into the conference's sum row in LDS (mix);
//   (D) lane = (member, eight columns), for every pin with its output enabled: saturate(sum - own) (channel_process_out),
//       stored as 16 bytes of PCM or encoded to 8 code words -- or, for a member with an out_resampler, written over its
//       own row (mix_minus);
//   (W) with resamplers only, one wavefront per member: the out_resampler of a pin with its output on, then the leg's store
//       or encoder (resample_out).
// A member's ratio -- conference rate / leg rate 1, 2, 3 or 6, the same above the mix, 3/2 either way -- and its codec pair
// are data: one conference holds 8, 16 and 48 kHz legs, A-law and mu-law trunks and PCM members side by side.  The rows in
// LDS are as wide as the widest leg's tick; a narrower leg's tick sits at the head of its row until its up-sampler has run.
// The five kernels below differ in which forms they are built for, so that a bridge pays only for what its legs need:
// compile-time codecs or per-leg ones, no resamplers, those of legs below the mix, above it, at 3/2 and 2/3 of it.
//
// Geometry: an 8 kHz conference of 32 is 5.4 KB of LDS and four waves, so eight such workgroups share a CU (32 waves);
// 1000 conferences are 1000 workgroups dealt over the 256 CUs, about four per CU = one wave per SIMD and conference
// phase, every conference resident at once.  48 kHz x 50 members is 50 KB: three per CU.  HBM traffic per 8 kHz G.711
// leg-tick: 80 B in, 80 B out, + 130 B of meter parameters / state / window.
#include "common.hpp"
#include "conference.hpp"
#include "tick_pipe.hpp"

#include "bridge_phases.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int SLOTS = 3; // upload | compute | download can each hold a different tick
constexpr size_t BRIDGE_LDS_MAX = 64 * 1024;
constexpr size_t RATED_STATIC_LDS = 2048; // bound on a kernel's static LDS (tests/test_bridge_rates_cpu.py holds it)

// every leg at the conference's rate, one compile-time codec pair (mi_bridge_create): (0) (A) (B) (C) with the gain (D).
// (0) (A) (B) stand written out here, word for word load_member / stage_rows / meter at F_SAME with FixedSrc<IN>: composed from
// those helpers the A-law instantiations come out one VGPR lower and all nine eight SGPRs higher (four of the meter's tests
// folded into phase (0), as in the other kernels), and tests/test_bridge_rates_cpu.py pins this kernel's figures exactly.
template <int IN, int OUT>
__global__ __launch_bounds__(BT) void bridge_tick_kernel(BridgeArgs a) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	const Conf k = conf_view(a, smem, s_pk, s_dc, s_par);
	uint2 *rows = k.rows;
	int *s_sum = k.s_sum;
	const int t = k.t, mm = k.mm, ns = k.ns, nw = k.nw, ng = k.ng, s0 = k.s0;

	// ---- (0)
	mi_volume_params p;
	mi_volume_state st;
	float2 win = make_float2(0, 0);
	unsigned mflag = 0;
	int mgain_bits = 0;
	bool here = false;
	if (t < mm) {
		const int s = s0 + t;
		p = a.params[s];
		st = a.state[s];
		win = a.win[s];
		mflag = a.flags[s];
		mgain_bits = __float_as_int(a.gain[s]);
		here = !a.present || a.present[s] != 0;
	}
	for (int i = t; i < ns; i += BT) s_sum[i] = 0;

	// ---- (A)
	for (int mb = 0; mb < mm; mb += BT / 8) {
		const int m = mb + (t >> 3), q = t & 7;
		const bool valid = m < mm;
		int pk = 0, dc = 0;
		if (valid) {
			const bool on = !a.present || a.present[s0 + m] != 0;
			for (int g0 = q; g0 < ng; g0 += 32) {
				uint4 v[4];
#pragma unroll
				for (int i = 0; i < 4; ++i) { // straight-line loads: all in flight at once
					v[i] = make_uint4(0, 0, 0, 0);
					if (on && g0 + 8 * i < ng) v[i] = load_group<IN>(a.in, (size_t)(s0 + m), ns, g0 + 8 * i);
				}
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const int g = g0 + 8 * i;
					if (g >= ng) continue;
					rows[m * a.row_w + 2 * g] = make_uint2(v[i].x, v[i].y);
					rows[m * a.row_w + 2 * g + 1] = make_uint2(v[i].z, v[i].w);
					const unsigned w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
					for (int j = 0; j < 4; ++j) {
						const int x0 = lo16(w[j]), x1 = hi16(w[j]);
						pk = max(pk, max(x0 < 0 ? -x0 : x0, x1 < 0 ? -x1 : x1));
						dc += x0 + x1;
					}
				}
			}
		}
#pragma unroll
		for (int off = 1; off < 8; off <<= 1) { // over the member's eight lanes
			pk = max(pk, __shfl_xor(pk, off));
			dc += __shfl_xor(dc, off);
		}
		if (valid && q == 0) s_pk[m] = pk, s_dc[m] = dc;
	}
	__syncthreads();

	// ---- (B)
	if (t < mm) {
		if (here) {
			const uint2 *r = rows + t * a.row_w;
			float acc = 0;
#pragma unroll 4
			for (int i = 0; i < nw; ++i) {
				const uint2 w = r[i];
				const int x0 = lo16(w.x), x1 = hi16(w.x), x2 = lo16(w.y), x3 = hi16(w.y);
				acc += (float)(x0 * x0);
				acc += (float)(x1 * x1);
				acc += (float)(x2 * x2);
				acc += (float)(x3 * x3);
			}
			const VolCtl o = volume_control(p, st, 0.f, acc, ns, s_pk[t], s_dc[t], a.sample_rate, win);
			s_par[t] = make_int4((int)mflag | (o.mode << 8), o.intgain, o.dcoff, mgain_bits);
			a.state[s0 + t] = st;
			a.win[s0 + t] = win;
		} else {
			s_par[t] = make_int4((int)mflag, 4096, 0, mgain_bits);
		}
	}
	__syncthreads();

	mix<true>(k, a.nslice);
	__syncthreads();
	mix_minus<F_SAME, OUT>(k, static_cast<uint8_t *>(a.out), k.ns);
}

// legs at or below the mix (mi_bridge_create_rated), one compile-time codec pair on rows of ra.pitch samples: in_resampler
// and out_resampler of plumb_to_conf (audioconference.c:209-257) folded into the tick -- every phase, (C) without the gain
template <int IN, int OUT>
__global__ __launch_bounds__(BT) void bridge_rated_kernel(RatedArgs ra) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	__shared__ unsigned char s_rt[BMAX], s_on[BMAX];
	const BridgeArgs &a = ra.b;
	const Conf k = conf_view(a, smem, s_pk, s_dc, s_par, s_rt, s_on);
	uint8_t *out = static_cast<uint8_t *>(a.out);
	float *scr = wave_scratch(smem, ra, k.t);
	mi_volume_params p;
	mi_volume_state st;
	Member me = load_member<F_BELOW, false>(k, a, ra.ratio, nullptr, p, st);
	stage_rows<F_BELOW>(k, a.present, ra.ratio, FixedSrc<IN>{a.in, ra.pitch});
	__syncthreads();
	meter<F_BELOW>(k, a, me, p, st);
	__syncthreads();
	level_legs<F_BELOW>(k, k.nw);
	__syncthreads();
	resample_in<F_BELOW>(k, ra, nullptr, nullptr, scr);
	__syncthreads();
	mix<false>(k, a.nslice);
	__syncthreads();
	mix_minus<F_BELOW, OUT>(k, out, ra.pitch);
	__syncthreads();
	resample_out<F_BELOW, OUT>(k, ra, nullptr, nullptr, scr, out, ra.pitch);
}

// every leg's own codec (mi_bridge_create_legs): plumb_to_conf hangs each endpoint's own decoder and encoder on its pin.  The
// host rows are byte rows at one pitch; a leg's tick is the first rate / 100 x 1 or 2 bytes of its row.  RATED false: the
// phases of bridge_tick_kernel; true: those of bridge_rated_kernel.  Only a bridge whose legs differ runs this kernel: a
// uniform one keeps the kernels above.
template <bool RATED>
__global__ __launch_bounds__(BT) void bridge_legs_kernel(LegsArgs la) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	__shared__ unsigned char s_rt[BMAX], s_on[BMAX], s_cd[BMAX];
	constexpr int FORMS = RATED ? F_BELOW : F_SAME;
	const RatedArgs &ra = la.r;
	const BridgeArgs &a = ra.b;
	const Conf k = conf_view(a, smem, s_pk, s_dc, s_par, s_rt, s_on, s_cd);
	uint8_t *out = static_cast<uint8_t *>(a.out);
	float *scr = RATED ? wave_scratch(smem, ra, k.t) : nullptr;
	mi_volume_params p;
	mi_volume_state st;
	Member me = load_member<FORMS, true>(k, a, ra.ratio, la.codec, p, st);
	stage_rows<FORMS>(k, a.present, ra.ratio, LegSrc{static_cast<const uint8_t *>(a.in), la.in_pitch, la.codec});
	__syncthreads();
	meter<FORMS>(k, a, me, p, st);
	__syncthreads();
	if (RATED) {
		level_legs<FORMS>(k, k.nw);
		__syncthreads();
		resample_in<FORMS>(k, ra, nullptr, nullptr, scr);
		__syncthreads();
	}
	mix<!RATED>(k, a.nslice);
	__syncthreads();
	mix_minus<FORMS, BY_KIND>(k, out, la.out_pitch);
	if (!RATED) return;
	__syncthreads();
	resample_out<FORMS, BY_KIND>(k, ra, nullptr, nullptr, scr, out, la.out_pitch);
}

// endpoints on either side of the mix (mi_bridge_create_endpoints): plumb_to_conf configures both resamplers from the
// endpoint's rate and the conference's whichever is larger, so a leg ABOVE the mix -- a 48 kHz PCM member of a 16 kHz room --
// has the down-sampler in front of its pin and the up-sampler behind it.  bridge_legs_kernel<true> with those forms, the rows
// ua.wide samples.  Only a bridge with at least one such leg runs this kernel.
__global__ __launch_bounds__(BT) void bridge_updown_kernel(UpdownArgs ua) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	__shared__ unsigned char s_rt[BMAX], s_on[BMAX], s_cd[BMAX];
	const LegsArgs &la = ua.l;
	const RatedArgs &ra = la.r;
	const BridgeArgs &a = ra.b;
	const Conf k = conf_view(a, smem, s_pk, s_dc, s_par, s_rt, s_on, s_cd);
	uint8_t *out = static_cast<uint8_t *>(a.out);
	float *scr = wave_scratch(smem, ra, k.t);
	mi_volume_params p;
	mi_volume_state st;
	Member me = load_member<F_ABOVE, true>(k, a, ra.ratio, la.codec, p, st);
	stage_rows<F_ABOVE>(k, a.present, ra.ratio, LegSrc{static_cast<const uint8_t *>(a.in), la.in_pitch, la.codec});
	__syncthreads();
	meter<F_ABOVE>(k, a, me, p, st);
	__syncthreads();
	level_legs<F_ABOVE>(k, ua.wide >> 2);
	__syncthreads();
	resample_in<F_ABOVE>(k, ra, &ua, nullptr, scr);
	__syncthreads();
	mix<false>(k, a.nslice);
	__syncthreads();
	mix_minus<F_ABOVE, BY_KIND>(k, out, la.out_pitch);
	__syncthreads();
	resample_out<F_ABOVE, BY_KIND>(k, ra, &ua, nullptr, scr, out, la.out_pitch);
}

// legs at 3/2 and 2/3 of the mix's rate as well (mi_bridge_create_rational): 32 kHz members of a 48 kHz room, 24 kHz members
// of a 16 kHz one.  bridge_updown_kernel with those forms.  Only a bridge with at least one such leg runs this kernel.
__global__ __launch_bounds__(BT) void bridge_rational_kernel(RationalArgs qa) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	__shared__ unsigned char s_rt[BMAX], s_on[BMAX], s_cd[BMAX];
	const UpdownArgs &ua = qa.u;
	const LegsArgs &la = ua.l;
	const RatedArgs &ra = la.r;
	const BridgeArgs &a = ra.b;
	const Conf k = conf_view(a, smem, s_pk, s_dc, s_par, s_rt, s_on, s_cd);
	uint8_t *out = static_cast<uint8_t *>(a.out);
	float *scr = wave_scratch(smem, ra, k.t);
	mi_volume_params p;
	mi_volume_state st;
	Member me = load_member<F_R32, true>(k, a, ra.ratio, la.codec, p, st);
	stage_rows<F_R32>(k, a.present, ra.ratio, LegSrc{static_cast<const uint8_t *>(a.in), la.in_pitch, la.codec});
	__syncthreads();
	meter<F_R32>(k, a, me, p, st);
	__syncthreads();
	level_legs<F_R32>(k, ua.wide >> 2);
	__syncthreads();
	resample_in<F_R32>(k, ra, &ua, &qa, scr);
	__syncthreads();
	mix<false>(k, a.nslice);
	__syncthreads();
	mix_minus<F_R32, BY_KIND>(k, out, la.out_pitch);
	__syncthreads();
	resample_out<F_R32, BY_KIND>(k, ra, &ua, &qa, scr, out, la.out_pitch);
}

} // namespace

struct mi_bridge {
	mi_ctx *ctx = nullptr;
	mi_bridge_config cfg;
	int n = 0, nconf = 0, mm = 0, len = 0;
	size_t in_bytes = 0, out_bytes = 0; // per stream and tick, on the host side
	int row_w = 0, nslice = 0, sum_off = 0;
	size_t lds = 0;
	mi_volume *vol = nullptr; // the meters: parameters, state, one-second windows
	mi_mixer *mix = nullptr;  // the pins' controls
	mi_plc *plc = nullptr;
	mi::TickPipe pipe;
	uint8_t *h_in[SLOTS] = {}, *h_present[SLOTS] = {}, *h_ev[SLOTS] = {}, *h_out[SLOTS] = {};
	uint8_t *d_in[SLOTS] = {}, *d_present[SLOTS] = {}, *d_ev[SLOTS] = {}, *d_out[SLOTS] = {};
	int16_t *d_pcm = nullptr; // plc behind a decoder: the decoded rows the concealer edits
	int32_t *d_evlen = nullptr;
	mi::Roster roster;
	// legs at their own rate (mi_bridge_create_rated); a same-rate bridge has none of it and pitch == len
	bool rated = false;
	int pitch = 0;                 // samples per row of the host buffers: the widest leg's tick
	std::vector<int32_t> leg_rate; // [n], empty: every leg at cfg.rate
	uint8_t *d_ratio = nullptr;
	int16_t *d_hist_in = nullptr, *d_hist_out = nullptr;
	float *d_tab = nullptr;
	int tab_up[7] = {}, tab_down[7] = {};
	int hout_stride = 0, scratch_off = 0, scratch_per_wave = 0;
	// every leg's own codec (mi_bridge_create_legs) where the legs differ: in_bytes / out_bytes are the byte rows' pitch
	std::vector<uint8_t> leg_codec; // [n] in_codec | out_codec << 2; empty: cfg's pair on every leg
	uint8_t *d_codec = nullptr;
	// endpoints on either side of the mix (mi_bridge_create_endpoints) with a leg ABOVE it: bridge_updown_kernel.  d_ratio then
	// carries UD_ABOVE, d_codec is there whether the legs differ or not ([2][n] with plc: the second row names PCM in)
	bool updown = false;
	int wide = 0;                  // samples per LDS row: the widest leg's tick
	int hin_stride = RS_FILT;      // samples per member of d_hist_in
	int tab_down_in[7] = {}, tab_up_out[7] = {};
	// the per-leg concealer (mi_bridge_create_concealed where the legs differ): `plc` is mi_plc_create_legs' and has the
	// decoders; d_pcm [n][pitch] is what it makes of d_in, d_codec is [2][n] as above
	bool leg_plc = false;
	// legs at 3/2 or 2/3 of the mix (mi_bridge_create_rational) where there is one: bridge_rational_kernel.  d_ratio then carries
	// UD_R32, everything else is held as for `updown`: d_codec always there, rows `wide` samples, both histories one stride
	bool rational = false;
	int tab_above_in = 0, tab_above_out = 0, tab_below_in = 0, tab_below_out = 0;
};

namespace {

// the kernels with compile-time codecs, [in kind][out kind] (MI_SESSION_PCM16, MI_SESSION_PCMA, MI_SESSION_PCMU: 0, 1, 2)
#define CODEC_TABLE(K) {{K<0, 0>, K<0, 1>, K<0, 2>}, {K<1, 0>, K<1, 1>, K<1, 2>}, {K<2, 0>, K<2, 1>, K<2, 2>}}
void (*const TICK_KERNELS[3][3])(BridgeArgs) = CODEC_TABLE(bridge_tick_kernel);
void (*const RATED_KERNELS[3][3])(RatedArgs) = CODEC_TABLE(bridge_rated_kernel);
#undef CODEC_TABLE

// a tick's arguments: what a bridge does not have (no resamplers, no codec rows) stays zero and is not read by its kernel
RationalArgs tick_args(const mi_bridge *b, int slot, const void *in, const uint8_t *present) {
	RationalArgs qa = {};
	UpdownArgs &ua = qa.u;
	LegsArgs &la = ua.l;
	RatedArgs &ra = la.r;
	BridgeArgs &a = ra.b;
	VolumeView vv;
	MixerView mv;
	mi_volume_view(b->vol, &vv);
	mi_mixer_view(b->mix, &mv);
	a.in = in, a.present = present, a.out = b->d_out[slot];
	a.params = vv.params, a.state = vv.state, a.win = vv.win;
	a.flags = mv.flags, a.gain = mv.gain;
	a.mm = b->mm, a.ns = b->len, a.row_w = b->row_w, a.nslice = b->nslice, a.sum_off = b->sum_off;
	a.sample_rate = b->cfg.rate;
	ra.ratio = b->d_ratio, ra.hist_in = b->d_hist_in, ra.hist_out = b->d_hist_out, ra.tab = b->d_tab;
	memcpy(ra.tab_up, b->tab_up, sizeof(ra.tab_up));
	memcpy(ra.tab_down, b->tab_down, sizeof(ra.tab_down));
	ra.pitch = b->pitch, ra.hout_stride = b->hout_stride;
	ra.scratch_off = b->scratch_off, ra.scratch_per_wave = b->scratch_per_wave;
	if (b->d_codec) { // behind the concealer every leg's input is the PCM it worked on, at the pitch of its rows
		la.codec = b->plc ? b->d_codec + b->n : b->d_codec;
		la.in_pitch = b->plc ? b->pitch * 2 : (int)b->in_bytes, la.out_pitch = (int)b->out_bytes;
	}
	ua.wide = b->wide, ua.hin_stride = b->hin_stride;
	memcpy(ua.tab_down_in, b->tab_down_in, sizeof(ua.tab_down_in));
	memcpy(ua.tab_up_out, b->tab_up_out, sizeof(ua.tab_up_out));
	qa.tab_above_in = b->tab_above_in, qa.tab_above_out = b->tab_above_out;
	qa.tab_below_in = b->tab_below_in, qa.tab_below_out = b->tab_below_out;
	return qa;
}

int run_tick_kernels(mi_bridge *b, int slot) { // everything on the context's stream
	const mi_bridge_config &cf = b->cfg;
	int rc, in_kind = cf.in_codec;
	const void *in = b->d_in[slot];
	const uint8_t *present = b->d_present[slot];
	if (b->leg_plc) { // every leg's decoder and MSGenericPLC in the concealer's three launches: byte rows in, PCM rows out
		if ((rc = mi_plc_process_legs(b->plc, b->d_in[slot], b->in_bytes, b->d_pcm, (size_t)b->pitch, b->d_ev[slot])) != MI_OK) return rc;
		in = b->d_pcm, present = nullptr; // a concealed leg counts as present
	} else if (b->plc) { // MSAlawDec / MSUlawDec as a launch of its own, then MSGenericPLC on the PCM rows, in place
		int16_t *rows = reinterpret_cast<int16_t *>(b->d_in[slot]);
		if (cf.in_codec) {
			if ((rc = mi_g711_decode(b->ctx, cf.in_codec == MI_SESSION_PCMA ? MI_LAW_PCMA : MI_LAW_PCMU, b->d_in[slot], b->in_bytes, b->d_pcm,
			                         (size_t)b->pitch, nullptr, b->pitch, (size_t)b->n)) != MI_OK)
				return rc;
			rows = b->d_pcm;
		}
		if ((rc = mi_plc_process(b->plc, rows, (size_t)b->pitch, b->d_evlen, b->d_ev[slot])) != MI_OK) return rc;
		in = rows, in_kind = MI_SESSION_PCM16, present = nullptr; // a concealed leg counts as present
	}
	// the widest kernel's arguments, filled once; each kernel is passed the part that is its own
	const RationalArgs qa = tick_args(b, slot, in, present);
	const UpdownArgs &ua = qa.u;
	const LegsArgs &la = ua.l;
	const RatedArgs &ra = la.r;
	auto launch = [&](auto kernel, const auto &args) { hipLaunchKernelGGL(kernel, dim3((unsigned)b->nconf), dim3(BT), b->lds, b->ctx->stream, args); };
	if (b->rational) launch(bridge_rational_kernel, qa);
	else if (b->updown) launch(bridge_updown_kernel, ua);
	else if (b->d_codec) launch(b->rated ? bridge_legs_kernel<true> : bridge_legs_kernel<false>, la);
	else if (b->rated) launch(RATED_KERNELS[in_kind][cf.out_codec], ra);
	else launch(TICK_KERNELS[in_kind][cf.out_codec], ra.b);
	MI_LAUNCH_CHECK();
	return MI_OK;
}

// ---- the resamplers' state, next to the meters' (conference.hpp): a NEW endpoint brings new resamplers, their histories
// zero as speex_resampler_init leaves them.  On the context's stream, behind the ticks submitted.
int reset_resamplers(mi_bridge *b, int first, int count) {
	if (!b->rated || count == 0) return MI_OK;
	if (b->ctx->activate() != MI_OK) return MI_ENODEV;
	MI_HIP(hipMemsetAsync(b->d_hist_in + (size_t)first * b->hin_stride, 0, (size_t)count * b->hin_stride * sizeof(int16_t), b->ctx->stream));
	MI_HIP(hipMemsetAsync(b->d_hist_out + (size_t)first * b->hout_stride, 0, (size_t)count * b->hout_stride * sizeof(int16_t), b->ctx->stream));
	return MI_OK;
}

// the polyphase table of mi_resampler's own design code (quality 3, what msresample.c uses) for in_rate -> out_rate
int design_table(mi_ctx *ctx, int in_rate, int out_rate, std::vector<float> &table) {
	mi_resampler *r = nullptr;
	int rc = mi_resampler_create(ctx, 1, (uint32_t)in_rate, (uint32_t)out_rate, 3, &r);
	if (rc != MI_OK) return rc;
	table.resize((size_t)mi_resampler_get_table(r, nullptr, 0));
	mi_resampler_get_table(r, table.data(), (int)table.size());
	mi_resampler_destroy(r);
	return MI_OK;
}

// one table per distinct ratio and direction, built once: ratio r up [r][48] as designed, down [r][48] phase-major
// (`above`: the ratios of legs above the mix, whose down-sampler is the in_resampler and runs from rate * r)
// (`r32_above`, `r32_below`: a leg at 3/2 or at 2/3 of the mix; their tables [L][24 * M] rearranged into the rows
// rational_run's lanes read, [r * M + p'][k] = table[(r * M) % L][k * M + p'])
int build_tables(mi_bridge *b, const bool (&used)[7], const bool (&above)[7], bool r32_above = false, bool r32_below = false) {
	std::vector<float> all, t;
	auto rational = [&](int in_rate, int out_rate, int L, int M, int *off) {
		const int rc = design_table(b->ctx, in_rate, out_rate, t);
		if (rc != MI_OK) return rc;
		if (t.size() != (size_t)L * M * RQ_FT) return (int)MI_ENOTSUP;
		*off = (int)all.size();
		for (int r = 0; r < L; ++r)
			for (int pp = 0; pp < M; ++pp)
				for (int k = 0; k < RQ_FT; ++k) all.push_back(t[(size_t)((r * M) % L) * RQ_FT * M + (size_t)k * M + pp]);
		return (int)MI_OK;
	};
	const int conf = b->cfg.rate;
	int qrc;
	if (r32_above) {
		if ((qrc = rational(conf / 2 * 3, conf, 2, 3, &b->tab_above_in)) != MI_OK) return qrc;
		if ((qrc = rational(conf, conf / 2 * 3, 3, 2, &b->tab_above_out)) != MI_OK) return qrc;
	}
	if (r32_below) {
		if ((qrc = rational(conf / 3 * 2, conf, 3, 2, &b->tab_below_in)) != MI_OK) return qrc;
		if ((qrc = rational(conf, conf / 3 * 2, 2, 3, &b->tab_below_out)) != MI_OK) return qrc;
	}
	for (int r = 2; r < 7; ++r) {
		int rc;
		if (above[r]) {
			if ((rc = design_table(b->ctx, b->cfg.rate * r, b->cfg.rate, t)) != MI_OK) return rc;
			if (t.size() != (size_t)r * RS_FILT) return MI_ENOTSUP;
			b->tab_down_in[r] = (int)all.size();
			for (int p = 0; p < r; ++p)
				for (int i = 0; i < RS_FILT; ++i) all.push_back(t[(size_t)i * r + p]);
			if ((rc = design_table(b->ctx, b->cfg.rate, b->cfg.rate * r, t)) != MI_OK) return rc;
			if (t.size() != (size_t)r * RS_FILT) return MI_ENOTSUP;
			b->tab_up_out[r] = (int)all.size();
			all.insert(all.end(), t.begin(), t.end());
		}
		if (!used[r]) continue;
		if ((rc = design_table(b->ctx, b->cfg.rate / r, b->cfg.rate, t)) != MI_OK) return rc;
		if (t.size() != (size_t)r * RS_FILT) return MI_ENOTSUP;
		b->tab_up[r] = (int)all.size();
		all.insert(all.end(), t.begin(), t.end());
		if ((rc = design_table(b->ctx, b->cfg.rate, b->cfg.rate / r, t)) != MI_OK) return rc;
		if (t.size() != (size_t)r * RS_FILT) return MI_ENOTSUP;
		b->tab_down[r] = (int)all.size();
		for (int p = 0; p < r; ++p)
			for (int i = 0; i < RS_FILT; ++i) all.push_back(t[(size_t)i * r + p]);
	}
	if (!(b->d_tab = (float *)mi_dev_alloc(b->ctx, all.size() * sizeof(float)))) return MI_ENOMEM;
	MI_HIP(hipMemcpy(b->d_tab, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
	return MI_OK;
}

} // namespace

extern "C" {

void mi_bridge_default_config(mi_bridge_config *c) {
	if (!c) return;
	memset(c, 0, sizeof(*c));
	c->nstreams = 32 * 32;
	c->members_per_conference = 32;
	c->rate = 8000;
	c->in_codec = c->out_codec = MI_SESSION_PCMU;
}

void mi_bridge_destroy(mi_bridge *b) {
	if (!b) return;
	mi_ctx *c = b->ctx;
	(void)c->activate();
	b->pipe.drain();
	for (int i = 0; i < SLOTS; ++i) {
		for (uint8_t *p : {b->h_in[i], b->h_present[i], b->h_ev[i], b->h_out[i]})
			if (p) mi_host_free(c, p);
		for (uint8_t *p : {b->d_in[i], b->d_present[i], b->d_ev[i], b->d_out[i]})
			if (p) mi_dev_free(c, p);
	}
	for (void *p : {(void *)b->d_ratio, (void *)b->d_hist_in, (void *)b->d_hist_out, (void *)b->d_tab, (void *)b->d_codec})
		if (p) mi_dev_free(c, p);
	if (b->d_pcm) mi_dev_free(c, b->d_pcm);
	if (b->d_evlen) mi_dev_free(c, b->d_evlen);
	if (b->plc) mi_plc_destroy(b->plc);
	if (b->vol) mi_volume_destroy(b->vol);
	if (b->mix) mi_mixer_destroy(b->mix);
	b->pipe.destroy();
	delete b;
}

int mi_bridge_create(mi_ctx *ctx, const mi_bridge_config *cfg, mi_bridge **out) { return mi_bridge_create_rated(ctx, cfg, nullptr, out); }

// h_codec [nstreams]: in_codec | out_codec << 2 of legs that differ (mi_bridge_create_legs, which has checked them), or null.
// endpoints: mi_bridge_create_endpoints' rules -- a leg may be above cfg->rate, and h_codec is there whenever one is
// leg_plc: mi_bridge_create_concealed with cfg->plc and legs that differ -- the concealer is the per-leg one (h_codec is there)
// rational: mi_bridge_create_rational with a leg at 3/2 or 2/3 of cfg->rate (endpoints' rules besides; h_codec is there)
static int create_bridge(mi_ctx *ctx, const mi_bridge_config *cfg, const int32_t *h_leg_rate, const uint8_t *h_codec, mi_bridge **out,
                         bool endpoints = false, bool leg_plc = false, bool rational = false) {
	const char *fn = rational ? "mi_bridge_create_rational"
	                 : leg_plc ? "mi_bridge_create_concealed"
	                 : endpoints ? "mi_bridge_create_endpoints"
	                             : "mi_bridge_create_rated";
	MI_CHECK_ARG(ctx && cfg && out);
	*out = nullptr;
	MI_CHECK_ARG(cfg->nstreams > 0 && cfg->members_per_conference > 0 && cfg->members_per_conference <= MI_MIXER_MAX_CHANNELS &&
	             cfg->nstreams % cfg->members_per_conference == 0);
	MI_CHECK_ARG(cfg->rate > 0);
	MI_CHECK_ARG(cfg->in_codec >= MI_SESSION_PCM16 && cfg->in_codec <= MI_SESSION_PCMU && cfg->out_codec >= MI_SESSION_PCM16 &&
	             cfg->out_codec <= MI_SESSION_PCMU);
	if (cfg->rate % 800 != 0) {
		mi::set_error("mi_bridge_create: rate %d is no multiple of 800 (a 10 ms tick must be whole groups of 8 samples)", cfg->rate);
		return MI_ENOTSUP;
	}
	const int len = cfg->rate / 100, mm = cfg->members_per_conference;
	// ---- the legs' rates: every refusal before anything is allocated
	bool used[7] = {}, above[7] = {}; // the ratios of legs below the mix, and of legs above it
	int widest = 0, common = 0, max_ratio = 1;
	bool rated = false, updown = false, r32_above = false, r32_below = false;
	// what holds for a leg of any ratio, checked once that ratio is known to be served: a tick of whole groups, and one rate
	// for the one concealer batch
	auto leg_fits = [&](int s, int lr) {
		if (lr % 800 != 0) {
			mi::set_error("%s: leg %d's rate %d is no multiple of 800 (a 10 ms tick must be whole groups of 8 samples)", fn, s, lr);
			return false;
		}
		if (cfg->plc && !leg_plc && common && lr != common) {
			mi::set_error("%s: plc with legs at %d Hz and %d Hz: the concealer batch has one rate", fn, common, lr);
			return false;
		}
		if (!common) common = lr;
		widest = std::max(widest, lr);
		return true;
	};
	if (h_leg_rate) {
		for (int s = 0; s < cfg->nstreams; ++s) {
			const int lr = h_leg_rate[s];
			MI_CHECK_ARG(lr > 0);
			const bool up = lr > cfg->rate;
			// 3/2 or 2/3, both rates multiples of 800: leg and mix are 2400 k and 1600 k Hz, their ticks 24 k and 16 k samples --
			// 8 k periods of 3 samples against 2: whole periods and whole eight-period tiles, eight-sample groups, both ways
			if (rational && ((int64_t)2 * lr == (int64_t)3 * cfg->rate || (int64_t)3 * lr == (int64_t)2 * cfg->rate)) {
				if (!leg_fits(s, lr)) return MI_ENOTSUP;
				(up ? r32_above : r32_below) = true;
				continue;
			}
			if (up && !endpoints) {
				mi::set_error("mi_bridge_create_rated: leg %d at %d Hz is above its conference's %d Hz (only legs at or below the mix are resampled)",
				              s, lr, cfg->rate);
				return MI_ENOTSUP;
			}
			const int hi = up ? lr : cfg->rate, lo = up ? cfg->rate : lr;
			if (hi % lo != 0) {
				mi::set_error("%s: leg %d at %d Hz in a %d Hz conference is no whole ratio (%.3f); supported: 1, 2, 3, 6%s", fn, s, lr, cfg->rate,
				              (double)hi / lo, rational ? ", and 3/2 either way" : "");
				return MI_ENOTSUP;
			}
			const int r = hi / lo;
			if (r != 1 && r != 2 && r != 3 && r != 6) {
				mi::set_error("%s: leg %d at %d Hz in a %d Hz conference is ratio %d; supported: 1, 2, 3, 6%s", fn, s, lr, cfg->rate, r,
				              rational ? ", and 3/2 either way" : "");
				return MI_ENOTSUP;
			}
			if (!leg_fits(s, lr)) return MI_ENOTSUP;
			(up ? above : used)[r] = true;
			updown |= up;
			max_ratio = std::max(max_ratio, r);
		}
		rated = max_ratio > 1 || r32_above || r32_below;
	}
	rational = r32_above || r32_below; // without such a leg: mi_bridge_create_concealed's bridge exactly
	// samples per row in LDS: the widest leg's tick where one is above the mix
	const int wide = updown ? widest / 100 : rational ? std::max(len, widest / 100) : len;
	const int row_w = (wide >> 2) | 1;             // 8-byte words per row, odd
	const size_t sum_off = mi::round_up((size_t)mm * row_w * 8, 16);
	size_t lds = sum_off + (size_t)len * 4, scratch_off = 0, scratch = 0;
	if (rated) {
		for (int r = 2; r < 7; ++r) {
			// each wavefront's scratch: the larger of the forms per used ratio -- up-sampler and down-sampler of a leg below the
			// mix (in front of the pin, behind it), down-sampler and up-sampler of a leg above it
			size_t up = 0, down = 0;
			if (used[r]) {
				up = (size_t)((RS_FILT - 1 + len / r + RS_R + 1 + 3) & ~3) * 4;
				down = ((size_t)r * rated_plen(r, len) + (size_t)len) * 4;
			}
			if (above[r]) {
				up = std::max(up, (size_t)((RS_FILT - 1 + len + RS_R + 1 + 3) & ~3) * 4);
				down = std::max(down, ((size_t)r * updown_plen(r, r * len) + (size_t)r * len) * 4);
			}
			scratch = std::max(scratch, mi::round_up(std::max(up, down), 16));
		}
		// a leg at 3/2 of the mix: x 2/3 from its tick in front of the pin, x 3/2 from the mix's behind it; one at 2/3: x 3/2 from
		// its tick, x 2/3 from the mix's
		if (r32_above) scratch = std::max(scratch, std::max(rational_scratch(3, len / 2 * 3), rational_scratch(2, len)));
		if (r32_below) scratch = std::max(scratch, std::max(rational_scratch(2, len / 3 * 2), rational_scratch(3, len)));
		scratch_off = mi::round_up(lds, 16);
		lds = scratch_off + (BT / 64) * scratch;
		if (lds + RATED_STATIC_LDS > BRIDGE_LDS_MAX) {
			mi::set_error("%s: a conference's tick and its resamplers' scratch must fit %zu bytes of LDS (%d members x %d samples "
			              "= %zu, + %d wavefronts x %zu for ratio %d%s, + %zu of the kernel's own: %zu)",
			              fn, BRIDGE_LDS_MAX, mm, wide, scratch_off, BT / 64, scratch, max_ratio, rational ? " and 3/2" : "", RATED_STATIC_LDS,
			              lds + RATED_STATIC_LDS);
			return MI_ENOTSUP;
		}
	} else if (lds > BRIDGE_LDS_MAX) {
		mi::set_error("mi_bridge_create: a conference's tick must fit %zu bytes of LDS (%d members x %d samples need %zu)", BRIDGE_LDS_MAX, mm,
		              len, lds);
		return MI_ENOTSUP;
	}
	const int pitch = rated ? widest / 100 : len;
	size_t in_bytes = (size_t)pitch * (cfg->in_codec ? 1 : 2), out_bytes = (size_t)pitch * (cfg->out_codec ? 1 : 2);
	if (h_codec) { // byte rows: the widest leg's tick in bytes, rounded up to the 16 bytes a lane loads
		in_bytes = out_bytes = 0;
		for (int s = 0; s < cfg->nstreams; ++s) {
			const size_t ll = (size_t)(h_leg_rate ? h_leg_rate[s] : cfg->rate) / 100;
			in_bytes = std::max(in_bytes, ll * ((h_codec[s] & 3) ? 1 : 2));
			out_bytes = std::max(out_bytes, ll * ((h_codec[s] >> 2) ? 1 : 2));
		}
		in_bytes = mi::round_up(in_bytes, 16), out_bytes = mi::round_up(out_bytes, 16);
	}
	if (ctx->activate() != MI_OK) return MI_ENODEV;
	mi_bridge *b = new mi_bridge();
	b->ctx = b->pipe.ctx = ctx;
	b->cfg = *cfg;
	b->n = cfg->nstreams;
	b->mm = mm;
	b->nconf = cfg->nstreams / mm;
	b->len = len;
	b->row_w = row_w;
	b->sum_off = (int)sum_off;
	b->lds = lds;
	b->nslice = std::max(1, std::min(mm, BT / (len >> 2)));
	b->rated = rated, b->pitch = pitch;
	b->updown = updown, b->wide = wide;
	b->rational = rational;
	b->in_bytes = in_bytes, b->out_bytes = out_bytes;
	if (h_leg_rate) b->leg_rate.assign(h_leg_rate, h_leg_rate + cfg->nstreams);
	b->roster.init(b->n, mm);
	int rc = MI_OK;
	auto fail = [&](int code) {
		mi_bridge_destroy(b);
		return code;
	};
	if ((rc = mi_volume_create(ctx, b->n, cfg->rate, &b->vol)) != MI_OK) return fail(rc);
	if ((rc = mi_mixer_create(ctx, b->nconf, mm, len, &b->mix)) != MI_OK) return fail(rc);
	if ((rc = b->pipe.create(ctx, SLOTS)) != MI_OK) return fail(rc);
	const size_t n = (size_t)b->n;
	for (int i = 0; i < SLOTS; ++i) {
		b->h_in[i] = (uint8_t *)mi_host_alloc(ctx, n * b->in_bytes);
		b->h_present[i] = (uint8_t *)mi_host_alloc(ctx, n);
		b->h_out[i] = (uint8_t *)mi_host_alloc(ctx, n * b->out_bytes);
		b->d_in[i] = (uint8_t *)mi_dev_alloc(ctx, n * b->in_bytes);
		b->d_present[i] = (uint8_t *)mi_dev_alloc(ctx, n);
		b->d_out[i] = (uint8_t *)mi_dev_alloc(ctx, n * b->out_bytes);
		if (!b->h_in[i] || !b->h_present[i] || !b->h_out[i] || !b->d_in[i] || !b->d_present[i] || !b->d_out[i]) return fail(MI_ENOMEM);
		// rows of pins whose output is off are never written: they read as zeros
		MI_HIP(hipMemsetAsync(b->d_out[i], 0, n * b->out_bytes, ctx->stream));
		memset(b->h_out[i], 0, n * b->out_bytes);
	}
	if (rated) {
		b->scratch_off = (int)scratch_off, b->scratch_per_wave = (int)scratch;
		b->hout_stride = max_ratio * RS_FILT; // mi_resampler's round_up(filt_len - 1, 8) of the longest filter
		if (rational) b->hout_stride = std::max(b->hout_stride, 3 * RQ_FT); // x 2/3 keeps 71 samples (x 3/2: 47)
		if (updown || rational) b->hin_stride = b->hout_stride; // a down-sampler's history on either side of the pin
		std::vector<uint8_t> ratio(n);
		for (size_t s = 0; s < n; ++s) {
			const int lr = h_leg_rate[s];
			ratio[s] = lr > cfg->rate ? (uint8_t)(UD_ABOVE | (unsigned)(lr / cfg->rate)) : (uint8_t)(cfg->rate / lr);
			if ((int64_t)2 * lr == (int64_t)3 * cfg->rate || (int64_t)3 * lr == (int64_t)2 * cfg->rate) ratio[s] |= UD_R32; // (the whole part: 1)
		}
		b->d_ratio = (uint8_t *)mi_dev_alloc(ctx, n);
		b->d_hist_in = (int16_t *)mi_dev_alloc(ctx, n * b->hin_stride * sizeof(int16_t));
		b->d_hist_out = (int16_t *)mi_dev_alloc(ctx, n * b->hout_stride * sizeof(int16_t));
		if (!b->d_ratio || !b->d_hist_in || !b->d_hist_out) return fail(MI_ENOMEM);
		if (hipMemcpy(b->d_ratio, ratio.data(), n, hipMemcpyHostToDevice) != hipSuccess) return fail(MI_ENODEV);
		if ((rc = reset_resamplers(b, 0, b->n)) != MI_OK) return fail(rc);
		if ((rc = build_tables(b, used, above, r32_above, r32_below)) != MI_OK) return fail(rc);
	}
	if (h_codec) {
		b->leg_codec.assign(h_codec, h_codec + n);
		if (cfg->plc) // (one pair on every leg) a second row for the kernel behind the concealer, whose input is PCM
			for (size_t s = 0; s < n; ++s) b->leg_codec.push_back((uint8_t)(h_codec[s] & ~3u));
		if (!(b->d_codec = (uint8_t *)mi_dev_alloc(ctx, b->leg_codec.size()))) return fail(MI_ENOMEM);
		if (hipMemcpy(b->d_codec, b->leg_codec.data(), b->leg_codec.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(MI_ENODEV);
		b->leg_codec.resize(n);
	}
	if (cfg->plc) {
		if (leg_plc) { // at every leg's own rate behind its own decoder, into PCM rows of `pitch` samples
			std::vector<uint8_t> kind(n);
			for (size_t s = 0; s < n; ++s) kind[s] = h_codec[s] & 3;
			b->leg_plc = true;
			if ((rc = mi_plc_create_legs(ctx, b->n, h_leg_rate, kind.data(), pitch, &b->plc)) != MI_OK) return fail(rc);
			if (!(b->d_pcm = (int16_t *)mi_dev_alloc(ctx, n * pitch * 2))) return fail(MI_ENOMEM);
			if (hipMemsetAsync(b->d_pcm, 0, n * pitch * 2, ctx->stream) != hipSuccess) return fail(MI_ENODEV);
		} else { // at the legs' one rate, on rows of the host buffers' pitch
			if ((rc = mi_plc_create(ctx, b->n, rated ? common : cfg->rate, pitch, &b->plc)) != MI_OK) return fail(rc);
			std::vector<int32_t> lens(n, pitch);
			if (!(b->d_evlen = (int32_t *)mi_dev_alloc(ctx, n * 4))) return fail(MI_ENOMEM);
			if (hipMemcpy(b->d_evlen, lens.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(MI_ENODEV);
			if (cfg->in_codec && !(b->d_pcm = (int16_t *)mi_dev_alloc(ctx, n * pitch * 2))) return fail(MI_ENOMEM);
		}
		for (int i = 0; i < SLOTS; ++i) {
			b->h_ev[i] = (uint8_t *)mi_host_alloc(ctx, n);
			b->d_ev[i] = (uint8_t *)mi_dev_alloc(ctx, n);
			if (!b->h_ev[i] || !b->d_ev[i]) return fail(MI_ENOMEM);
		}
	}
	if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(MI_ENODEV);
	*out = b;
	return MI_OK;
}

int mi_bridge_create_rated(mi_ctx *ctx, const mi_bridge_config *cfg, const int32_t *h_leg_rate, mi_bridge **out) {
	return create_bridge(ctx, cfg, h_leg_rate, nullptr, out);
}

// mi_bridge_create_legs and mi_bridge_create_endpoints: the legs' codecs checked, then create_bridge with the first's rules on
// rates or the second's.  concealed: mi_bridge_create_concealed -- the second's rules, and cfg->plc with legs that differ is
// served by the per-leg concealer instead of refused.  rational: mi_bridge_create_rational -- the third's rules, and a leg may
// be at 3/2 or 2/3 of cfg->rate
static int create_from_legs(const char *fn, bool endpoints, mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs,
                            mi_bridge **out, bool concealed = false, bool rational = false) {
	if (!h_legs) return mi_bridge_create(ctx, cfg, out);
	MI_CHECK_ARG(ctx && cfg && out);
	*out = nullptr;
	MI_CHECK_ARG(cfg->nstreams > 0);
	const size_t n = (size_t)cfg->nstreams;
	std::vector<int32_t> rate(n);
	std::vector<uint8_t> codec(n);
	int differs = -1; // the first leg whose pair is not leg 0's
	bool above = false;
	for (size_t s = 0; s < n; ++s) {
		const mi_bridge_leg &l = h_legs[s];
		for (int v : {l.in_codec, l.out_codec})
			if (v < MI_SESSION_PCM16 || v > MI_SESSION_PCMU) {
				mi::set_error("%s: leg %zu names codec %d; supported: MI_SESSION_PCM16 (0), MI_SESSION_PCMA (1), "
				              "MI_SESSION_PCMU (2)", fn, s, v);
				return MI_ENOTSUP;
			}
		rate[s] = l.rate;
		codec[s] = (uint8_t)(l.in_codec | l.out_codec << 2);
		if (differs < 0 && codec[s] != codec[0]) differs = (int)s;
		above |= l.rate > cfg->rate;
		// (such a leg brings the codecs as data and byte rows, as one above the mix does)
		if (rational) above |= (int64_t)3 * l.rate == (int64_t)2 * cfg->rate;
	}
	if (concealed && cfg->plc) {
		bool one_rate = true;
		for (size_t s = 0; s < n; ++s) { // what the concealer cannot serve, before anything is allocated
			const int rc = mi_plc_check_rate(fn, "leg", (int)s, rate[s]);
			if (rc != MI_OK) return rc;
			one_rate &= rate[s] == rate[0];
		}
		if (differs >= 0 || !one_rate) {
			mi_bridge_config c = *cfg; // (its pair is not read: the codecs are the kernel's data)
			c.in_codec = h_legs[0].in_codec, c.out_codec = h_legs[0].out_codec;
			return create_bridge(ctx, &c, rate.data(), codec.data(), out, true, true, rational);
		}
	}
	if (differs >= 0 && cfg->plc) {
		mi::set_error("%s: plc with leg %d's codecs (in %d, out %d) unlike leg 0's (in %d, out %d): the concealer batch "
		              "sits behind one decoder", fn, differs, h_legs[differs].in_codec, h_legs[differs].out_codec, h_legs[0].in_codec,
		              h_legs[0].out_codec);
		return MI_ENOTSUP;
	}
	mi_bridge_config c = *cfg; // a uniform bridge is mi_bridge_create_rated's, its one pair compile-time in the kernels
	c.in_codec = h_legs[0].in_codec, c.out_codec = h_legs[0].out_codec;
	// with a leg above the mix (endpoints; create_bridge refuses it otherwise) the codecs are the kernel's data whether they
	// differ or not, and the host rows byte rows
	return create_bridge(ctx, &c, rate.data(), differs >= 0 || (endpoints && above) ? codec.data() : nullptr, out, endpoints, false, rational);
}

int mi_bridge_create_legs(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, mi_bridge **out) {
	return create_from_legs("mi_bridge_create_legs", false, ctx, cfg, h_legs, out);
}

int mi_bridge_create_endpoints(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, mi_bridge **out) {
	return create_from_legs("mi_bridge_create_endpoints", true, ctx, cfg, h_legs, out);
}

int mi_bridge_create_concealed(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, mi_bridge **out) {
	return create_from_legs("mi_bridge_create_concealed", true, ctx, cfg, h_legs, out, true);
}

int mi_bridge_create_rational(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, mi_bridge **out) {
	return create_from_legs("mi_bridge_create_rational", true, ctx, cfg, h_legs, out, true, true);
}

int mi_bridge_leg_codec(const mi_bridge *b, int stream, int *in_codec, int *out_codec) {
	if (!b || stream < 0 || stream >= b->n) return MI_EINVAL;
	const int pair = b->leg_codec.empty() ? b->cfg.in_codec | b->cfg.out_codec << 2 : b->leg_codec[(size_t)stream];
	if (in_codec) *in_codec = pair & 3;
	if (out_codec) *out_codec = pair >> 2;
	return MI_OK;
}

int mi_bridge_leg_bytes(const mi_bridge *b, int stream, int *in_bytes, int *out_bytes) {
	int in_codec, out_codec;
	if (mi_bridge_leg_codec(b, stream, &in_codec, &out_codec) != MI_OK) return MI_EINVAL;
	const int len = mi_bridge_leg_rate(b, stream) / 100;
	if (in_bytes) *in_bytes = len * (in_codec ? 1 : 2);
	if (out_bytes) *out_bytes = len * (out_codec ? 1 : 2);
	return MI_OK;
}

int mi_bridge_leg_rate(const mi_bridge *b, int stream) {
	if (!b || stream < 0 || stream >= b->n) return MI_EINVAL;
	return b->leg_rate.empty() ? b->cfg.rate : b->leg_rate[(size_t)stream];
}

int mi_bridge_tick_bytes(const mi_bridge *b, int *in_bytes, int *out_bytes) {
	MI_CHECK_ARG(b != nullptr);
	if (in_bytes) *in_bytes = (int)b->in_bytes;
	if (out_bytes) *out_bytes = (int)b->out_bytes;
	return MI_OK;
}

int mi_bridge_acquire(mi_bridge *b, void **h_in, uint8_t **h_present) {
	MI_CHECK_ARG(b && h_in && h_present);
	int slot;
	// the slot's previous upload must have been consumed by its kernels before the host overwrites the staging
	const int rc = b->pipe.acquire(mi::TickPipe::CONSUMED, &slot);
	if (rc == mi::TickPipe::FULL) mi::set_error("all %d ticks in flight: collect one first", SLOTS);
	if (rc != MI_OK) return rc;
	*h_in = b->h_in[slot];
	*h_present = b->h_present[slot];
	memset(b->h_present[slot], 1, (size_t)b->n);
	return MI_OK;
}

int mi_bridge_submit(mi_bridge *b) {
	MI_CHECK_ARG(b != nullptr);
	if (!b->pipe.acquired) {
		mi::set_error("mi_bridge_submit without mi_bridge_acquire");
		return MI_EINVAL;
	}
	const size_t n = (size_t)b->n;
	return b->pipe.submit(
	    [&](int slot) {
		    MI_HIP(hipMemcpyAsync(b->d_in[slot], b->h_in[slot], n * b->in_bytes, hipMemcpyHostToDevice, b->pipe.s_up));
		    if (b->plc) { // an absent leg is the concealer's to fill
			    for (size_t i = 0; i < n; ++i) b->h_ev[slot][i] = b->h_present[slot][i] ? MI_PLC_RECEIVED : MI_PLC_CONCEAL;
			    MI_HIP(hipMemcpyAsync(b->d_ev[slot], b->h_ev[slot], n, hipMemcpyHostToDevice, b->pipe.s_up));
		    } else {
			    MI_HIP(hipMemcpyAsync(b->d_present[slot], b->h_present[slot], n, hipMemcpyHostToDevice, b->pipe.s_up));
		    }
		    return MI_OK;
	    },
	    [&](int slot) { return run_tick_kernels(b, slot); },
	    [&](int slot) {
		    MI_HIP(hipMemcpyAsync(b->h_out[slot], b->d_out[slot], n * b->out_bytes, hipMemcpyDeviceToHost, b->pipe.s_down));
		    return MI_OK;
	    });
}

int mi_bridge_collect(mi_bridge *b, const void **h_out) {
	MI_CHECK_ARG(b && h_out);
	int slot;
	const int rc = b->pipe.collect(&slot);
	if (rc == mi::TickPipe::EMPTY) mi::set_error("nothing in flight");
	if (rc != MI_OK) return rc;
	*h_out = b->h_out[slot];
	return MI_OK;
}

int mi_bridge_in_flight(const mi_bridge *b) { return b ? b->pipe.in_flight() : 0; }

// ---- control plane, as mi_session's (session.hip).  The mixer's and the meter's setters wait for the ticks submitted.
int mi_bridge_set_controls(mi_bridge *b, const uint8_t *h_flags, const float *h_gain) {
	MI_CHECK_ARG(b && (h_flags || h_gain));
	if (h_flags) b->roster.set_flags(h_flags);
	return mi_mixer_set_controls(b->mix, h_flags, h_gain); // [nconf][members] == [nstreams]
}

int mi_bridge_set_volume_params(mi_bridge *b, int first, int count, const mi_volume_params *h_params) {
	MI_CHECK_ARG(b && h_params && first >= 0 && count >= 0 && first + count <= b->n);
	for (int i = 0; i < count; ++i)
		if (h_params[i].peer != -1) {
			mi::set_error("mi_bridge_set_volume_params: stream %d names an echo-limiter peer (%d); a bridge has no far end to limit against",
			              first + i, h_params[i].peer);
			return MI_ENOTSUP;
		}
	return mi_volume_set_params(b->vol, first, count, h_params);
}

int mi_bridge_reset_streams(mi_bridge *b, int first, int count) {
	MI_CHECK_ARG(b && first >= 0 && count >= 0 && first + count <= b->n);
	if (count == 0) return MI_OK;
	int rc;
	if ((rc = mi::reset_meters(b->vol, first, count)) != MI_OK) return rc;
	if (b->plc && (rc = mi_plc_reset(b->plc, first, count)) != MI_OK) return rc;
	return reset_resamplers(b, first, count);
}

int mi_bridge_add_member(mi_bridge *b, int stream) {
	MI_CHECK_ARG(b && stream >= 0 && stream < b->n);
	if (b->roster.is_member(stream)) {
		mi::set_error("mi_bridge_add_member: stream %d is a member already", stream);
		return MI_EINVAL;
	}
	const int rc = mi_bridge_reset_streams(b, stream, 1);
	if (rc != MI_OK) return rc;
	b->roster.join(stream);
	return mi_mixer_set_controls(b->mix, b->roster.flags.data(), nullptr);
}

int mi_bridge_remove_member(mi_bridge *b, int stream) {
	MI_CHECK_ARG(b && stream >= 0 && stream < b->n);
	if (!b->roster.leave(stream)) {
		mi::set_error("mi_bridge_remove_member: stream %d is no member", stream);
		return MI_EINVAL;
	}
	const int rc = mi_mixer_set_controls(b->mix, b->roster.flags.data(), nullptr);
	if (rc != MI_OK) return rc;
	if (b->ctx->activate() != MI_OK) return MI_ENODEV;
	// an unplumbed pin's row is left alone from now on: what the departed leg last heard must not linger in the buffers
	MI_HIP(hipStreamSynchronize(b->ctx->stream));
	MI_HIP(hipStreamSynchronize(b->pipe.s_down));
	for (int i = 0; i < SLOTS; ++i) {
		MI_HIP(hipMemsetAsync(b->d_out[i] + (size_t)stream * b->out_bytes, 0, b->out_bytes, b->ctx->stream));
		memset(b->h_out[i] + (size_t)stream * b->out_bytes, 0, b->out_bytes);
	}
	return MI_OK;
}

int mi_bridge_member_count(const mi_bridge *b, int conference) {
	if (!b || conference < 0 || conference >= b->nconf) return MI_EINVAL;
	return b->roster.count(conference);
}

int mi_bridge_get_levels(mi_bridge *b, float *h_linear) {
	MI_CHECK_ARG(b && h_linear);
	return mi::get_levels(b->vol, b->n, h_linear);
}

int mi_bridge_active_speakers(mi_bridge *b, uint64_t now_ms, int32_t *h_winner, float *h_max_db) {
	MI_CHECK_ARG(b && h_winner);
	(void)now_ms; // not read (mi::active_speakers)
	return mi::active_speakers(b->vol, b->roster, h_winner, h_max_db);
}

int mi_bridge_get_volume_state(mi_bridge *b, int first, int count, mi_volume_state *h_state) {
	MI_CHECK_ARG(b != nullptr);
	return mi_volume_get_state(b->vol, first, count, h_state);
}

int mi_bridge_get_volume_max(mi_bridge *b, int first, int count, float *h_max) {
	MI_CHECK_ARG(b != nullptr);
	return mi_volume_get_max(b->vol, first, count, h_max);
}

} // extern "C"

// (mi_warmup, ctx.hip: this unit's code object is loaded when the library is, not under a tick's first launch)
static const mi::WarmEntry g_warm_bridge(reinterpret_cast<const void *>(&bridge_tick_kernel<2, 2>));
