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
// compile-time codecs or per-leg ones, no resamplers, those of legs below the mix, above it, at 3/2 and 2/3 of it.  A sixth,
// for legs at 4, 1/4 and a : b of the mix (mi_bridge_create_ratios), is a unit of its own: bridge_ratios.hip; so is the seventh,
// for legs at 44 100 Hz (mi_bridge_create_offgrid): bridge_offgrid.hip.
//
// Geometry: an 8 kHz conference of 32 is 5.4 KB of LDS and four waves, so eight such workgroups share a CU (32 waves);
// 1000 conferences are 1000 workgroups dealt over the 256 CUs, about four per CU = one wave per SIMD and conference
// phase, every conference resident at once.  48 kHz x 50 members is 50 KB: three per CU.  HBM traffic per 8 kHz G.711
// leg-tick: 80 B in, 80 B out, + 130 B of meter parameters / state / window.
// Membership, controls and reports -- waiting or carried by the ticks -- are mi::ConferencePlane's (controls.hpp); here is what
// is the bridge's own: launch_seats, a JOIN's kind, reset_streams, set_volume_params' peer check, the rows cleared, two read-outs.
#include "common.hpp"

#include "bridge_phases.hpp"
#include "bridge_roster.hpp"
#include "controls.hpp"
#include "resample_tables.hpp"

#pragma clang fp contract(off)

static_assert(PLAN_MAX_RATE_CLASSES == PLC_MAX_CLASSES, "the plan refuses what the concealer cannot hold");

// bridge_ratios.hip: bridge_ratios_kernel on `nconf` workgroups; args: a RatiosArgs, as bytes
int mi_bridge_ratios_launch(const void *args, size_t bytes, int nconf, size_t lds, hipStream_t stream);
// bridge_offgrid.hip: bridge_offgrid_kernel likewise; args: an OffgridArgs
int mi_bridge_offgrid_launch(const void *args, size_t bytes, int nconf, size_t lds, hipStream_t stream);

namespace {

constexpr int SLOTS = 3; // upload | compute | download can each hold a different tick

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

// The host side is plan / build / tick: plan_bridge (bridge_plan.hpp, no HIP in it) decides everything from the configuration
// or refuses; build_bridge allocates what the plan says and fills the kernels' arguments; a tick sets three pointers and
// launches the plan's kernel family.
struct mi_bridge {
	mi_ctx *ctx = nullptr;
	Plan plan;              // what creation decided: geometry, family, the legs' rates, codecs and ratio bytes
	OffgridArgs args = {};  // the widest kernel's arguments, filled at creation (fill_args, build_tables) but for in, present, out
	mi_volume *vol = nullptr; // the meters: parameters, state, one-second windows
	mi_mixer *mix = nullptr;  // the pins' controls
	mi_plc *plc = nullptr;    // plan.leg_plc: mi_plc_create_legs', with the decoders; else mi_plc_create's at the legs' one rate
	mi::TickPipe pipe;
	uint8_t *h_in[SLOTS] = {}, *h_present[SLOTS] = {}, *h_ev[SLOTS] = {}, *h_out[SLOTS] = {};
	uint8_t *d_in[SLOTS] = {}, *d_present[SLOTS] = {}, *d_ev[SLOTS] = {}, *d_out[SLOTS] = {};
	int16_t *d_pcm = nullptr; // plc behind a decoder: the decoded rows [n][pitch] the concealer edits
	int32_t *d_evlen = nullptr;
	// with resamplers (plan.rated): the ratio bytes, both histories at the plan's strides, every table back to back
	uint8_t *d_ratio = nullptr;
	int16_t *d_hist_in = nullptr, *d_hist_out = nullptr;
	float *d_tab = nullptr;
	int2 *d_gen = nullptr; // plan.generic: RatiosArgs::gen_tab
	uint8_t *d_codec = nullptr; // the codecs as data ([n]; [2][n] with plc: the second row names PCM in, behind the concealer)
	// conference membership, controls and reports, the waiting calls' and what travels with the ticks: controls.hpp
	mi::ConferencePlane conf;
};

namespace {

// the kernels with compile-time codecs, [in kind][out kind] (MI_SESSION_PCM16, MI_SESSION_PCMA, MI_SESSION_PCMU: 0, 1, 2)
#define CODEC_TABLE(K) {{K<0, 0>, K<0, 1>, K<0, 2>}, {K<1, 0>, K<1, 1>, K<1, 2>}, {K<2, 0>, K<2, 1>, K<2, 2>}}
void (*const TICK_KERNELS[3][3])(BridgeArgs) = CODEC_TABLE(bridge_tick_kernel);
void (*const RATED_KERNELS[3][3])(RatedArgs) = CODEC_TABLE(bridge_rated_kernel);
#undef CODEC_TABLE

// every argument that holds from creation on; what a bridge does not have (no resamplers, no codec rows) stays zero and is not
// read by its kernel.  The meters' and the pins' pointers are among them: mi_volume_view and mi_mixer_view hand out arrays that
// mi_volume_create / mi_mixer_create allocate and only their destroy frees; no setter reallocates them.
void fill_args(mi_bridge *b) {
	const Plan &pl = b->plan;
	LegsArgs &la = b->args.g.q.u.l;
	RatedArgs &ra = la.r;
	BridgeArgs &a = ra.b;
	VolumeView vv;
	MixerView mv;
	mi_volume_view(b->vol, &vv);
	mi_mixer_view(b->mix, &mv);
	a.params = vv.params, a.state = vv.state, a.win = vv.win;
	a.flags = mv.flags, a.gain = mv.gain;
	a.mm = pl.mm, a.ns = pl.len, a.row_w = pl.row_w, a.nslice = pl.nslice, a.sum_off = pl.sum_off, a.sample_rate = pl.cfg.rate;
	ra.ratio = b->d_ratio, ra.hist_in = b->d_hist_in, ra.hist_out = b->d_hist_out, ra.tab = b->d_tab;
	ra.pitch = pl.pitch, ra.hout_stride = pl.hout_stride, ra.scratch_off = pl.scratch_off, ra.scratch_per_wave = pl.scratch_per_wave;
	if (b->d_codec) { // behind the concealer every leg's input is the PCM it worked on, at the pitch of its rows
		la.codec = b->plc ? b->d_codec + pl.n : b->d_codec;
		la.in_pitch = b->plc ? pl.pcm_pitch() * 2 : (int)pl.in_bytes, la.out_pitch = (int)pl.out_bytes;
	}
	b->args.g.q.u.wide = pl.wide, b->args.g.q.u.hin_stride = pl.hin_stride;
	b->args.g.gen_tab = b->d_gen;
	b->args.num = pl.off_num, b->args.den = pl.off_den, b->args.filt_in = pl.off_fin, b->args.filt_out = pl.off_fout;
}

// a tick that carries membership changes: the bridge's own state in one launch (mi::ConferencePlane::apply's seat_launch)
int launch_seats(mi_bridge *b, int slot, const mi_seat_cmd *d_cmd, int count) {
	const Plan &pl = b->plan;
	RosterArgs ra = {};
	ra.cmd = d_cmd, ra.count = count, ra.nstreams = pl.n;
	ra.ratio = b->d_ratio, ra.codec = b->d_codec, ra.codec_pcm = b->d_codec && b->plc ? b->d_codec + pl.n : nullptr;
	MixerEdit me;
	mi_volume_edit(b->vol, &ra.vol);
	mi_mixer_edit(b->mix, &me);
	ra.flags = me.flags;
	ra.hist_in = b->d_hist_in, ra.hist_out = b->d_hist_out, ra.hin_stride = pl.hin_stride, ra.hout_stride = pl.hout_stride;
	ra.out = b->d_out[slot], ra.out_bytes = (int)pl.out_bytes;
	return mi_bridge_roster_launch(ra, b->ctx->stream);
}

int run_tick_kernels(mi_bridge *b, int slot) { // everything on the context's stream
	const Plan &pl = b->plan;
	const mi_bridge_config &cf = pl.cfg;
	int rc, in_kind = cf.in_codec;
	OffgridArgs oa = b->args; // each kernel is passed the part that is its own
	RatiosArgs &ga = oa.g;
	RationalArgs &qa = ga.q;
	BridgeArgs &a = qa.u.l.r.b;
	a.in = b->d_in[slot], a.present = b->d_present[slot], a.out = b->d_out[slot];
	if (pl.leg_plc) { // every leg's decoder and MSGenericPLC in the concealer's three launches: byte rows in, PCM rows out
		if ((rc = mi_plc_process_legs(b->plc, b->d_in[slot], pl.in_bytes, b->d_pcm, (size_t)pl.pcm_pitch(), b->d_ev[slot])) != MI_OK) return rc;
		a.in = b->d_pcm, a.present = nullptr; // a concealed leg counts as present
	} else if (b->plc) { // MSAlawDec / MSUlawDec as a launch of its own, then MSGenericPLC on the PCM rows, in place
		int16_t *rows = reinterpret_cast<int16_t *>(b->d_in[slot]);
		if (cf.in_codec) {
			if ((rc = mi_g711_decode(b->ctx, cf.in_codec == MI_SESSION_PCMA ? MI_LAW_PCMA : MI_LAW_PCMU, b->d_in[slot], pl.in_bytes, b->d_pcm,
			                         (size_t)pl.pitch, nullptr, pl.pitch, (size_t)pl.n)) != MI_OK)
				return rc;
			rows = b->d_pcm;
		}
		if ((rc = mi_plc_process(b->plc, rows, (size_t)pl.pitch, b->d_evlen, b->d_ev[slot])) != MI_OK) return rc;
		a.in = rows, in_kind = MI_SESSION_PCM16, a.present = nullptr; // a concealed leg counts as present
	}
	auto launch = [&](auto kernel, const auto &args) { hipLaunchKernelGGL(kernel, dim3((unsigned)pl.nconf), dim3(BT), pl.lds, b->ctx->stream, args); };
	switch (pl.family) {
	case Plan::OFFGRID: return mi_bridge_offgrid_launch(&oa, sizeof(oa), pl.nconf, pl.lds, b->ctx->stream);
	case Plan::RATIOS: return mi_bridge_ratios_launch(&ga, sizeof(ga), pl.nconf, pl.lds, b->ctx->stream);
	case Plan::RATIONAL: launch(bridge_rational_kernel, qa); break;
	case Plan::UPDOWN: launch(bridge_updown_kernel, qa.u); break;
	case Plan::LEGS_RATED: launch(bridge_legs_kernel<true>, qa.u.l); break;
	case Plan::LEGS: launch(bridge_legs_kernel<false>, qa.u.l); break;
	case Plan::RATED: launch(RATED_KERNELS[in_kind][cf.out_codec], qa.u.l.r); break;
	case Plan::TICK: launch(TICK_KERNELS[in_kind][cf.out_codec], a); break;
	}
	MI_LAUNCH_CHECK();
	return MI_OK;
}

// ---- the resamplers' state, next to the meters' (conference.hpp): a NEW endpoint brings new resamplers, their histories
// zero as speex_resampler_init leaves them.  On the context's stream, behind the ticks submitted.
int reset_resamplers(mi_bridge *b, int first, int count) {
	const Plan &pl = b->plan;
	if (!pl.rated || count == 0) return MI_OK;
	if (b->ctx->activate() != MI_OK) return MI_ENODEV;
	MI_HIP(hipMemsetAsync(b->d_hist_in + (size_t)first * pl.hin_stride, 0, (size_t)count * pl.hin_stride * sizeof(int16_t), b->ctx->stream));
	MI_HIP(hipMemsetAsync(b->d_hist_out + (size_t)first * pl.hout_stride, 0, (size_t)count * pl.hout_stride * sizeof(int16_t), b->ctx->stream));
	return MI_OK;
}

// (design_table, the polyphase table of mi_resampler's own design code: resample_tables.hpp)
// one table per distinct ratio and direction, built once and back to back in d_tab, its float offset noted in b->args.  A table
// is designed as [L][taps] polyphase rows for in_rate : out_rate = M : L and laid out as its reader wants it: AS_DESIGNED, an
// up-sampler by r: [r][48]; PHASE_MAJOR, a down-sampler by r: tap r * i + p at [p][i]; REARRANGED, x 3/2 and x 2/3: [L][24 * M]
// into the rows rational_run's lanes read, [r * M + p'][k] = table[(r * M) % L][k * M + p'].  size: the floats mi_resampler
// designs; anything else is a design this unit was not written for.  A leg at a : b (generic_run) reads both its tables
// AS_DESIGNED, [L][filt_len]: filt_len is the plan's (filter_rule), and mi_resampler_info must agree with it and call the table
// direct -- the plan accepted the leg on that rule alone
enum Layout { AS_DESIGNED, PHASE_MAJOR, REARRANGED };
struct Table { int in_rate, out_rate; size_t size; Layout layout; int *offset; int filt_len = 0; };

int build_tables(mi_bridge *b) {
	const Plan &pl = b->plan;
	UpdownArgs &ua = b->args.g.q.u;
	RationalArgs &qa = b->args.g.q;
	RatedArgs &ra = ua.l.r;
	const int conf = pl.cfg.rate;
	std::vector<Table> want;
	if (pl.r32_above) { // the in_resampler's, then the out_resampler's
		want.push_back({conf / 2 * 3, conf, 6 * RQ_FT, REARRANGED, &qa.tab_above_in});
		want.push_back({conf, conf / 2 * 3, 6 * RQ_FT, REARRANGED, &qa.tab_above_out});
	}
	if (pl.r32_below) {
		want.push_back({conf / 3 * 2, conf, 6 * RQ_FT, REARRANGED, &qa.tab_below_in});
		want.push_back({conf, conf / 3 * 2, 6 * RQ_FT, REARRANGED, &qa.tab_below_out});
	}
	for (int r = 2; r < 7; ++r) {
		const size_t size = (size_t)r * RS_FILT;
		if (pl.above[r]) { // (whose down-sampler is the in_resampler and runs from rate * r)
			want.push_back({conf * r, conf, size, PHASE_MAJOR, &ua.tab_down_in[r]});
			want.push_back({conf, conf * r, size, AS_DESIGNED, &ua.tab_up_out[r]});
		}
		if (pl.used[r]) {
			want.push_back({conf / r, conf, size, AS_DESIGNED, &ra.tab_up[r]});
			want.push_back({conf, conf / r, size, PHASE_MAJOR, &ra.tab_down[r]});
		}
	}
	std::vector<int2> gen(64, make_int2(0, 0));
	for (const uint8_t rb : pl.generic) { // conf = cb * unit, the leg's rate la * unit
		const int la = gen_a(rb), cb = gen_b(rb), unit = conf / cb, fin = filter_rule(la, cb).filt_len, fout = filter_rule(cb, la).filt_len;
		want.push_back({la * unit, conf, (size_t)cb * fin, AS_DESIGNED, &gen[(size_t)gen_code(rb)].x, fin});
		want.push_back({conf, la * unit, (size_t)la * fout, AS_DESIGNED, &gen[(size_t)gen_code(rb)].y, fout});
	}
	std::vector<float> all, t;
	for (const Table &w : want) {
		int filt_len = 0, direct = 0;
		const int rc = design_table(b->ctx, w.in_rate, w.out_rate, t, &filt_len, &direct);
		if (rc != MI_OK) return rc;
		if (w.filt_len && (filt_len != w.filt_len || !direct)) {
			mi::set_error("mi_bridge: the plan's filter for %d -> %d Hz (%d taps, direct) is not mi_resampler's (%d taps, %s): "
			              "filter_rule (bridge_plan.hpp) and design_filter (resample.hip) disagree",
			              w.in_rate, w.out_rate, w.filt_len, filt_len, direct ? "direct" : "interpolated");
			return MI_ENOTSUP;
		}
		if (t.size() != w.size) return MI_ENOTSUP;
		*w.offset = (int)all.size();
		const int g = std::min(w.in_rate, w.out_rate) / (w.layout == REARRANGED ? 2 : 1); // the rates are M * g and L * g
		const int L = w.out_rate / g, M = w.in_rate / g;
		if (w.layout == AS_DESIGNED) all.insert(all.end(), t.begin(), t.end());
		else if (w.layout == PHASE_MAJOR) append_phase_major(all, t, M, RS_FILT);
		else
			for (int r = 0; r < L; ++r)
				for (int pp = 0; pp < M; ++pp)
					for (int k = 0; k < RQ_FT; ++k) all.push_back(t[(size_t)((r * M) % L) * RQ_FT * M + (size_t)k * M + pp]);
	}
	if (pl.offgrid) { // the 44 100 Hz legs' pair: the PER-PHASE tables mi_resampler's generic kernel reads, [rows][taps], on 16 bytes
		const struct { int in_rate, out_rate, rows, taps, *offset; } pair[2] = {{OFFGRID_RATE, conf, pl.off_den, pl.off_fin, &b->args.tab_in},
		                                                                        {conf, OFFGRID_RATE, pl.off_num, pl.off_fout, &b->args.tab_out}};
		for (const auto &w : pair) {
			mi_resampler *r = nullptr;
			int rc = mi_resampler_create(b->ctx, 1, (uint32_t)w.in_rate, (uint32_t)w.out_rate, 3, &r), filt_len = 0;
			if (rc != MI_OK) return rc;
			t.resize((size_t)mi_resampler_get_phase_table(r, nullptr, 0));
			mi_resampler_get_phase_table(r, t.data(), (int)t.size());
			rc = mi_resampler_info(r, &filt_len, nullptr, nullptr, nullptr);
			mi_resampler_destroy(r);
			if (rc != MI_OK) return rc;
			if (filt_len != w.taps || t.size() != (size_t)w.rows * w.taps) {
				mi::set_error("mi_bridge: the plan's filter for %d -> %d Hz (%d rows of %d taps) is not mi_resampler's per-phase table (%zu floats, "
				              "%d taps): filter_rule (bridge_plan.hpp) and design_filter (resample.hip) disagree",
				              w.in_rate, w.out_rate, w.rows, w.taps, t.size(), filt_len);
				return MI_ENOTSUP;
			}
			all.resize((all.size() + 3) & ~(size_t)3, 0.f);
			*w.offset = (int)all.size();
			all.insert(all.end(), t.begin(), t.end());
		}
	}
	if (!(b->d_tab = (float *)mi_dev_alloc(b->ctx, all.size() * sizeof(float)))) return MI_ENOMEM;
	MI_HIP(hipMemcpy(b->d_tab, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
	if (pl.generic.empty()) return MI_OK;
	if (!(b->d_gen = (int2 *)mi_dev_alloc(b->ctx, gen.size() * sizeof(int2)))) return MI_ENOMEM;
	MI_HIP(hipMemcpy(b->d_gen, gen.data(), gen.size() * sizeof(int2), hipMemcpyHostToDevice));
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
	b->conf.destroy();
	void *const rest[] = {b->d_ratio, b->d_hist_in, b->d_hist_out, b->d_tab, b->d_gen, b->d_codec, b->d_pcm, b->d_evlen};
	for (void *p : rest)
		if (p) mi_dev_free(c, p);
	if (b->plc) mi_plc_destroy(b->plc);
	if (b->vol) mi_volume_destroy(b->vol);
	if (b->mix) mi_mixer_destroy(b->mix);
	b->pipe.destroy();
	delete b;
}

// allocation only: everything is sized by the plan, which has refused what cannot be served
static int build_bridge(mi_ctx *ctx, Plan &plan, mi_bridge **out) {
	if (ctx->activate() != MI_OK) return MI_ENODEV;
	mi_bridge *b = new mi_bridge();
	b->ctx = b->pipe.ctx = ctx;
	b->plan = std::move(plan);
	const Plan &pl = b->plan;
	const size_t n = (size_t)pl.n;
	int rc = MI_OK;
	auto fail = [&](int code) { return mi_bridge_destroy(b), code; };
	if ((rc = mi_volume_create(ctx, pl.n, pl.cfg.rate, &b->vol)) != MI_OK) return fail(rc);
	if ((rc = mi_mixer_create(ctx, pl.nconf, pl.mm, pl.len, &b->mix)) != MI_OK) return fail(rc);
	if ((rc = b->pipe.create(ctx, SLOTS)) != MI_OK) return fail(rc);
	for (int i = 0; i < SLOTS; ++i) {
		b->h_in[i] = (uint8_t *)mi_host_alloc(ctx, n * pl.in_bytes);
		b->h_present[i] = (uint8_t *)mi_host_alloc(ctx, n);
		b->h_out[i] = (uint8_t *)mi_host_alloc(ctx, n * pl.out_bytes);
		b->d_in[i] = (uint8_t *)mi_dev_alloc(ctx, n * pl.in_bytes);
		b->d_present[i] = (uint8_t *)mi_dev_alloc(ctx, n);
		b->d_out[i] = (uint8_t *)mi_dev_alloc(ctx, n * pl.out_bytes);
		if (!b->h_in[i] || !b->h_present[i] || !b->h_out[i] || !b->d_in[i] || !b->d_present[i] || !b->d_out[i]) return fail(MI_ENOMEM);
		if (pl.cfg.plc) b->h_ev[i] = (uint8_t *)mi_host_alloc(ctx, n), b->d_ev[i] = (uint8_t *)mi_dev_alloc(ctx, n);
		if (pl.cfg.plc && (!b->h_ev[i] || !b->d_ev[i])) return fail(MI_ENOMEM);
		// rows of pins whose output is off are never written: they read as zeros
		MI_HIP(hipMemsetAsync(b->d_out[i], 0, n * pl.out_bytes, ctx->stream));
		memset(b->h_out[i], 0, n * pl.out_bytes);
	}
	if (pl.rated) {
		b->d_ratio = (uint8_t *)mi_dev_alloc(ctx, n);
		b->d_hist_in = (int16_t *)mi_dev_alloc(ctx, n * pl.hin_stride * sizeof(int16_t));
		b->d_hist_out = (int16_t *)mi_dev_alloc(ctx, n * pl.hout_stride * sizeof(int16_t));
		if (!b->d_ratio || !b->d_hist_in || !b->d_hist_out) return fail(MI_ENOMEM);
		if (hipMemcpy(b->d_ratio, pl.ratio.data(), n, hipMemcpyHostToDevice) != hipSuccess) return fail(MI_ENODEV);
		if ((rc = reset_resamplers(b, 0, pl.n)) != MI_OK) return fail(rc);
		if ((rc = build_tables(b)) != MI_OK) return fail(rc);
	}
	if (pl.data) {
		std::vector<uint8_t> rows = pl.leg_codec;
		if (pl.cfg.plc) // (one pair on every leg) a second row for the kernel behind the concealer, whose input is PCM
			for (size_t s = 0; s < n; ++s) rows.push_back((uint8_t)(pl.leg_codec[s] & ~3u));
		if (!(b->d_codec = (uint8_t *)mi_dev_alloc(ctx, rows.size()))) return fail(MI_ENOMEM);
		if (hipMemcpy(b->d_codec, rows.data(), rows.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(MI_ENODEV);
	}
	if (pl.cfg.plc) {
		if (pl.leg_plc) { // at every leg's own rate behind its own decoder, into PCM rows of `pitch` samples
			std::vector<uint8_t> kind(n);
			for (size_t s = 0; s < n; ++s) kind[s] = pl.leg_codec[s] & 3;
			std::vector<int32_t> open; // an open bridge: a rate class for every kind that may come
			for (const mi_bridge_leg &k : pl.kinds)
				if (std::find(open.begin(), open.end(), k.rate) == open.end()) open.push_back(k.rate);
			if ((rc = mi_plc_create_legs(ctx, pl.n, pl.leg_rate.data(), kind.data(), pl.pcm_pitch(), &b->plc, open.data(), (int)open.size())) != MI_OK)
				return fail(rc);
			if (!(b->d_pcm = (int16_t *)mi_dev_alloc(ctx, n * pl.pcm_pitch() * 2))) return fail(MI_ENOMEM);
			if (hipMemsetAsync(b->d_pcm, 0, n * pl.pcm_pitch() * 2, ctx->stream) != hipSuccess) return fail(MI_ENODEV);
		} else { // at the legs' one rate, on rows of the host buffers' pitch
			if ((rc = mi_plc_create(ctx, pl.n, pl.rated ? pl.common : pl.cfg.rate, pl.pitch, &b->plc)) != MI_OK) return fail(rc);
			std::vector<int32_t> lens(n, pl.pitch);
			if (!(b->d_evlen = (int32_t *)mi_dev_alloc(ctx, n * 4))) return fail(MI_ENOMEM);
			if (hipMemcpy(b->d_evlen, lens.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(MI_ENODEV);
			if (pl.cfg.in_codec && !(b->d_pcm = (int16_t *)mi_dev_alloc(ctx, n * pl.pitch * 2))) return fail(MI_ENOMEM);
		}
	}
	mi_volume_params defaults;
	mi_volume_default_params(&defaults); // mi_volume_create's
	if ((rc = b->conf.create(ctx, pl.n, pl.mm, SLOTS, &defaults, b->vol, b->mix, b->plc)) != MI_OK) return fail(rc);
	fill_args(b);
	if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(MI_ENODEV);
	*out = b;
	return MI_OK;
}

// every public constructor: its rules' plan, then the build (legs null: rates or nothing, and no rule about codecs is read)
static int create(const Rules &rules, mi_ctx *ctx, const mi_bridge_config *cfg, const int32_t *rates, const mi_bridge_leg *legs, mi_bridge **out) {
	MI_CHECK_ARG(ctx && cfg && out);
	*out = nullptr;
	Plan plan;
	const int rc = legs ? plan_legs(rules, cfg, legs, &plan) : plan_bridge(rules, cfg, rates, nullptr, &plan);
	return rc != MI_OK ? rc : build_bridge(ctx, plan, out);
}

int mi_bridge_create(mi_ctx *ctx, const mi_bridge_config *cfg, mi_bridge **out) { return create(RULES_RATED, ctx, cfg, nullptr, nullptr, out); }

int mi_bridge_create_rated(mi_ctx *ctx, const mi_bridge_config *cfg, const int32_t *h_leg_rate, mi_bridge **out) {
	return create(RULES_RATED, ctx, cfg, h_leg_rate, nullptr, out);
}
int mi_bridge_create_legs(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, mi_bridge **out) {
	return create(RULES_LEGS, ctx, cfg, nullptr, h_legs, out);
}
int mi_bridge_create_endpoints(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, mi_bridge **out) {
	return create(RULES_ENDPOINTS, ctx, cfg, nullptr, h_legs, out);
}
int mi_bridge_create_concealed(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, mi_bridge **out) {
	return create(RULES_CONCEALED, ctx, cfg, nullptr, h_legs, out);
}
int mi_bridge_create_rational(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, mi_bridge **out) {
	return create(RULES_RATIONAL, ctx, cfg, nullptr, h_legs, out);
}
int mi_bridge_create_ratios(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, mi_bridge **out) {
	return create(RULES_RATIOS, ctx, cfg, nullptr, h_legs, out);
}
int mi_bridge_create_open(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, const mi_bridge_leg *h_admit, int nadmit,
                          mi_bridge **out) {
	MI_CHECK_ARG(ctx && cfg && h_legs && out && nadmit >= 0 && (h_admit || nadmit == 0));
	*out = nullptr;
	Plan plan;
	const int rc = plan_open(RULES_RATIOS, cfg, h_legs, h_admit, nadmit, &plan);
	return rc != MI_OK ? rc : build_bridge(ctx, plan, out);
}

int mi_bridge_create_offgrid(mi_ctx *ctx, const mi_bridge_config *cfg, const mi_bridge_leg *h_legs, const mi_bridge_leg *h_admit, int nadmit,
                             mi_bridge **out) {
	MI_CHECK_ARG(ctx && cfg && h_legs && out && nadmit >= 0 && (h_admit || nadmit == 0));
	*out = nullptr;
	Plan plan;
	const int rc = plan_open(RULES_OFFGRID, cfg, h_legs, h_admit, nadmit, &plan);
	return rc != MI_OK ? rc : build_bridge(ctx, plan, out);
}

int mi_bridge_leg_codec(const mi_bridge *b, int stream, int *in_codec, int *out_codec) {
	if (!b || stream < 0 || stream >= b->plan.n) return MI_EINVAL;
	const int pair = b->plan.leg_codec.empty() ? b->plan.cfg.in_codec | b->plan.cfg.out_codec << 2 : b->plan.leg_codec[(size_t)stream];
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
	if (!b || stream < 0 || stream >= b->plan.n) return MI_EINVAL;
	return b->plan.leg_rate.empty() ? b->plan.cfg.rate : b->plan.leg_rate[(size_t)stream];
}

int mi_bridge_tick_bytes(const mi_bridge *b, int *in_bytes, int *out_bytes) {
	MI_CHECK_ARG(b != nullptr);
	if (in_bytes) *in_bytes = (int)b->plan.in_bytes;
	if (out_bytes) *out_bytes = (int)b->plan.out_bytes;
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
	memset(b->h_present[slot], 1, (size_t)b->plan.n);
	return MI_OK;
}

int mi_bridge_submit(mi_bridge *b) {
	MI_CHECK_ARG(b != nullptr);
	if (!b->pipe.acquired) {
		mi::set_error("mi_bridge_submit without mi_bridge_acquire");
		return MI_EINVAL;
	}
	const size_t n = (size_t)b->plan.n;
	b->conf.stage(b->pipe.next_slot(), b->pipe.submitted);
	const int rc = b->pipe.submit(
	    [&](int slot) {
		    if (b->conf.upload(slot, b->pipe.s_up) != MI_OK) return (int)MI_ENODEV;
		    MI_HIP(hipMemcpyAsync(b->d_in[slot], b->h_in[slot], n * b->plan.in_bytes, hipMemcpyHostToDevice, b->pipe.s_up));
		    if (b->plc) { // an absent leg is the concealer's to fill
			    for (size_t i = 0; i < n; ++i) b->h_ev[slot][i] = b->h_present[slot][i] ? MI_PLC_RECEIVED : MI_PLC_CONCEAL;
			    MI_HIP(hipMemcpyAsync(b->d_ev[slot], b->h_ev[slot], n, hipMemcpyHostToDevice, b->pipe.s_up));
		    } else {
			    MI_HIP(hipMemcpyAsync(b->d_present[slot], b->h_present[slot], n, hipMemcpyHostToDevice, b->pipe.s_up));
		    }
		    return MI_OK;
	    },
	    [&](int slot) {
		    int rc = b->conf.apply(slot, [&](const mi_seat_cmd *d_cmd, int count) { return launch_seats(b, slot, d_cmd, count); });
		    if (rc != MI_OK || (rc = run_tick_kernels(b, slot)) != MI_OK) return rc;
		    return b->conf.report(slot);
	    },
	    [&](int slot) {
		    MI_HIP(hipMemcpyAsync(b->h_out[slot], b->d_out[slot], n * b->plan.out_bytes, hipMemcpyDeviceToHost, b->pipe.s_down));
		    return b->conf.download(slot, b->pipe.s_down);
	    });
	if (rc == MI_OK) b->conf.submitted();
	return rc;
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

// ---- conference control plane: every call's body is mi::ConferencePlane's (controls.hpp), the bridge brings what is its own
int mi_bridge_set_controls(mi_bridge *b, const uint8_t *h_flags, const float *h_gain) {
	MI_CHECK_ARG(b && (h_flags || h_gain));
	return b->conf.set_controls(h_flags, h_gain);
}

int mi_bridge_set_volume_params(mi_bridge *b, int first, int count, const mi_volume_params *h_params) {
	MI_CHECK_ARG(b && h_params && first >= 0 && count >= 0 && first + count <= b->plan.n);
	for (int i = 0; i < count; ++i)
		if (h_params[i].peer != -1) {
			mi::set_error("mi_bridge_set_volume_params: stream %d names an echo-limiter peer (%d); a bridge has no far end to limit against",
			              first + i, h_params[i].peer);
			return MI_ENOTSUP;
		}
	b->conf.book.set_params(first, count, h_params);
	return mi_volume_set_params(b->vol, first, count, h_params);
}

int mi_bridge_reset_streams(mi_bridge *b, int first, int count) {
	MI_CHECK_ARG(b && first >= 0 && count >= 0 && first + count <= b->plan.n);
	if (count == 0) return MI_OK;
	int rc;
	if ((rc = mi::reset_meters(b->vol, first, count)) != MI_OK) return rc;
	if (b->plc && (rc = mi_plc_reset(b->plc, first, count)) != MI_OK) return rc;
	return reset_resamplers(b, first, count);
}

int mi_bridge_add_member(mi_bridge *b, int stream) {
	MI_CHECK_ARG(b && stream >= 0 && stream < b->plan.n);
	return b->conf.add_member("mi_bridge_add_member", stream, [&](int seat) { return mi_bridge_reset_streams(b, seat, 1); });
}

int mi_bridge_remove_member(mi_bridge *b, int stream) {
	MI_CHECK_ARG(b && stream >= 0 && stream < b->plan.n);
	return b->conf.remove_member("mi_bridge_remove_member", stream, b->pipe, [&](int seat) -> int {
		for (int i = 0; i < SLOTS; ++i) {
			MI_HIP(hipMemsetAsync(b->d_out[i] + (size_t)seat * b->plan.out_bytes, 0, b->plan.out_bytes, b->ctx->stream));
			memset(b->h_out[i] + (size_t)seat * b->plan.out_bytes, 0, b->plan.out_bytes);
		}
		return MI_OK;
	});
}

// no stream, event or device synchronise and no blocking copy on this path: the book and the plan's per-seat vectors answer at
// once, the device follows with the next tick submitted (mi::ConferenceBook; mi::ConferencePlane::stage, ::apply)
int mi_bridge_change_members(mi_bridge *b, const mi_bridge_change *h_changes, int count) {
	MI_CHECK_ARG(b && count >= 0 && (h_changes || count == 0));
	Plan &pl = b->plan;
	mi::ConferenceBook &book = b->conf.book;
	std::vector<uint8_t> ratio;
	int rc = check_changes(pl, book.roster.flags.data(), h_changes, count, &ratio, &book.controls.scratch);
	if (rc != MI_OK) return rc;
	std::vector<uint8_t> cls((size_t)count, 0); // every JOIN's rate class in the concealer, before anything is applied
	for (int i = 0; b->plc && i < count; ++i) {
		if (h_changes[i].op != MI_BRIDGE_JOIN) continue;
		if ((rc = mi_plc_class_of(b->plc, h_changes[i].stream, h_changes[i].leg.rate)) < 0) return rc;
		cls[(size_t)i] = (uint8_t)rc;
	}
	for (int i = 0; i < count; ++i) {
		const mi_bridge_change &c = h_changes[i];
		const size_t s = (size_t)c.stream;
		mi::SeatChanges::Pending &p = book.change_member(c.stream, c.op == MI_BRIDGE_LEAVE ? MI_SEAT_LEAVE : MI_SEAT_JOIN);
		if (c.op == MI_BRIDGE_LEAVE) continue;
		p.ratio = ratio[(size_t)i], p.codec = (uint8_t)(c.leg.in_codec | c.leg.out_codec << 2), p.len = c.leg.rate / 100;
		p.cls = cls[(size_t)i];
		if (b->plc) mi_plc_seat(b->plc, c.stream, p.cls, c.leg.in_codec);
		if (!pl.leg_rate.empty()) pl.leg_rate[s] = c.leg.rate;
		if (!pl.leg_codec.empty()) pl.leg_codec[s] = p.codec;
		if (!pl.ratio.empty()) pl.ratio[s] = p.ratio;
	}
	return MI_OK;
}

int mi_bridge_change_controls(mi_bridge *b, const mi_bridge_control *h_changes, int count) {
	const char *fn = "mi_bridge_change_controls";
	if (!b) return mi::set_error("%s: a null bridge", fn), (int)MI_EINVAL;
	return b->conf.book.change_controls(fn, h_changes, count);
}

int mi_bridge_set_reports(mi_bridge *b, uint32_t what) {
	if (!b) return mi::set_error("mi_bridge_set_reports: a null bridge"), (int)MI_EINVAL;
	return b->conf.set_reports("mi_bridge_set_reports", what);
}

int mi_bridge_collected_report(mi_bridge *b, mi_bridge_report *out) {
	if (!b || !out) return mi::set_error("mi_bridge_collected_report: a null %s", b ? "report" : "bridge"), (int)MI_EINVAL;
	return b->conf.collected("mi_bridge_collected_report", b->pipe.collected, out);
}

int mi_bridge_member_count(const mi_bridge *b, int conference) { return b ? b->conf.book.member_count(conference) : (int)MI_EINVAL; }

// (a seat joined since the last submit still reads as its previous occupant's meter in these two: DESIGN.md 5.0a)

int mi_bridge_get_levels(mi_bridge *b, float *h_linear) {
	MI_CHECK_ARG(b && h_linear);
	return mi::get_levels(b->vol, b->plan.n, h_linear);
}

int mi_bridge_active_speakers(mi_bridge *b, uint64_t now_ms, int32_t *h_winner, float *h_max_db) {
	MI_CHECK_ARG(b && h_winner);
	(void)now_ms; // not read (mi::active_speakers)
	return mi::active_speakers(b->vol, b->conf.book.roster, h_winner, h_max_db);
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
