// bridge.hip -- mi_bridge (include/msmi355x_bridge.h): a conference server's member chain
//   decoder -> MSVolume (level / meter) -> MSAudioMixer pin -> encoder      (src/voip/audioconference.c:209-257)
// for a batch of conferences, a conference's whole 10 ms tick in ONE launch, fed from host buffers like mi_session
// (session.hip): three slots of pinned staging, upload / kernel / download on three HIP streams (mi::TickPipe,
// tick_pipe.hpp), up to three ticks in flight.  No echo canceller -- that is the endpoint's.  Built with
// -ffp-contract=off like volume.hip: MSVolume's control chain is float32 evaluated unfused in source order, and every
// output sample depends on it bit for bit.
//
// bridge_tick_kernel<IN, OUT>: one workgroup of 256 lanes = one conference; the members' ticks live in LDS as packed
// int16 rows whose pitch is an odd number of 8-byte words (volmix_kernel's layout, volume.hip), so the lanes that walk
// one row each in the serial meter read disjoint banks.
//   (0) lane m < members: its MSVolume parameters, state and window, its mixer controls, its `present` byte;
//   (A) eight lanes per member (32 members a round): the rows into LDS -- 16 bytes of PCM, or 8 code words decoded
//       with codec.hip's arithmetic (g711.hpp), per lane and group, four groups in flight --, integer peak and DC sum
//       reduced over the eight lanes in registers.  An absent member's row is zeros (audiomixer.c:88);
//   (B) lane m: the float32 sum of squares IN SAMPLE ORDER (the order is part of the reference's result) and the
//       control chain (volume_control, volume_ctl.hpp); state and one-second window written back.  An absent member
//       is skipped whole: MSVolume got no chunk (msvolume.c:480-486, what MI_VOLMIX_DRY_SKIPS does in volmix_kernel);
//   (C) lane = (member slice, four columns): the Q12 gain (apply_gain), then the pin's contribution as
//       channel_process_in leaves it (0 unless linked and active; input gain) back into the row, and the int32 sum
//       over the slice's members added into the conference's sum row in LDS (integer addition: any order);
//   (D) lane = (member, eight columns), for every pin with its output enabled: saturate(sum - own)
//       (channel_process_out), stored as 16 bytes of PCM or encoded to 8 code words; consecutive lanes, consecutive bytes.
// The members are sliced in (C) so that an 80-sample tick, 20 four-column words wide, still occupies 240 lanes.
//
// Geometry: an 8 kHz conference of 32 is 5.4 KB of LDS and four waves, so eight such workgroups share a CU (32 waves);
// 1000 conferences are 1000 workgroups dealt over the 256 CUs, about four per CU = one wave per SIMD and conference
// phase, every conference resident at once.  48 kHz x 50 members is 50 KB: three per CU.  HBM traffic per 8 kHz G.711
// leg-tick: 80 B in, 80 B out, + 130 B of meter parameters / state / window.
#include "common.hpp"
#include "conference.hpp"
#include "g711.hpp"
#include "tick_pipe.hpp"
#include "volume_ctl.hpp"

#include "../../include/msmi355x_bridge.h"

#pragma clang fp contract(off)

namespace {

constexpr int SLOTS = 3; // upload | compute | download can each hold a different tick
constexpr int BT = 256, BMAX = MI_MIXER_MAX_CHANNELS;
constexpr size_t BRIDGE_LDS_MAX = 64 * 1024;

struct BridgeArgs {
	const void *in;         // [nconf * mm][ns] uint8 code words or int16
	const uint8_t *present; // [nconf * mm], or null: every member present
	void *out;              // [nconf * mm][ns]
	const mi_volume_params *params;
	mi_volume_state *state;
	float2 *win;
	const uint8_t *flags; // mixer controls [nconf][mm]
	const float *gain;
	int mm, ns, row_w; // members per conference, samples per tick, row pitch in 8-byte words (odd)
	int nslice;        // member slices of (C)
	int sum_off;       // byte offset of the sum row in the dynamic LDS
	int sample_rate;
};

// eight samples of member row `row`, group g, as packed PCM.  KIND 0: 16-bit PCM, 1: A-law, 2: mu-law
template <int KIND>
__device__ __forceinline__ uint4 load_group(const void *in, size_t row, int ns, int g) {
	if (KIND == 0) return *reinterpret_cast<const uint4 *>(static_cast<const int16_t *>(in) + row * ns + 8 * g);
	const uint2 c = *reinterpret_cast<const uint2 *>(static_cast<const uint8_t *>(in) + row * ns + 8 * g);
	const uint32_t w[2] = {c.x, c.y};
	uint32_t o[4];
#pragma unroll
	for (int k = 0; k < 2; ++k) {
		const uint32_t lo = __builtin_amdgcn_perm(0u, w[k], 0x0c010c00u); // bytes 0,1 -> the two halves
		const uint32_t hi = __builtin_amdgcn_perm(0u, w[k], 0x0c030c02u); // bytes 2,3
		o[2 * k] = KIND == 2 ? ulaw2lin_x2(lo) : alaw2lin_x2(lo);
		o[2 * k + 1] = KIND == 2 ? ulaw2lin_x2(hi) : alaw2lin_x2(hi);
	}
	return make_uint4(o[0], o[1], o[2], o[3]);
}

__device__ __forceinline__ int lo16(unsigned w) { return (int)(short)(w & 0xffffu); }
__device__ __forceinline__ int hi16(unsigned w) { return (int)(short)(w >> 16); }
__device__ __forceinline__ unsigned pack16(int lo, int hi) { return (unsigned)(lo & 0xffff) | ((unsigned)hi << 16); }

template <int IN, int OUT>
__global__ __launch_bounds__(BT) void bridge_tick_kernel(BridgeArgs a) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	uint2 *rows = reinterpret_cast<uint2 *>(smem);           // [mm][row_w] four samples per word
	int *s_sum = reinterpret_cast<int *>(smem + a.sum_off); // [ns] the conference's int32 sum
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX]; // what (C) and (D) need of a member: (flags | mode << 8, Q12 gain, DC offset, pin gain)
	const int t = threadIdx.x, c = blockIdx.x, mm = a.mm, ns = a.ns, nw = ns >> 2, ng = ns >> 3;
	const int s0 = c * mm;

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
					for (int k = 0; k < 4; ++k) { // update_energy's integer part (msvolume.c:393-399): |x| up to 32768
						const int x0 = lo16(w[k]), x1 = hi16(w[k]);
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
			float acc = 0; // the same additions in the same order as update_energy's loop
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

	// ---- (C)
	for (int item = t; item < a.nslice * nw; item += BT) {
		const int r = item / nw, j = item - r * nw;
		int sum[4] = {0, 0, 0, 0};
		for (int m = r; m < mm; m += a.nslice) {
			const int4 par = s_par[m];
			const unsigned f = (unsigned)par.x & 0xffu;
			uint2 o = make_uint2(0, 0);
			if ((f & MI_MIX_LINKED) && (f & MI_MIX_ACTIVE)) {
				const uint2 cur = rows[m * a.row_w + j];
				int x[4] = {lo16(cur.x), hi16(cur.x), lo16(cur.y), hi16(cur.y)};
				const int mode = par.x >> 8;
				if (mode != 0) { // apply_gain (msvolume.c:440: a gain of exactly 1 leaves the samples alone)
					const int ig = par.y, dc = (mode == 2) ? par.z : 0;
#pragma unroll
					for (int k = 0; k < 4; ++k) x[k] = sat16(((x[k] - dc) * ig) / 4096);
				}
				const float gn = __int_as_float(par.w);
				if (gn != 1.0f) { // channel_process_in's input gain (audiomixer.c:46-51)
#pragma unroll
					for (int k = 0; k < 4; ++k) x[k] = sat16((int)(gn * (float)x[k]));
				}
#pragma unroll
				for (int k = 0; k < 4; ++k) sum[k] += x[k];
				o = make_uint2(pack16(x[0], x[1]), pack16(x[2], x[3]));
			}
			rows[m * a.row_w + j] = o;
		}
#pragma unroll
		for (int k = 0; k < 4; ++k) atomicAdd(&s_sum[4 * j + k], sum[k]);
	}
	__syncthreads();

	// ---- (D)
	for (int item = t; item < mm * ng; item += BT) {
		const int m = item / ng, g = item - m * ng;
		if (!((unsigned)s_par[m].x & MI_MIX_OUTPUT)) continue;
		const uint2 own0 = rows[m * a.row_w + 2 * g], own1 = rows[m * a.row_w + 2 * g + 1];
		const int4 sa = *reinterpret_cast<const int4 *>(s_sum + 8 * g), sb = *reinterpret_cast<const int4 *>(s_sum + 8 * g + 4);
		const int o[8] = {sat16(sa.x - lo16(own0.x)), sat16(sa.y - hi16(own0.x)), sat16(sa.z - lo16(own0.y)), sat16(sa.w - hi16(own0.y)),
		                  sat16(sb.x - lo16(own1.x)), sat16(sb.y - hi16(own1.x)), sat16(sb.z - lo16(own1.y)), sat16(sb.w - hi16(own1.y))};
		const size_t at = (size_t)(s0 + m) * ns + 8 * g;
		if (OUT == 0) {
			*reinterpret_cast<uint4 *>(static_cast<int16_t *>(a.out) + at) =
			    make_uint4(pack16(o[0], o[1]), pack16(o[2], o[3]), pack16(o[4], o[5]), pack16(o[6], o[7]));
		} else {
			uint32_t cw[2] = {0, 0};
#pragma unroll
			for (int k = 0; k < 8; ++k) cw[k >> 2] |= (OUT == 2 ? lin2ulaw(o[k]) : lin2alaw(o[k])) << (8 * (k & 3));
			*reinterpret_cast<uint2 *>(static_cast<uint8_t *>(a.out) + at) = make_uint2(cw[0], cw[1]);
		}
	}
}

template <int IN>
void launch_out(int out_kind, dim3 grid, size_t lds, hipStream_t st, const BridgeArgs &a) {
	if (out_kind == MI_SESSION_PCM16) hipLaunchKernelGGL((bridge_tick_kernel<IN, 0>), grid, dim3(BT), lds, st, a);
	else if (out_kind == MI_SESSION_PCMA) hipLaunchKernelGGL((bridge_tick_kernel<IN, 1>), grid, dim3(BT), lds, st, a);
	else hipLaunchKernelGGL((bridge_tick_kernel<IN, 2>), grid, dim3(BT), lds, st, a);
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
};

namespace {

int run_tick_kernels(mi_bridge *b, int slot) { // everything on the context's stream
	const mi_bridge_config &cf = b->cfg;
	int rc, in_kind = cf.in_codec;
	const void *in = b->d_in[slot];
	const uint8_t *present = b->d_present[slot];
	if (b->plc) { // MSAlawDec / MSUlawDec as a launch of its own, then MSGenericPLC on the PCM rows, in place
		int16_t *rows = reinterpret_cast<int16_t *>(b->d_in[slot]);
		if (cf.in_codec) {
			if ((rc = mi_g711_decode(b->ctx, cf.in_codec == MI_SESSION_PCMA ? MI_LAW_PCMA : MI_LAW_PCMU, b->d_in[slot], (size_t)b->len, b->d_pcm,
			                         (size_t)b->len, nullptr, b->len, (size_t)b->n)) != MI_OK)
				return rc;
			rows = b->d_pcm;
		}
		if ((rc = mi_plc_process(b->plc, rows, (size_t)b->len, b->d_evlen, b->d_ev[slot])) != MI_OK) return rc;
		in = rows, in_kind = MI_SESSION_PCM16, present = nullptr; // a concealed leg counts as present
	}
	VolumeView vv;
	MixerView mv;
	mi_volume_view(b->vol, &vv);
	mi_mixer_view(b->mix, &mv);
	BridgeArgs a;
	a.in = in, a.present = present, a.out = b->d_out[slot];
	a.params = vv.params, a.state = vv.state, a.win = vv.win;
	a.flags = mv.flags, a.gain = mv.gain;
	a.mm = b->mm, a.ns = b->len, a.row_w = b->row_w, a.nslice = b->nslice, a.sum_off = b->sum_off;
	a.sample_rate = cf.rate;
	const dim3 grid((unsigned)b->nconf);
	if (in_kind == MI_SESSION_PCM16) launch_out<0>(cf.out_codec, grid, b->lds, b->ctx->stream, a);
	else if (in_kind == MI_SESSION_PCMA) launch_out<1>(cf.out_codec, grid, b->lds, b->ctx->stream, a);
	else launch_out<2>(cf.out_codec, grid, b->lds, b->ctx->stream, a);
	MI_LAUNCH_CHECK();
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
	if (b->d_pcm) mi_dev_free(c, b->d_pcm);
	if (b->d_evlen) mi_dev_free(c, b->d_evlen);
	if (b->plc) mi_plc_destroy(b->plc);
	if (b->vol) mi_volume_destroy(b->vol);
	if (b->mix) mi_mixer_destroy(b->mix);
	b->pipe.destroy();
	delete b;
}

int mi_bridge_create(mi_ctx *ctx, const mi_bridge_config *cfg, mi_bridge **out) {
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
	const int row_w = (len >> 2) | 1; // 8-byte words per row, odd
	const size_t sum_off = mi::round_up((size_t)mm * row_w * 8, 16), lds = sum_off + (size_t)len * 4;
	if (lds > BRIDGE_LDS_MAX) {
		mi::set_error("mi_bridge_create: a conference's tick must fit %zu bytes of LDS (%d members x %d samples need %zu)", BRIDGE_LDS_MAX, mm,
		              len, lds);
		return MI_ENOTSUP;
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
	b->in_bytes = (size_t)len * (cfg->in_codec ? 1 : 2);
	b->out_bytes = (size_t)len * (cfg->out_codec ? 1 : 2);
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
	if (cfg->plc) {
		if ((rc = mi_plc_create(ctx, b->n, cfg->rate, len, &b->plc)) != MI_OK) return fail(rc);
		std::vector<int32_t> lens(n, len);
		if (!(b->d_evlen = (int32_t *)mi_dev_alloc(ctx, n * 4))) return fail(MI_ENOMEM);
		if (hipMemcpy(b->d_evlen, lens.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(MI_ENODEV);
		if (cfg->in_codec && !(b->d_pcm = (int16_t *)mi_dev_alloc(ctx, n * len * 2))) return fail(MI_ENOMEM);
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
	return MI_OK;
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
