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
// bridge_rated_kernel (legs at their own rate), bridge_legs_kernel (every leg's own codec, with or without the resamplers),
// bridge_updown_kernel (legs above the mix as well) and bridge_rational_kernel (legs at 3/2 and 2/3 of the mix as well) further
// down keep these phases; each says at its head what it adds.
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

// ---- a leg's codec as data (mi_bridge_create_legs): load_raw_leg / decode_group_leg (g711.hpp) read a leg's byte row
// eight samples of the leg's mix: 16 bytes of PCM, or 8 code words at the leg's law
__device__ __forceinline__ void store_group_leg(uint8_t *row, int kind, int g, const int (&o)[8]) {
	if (kind == MI_SESSION_PCM16) {
		*reinterpret_cast<uint4 *>(row + 16 * g) = make_uint4(pack16(o[0], o[1]), pack16(o[2], o[3]), pack16(o[4], o[5]), pack16(o[6], o[7]));
		return;
	}
	uint32_t cw[2] = {0, 0};
#pragma unroll
	for (int k = 0; k < 8; ++k) { // both laws and a select: a wavefront of (D) holds legs of either
		const uint32_t a = lin2alaw(o[k]), u = lin2ulaw(o[k]);
		cw[k >> 2] |= (kind == MI_SESSION_PCMU ? u : a) << (8 * (k & 3));
	}
	*reinterpret_cast<uint2 *>(row + 8 * g) = make_uint2(cw[0], cw[1]);
}

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

// ---- legs at their own rate (mi_bridge_create_rated): in_resampler and out_resampler of plumb_to_conf
// (audioconference.c:209-257) folded into the tick.  A member's ratio -- conference rate / leg rate, 1, 2, 3 or 6 -- is
// data: one conference holds 8, 16 and 48 kHz legs side by side.  The rows in LDS are at the conference's rate; a
// narrower leg's tick sits at the head of its row until its up-sampler has run.
#include "resample_tile.hpp"

constexpr int RS_FILT = 48, RS_R = 8;       // quality 3: 48 taps per polyphase row, fir_tile's eight positions
constexpr size_t RATED_STATIC_LDS = 2048;   // bound on the kernel's static LDS (tests/test_bridge_rates_cpu.py holds it)

struct RatedArgs {
	BridgeArgs b;         // ns, row_w, sum_off, sample_rate: the conference's
	const uint8_t *ratio; // [nconf * mm] conference rate / leg rate
	int16_t *hist_in;     // [nconf * mm][48] in_resampler: the last 47 leg-rate samples, as mi_resampler keeps them
	int16_t *hist_out;    // [nconf * mm][hout_stride] out_resampler: the last ratio * 48 - 1 conference-rate samples
	const float *tab;     // every table of the bridge, back to back
	int tab_up[7];        // float offset of ratio r's up table [r][48] (polyphase rows, mi_resampler's own layout)
	int tab_down[7];      // and of its down table, phase-major [r][48]: tap r * i + p at [p][i]
	int pitch;            // samples per row of in / out: the widest leg's tick
	int hout_stride;
	int scratch_off, scratch_per_wave; // bytes: each wavefront's resampler scratch in the dynamic LDS
};

// floats per phase array of the down-sampler (history ++ tick split by input phase, + the tile FIR's look-ahead)
__host__ __device__ inline int rated_plen(int num, int in_len) { return ((num * RS_FILT - 1 + in_len + num - 1) / num + RS_R + 8 + 3) & ~3; }

__device__ __forceinline__ void load_taps(const float *row, f2 (&t2)[RS_FILT / 2]) {
	const float4 *tp = reinterpret_cast<const float4 *>(row);
#pragma unroll
	for (int j = 0; j < RS_FILT / 4; ++j) {
		const float4 v = tp[j];
		t2[2 * j] = (f2){v.x, v.y}, t2[2 * j + 1] = (f2){v.z, v.w};
	}
}

// One wavefront runs one member's in_resampler: resample_up_kernel's arithmetic in its order (resample.hip) --
// out[m * den + p] = sum_j table[p][j] * x[m + j] through fir_tile from a zero accumulator, then rs_word2int --, the
// tick read from the head of the member's row, the result written over the row.  x: [47 + in_len + slack] floats.
__device__ __forceinline__ void rated_up(float *x, int16_t *row, int16_t *hist, const float *tab, int den, int in_len, int lane) {
	constexpr int HIST = RS_FILT - 1, HQ = RS_FILT / 4;
	const int xn = (HIST + in_len + RS_R + 1 + 3) & ~3;
	for (int q = lane; q < HQ + (in_len >> 2); q += 64) {
		const bool h = q < HQ;
		const short4 v = h ? *reinterpret_cast<const short4 *>(hist + 4 * q) : *reinterpret_cast<const short4 *>(row + 4 * (q - HQ));
		const int b = h ? 4 * q : HIST + 4 * (q - HQ);
		x[b] = (float)v.x, x[b + 1] = (float)v.y, x[b + 2] = (float)v.z;
		if (!h || b + 3 < HIST) x[b + 3] = (float)v.w; // the history row's pad slot is not a sample
	}
	for (int i = HIST + in_len + lane; i < xn; i += 64) x[i] = 0.f;
	wave_sync(); // the whole tick is staged before the first output lands on the row
	const int nlanes = den * (in_len >> 3);
	for (int base = 0; base < nlanes; base += 64) {
		const int l = base + lane;
		const bool on = l < nlanes;
		const int tile = on ? l / den : 0, p = on ? l - tile * den : 0;
		f2 t2[RS_FILT / 2], acc2[RS_R / 2];
		load_taps(tab + p * RS_FILT, t2);
#pragma unroll
		for (int q = 0; q < RS_R / 2; ++q) acc2[q] = (f2){0.f, 0.f};
		fir_tile<RS_FILT, RS_R>(x + tile * RS_R, t2, acc2);
		if (on) {
#pragma unroll
			for (int q = 0; q < RS_R / 2; ++q) {
				row[(tile * RS_R + 2 * q) * den + p] = rs_word2int(acc2[q].x);
				row[(tile * RS_R + 2 * q + 1) * den + p] = rs_word2int(acc2[q].y);
			}
		}
	}
	// new history = the last 47 samples of history ++ tick; the pad slot takes the zero slack
	if (lane < HQ) {
		const float *hx = x + in_len + 4 * lane;
		short4 h;
		h.x = (int16_t)hx[0], h.y = (int16_t)hx[1], h.z = (int16_t)hx[2], h.w = (int16_t)hx[3];
		*reinterpret_cast<short4 *>(hist + 4 * lane) = h;
	}
	wave_sync(); // x is read out before the wave's next member stages over it
}

// One wavefront runs one member's out_resampler: resample_down_kernel's arithmetic in its order -- history ++ row split by
// input phase, each phase's share of eight outputs through fir_tile, the shares added phase upward, rs_word2int --; the
// leg-rate tick leaves as 16 bytes of PCM or 8 code words per lane.  xp: [num][plen] ++ [in_len] floats.  OUT < 0: the
// codec is `kind`, the same in every lane of the wave, and `at` is the byte offset of the leg's row.
template <int OUT>
__device__ __forceinline__ void rated_down(float *xp, const int16_t *row, int16_t *hist, const float *tab, void *out, size_t at, int num,
                                           int in_len, int lane, int kind = OUT) {
	const int HIST = num * RS_FILT - 1, hq = (num * RS_FILT) >> 2, nq = hq + (in_len >> 2);
	const int out_len = in_len / num, plen = rated_plen(num, in_len);
	float *part = xp + num * plen; // [out_len][num] partial sums
	for (int i = lane; i < num * plen; i += 64) xp[i] = 0.f;
	wave_sync();
	for (int q = lane; q < nq; q += 64) {
		const bool h = q < hq;
		const short4 v = h ? *reinterpret_cast<const short4 *>(hist + 4 * q) : *reinterpret_cast<const short4 *>(row + 4 * (q - hq));
		const int b = h ? 4 * q : HIST + 4 * (q - hq); // index in history ++ row
		const short e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const int i = b + k;
			if (!h || i < HIST) xp[(i % num) * plen + i / num] = (float)e[k];
		}
	}
	wave_sync();
	const int nlanes = num * (out_len >> 3);
	for (int base = 0; base < nlanes; base += 64) {
		const int l = base + lane;
		const bool on = l < nlanes;
		const int tile = on ? l / num : 0, p = on ? l - tile * num : 0;
		f2 t2[RS_FILT / 2], acc2[RS_R / 2];
		load_taps(tab + p * RS_FILT, t2);
#pragma unroll
		for (int q = 0; q < RS_R / 2; ++q) acc2[q] = (f2){0.f, 0.f};
		fir_tile<RS_FILT, RS_R>(xp + p * plen + tile * RS_R, t2, acc2);
		if (on) {
			float *d = part + (tile * RS_R) * num + p;
#pragma unroll
			for (int q = 0; q < RS_R / 2; ++q) d[(2 * q) * num] = acc2[q].x, d[(2 * q + 1) * num] = acc2[q].y;
		}
	}
	wave_sync();
	for (int g = lane; g < (out_len >> 3); g += 64) {
		const float *ps = part + g * 8 * num;
		int o[8];
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			float sum = 0.f;
			for (int p = 0; p < num; ++p) sum += ps[k * num + p];
			o[k] = rs_word2int(sum);
		}
		if (OUT < 0) {
			store_group_leg(static_cast<uint8_t *>(out) + at, kind, g, o);
		} else if (OUT == 0) {
			*reinterpret_cast<uint4 *>(static_cast<int16_t *>(out) + at + 8 * g) =
			    make_uint4(pack16(o[0], o[1]), pack16(o[2], o[3]), pack16(o[4], o[5]), pack16(o[6], o[7]));
		} else {
			uint32_t cw[2] = {0, 0};
#pragma unroll
			for (int k = 0; k < 8; ++k) cw[k >> 2] |= (OUT == 2 ? lin2ulaw(o[k]) : lin2alaw(o[k])) << (8 * (k & 3));
			*reinterpret_cast<uint2 *>(static_cast<uint8_t *>(out) + at + 8 * g) = make_uint2(cw[0], cw[1]);
		}
	}
	// new history = the last HIST samples of history ++ row; the pad slot of the row takes a zero
	for (int q = lane; q < hq; q += 64) {
		short4 h;
		short *hp = &h.x;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const int i = in_len + 4 * q + k;
			hp[k] = (4 * q + k < HIST) ? (short)xp[(i % num) * plen + i / num] : (short)0;
		}
		*reinterpret_cast<short4 *>(hist + 4 * q) = h;
	}
	wave_sync();
}

// bridge_tick_kernel with the two resamplers of every member whose ratio is not 1.  Phases (0) (A) (B) as there, on the leg's
// own samples (MSVolume sits in front of the in_resampler: chunk length and sample rate are the leg's);
//   (G) the Q12 gain on the leg-rate samples, in the row;
//   (U) one wavefront per member, the four waves taking members in turn: the in_resampler of a present, plumbed leg
//       (the run mask present & linked of mi_resampler_process_masked; any other keeps its history);
//   (C) (D) at the conference's rate; (D) writes a narrower leg's mix over its own row instead of storing it;
//   (W) one wavefront per member: the out_resampler of a pin with its output on, then the store / encoder.
template <int IN, int OUT>
__global__ __launch_bounds__(BT) void bridge_rated_kernel(RatedArgs ra) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const BridgeArgs &a = ra.b;
	uint2 *rows = reinterpret_cast<uint2 *>(smem);
	int *s_sum = reinterpret_cast<int *>(smem + a.sum_off);
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	__shared__ unsigned char s_rt[BMAX], s_on[BMAX]; // a member's ratio; whether it is here this tick
	const int t = threadIdx.x, c = blockIdx.x, mm = a.mm, ns = a.ns, nw = ns >> 2, ng = ns >> 3;
	const int s0 = c * mm;

	// ---- (0)
	mi_volume_params p;
	mi_volume_state st;
	float2 win = make_float2(0, 0);
	unsigned mflag = 0;
	int mgain_bits = 0, rt = 1;
	bool here = false;
	if (t < mm) {
		const int s = s0 + t;
		p = a.params[s];
		st = a.state[s];
		win = a.win[s];
		mflag = a.flags[s];
		mgain_bits = __float_as_int(a.gain[s]);
		here = !a.present || a.present[s] != 0;
		rt = ra.ratio[s];
		s_rt[t] = (unsigned char)rt, s_on[t] = here;
	}
	for (int i = t; i < ns; i += BT) s_sum[i] = 0;

	// ---- (A) the leg's own groups; the rest of the row is zeros
	for (int mb = 0; mb < mm; mb += BT / 8) {
		const int m = mb + (t >> 3), q = t & 7;
		const bool valid = m < mm;
		int pk = 0, dc = 0;
		if (valid) {
			const bool on = !a.present || a.present[s0 + m] != 0;
			const int ngl = ng / ra.ratio[s0 + m];
			for (int g0 = q; g0 < ng; g0 += 32) {
				uint4 v[4];
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					v[i] = make_uint4(0, 0, 0, 0);
					if (on && g0 + 8 * i < ngl) v[i] = load_group<IN>(a.in, (size_t)(s0 + m), ra.pitch, g0 + 8 * i);
				}
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const int g = g0 + 8 * i;
					if (g >= ng) continue;
					rows[m * a.row_w + 2 * g] = make_uint2(v[i].x, v[i].y);
					rows[m * a.row_w + 2 * g + 1] = make_uint2(v[i].z, v[i].w);
					const unsigned w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						const int x0 = lo16(w[k]), x1 = hi16(w[k]);
						pk = max(pk, max(x0 < 0 ? -x0 : x0, x1 < 0 ? -x1 : x1));
						dc += x0 + x1;
					}
				}
			}
		}
#pragma unroll
		for (int off = 1; off < 8; off <<= 1) {
			pk = max(pk, __shfl_xor(pk, off));
			dc += __shfl_xor(dc, off);
		}
		if (valid && q == 0) s_pk[m] = pk, s_dc[m] = dc;
	}
	__syncthreads();

	// ---- (B) over the leg's rate / 100 samples
	if (t < mm) {
		if (here) {
			const uint2 *r = rows + t * a.row_w;
			const int nwl = nw / rt;
			float acc = 0;
#pragma unroll 4
			for (int i = 0; i < nwl; ++i) {
				const uint2 w = r[i];
				const int x0 = lo16(w.x), x1 = hi16(w.x), x2 = lo16(w.y), x3 = hi16(w.y);
				acc += (float)(x0 * x0);
				acc += (float)(x1 * x1);
				acc += (float)(x2 * x2);
				acc += (float)(x3 * x3);
			}
			const VolCtl o = volume_control(p, st, 0.f, acc, ns / rt, s_pk[t], s_dc[t], a.sample_rate / rt, win);
			s_par[t] = make_int4((int)mflag | (o.mode << 8), o.intgain, o.dcoff, mgain_bits);
			a.state[s0 + t] = st;
			a.win[s0 + t] = win;
		} else {
			s_par[t] = make_int4((int)mflag, 4096, 0, mgain_bits);
		}
	}
	__syncthreads();

	// ---- (G) apply_gain (msvolume.c:440) in front of the in_resampler, whose history keeps the levelled samples
	for (int item = t; item < mm * nw; item += BT) {
		const int m = item / nw, j = item - m * nw;
		const int4 par = s_par[m];
		const int mode = par.x >> 8;
		if (mode == 0 || j >= nw / s_rt[m]) continue;
		const uint2 cur = rows[m * a.row_w + j];
		int x[4] = {lo16(cur.x), hi16(cur.x), lo16(cur.y), hi16(cur.y)};
		const int ig = par.y, dc = (mode == 2) ? par.z : 0;
#pragma unroll
		for (int k = 0; k < 4; ++k) x[k] = sat16(((x[k] - dc) * ig) / 4096);
		rows[m * a.row_w + j] = make_uint2(pack16(x[0], x[1]), pack16(x[2], x[3]));
	}
	__syncthreads();

	// ---- (U)
	const int wave = t >> 6, lane = t & 63;
	float *scr = reinterpret_cast<float *>(smem + ra.scratch_off + wave * ra.scratch_per_wave);
	for (int m = wave; m < mm; m += BT / 64) {
		const int den = s_rt[m];
		if (den == 1 || !s_on[m] || !((unsigned)s_par[m].x & MI_MIX_LINKED)) continue;
		rated_up(scr, reinterpret_cast<int16_t *>(rows + m * a.row_w), ra.hist_in + (size_t)(s0 + m) * RS_FILT, ra.tab + ra.tab_up[den], den,
		         ns / den, lane);
	}
	__syncthreads();

	// ---- (C) the gain is in the rows already
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
				const float gn = __int_as_float(par.w);
				if (gn != 1.0f) {
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
		if (s_rt[m] != 1) { // the out_resampler's input
			rows[m * a.row_w + 2 * g] = make_uint2(pack16(o[0], o[1]), pack16(o[2], o[3]));
			rows[m * a.row_w + 2 * g + 1] = make_uint2(pack16(o[4], o[5]), pack16(o[6], o[7]));
			continue;
		}
		const size_t at = (size_t)(s0 + m) * ra.pitch + 8 * g;
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
	__syncthreads();

	// ---- (W)
	for (int m = wave; m < mm; m += BT / 64) {
		const int num = s_rt[m];
		if (num == 1 || !((unsigned)s_par[m].x & MI_MIX_OUTPUT)) continue;
		rated_down<OUT>(scr, reinterpret_cast<const int16_t *>(rows + m * a.row_w), ra.hist_out + (size_t)(s0 + m) * ra.hout_stride,
		                ra.tab + ra.tab_down[num], a.out, (size_t)(s0 + m) * ra.pitch, num, ns, lane);
	}
}

template <int IN>
void launch_rated_out(int out_kind, dim3 grid, size_t lds, hipStream_t st, const RatedArgs &a) {
	if (out_kind == MI_SESSION_PCM16) hipLaunchKernelGGL((bridge_rated_kernel<IN, 0>), grid, dim3(BT), lds, st, a);
	else if (out_kind == MI_SESSION_PCMA) hipLaunchKernelGGL((bridge_rated_kernel<IN, 1>), grid, dim3(BT), lds, st, a);
	else hipLaunchKernelGGL((bridge_rated_kernel<IN, 2>), grid, dim3(BT), lds, st, a);
}

// ---- every leg's own codec (mi_bridge_create_legs): plumb_to_conf hangs each endpoint's own decoder and encoder on its
// pin, so the pair is data like the ratio -- A-law and mu-law trunks, and PCM members, in one mix.  The host rows are byte
// rows at one pitch (a multiple of 16); a leg's tick is the first rate / 100 x 1 or 2 bytes of its row.  Only a bridge
// whose legs differ runs this kernel: a uniform one keeps the kernels above, whose codecs are compile-time.
struct LegsArgs {
	RatedArgs r;             // r.b.in / r.b.out: the byte rows; r.pitch is not read; !RATED reads r.b only
	const uint8_t *codec;    // [nconf * mm] in_codec | out_codec << 2
	int in_pitch, out_pitch; // bytes per row
};

// The phases of bridge_tick_kernel (RATED false: the gain in (C)) or of bridge_rated_kernel (RATED true: (G), (U), (W)),
// their arithmetic word for word; what differs is where a codec is chosen:
//   (0) the member's codec pair into LDS, next to its ratio;
//   (A) the kind is uniform over a member's eight lanes: load_raw_leg straight-line as there, then decode_group_leg;
//   (D) store_group_leg per member; (W) the same, uniform over the wave that runs the member's out_resampler.
template <bool RATED>
__global__ __launch_bounds__(BT) void bridge_legs_kernel(LegsArgs la) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const RatedArgs &ra = la.r;
	const BridgeArgs &a = ra.b;
	uint2 *rows = reinterpret_cast<uint2 *>(smem);
	int *s_sum = reinterpret_cast<int *>(smem + a.sum_off);
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	__shared__ unsigned char s_rt[BMAX], s_on[BMAX], s_cd[BMAX]; // a member's ratio; whether it is here this tick; its codec pair
	const int t = threadIdx.x, c = blockIdx.x, mm = a.mm, ns = a.ns, nw = ns >> 2, ng = ns >> 3;
	const int s0 = c * mm;
	const uint8_t *in = static_cast<const uint8_t *>(a.in);
	uint8_t *out = static_cast<uint8_t *>(a.out);

	// ---- (0)
	mi_volume_params p;
	mi_volume_state st;
	float2 win = make_float2(0, 0);
	unsigned mflag = 0;
	int mgain_bits = 0, rt = 1;
	bool here = false;
	if (t < mm) {
		const int s = s0 + t;
		p = a.params[s];
		st = a.state[s];
		win = a.win[s];
		mflag = a.flags[s];
		mgain_bits = __float_as_int(a.gain[s]);
		here = !a.present || a.present[s] != 0;
		s_cd[t] = la.codec[s];
		if (RATED) {
			rt = ra.ratio[s];
			s_rt[t] = (unsigned char)rt, s_on[t] = here;
		}
	}
	for (int i = t; i < ns; i += BT) s_sum[i] = 0;

	// ---- (A) the leg's own groups; the rest of the row is zeros
	for (int mb = 0; mb < mm; mb += BT / 8) {
		const int m = mb + (t >> 3), q = t & 7;
		const bool valid = m < mm;
		int pk = 0, dc = 0;
		if (valid) {
			const bool on = !a.present || a.present[s0 + m] != 0;
			const int kind = la.codec[s0 + m] & 3;
			const int ngl = RATED ? ng / ra.ratio[s0 + m] : ng;
			const uint8_t *src = in + (size_t)(s0 + m) * la.in_pitch;
			for (int g0 = q; g0 < ng; g0 += 32) {
				uint4 v[4];
#pragma unroll
				for (int i = 0; i < 4; ++i) { // straight-line loads: all in flight at once
					v[i] = make_uint4(0, 0, 0, 0);
					if (on && g0 + 8 * i < ngl) v[i] = load_raw_leg(src, kind, g0 + 8 * i);
				}
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const int g = g0 + 8 * i;
					if (g >= ng) continue;
					const uint4 d = decode_group_leg(v[i], kind, g);
					if (on && g < ngl) v[i] = d; // (code bytes of zero are not silence)
					rows[m * a.row_w + 2 * g] = make_uint2(v[i].x, v[i].y);
					rows[m * a.row_w + 2 * g + 1] = make_uint2(v[i].z, v[i].w);
					const unsigned w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						const int x0 = lo16(w[k]), x1 = hi16(w[k]);
						pk = max(pk, max(x0 < 0 ? -x0 : x0, x1 < 0 ? -x1 : x1));
						dc += x0 + x1;
					}
				}
			}
		}
#pragma unroll
		for (int off = 1; off < 8; off <<= 1) {
			pk = max(pk, __shfl_xor(pk, off));
			dc += __shfl_xor(dc, off);
		}
		if (valid && q == 0) s_pk[m] = pk, s_dc[m] = dc;
	}
	__syncthreads();

	// ---- (B) over the leg's rate / 100 samples
	if (t < mm) {
		if (here) {
			const uint2 *r = rows + t * a.row_w;
			const int nwl = nw / rt;
			float acc = 0;
#pragma unroll 4
			for (int i = 0; i < nwl; ++i) {
				const uint2 w = r[i];
				const int x0 = lo16(w.x), x1 = hi16(w.x), x2 = lo16(w.y), x3 = hi16(w.y);
				acc += (float)(x0 * x0);
				acc += (float)(x1 * x1);
				acc += (float)(x2 * x2);
				acc += (float)(x3 * x3);
			}
			const VolCtl o = volume_control(p, st, 0.f, acc, ns / rt, s_pk[t], s_dc[t], a.sample_rate / rt, win);
			s_par[t] = make_int4((int)mflag | (o.mode << 8), o.intgain, o.dcoff, mgain_bits);
			a.state[s0 + t] = st;
			a.win[s0 + t] = win;
		} else {
			s_par[t] = make_int4((int)mflag, 4096, 0, mgain_bits);
		}
	}
	__syncthreads();

	const int wave = t >> 6, lane = t & 63;
	float *scr = RATED ? reinterpret_cast<float *>(smem + ra.scratch_off + wave * ra.scratch_per_wave) : nullptr;
	if (RATED) {
		// ---- (G)
		for (int item = t; item < mm * nw; item += BT) {
			const int m = item / nw, j = item - m * nw;
			const int4 par = s_par[m];
			const int mode = par.x >> 8;
			if (mode == 0 || j >= nw / s_rt[m]) continue;
			const uint2 cur = rows[m * a.row_w + j];
			int x[4] = {lo16(cur.x), hi16(cur.x), lo16(cur.y), hi16(cur.y)};
			const int ig = par.y, dc = (mode == 2) ? par.z : 0;
#pragma unroll
			for (int k = 0; k < 4; ++k) x[k] = sat16(((x[k] - dc) * ig) / 4096);
			rows[m * a.row_w + j] = make_uint2(pack16(x[0], x[1]), pack16(x[2], x[3]));
		}
		__syncthreads();

		// ---- (U)
		for (int m = wave; m < mm; m += BT / 64) {
			const int den = s_rt[m];
			if (den == 1 || !s_on[m] || !((unsigned)s_par[m].x & MI_MIX_LINKED)) continue;
			rated_up(scr, reinterpret_cast<int16_t *>(rows + m * a.row_w), ra.hist_in + (size_t)(s0 + m) * RS_FILT, ra.tab + ra.tab_up[den],
			         den, ns / den, lane);
		}
		__syncthreads();
	}

	// ---- (C) RATED: the gain is in the rows already
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
				if (!RATED && mode != 0) { // apply_gain (msvolume.c:440)
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
		if (RATED && s_rt[m] != 1) { // the out_resampler's input
			rows[m * a.row_w + 2 * g] = make_uint2(pack16(o[0], o[1]), pack16(o[2], o[3]));
			rows[m * a.row_w + 2 * g + 1] = make_uint2(pack16(o[4], o[5]), pack16(o[6], o[7]));
			continue;
		}
		store_group_leg(out + (size_t)(s0 + m) * la.out_pitch, s_cd[m] >> 2, g, o);
	}
	if (!RATED) return;
	__syncthreads();

	// ---- (W)
	for (int m = wave; m < mm; m += BT / 64) {
		const int num = s_rt[m];
		if (num == 1 || !((unsigned)s_par[m].x & MI_MIX_OUTPUT)) continue;
		rated_down<-1>(scr, reinterpret_cast<const int16_t *>(rows + m * a.row_w), ra.hist_out + (size_t)(s0 + m) * ra.hout_stride,
		               ra.tab + ra.tab_down[num], out, (size_t)(s0 + m) * la.out_pitch, num, ns, lane, __builtin_amdgcn_readfirstlane(s_cd[m] >> 2));
	}
}

// ---- endpoints on either side of the mix (mi_bridge_create_endpoints): plumb_to_conf configures both resamplers from the
// endpoint's rate and the conference's whichever is larger, so a leg ABOVE the mix -- a 48 kHz PCM member of a 16 kHz room --
// has the down-sampler in front of its pin and the up-sampler behind it.  The ratio byte of such a member carries UD_ABOVE.
// Only a bridge with at least one such leg runs this kernel; its rows in LDS are as wide as the widest leg's tick.
constexpr unsigned UD_ABOVE = 0x80;

struct UpdownArgs {
	LegsArgs l;         // l.r.b.ns, sum_off, sample_rate: the conference's; l.r.b.row_w: of a row of `wide` samples
	int wide;           // samples per LDS row: the widest leg's tick (>= ns)
	int hin_stride;     // samples per member of l.r.hist_in (l.r.hout_stride: of hist_out); either holds 47 or ratio * 48 - 1
	int tab_down_in[7]; // a leg above by ratio k: its in_resampler's table (leg -> conference), phase-major [k][48]
	int tab_up_out[7];  // and its out_resampler's (conference -> leg), polyphase rows [k][48]
};

// floats per phase array of the down-sampler in FRONT of a pin: rated_plen with plen / 4 odd.  Lane l of the tile FIR reads
// 16 bytes at phase (l % num) * plen + 8 * (l / num): the tiles fall on the even 16-byte slots of the 256-byte bank row,
// an odd plen / 4 puts the neighbouring phase on the odd ones (an even one -- 144, 224 -- stacks the phases on one slot).
__host__ __device__ inline int updown_plen(int num, int in_len) { return rated_plen(num, in_len) | 4; }

// rated_down with the row as its sink: one wavefront runs the in_resampler of one member above the mix --
// resample_down_kernel's arithmetic in its order, history ++ the row's num * out_len leg-rate samples split by input phase,
// each phase's share of eight outputs through fir_tile, the shares added phase upward, rs_word2int -- and writes the
// out_len conference-rate samples over the head of the row.  xp: [num][plen] ++ [in_len] floats.
__device__ __forceinline__ void updown_down(float *xp, int16_t *row, int16_t *hist, const float *tab, int num, int in_len, int lane) {
	const int HIST = num * RS_FILT - 1, hq = (num * RS_FILT) >> 2, nq = hq + (in_len >> 2);
	const int out_len = in_len / num, plen = updown_plen(num, in_len);
	float *part = xp + num * plen; // [out_len][num] partial sums
	for (int i = lane; i < num * plen; i += 64) xp[i] = 0.f;
	wave_sync();
	for (int q = lane; q < nq; q += 64) { // (a 287-sample history is more than one pass of the 64 lanes)
		const bool h = q < hq;
		const short4 v = h ? *reinterpret_cast<const short4 *>(hist + 4 * q) : *reinterpret_cast<const short4 *>(row + 4 * (q - hq));
		const int b = h ? 4 * q : HIST + 4 * (q - hq); // index in history ++ row
		const short e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const int i = b + k;
			if (!h || i < HIST) xp[(i % num) * plen + i / num] = (float)e[k];
		}
	}
	wave_sync(); // the whole tick is staged before the first output lands on the row
	const int nlanes = num * (out_len >> 3);
	for (int base = 0; base < nlanes; base += 64) {
		const int l = base + lane;
		const bool on = l < nlanes;
		const int tile = on ? l / num : 0, p = on ? l - tile * num : 0;
		f2 t2[RS_FILT / 2], acc2[RS_R / 2];
		load_taps(tab + p * RS_FILT, t2);
#pragma unroll
		for (int q = 0; q < RS_R / 2; ++q) acc2[q] = (f2){0.f, 0.f};
		fir_tile<RS_FILT, RS_R>(xp + p * plen + tile * RS_R, t2, acc2);
		if (on) {
			float *d = part + (tile * RS_R) * num + p;
#pragma unroll
			for (int q = 0; q < RS_R / 2; ++q) d[(2 * q) * num] = acc2[q].x, d[(2 * q + 1) * num] = acc2[q].y;
		}
	}
	wave_sync();
	for (int g = lane; g < (out_len >> 3); g += 64) {
		const float *ps = part + g * 8 * num;
		int o[8];
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			float sum = 0.f;
			for (int p = 0; p < num; ++p) sum += ps[k * num + p];
			o[k] = rs_word2int(sum);
		}
		uint2 *d = reinterpret_cast<uint2 *>(row + 8 * g);
		d[0] = make_uint2(pack16(o[0], o[1]), pack16(o[2], o[3])), d[1] = make_uint2(pack16(o[4], o[5]), pack16(o[6], o[7]));
	}
	// new history = the last HIST samples of history ++ tick; the pad slot takes a zero
	for (int q = lane; q < hq; q += 64) {
		short4 h;
		short *hp = &h.x;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const int i = in_len + 4 * q + k;
			hp[k] = (4 * q + k < HIST) ? (short)xp[(i % num) * plen + i / num] : (short)0;
		}
		*reinterpret_cast<short4 *>(hist + 4 * q) = h;
	}
	wave_sync(); // xp is read out before the wave's next member stages over it
}

// what rated_up left on the row of a member above the mix -- its out_resampler's `len` leg-rate samples -- through the
// leg's store or encoder, 16 bytes of PCM or 8 code words per lane
__device__ __forceinline__ void updown_store(const int16_t *row, uint8_t *out, int kind, int len, int lane) {
	for (int g = lane; g < (len >> 3); g += 64) {
		const uint2 *r = reinterpret_cast<const uint2 *>(row + 8 * g);
		const uint2 w0 = r[0], w1 = r[1];
		const int o[8] = {lo16(w0.x), hi16(w0.x), lo16(w0.y), hi16(w0.y), lo16(w1.x), hi16(w1.x), lo16(w1.y), hi16(w1.y)};
		store_group_leg(out, kind, g, o);
	}
}

// The phases of bridge_legs_kernel<true>, their arithmetic word for word, with the direction of a member's resamplers as
// data next to its ratio and its codec pair:
//   (0) (A) (B) (G) on the leg's own samples, ratio * ns of them for a leg above the mix: the row is `wide` samples;
//   (U) one wavefront per member: rated_up for a leg below the mix, updown_down for one above it;
//   (C) (D) at the conference's rate on the head of the rows;
//   (W) one wavefront per member: rated_down for a leg below the mix; for one above it rated_up from the head of the row
//       back over the row (which held the leg's input, so it is wide enough), then updown_store.
__global__ __launch_bounds__(BT) void bridge_updown_kernel(UpdownArgs ua) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const LegsArgs &la = ua.l;
	const RatedArgs &ra = la.r;
	const BridgeArgs &a = ra.b;
	uint2 *rows = reinterpret_cast<uint2 *>(smem);
	int *s_sum = reinterpret_cast<int *>(smem + a.sum_off);
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	__shared__ unsigned char s_rt[BMAX], s_on[BMAX], s_cd[BMAX]; // a member's ratio | UD_ABOVE; whether it is here this tick; its codec pair
	const int t = threadIdx.x, c = blockIdx.x, mm = a.mm, ns = a.ns, nw = ns >> 2, ng = ns >> 3;
	const int s0 = c * mm;
	const uint8_t *in = static_cast<const uint8_t *>(a.in);
	uint8_t *out = static_cast<uint8_t *>(a.out);

	// ---- (0)
	mi_volume_params p;
	mi_volume_state st;
	float2 win = make_float2(0, 0);
	unsigned mflag = 0;
	int mgain_bits = 0, rt = 1;
	bool here = false;
	if (t < mm) {
		const int s = s0 + t;
		p = a.params[s];
		st = a.state[s];
		win = a.win[s];
		mflag = a.flags[s];
		mgain_bits = __float_as_int(a.gain[s]);
		here = !a.present || a.present[s] != 0;
		s_cd[t] = la.codec[s];
		rt = ra.ratio[s];
		s_rt[t] = (unsigned char)rt, s_on[t] = here;
	}
	for (int i = t; i < ns; i += BT) s_sum[i] = 0;

	// ---- (A) the leg's own groups; the rest of the row is zeros as far as the conference's tick reaches
	for (int mb = 0; mb < mm; mb += BT / 8) {
		const int m = mb + (t >> 3), q = t & 7;
		const bool valid = m < mm;
		int pk = 0, dc = 0;
		if (valid) {
			const bool on = !a.present || a.present[s0 + m] != 0;
			const int kind = la.codec[s0 + m] & 3, r = ra.ratio[s0 + m];
			const int ngl = (r & UD_ABOVE) ? ng * (r & 7) : ng / r, nz = max(ng, ngl);
			const uint8_t *src = in + (size_t)(s0 + m) * la.in_pitch;
			for (int g0 = q; g0 < nz; g0 += 32) {
				uint4 v[4];
#pragma unroll
				for (int i = 0; i < 4; ++i) { // straight-line loads: all in flight at once
					v[i] = make_uint4(0, 0, 0, 0);
					if (on && g0 + 8 * i < ngl) v[i] = load_raw_leg(src, kind, g0 + 8 * i);
				}
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const int g = g0 + 8 * i;
					if (g >= nz) continue;
					const uint4 d = decode_group_leg(v[i], kind, g);
					if (on && g < ngl) v[i] = d; // (code bytes of zero are not silence)
					rows[m * a.row_w + 2 * g] = make_uint2(v[i].x, v[i].y);
					rows[m * a.row_w + 2 * g + 1] = make_uint2(v[i].z, v[i].w);
					const unsigned w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						const int x0 = lo16(w[k]), x1 = hi16(w[k]);
						pk = max(pk, max(x0 < 0 ? -x0 : x0, x1 < 0 ? -x1 : x1));
						dc += x0 + x1;
					}
				}
			}
		}
#pragma unroll
		for (int off = 1; off < 8; off <<= 1) {
			pk = max(pk, __shfl_xor(pk, off));
			dc += __shfl_xor(dc, off);
		}
		if (valid && q == 0) s_pk[m] = pk, s_dc[m] = dc;
	}
	__syncthreads();

	// ---- (B) over the leg's rate / 100 samples, at the leg's rate
	if (t < mm) {
		if (here) {
			const uint2 *r = rows + t * a.row_w;
			const bool above = rt & UD_ABOVE;
			const int k = rt & 7, nwl = above ? nw * k : nw / k;
			float acc = 0;
#pragma unroll 4
			for (int i = 0; i < nwl; ++i) {
				const uint2 w = r[i];
				const int x0 = lo16(w.x), x1 = hi16(w.x), x2 = lo16(w.y), x3 = hi16(w.y);
				acc += (float)(x0 * x0);
				acc += (float)(x1 * x1);
				acc += (float)(x2 * x2);
				acc += (float)(x3 * x3);
			}
			const VolCtl o = volume_control(p, st, 0.f, acc, 4 * nwl, s_pk[t], s_dc[t], above ? a.sample_rate * k : a.sample_rate / k, win);
			s_par[t] = make_int4((int)mflag | (o.mode << 8), o.intgain, o.dcoff, mgain_bits);
			a.state[s0 + t] = st;
			a.win[s0 + t] = win;
		} else {
			s_par[t] = make_int4((int)mflag, 4096, 0, mgain_bits);
		}
	}
	__syncthreads();

	// ---- (G) apply_gain (msvolume.c:440) in front of the in_resampler, on the leg-rate samples
	const int nww = ua.wide >> 2;
	for (int item = t; item < mm * nww; item += BT) {
		const int m = item / nww, j = item - m * nww;
		const int4 par = s_par[m];
		const int mode = par.x >> 8, r = s_rt[m];
		if (mode == 0 || j >= ((r & UD_ABOVE) ? nw * (r & 7) : nw / r)) continue;
		const uint2 cur = rows[m * a.row_w + j];
		int x[4] = {lo16(cur.x), hi16(cur.x), lo16(cur.y), hi16(cur.y)};
		const int ig = par.y, dc = (mode == 2) ? par.z : 0;
#pragma unroll
		for (int k = 0; k < 4; ++k) x[k] = sat16(((x[k] - dc) * ig) / 4096);
		rows[m * a.row_w + j] = make_uint2(pack16(x[0], x[1]), pack16(x[2], x[3]));
	}
	__syncthreads();

	// ---- (U) the in_resampler of a present, plumbed leg; any other keeps its history
	const int wave = t >> 6, lane = t & 63;
	float *scr = reinterpret_cast<float *>(smem + ra.scratch_off + wave * ra.scratch_per_wave);
	for (int m = wave; m < mm; m += BT / 64) {
		const int r = __builtin_amdgcn_readfirstlane(s_rt[m]), k = r & 7;
		if (r == 1 || !s_on[m] || !((unsigned)s_par[m].x & MI_MIX_LINKED)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(rows + m * a.row_w), *hist = ra.hist_in + (size_t)(s0 + m) * ua.hin_stride;
		if (r & UD_ABOVE) updown_down(scr, row, hist, ra.tab + ua.tab_down_in[k], k, ns * k, lane);
		else rated_up(scr, row, hist, ra.tab + ra.tab_up[k], k, ns / k, lane);
	}
	__syncthreads();

	// ---- (C) the gain is in the rows already
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
		if (s_rt[m] != 1) { // the out_resampler's input, either direction
			rows[m * a.row_w + 2 * g] = make_uint2(pack16(o[0], o[1]), pack16(o[2], o[3]));
			rows[m * a.row_w + 2 * g + 1] = make_uint2(pack16(o[4], o[5]), pack16(o[6], o[7]));
			continue;
		}
		store_group_leg(out + (size_t)(s0 + m) * la.out_pitch, s_cd[m] >> 2, g, o);
	}
	__syncthreads();

	// ---- (W) the out_resampler of a pin with its output on, then the leg's store / encoder
	for (int m = wave; m < mm; m += BT / 64) {
		const int r = __builtin_amdgcn_readfirstlane(s_rt[m]), k = r & 7;
		if (r == 1 || !((unsigned)s_par[m].x & MI_MIX_OUTPUT)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(rows + m * a.row_w), *hist = ra.hist_out + (size_t)(s0 + m) * ra.hout_stride;
		const int kind = __builtin_amdgcn_readfirstlane(s_cd[m] >> 2);
		const size_t at = (size_t)(s0 + m) * la.out_pitch;
		if (r & UD_ABOVE) {
			rated_up(scr, row, hist, ra.tab + ua.tab_up_out[k], k, ns, lane);
			updown_store(row, out + at, kind, ns * k, lane);
		} else {
			rated_down<-1>(scr, row, hist, ra.tab + ra.tab_down[k], out, at, k, ns, lane, kind);
		}
	}
}

// ---- legs at 3/2 and 2/3 of the mix's rate (mi_bridge_create_rational): 32 kHz members of a 48 kHz room, 24 kHz members of
// a 16 kHz one.  The ratio byte of such a member carries UD_R32 -- "x 3/2" -- with UD_ABOVE still giving the direction: the
// leg is at 3/2 of the mix with it, at 2/3 without.  Only a bridge with at least one such leg runs this kernel.
constexpr unsigned UD_R32 = 0x40;
constexpr int RQ_FT = 24; // taps per lane of the rational resamplers: filt_len / M, 48 / 2 and 72 / 3

struct RationalArgs {
	UpdownArgs u;
	// the four rational resamplers' taps, rearranged per (r, p') [L * M][24] (build_tables): of a leg ABOVE the mix the
	// in_resampler's (x 2/3) and the out_resampler's (x 3/2), of a leg below it the in_resampler's (x 3/2) and the
	// out_resampler's (x 2/3)
	int tab_above_in, tab_above_out, tab_below_in, tab_below_out;
};

// a member's own tick in samples and its rate, from its ratio byte and the conference's
__host__ __device__ inline int rational_leg(int r, int conf) {
	if (r & UD_R32) return (r & UD_ABOVE) ? conf / 2 * 3 : conf / 3 * 2;
	return (r & UD_ABOVE) ? conf * (r & 7) : conf / (r & 7);
}

// floats per phase array copy of a rational resampler: resample_ratio_kernel's length (history ++ tick split by input phase,
// + the tile FIR's look-ahead) with plen / 4 odd, as updown_plen and for its reason: lanes (tile, r) and (tile, r + 1) read
// neighbouring arrays at one offset
__host__ __device__ inline int rational_plen(int m, int in_len) { return (((RQ_FT * m - 1 + in_len + m - 1) / m + RS_R + 8 + 3) & ~3) | 4; }
// bytes of a wavefront's scratch for it: two copies of M phase arrays
__host__ __device__ inline size_t rational_scratch(int m, int in_len) { return (size_t)2 * m * rational_plen(m, in_len) * sizeof(float); }

// One wavefront runs one member's rational resampler, L / M = 3/2 or 2/3: resample_ratio_kernel's arithmetic in its order
// (resample.hip).  Output n = q * L + r is the sum of M shares p' = 0 .. M - 1 added upward from 0.f, each share fir_tile<24, 8>
// from a zero accumulator over taps table[(r * M) % L][k * M + p'] -- rearranged on the host: tab [r * M + p'][24] -- and the
// window X_{u % M}[q + k + u / M], u = (r * M) / L + p', of the input split into M phases and staged twice, the second copy
// one float early (u / M is 0 or 1 and a window starts on 16 bytes); then rs_word2int.  Lane (tile, r) computes the M shares
// of its eight outputs one after the other into accumulators of their own and adds them in that order: the bits of the
// batch kernel's partial-sum array without the array.  The in_len samples at the head of `row` are the input, the
// in_len / M * L outputs are written back over the row once the whole tick is staged -- the in_resampler in front of a pin
// as it stands, the out_resampler behind it with updown_store after it.  xp: [2][M][plen] floats.
template <int L, int M>
__device__ __forceinline__ void rational_run(float *xp, int16_t *row, int16_t *hist, const float *tab, int in_len, int lane) {
	constexpr int NT = RQ_FT * M, HIST = NT - 1, HQ = NT / 4;
	static_assert((L - 1) * M / L + M - 1 < 2 * M, "u / M is 0 or 1: two copies of the phase arrays");
	const int plen = rational_plen(M, in_len), periods = in_len / M;
	for (int i = lane; i < 2 * M * plen; i += 64) xp[i] = 0.f;
	wave_sync();
	for (int q = lane; q < HQ + (in_len >> 2); q += 64) {
		const bool h = q < HQ;
		const short4 v = h ? *reinterpret_cast<const short4 *>(hist + 4 * q) : *reinterpret_cast<const short4 *>(row + 4 * (q - HQ));
		const int b = h ? 4 * q : HIST + 4 * (q - HQ); // index in history ++ tick
		const short e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const int i = b + k;
			if (!h || i < HIST) { // the history row's pad slot is not a sample
				const int ph = i % M, m = i / M;
				const float f = (float)e[k];
				xp[ph * plen + m] = f;                       // copy 0
				if (m >= 1) xp[(M + ph) * plen + m - 1] = f; // copy 1: X_p[m] at m - 1
			}
		}
	}
	wave_sync(); // the whole tick is staged before the first output lands on the row
	const int nlanes = L * (periods >> 3);
	for (int base = 0; base < nlanes; base += 64) {
		const int l = base + lane;
		const bool on = l < nlanes;
		const int tile = on ? l / L : 0, r = on ? l - tile * L : 0;
		f2 acc2[M][RS_R / 2];
#pragma unroll
		for (int pp = 0; pp < M; ++pp) {
			const int u = (r * M) / L + pp; // copy u / M, phase u % M: array u
			f2 t2[RQ_FT / 2];
			const float4 *tp = reinterpret_cast<const float4 *>(tab + (r * M + pp) * RQ_FT);
#pragma unroll
			for (int j = 0; j < RQ_FT / 4; ++j) {
				const float4 w = tp[j];
				t2[2 * j] = (f2){w.x, w.y}, t2[2 * j + 1] = (f2){w.z, w.w};
			}
#pragma unroll
			for (int q = 0; q < RS_R / 2; ++q) acc2[pp][q] = (f2){0.f, 0.f};
			fir_tile<RQ_FT, RS_R>(xp + u * plen + tile * RS_R, t2, acc2[pp]);
		}
		if (on) {
#pragma unroll
			for (int q = 0; q < RS_R / 2; ++q) {
				float s0 = 0.f, s1 = 0.f;
#pragma unroll
				for (int pp = 0; pp < M; ++pp) s0 += acc2[pp][q].x, s1 += acc2[pp][q].y;
				row[(tile * RS_R + 2 * q) * L + r] = rs_word2int(s0);
				row[(tile * RS_R + 2 * q + 1) * L + r] = rs_word2int(s1);
			}
		}
	}
	// new history = the last 24 * M - 1 samples of history ++ tick; the pad slot takes a zero
	if (lane < HQ) {
		short4 h;
		short *hp = &h.x;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const int i = in_len + 4 * lane + k;
			hp[k] = (4 * lane + k < HIST) ? (short)xp[(i % M) * plen + i / M] : (short)0;
		}
		*reinterpret_cast<short4 *>(hist + 4 * lane) = h;
	}
	wave_sync(); // xp is read out before the wave's next member stages over it
}

// The phases of bridge_updown_kernel, their arithmetic word for word, with one more flag in a member's ratio byte:
//   (0) (A) (B) (G) on the leg's own rate / 100 samples at the leg's rate (rational_leg), the row `wide` samples;
//   (U) one wavefront per member: rated_up / updown_down as there, or for UD_R32 rational_run -- x 2/3 for a leg above the
//       mix, x 3/2 for one below it -- from the head of the row back over it;
//   (C) (D) at the conference's rate on the head of the rows;
//   (W) one wavefront per member: as there, or for UD_R32 rational_run the other way from the head of the row back over the
//       row (which held the leg's input, so it is wide enough), then updown_store.
__global__ __launch_bounds__(BT) void bridge_rational_kernel(RationalArgs qa) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const UpdownArgs &ua = qa.u;
	const LegsArgs &la = ua.l;
	const RatedArgs &ra = la.r;
	const BridgeArgs &a = ra.b;
	uint2 *rows = reinterpret_cast<uint2 *>(smem);
	int *s_sum = reinterpret_cast<int *>(smem + a.sum_off);
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	__shared__ unsigned char s_rt[BMAX], s_on[BMAX], s_cd[BMAX]; // a member's ratio | UD_ABOVE | UD_R32; whether it is here this tick; its codec pair
	const int t = threadIdx.x, c = blockIdx.x, mm = a.mm, ns = a.ns, nw = ns >> 2, ng = ns >> 3;
	const int s0 = c * mm;
	const uint8_t *in = static_cast<const uint8_t *>(a.in);
	uint8_t *out = static_cast<uint8_t *>(a.out);

	// ---- (0)
	mi_volume_params p;
	mi_volume_state st;
	float2 win = make_float2(0, 0);
	unsigned mflag = 0;
	int mgain_bits = 0, rt = 1;
	bool here = false;
	if (t < mm) {
		const int s = s0 + t;
		p = a.params[s];
		st = a.state[s];
		win = a.win[s];
		mflag = a.flags[s];
		mgain_bits = __float_as_int(a.gain[s]);
		here = !a.present || a.present[s] != 0;
		s_cd[t] = la.codec[s];
		rt = ra.ratio[s];
		s_rt[t] = (unsigned char)rt, s_on[t] = here;
	}
	for (int i = t; i < ns; i += BT) s_sum[i] = 0;

	// ---- (A) the leg's own groups; the rest of the row is zeros as far as the conference's tick reaches
	for (int mb = 0; mb < mm; mb += BT / 8) {
		const int m = mb + (t >> 3), q = t & 7;
		const bool valid = m < mm;
		int pk = 0, dc = 0;
		if (valid) {
			const bool on = !a.present || a.present[s0 + m] != 0;
			const int kind = la.codec[s0 + m] & 3, r = ra.ratio[s0 + m];
			const int ngl = rational_leg(r, ng), nz = max(ng, ngl);
			const uint8_t *src = in + (size_t)(s0 + m) * la.in_pitch;
			for (int g0 = q; g0 < nz; g0 += 32) {
				uint4 v[4];
#pragma unroll
				for (int i = 0; i < 4; ++i) { // straight-line loads: all in flight at once
					v[i] = make_uint4(0, 0, 0, 0);
					if (on && g0 + 8 * i < ngl) v[i] = load_raw_leg(src, kind, g0 + 8 * i);
				}
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const int g = g0 + 8 * i;
					if (g >= nz) continue;
					const uint4 d = decode_group_leg(v[i], kind, g);
					if (on && g < ngl) v[i] = d; // (code bytes of zero are not silence)
					rows[m * a.row_w + 2 * g] = make_uint2(v[i].x, v[i].y);
					rows[m * a.row_w + 2 * g + 1] = make_uint2(v[i].z, v[i].w);
					const unsigned w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						const int x0 = lo16(w[k]), x1 = hi16(w[k]);
						pk = max(pk, max(x0 < 0 ? -x0 : x0, x1 < 0 ? -x1 : x1));
						dc += x0 + x1;
					}
				}
			}
		}
#pragma unroll
		for (int off = 1; off < 8; off <<= 1) {
			pk = max(pk, __shfl_xor(pk, off));
			dc += __shfl_xor(dc, off);
		}
		if (valid && q == 0) s_pk[m] = pk, s_dc[m] = dc;
	}
	__syncthreads();

	// ---- (B) over the leg's rate / 100 samples, at the leg's rate
	if (t < mm) {
		if (here) {
			const uint2 *r = rows + t * a.row_w;
			const int nwl = rational_leg(rt, nw);
			float acc = 0;
#pragma unroll 4
			for (int i = 0; i < nwl; ++i) {
				const uint2 w = r[i];
				const int x0 = lo16(w.x), x1 = hi16(w.x), x2 = lo16(w.y), x3 = hi16(w.y);
				acc += (float)(x0 * x0);
				acc += (float)(x1 * x1);
				acc += (float)(x2 * x2);
				acc += (float)(x3 * x3);
			}
			const VolCtl o = volume_control(p, st, 0.f, acc, 4 * nwl, s_pk[t], s_dc[t], rational_leg(rt, a.sample_rate), win);
			s_par[t] = make_int4((int)mflag | (o.mode << 8), o.intgain, o.dcoff, mgain_bits);
			a.state[s0 + t] = st;
			a.win[s0 + t] = win;
		} else {
			s_par[t] = make_int4((int)mflag, 4096, 0, mgain_bits);
		}
	}
	__syncthreads();

	// ---- (G) apply_gain (msvolume.c:440) in front of the in_resampler, on the leg-rate samples
	const int nww = ua.wide >> 2;
	for (int item = t; item < mm * nww; item += BT) {
		const int m = item / nww, j = item - m * nww;
		const int4 par = s_par[m];
		const int mode = par.x >> 8;
		if (mode == 0 || j >= rational_leg(s_rt[m], nw)) continue;
		const uint2 cur = rows[m * a.row_w + j];
		int x[4] = {lo16(cur.x), hi16(cur.x), lo16(cur.y), hi16(cur.y)};
		const int ig = par.y, dc = (mode == 2) ? par.z : 0;
#pragma unroll
		for (int k = 0; k < 4; ++k) x[k] = sat16(((x[k] - dc) * ig) / 4096);
		rows[m * a.row_w + j] = make_uint2(pack16(x[0], x[1]), pack16(x[2], x[3]));
	}
	__syncthreads();

	// ---- (U) the in_resampler of a present, plumbed leg; any other keeps its history
	const int wave = t >> 6, lane = t & 63;
	float *scr = reinterpret_cast<float *>(smem + ra.scratch_off + wave * ra.scratch_per_wave);
	for (int m = wave; m < mm; m += BT / 64) {
		const int r = __builtin_amdgcn_readfirstlane(s_rt[m]), k = r & 7;
		if (r == 1 || (r & UD_R32) || !s_on[m] || !((unsigned)s_par[m].x & MI_MIX_LINKED)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(rows + m * a.row_w), *hist = ra.hist_in + (size_t)(s0 + m) * ua.hin_stride;
		if (r & UD_ABOVE) updown_down(scr, row, hist, ra.tab + ua.tab_down_in[k], k, ns * k, lane);
		else rated_up(scr, row, hist, ra.tab + ra.tab_up[k], k, ns / k, lane);
	}
	// (the legs at 3/2 and 2/3 in a loop of their own: what a helper keeps per lane stays live over its own loop only)
	for (int m = wave; m < mm; m += BT / 64) {
		const int r = __builtin_amdgcn_readfirstlane(s_rt[m]);
		if (!(r & UD_R32) || !s_on[m] || !((unsigned)s_par[m].x & MI_MIX_LINKED)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(rows + m * a.row_w), *hist = ra.hist_in + (size_t)(s0 + m) * ua.hin_stride;
		if (r & UD_ABOVE) rational_run<2, 3>(scr, row, hist, ra.tab + qa.tab_above_in, ns / 2 * 3, lane);
		else rational_run<3, 2>(scr, row, hist, ra.tab + qa.tab_below_in, ns / 3 * 2, lane);
	}
	__syncthreads();

	// ---- (C) the gain is in the rows already
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
		if (s_rt[m] != 1) { // the out_resampler's input, either direction
			rows[m * a.row_w + 2 * g] = make_uint2(pack16(o[0], o[1]), pack16(o[2], o[3]));
			rows[m * a.row_w + 2 * g + 1] = make_uint2(pack16(o[4], o[5]), pack16(o[6], o[7]));
			continue;
		}
		store_group_leg(out + (size_t)(s0 + m) * la.out_pitch, s_cd[m] >> 2, g, o);
	}
	__syncthreads();

	// ---- (W) the out_resampler of a pin with its output on, then the leg's store / encoder
	for (int m = wave; m < mm; m += BT / 64) {
		const int r = __builtin_amdgcn_readfirstlane(s_rt[m]), k = r & 7;
		if (r == 1 || (r & UD_R32) || !((unsigned)s_par[m].x & MI_MIX_OUTPUT)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(rows + m * a.row_w), *hist = ra.hist_out + (size_t)(s0 + m) * ra.hout_stride;
		const int kind = __builtin_amdgcn_readfirstlane(s_cd[m] >> 2);
		const size_t at = (size_t)(s0 + m) * la.out_pitch;
		if (r & UD_ABOVE) {
			rated_up(scr, row, hist, ra.tab + ua.tab_up_out[k], k, ns, lane);
			updown_store(row, out + at, kind, ns * k, lane);
		} else {
			rated_down<-1>(scr, row, hist, ra.tab + ra.tab_down[k], out, at, k, ns, lane, kind);
		}
	}
	for (int m = wave; m < mm; m += BT / 64) { // the legs at 3/2 and 2/3, in a loop of their own as in (U)
		const int r = __builtin_amdgcn_readfirstlane(s_rt[m]);
		if (!(r & UD_R32) || !((unsigned)s_par[m].x & MI_MIX_OUTPUT)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(rows + m * a.row_w), *hist = ra.hist_out + (size_t)(s0 + m) * ra.hout_stride;
		if (r & UD_ABOVE) rational_run<3, 2>(scr, row, hist, ra.tab + qa.tab_above_out, ns, lane);
		else rational_run<2, 3>(scr, row, hist, ra.tab + qa.tab_below_out, ns, lane);
		updown_store(row, out + (size_t)(s0 + m) * la.out_pitch, __builtin_amdgcn_readfirstlane(s_cd[m] >> 2), rational_leg(r, ns), lane);
	}
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
	RatedArgs ra = {};
	if (b->rated) {
		ra.b = a;
		ra.ratio = b->d_ratio, ra.hist_in = b->d_hist_in, ra.hist_out = b->d_hist_out, ra.tab = b->d_tab;
		memcpy(ra.tab_up, b->tab_up, sizeof(ra.tab_up));
		memcpy(ra.tab_down, b->tab_down, sizeof(ra.tab_down));
		ra.pitch = b->pitch, ra.hout_stride = b->hout_stride;
		ra.scratch_off = b->scratch_off, ra.scratch_per_wave = b->scratch_per_wave;
	}
	if (b->updown || b->rational) {
		UpdownArgs ua;
		ua.l.r = ra;
		// behind the concealer every leg's input is the PCM it worked on, at the pitch of its rows
		ua.l.codec = b->plc ? b->d_codec + b->n : b->d_codec;
		ua.l.in_pitch = b->plc ? b->pitch * 2 : (int)b->in_bytes, ua.l.out_pitch = (int)b->out_bytes;
		ua.wide = b->wide, ua.hin_stride = b->hin_stride;
		memcpy(ua.tab_down_in, b->tab_down_in, sizeof(ua.tab_down_in));
		memcpy(ua.tab_up_out, b->tab_up_out, sizeof(ua.tab_up_out));
		if (b->rational) {
			RationalArgs qa;
			qa.u = ua;
			qa.tab_above_in = b->tab_above_in, qa.tab_above_out = b->tab_above_out;
			qa.tab_below_in = b->tab_below_in, qa.tab_below_out = b->tab_below_out;
			hipLaunchKernelGGL(bridge_rational_kernel, grid, dim3(BT), b->lds, b->ctx->stream, qa);
			MI_LAUNCH_CHECK();
			return MI_OK;
		}
		hipLaunchKernelGGL(bridge_updown_kernel, grid, dim3(BT), b->lds, b->ctx->stream, ua);
		MI_LAUNCH_CHECK();
		return MI_OK;
	}
	if (b->d_codec) {
		LegsArgs la;
		la.r = ra, la.r.b = a;
		// behind the concealer, as above
		la.codec = b->plc ? b->d_codec + b->n : b->d_codec;
		la.in_pitch = b->plc ? b->pitch * 2 : (int)b->in_bytes, la.out_pitch = (int)b->out_bytes;
		if (b->rated) hipLaunchKernelGGL((bridge_legs_kernel<true>), grid, dim3(BT), b->lds, b->ctx->stream, la);
		else hipLaunchKernelGGL((bridge_legs_kernel<false>), grid, dim3(BT), b->lds, b->ctx->stream, la);
		MI_LAUNCH_CHECK();
		return MI_OK;
	}
	if (b->rated) {
		if (in_kind == MI_SESSION_PCM16) launch_rated_out<0>(cf.out_codec, grid, b->lds, b->ctx->stream, ra);
		else if (in_kind == MI_SESSION_PCMA) launch_rated_out<1>(cf.out_codec, grid, b->lds, b->ctx->stream, ra);
		else launch_rated_out<2>(cf.out_codec, grid, b->lds, b->ctx->stream, ra);
		MI_LAUNCH_CHECK();
		return MI_OK;
	}
	if (in_kind == MI_SESSION_PCM16) launch_out<0>(cf.out_codec, grid, b->lds, b->ctx->stream, a);
	else if (in_kind == MI_SESSION_PCMA) launch_out<1>(cf.out_codec, grid, b->lds, b->ctx->stream, a);
	else launch_out<2>(cf.out_codec, grid, b->lds, b->ctx->stream, a);
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
	if (h_leg_rate) {
		for (int s = 0; s < cfg->nstreams; ++s) {
			const int lr = h_leg_rate[s];
			MI_CHECK_ARG(lr > 0);
			const bool up = lr > cfg->rate;
			// 3/2 or 2/3, both rates multiples of 800: leg and mix are 2400 k and 1600 k Hz, their ticks 24 k and 16 k samples --
			// 8 k periods of 3 samples against 2: whole periods and whole eight-period tiles, eight-sample groups, both ways
			if (rational && ((int64_t)2 * lr == (int64_t)3 * cfg->rate || (int64_t)3 * lr == (int64_t)2 * cfg->rate)) {
				if (lr % 800 != 0) {
					mi::set_error("%s: leg %d's rate %d is no multiple of 800 (a 10 ms tick must be whole groups of 8 samples)", fn, s, lr);
					return MI_ENOTSUP;
				}
				if (cfg->plc && !leg_plc && common && lr != common) {
					mi::set_error("%s: plc with legs at %d Hz and %d Hz: the concealer batch has one rate", fn, common, lr);
					return MI_ENOTSUP;
				}
				if (!common) common = lr;
				(up ? r32_above : r32_below) = true;
				widest = std::max(widest, lr);
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
			if (lr % 800 != 0) {
				mi::set_error("%s: leg %d's rate %d is no multiple of 800 (a 10 ms tick must be whole groups of 8 samples)", fn, s, lr);
				return MI_ENOTSUP;
			}
			if (cfg->plc && !leg_plc && common && lr != common) {
				mi::set_error("%s: plc with legs at %d Hz and %d Hz: the concealer batch has one rate", fn, common, lr);
				return MI_ENOTSUP;
			}
			if (!common) common = lr;
			(up ? above : used)[r] = true;
			updown |= up;
			widest = std::max(widest, lr);
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
