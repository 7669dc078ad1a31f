// bridge_phases.hpp -- the phases of a conference tick (the head of bridge.hip describes them), each written ONCE as a
// __device__ __forceinline__ function; bridge.hip's five kernels, bridge_ratios.hip's one and bridge_offgrid.hip's one are
// compositions of them with the barriers in between (bridge_tick_kernel keeps three of them written out, for its pinned
// register figures: see its head).
// What differs between the kernels is a template parameter or data here:
//   FORMS  which resamplers a kernel has (Forms below), and with it how a member's ratio byte is read (leg_span);
//   SRC    where (A) takes a group from: FixedSrc<IN>, one compile-time codec on rows of samples, or LegSrc, every leg's own
//          codec on byte rows;
//   OUT    where eight samples of a mix go (store_group): a compile-time codec, the leg's own (BY_KIND), or back onto the
//          row in LDS (ON_ROW);
//   GAIN   whether (C) applies the Q12 gain or (G) has done so at the leg's rate.
// The helpers take the kernel's locals (Conf, built once at the kernel's head), not the argument structs: a phase inlined
// into a kernel reads what the kernel has in registers already.
#pragma once
#include "common.hpp"
#include "g711.hpp"
#include "volume_ctl.hpp"

#include "bridge_plan.hpp" // BT, the resamplers' constants, lengths and steps, the ratio byte's bits: what the host's plan shares

#pragma clang fp contract(off)

namespace {

// ---- the kernels' arguments.  Each kernel's struct holds the one before it, so the host fills an OffgridArgs once per bridge
// (mi_bridge::args, bridge.hip) and every kernel is passed its own part of it.
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

struct RatedArgs {
	BridgeArgs b;         // ns, sum_off, sample_rate: the conference's; row_w: of a row of UpdownArgs::wide samples where there is one
	const uint8_t *ratio; // [nconf * mm] a member's ratio byte (leg_span)
	int16_t *hist_in;     // [nconf * mm][48 or hin_stride] in_resampler: the last leg-side samples, as mi_resampler keeps them
	int16_t *hist_out;    // [nconf * mm][hout_stride] out_resampler: the last ratio * 48 - 1 conference-rate samples
	const float *tab;     // every table of the bridge, back to back
	int tab_up[7];        // float offset of ratio r's up table [r][48] (polyphase rows, mi_resampler's own layout)
	int tab_down[7];      // and of its down table, phase-major [r][48]: tap r * i + p at [p][i]
	int pitch;            // samples per row of in / out: the widest leg's tick (the kernels with compile-time codecs)
	int hout_stride;
	int scratch_off, scratch_per_wave; // bytes: each wavefront's resampler scratch in the dynamic LDS
};

struct LegsArgs {
	RatedArgs r;             // r.b.in / r.b.out: byte rows at one pitch (a multiple of 16); r.pitch is not read
	const uint8_t *codec;    // [nconf * mm] in_codec | out_codec << 2
	int in_pitch, out_pitch; // bytes per row
};

struct UpdownArgs {
	LegsArgs l;
	int wide;           // samples per LDS row: the widest leg's tick (>= ns)
	int hin_stride;     // samples per member of hist_in (hout_stride: of hist_out); either holds 47 or ratio * 48 - 1
	int tab_down_in[7]; // a leg above by ratio k: its in_resampler's table (leg -> conference), phase-major [k][48]
	int tab_up_out[7];  // and its out_resampler's (conference -> leg), polyphase rows [k][48]
};

struct RationalArgs {
	UpdownArgs u;
	// the four rational resamplers' taps, rearranged per (r, p') [L * M][24] (build_tables): of a leg ABOVE the mix the
	// in_resampler's (x 2/3) and the out_resampler's (x 3/2), of a leg below it the in_resampler's (x 3/2) and the
	// out_resampler's (x 2/3)
	int tab_above_in, tab_above_out, tab_below_in, tab_below_out;
};

struct RatiosArgs {
	RationalArgs q;
	// [64] by gen_code of a leg's ratio byte: the float offsets in `tab` of its in_resampler's table (leg -> conference, b rows)
	// and its out_resampler's (conference -> leg, a rows), polyphase rows as mi_resampler designs them
	const int2 *gen_tab;
};

struct OffgridArgs {
	RatiosArgs g;
	// the one pair of resamplers of the bridge's 44 100 Hz legs: leg : mix = num : den in lowest terms; the float offsets in
	// `tab` (multiples of four: a lane reads its row in 16-byte loads) of the in_resampler's per-phase table [den][filt_in] and
	// the out_resampler's [num][filt_out], as mi_resampler's generic kernel reads them
	int num, den, filt_in, filt_out, tab_in, tab_out;
};

// ---- a member's ratio byte (bridge_plan.hpp writes it).  A kernel meets only the forms it was built for:
enum Forms {
	F_SAME,  // every leg at the conference's rate: no ratio byte, no resampler
	F_BELOW, // legs at or below the mix
	F_ABOVE, // and above it
	F_R32,   // and at 3/2 or 2/3 of it
	F_GEN,   // and at a : b of it in the generic order (UD_GEN); at 4 and 1/4 through the forms above
	F_OFF,   // and at 44 100 Hz (UD_OFF): a tick of 441 samples, no whole groups of eight
};

// The one place where a ratio byte becomes a length or a rate: the leg's share of `conf` -- groups, words or samples of the
// conference's tick, or its sample rate.  F_SAME folds to `conf` at compile time.  off: what a leg at 44 100 Hz has of that
// unit, which is no share of the conference's -- OFFGRID_GROUPS, OFFGRID_WORDS (the tail group and word counted), OFFGRID_LEN or
// OFFGRID_RATE; read by a kernel with F_OFF only.
template <int FORMS>
__device__ __forceinline__ int leg_span(int r, int conf, int off = 0) {
	if (FORMS == F_SAME) return conf;
	if (FORMS >= F_OFF && is_offgrid(r)) return off;
	if (FORMS >= F_GEN && (r & UD_GEN)) return conf / gen_b(r) * gen_a(r);
	if (FORMS >= F_R32 && (r & UD_R32)) return (r & UD_ABOVE) ? conf / 2 * 3 : conf / 3 * 2;
	if (FORMS >= F_ABOVE && (r & UD_ABOVE)) return conf * (r & 7);
	return conf / r;
}

__device__ __forceinline__ int lo16(unsigned w) { return (int)(short)(w & 0xffffu); }
__device__ __forceinline__ int hi16(unsigned w) { return (int)(short)(w >> 16); }

// ---- a kernel's view of its conference, built once at its head: the dynamic LDS, the kernel's static arrays (null where it
// has none) and the locals every phase reads
struct Conf {
	uint2 *rows;      // [mm][row_w] the members' ticks, four samples per word
	int *s_sum;       // [ns] the conference's int32 sum
	int *s_pk, *s_dc; // [BMAX] a member's integer peak and DC sum
	int4 *s_par;      // [BMAX] what (C) and (D) need of a member: (flags | mode << 8, Q12 gain, DC offset, pin gain)
	unsigned char *s_rt, *s_on, *s_cd; // [BMAX] a member's ratio byte; whether it is here this tick; its codec pair
	int t, s0;        // the lane; the conference's first stream
	int mm, ns, nw, ng, row_w; // members; the conference's tick in samples, four-sample words and eight-sample groups; the row pitch
};

__device__ __forceinline__ Conf conf_view(const BridgeArgs &a, char *smem, int *s_pk, int *s_dc, int4 *s_par, unsigned char *s_rt = nullptr,
                                          unsigned char *s_on = nullptr, unsigned char *s_cd = nullptr) {
	return {reinterpret_cast<uint2 *>(smem), reinterpret_cast<int *>(smem + a.sum_off), s_pk, s_dc, s_par, s_rt, s_on, s_cd,
	        (int)threadIdx.x, (int)blockIdx.x * a.mm, a.mm, a.ns, a.ns >> 2, a.ns >> 3, a.row_w};
}

// ---- where (A) takes a member's groups from.  fetch is the load, issued four deep before `decoded` touches the first.
// One compile-time codec (KIND 0: 16-bit PCM, 1: A-law, 2: mu-law) on rows of `pitch` samples: eight samples of row s, group
// g, as packed PCM straight from the load
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

template <int IN>
struct FixedSrc {
	const void *in;
	int pitch;
	__device__ __forceinline__ int kind(int) const { return IN; }
	__device__ __forceinline__ uint4 fetch(int s, int, int g) const { return load_group<IN>(in, (size_t)s, pitch, g); }
	__device__ __forceinline__ uint4 decoded(uint4 v, int, int) const { return v; }
};

// every leg's own codec on byte rows of `pitch` bytes (load_raw_leg / decode_group_leg, g711.hpp): the kind is uniform over
// a member's eight lanes
struct LegSrc {
	const uint8_t *in;
	int pitch;
	const uint8_t *codec;
	__device__ __forceinline__ int kind(int s) const { return codec[s] & 3; }
	__device__ __forceinline__ uint4 fetch(int s, int kind, int g) const { return load_raw_leg(in + (size_t)s * pitch, kind, g); }
	__device__ __forceinline__ uint4 decoded(uint4 v, int kind, int g) const { return decode_group_leg(v, kind, g); }
	// the first REM < 8 code units of group g, one load each and not a byte past them, where fetch's 16 bytes have them
	template <int REM>
	__device__ __forceinline__ uint4 fetch_tail(int s, int kind, int g) const {
		const uint8_t *row = in + (size_t)s * pitch;
		uint32_t w[4] = {0, 0, 0, 0}, c[2] = {0, 0};
		if (kind == MI_SESSION_PCM16) {
			const uint16_t *p = reinterpret_cast<const uint16_t *>(row + 16 * g);
#pragma unroll
			for (int j = 0; j < REM; ++j) w[j >> 1] |= (uint32_t)p[j] << (16 * (j & 1));
			return make_uint4(w[0], w[1], w[2], w[3]);
		}
#pragma unroll
		for (int j = 0; j < REM; ++j) c[j >> 2] |= (uint32_t)row[8 * g + j] << (8 * (j & 3));
		return (g & 1) ? make_uint4(0, 0, c[0], c[1]) : make_uint4(c[0], c[1], 0, 0);
	}
};

// eight packed samples with all but the first REM zero: a tail group as it stands on a row (a code byte of zero is no silence)
template <int REM>
__device__ __forceinline__ uint4 keep_head(uint4 d) {
	uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
	for (int i = 0; i < 4; ++i) w[i] &= 2 * i + 1 < REM ? 0xffffffffu : 2 * i < REM ? 0xffffu : 0u;
	return make_uint4(w[0], w[1], w[2], w[3]);
}
constexpr int OFFGRID_TAIL = OFFGRID_LEN & 7; // samples in the tail group of a 441-sample tick: one

// ---- where eight samples of a mix go: group g of the row that starts `at` code units into `out`, as 16 bytes of PCM or 8
// code words.  OUT 0, 1, 2: the codec at compile time, a unit one sample of it; BY_KIND: the leg's own, `kind`, a unit one
// byte; ON_ROW: PCM onto a row in LDS, whose pitch keeps 8 bytes' alignment
constexpr int BY_KIND = -1, ON_ROW = -2;

template <int OUT>
__device__ __forceinline__ void store_group(uint8_t *out, size_t at, int g, const int (&o)[8], int kind = OUT) {
	const uint4 pcm = make_uint4(pack16(o[0], o[1]), pack16(o[2], o[3]), pack16(o[4], o[5]), pack16(o[6], o[7]));
	if (OUT == ON_ROW) {
		uint2 *d = reinterpret_cast<uint2 *>(out + at + 16 * g);
		d[0] = make_uint2(pcm.x, pcm.y), d[1] = make_uint2(pcm.z, pcm.w);
		return;
	}
	if (OUT == 0) {
		*reinterpret_cast<uint4 *>(reinterpret_cast<int16_t *>(out) + at + 8 * g) = pcm;
		return;
	}
	uint8_t *row = out + at;
	if (OUT == BY_KIND && kind == MI_SESSION_PCM16) {
		*reinterpret_cast<uint4 *>(row + 16 * g) = pcm;
		return;
	}
	uint32_t cw[2] = {0, 0};
#pragma unroll
	for (int k = 0; k < 8; ++k) { // BY_KIND: both laws and a select -- a wavefront of (D) holds legs of either
		const uint32_t a = OUT == 2 ? 0u : lin2alaw(o[k]), u = OUT == 1 ? 0u : lin2ulaw(o[k]);
		cw[k >> 2] |= ((OUT == BY_KIND ? kind == MI_SESSION_PCMU : OUT == 2) ? u : a) << (8 * (k & 3));
	}
	*reinterpret_cast<uint2 *>(row + 8 * g) = make_uint2(cw[0], cw[1]);
}

// ---- (0) lane t < mm: its member's MSVolume parameters, state and window, its mixer controls, its `present` byte; its
// ratio byte and codec pair into LDS where the kernel has them.  All lanes: the sum row zeroed.
// p, st: the kernel's own locals, handed to volume_control as they are; left unset in a lane without a member
struct Member {
	float2 win = make_float2(0, 0);
	unsigned mflag = 0;
	int mgain_bits = 0, rt = 1;
	bool here = false;
};

template <int FORMS, bool CODEC>
__device__ __forceinline__ Member load_member(const Conf &k, const BridgeArgs &a, const uint8_t *ratio, const uint8_t *codec, mi_volume_params &p,
                                              mi_volume_state &st) {
	Member me;
	if (k.t < k.mm) {
		const int s = k.s0 + k.t;
		p = a.params[s];
		st = a.state[s];
		me.win = a.win[s];
		me.mflag = a.flags[s];
		me.mgain_bits = __float_as_int(a.gain[s]);
		me.here = !a.present || a.present[s] != 0;
		if (CODEC) k.s_cd[k.t] = codec[s];
		if (FORMS != F_SAME) {
			me.rt = ratio[s];
			k.s_rt[k.t] = (unsigned char)me.rt, k.s_on[k.t] = me.here;
		}
	}
	for (int i = k.t; i < k.ns; i += BT) k.s_sum[i] = 0;
	return me;
}

// ---- (A) eight lanes per member (32 members a round): the leg's own groups into its row, four groups in flight per lane,
// the rest of the row zeros as far as the conference's tick reaches; integer peak and DC sum (update_energy's integer part,
// msvolume.c:393-399: |x| up to 32768) reduced over the eight lanes in registers.  An absent member's row is zeros
// (audiomixer.c:88).
template <int FORMS, class SRC>
__device__ __forceinline__ void stage_rows(const Conf &k, const uint8_t *present, const uint8_t *ratio, const SRC &src) {
	for (int mb = 0; mb < k.mm; mb += BT / 8) {
		const int m = mb + (k.t >> 3), q = k.t & 7;
		const bool valid = m < k.mm;
		int pk = 0, dc = 0;
		if (valid) {
			const int s = k.s0 + m;
			const bool on = !present || present[s] != 0;
			const int kind = src.kind(s);
			const int rb = FORMS == F_SAME ? 1 : ratio[s];
			const int ngl = leg_span<FORMS>(rb, k.ng, OFFGRID_GROUPS), nz = FORMS >= F_ABOVE ? max(k.ng, ngl) : k.ng;
			// a 441-sample tick's last group holds one sample: read alone, the group's other seven zeros on the row
			const int tail = FORMS >= F_OFF && is_offgrid(rb) ? OFFGRID_GROUPS - 1 : -1;
			for (int g0 = q; g0 < nz; g0 += 32) {
				uint4 v[4];
#pragma unroll
				for (int i = 0; i < 4; ++i) { // straight-line loads: all in flight at once
					v[i] = make_uint4(0, 0, 0, 0);
					if constexpr (FORMS >= F_OFF) {
						if (on && g0 + 8 * i == tail) v[i] = src.template fetch_tail<OFFGRID_TAIL>(s, kind, tail);
						else if (on && g0 + 8 * i < ngl) v[i] = src.fetch(s, kind, g0 + 8 * i);
					} else if (on && g0 + 8 * i < ngl) v[i] = src.fetch(s, kind, g0 + 8 * i);
				}
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const int g = g0 + 8 * i;
					if (g >= nz) continue;
					uint4 d = src.decoded(v[i], kind, g);
					if (FORMS >= F_OFF && g == tail) d = keep_head<OFFGRID_TAIL>(d);
					if (on && g < ngl) v[i] = d; // (code bytes of zero are not silence)
					k.rows[m * k.row_w + 2 * g] = make_uint2(v[i].x, v[i].y);
					k.rows[m * k.row_w + 2 * g + 1] = make_uint2(v[i].z, v[i].w);
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
		if (valid && q == 0) k.s_pk[m] = pk, k.s_dc[m] = dc;
	}
}

// ---- (B) lane t < mm: the float32 sum of squares IN SAMPLE ORDER (the same additions in the same order as update_energy's
// loop: the order is part of the reference's result) over the leg's own samples, and the control chain at the leg's rate
// (volume_control, volume_ctl.hpp: MSVolume sits in front of the in_resampler); state and one-second window written back.
// An absent member is skipped whole: MSVolume got no chunk (msvolume.c:480-486).
template <int FORMS>
__device__ __forceinline__ void meter(const Conf &k, const BridgeArgs &a, Member &me, const mi_volume_params &p, mi_volume_state &st) {
	if (k.t < k.mm) {
		if (me.here) {
			const uint2 *r = k.rows + k.t * k.row_w;
			const int nwl = leg_span<FORMS>(me.rt, k.nw, OFFGRID_WORDS); // (a tail word's other samples are zeros: + 0.f)
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
			const VolCtl o = volume_control(p, st, 0.f, acc, leg_span<FORMS>(me.rt, k.ns, OFFGRID_LEN), k.s_pk[k.t], k.s_dc[k.t],
			                                leg_span<FORMS>(me.rt, a.sample_rate, OFFGRID_RATE), me.win);
			k.s_par[k.t] = make_int4((int)me.mflag | (o.mode << 8), o.intgain, o.dcoff, me.mgain_bits);
			a.state[k.s0 + k.t] = st;
			a.win[k.s0 + k.t] = me.win;
		} else {
			k.s_par[k.t] = make_int4((int)me.mflag, 4096, 0, me.mgain_bits);
		}
	}
}

// apply_gain on four samples (msvolume.c:440: a gain of exactly 1 -- mode 0 -- leaves them alone)
__device__ __forceinline__ void apply_gain(int (&x)[4], const int4 &par) {
	const int mode = par.x >> 8;
	if (mode == 0) return;
	const int ig = par.y, dc = (mode == 2) ? par.z : 0;
#pragma unroll
	for (int j = 0; j < 4; ++j) x[j] = sat16(((x[j] - dc) * ig) / 4096);
}

// ---- (G) the Q12 gain on the leg-rate samples, in the row: apply_gain stands in front of the in_resampler, whose history
// keeps the levelled samples.  nww: words per row to walk, the widest leg's tick
template <int FORMS>
__device__ __forceinline__ void level_legs(const Conf &k, int nww) {
	for (int item = k.t; item < k.mm * nww; item += BT) {
		const int m = item / nww, j = item - m * nww;
		const int4 par = k.s_par[m];
		if ((par.x >> 8) == 0 || j >= leg_span<FORMS>(k.s_rt[m], k.nw, OFFGRID_WORDS)) continue;
		const uint2 cur = k.rows[m * k.row_w + j];
		int x[4] = {lo16(cur.x), hi16(cur.x), lo16(cur.y), hi16(cur.y)};
		apply_gain(x, par);
		if (FORMS >= F_OFF && is_offgrid(k.s_rt[m]) && j == OFFGRID_WORDS - 1) { // the tail word: no sample past the tick's last
#pragma unroll
			for (int i = OFFGRID_LEN & 3; i < 4; ++i) x[i] = 0;
		}
		k.rows[m * k.row_w + j] = make_uint2(pack16(x[0], x[1]), pack16(x[2], x[3]));
	}
}

// ---- (C) lane = (member slice, four columns): the Q12 gain where (G) has not applied it (GAIN), then the pin's
// contribution as channel_process_in leaves it (0 unless linked and active; input gain, audiomixer.c:46-51) back into the
// row, and the int32 sum over the slice's members added into the conference's sum row (integer addition: any order).  The
// members are sliced so that an 80-sample tick, 20 four-column words wide, still occupies 240 lanes.
template <bool GAIN>
__device__ __forceinline__ void mix(const Conf &k, int nslice) {
	for (int item = k.t; item < nslice * k.nw; item += BT) {
		const int r = item / k.nw, j = item - r * k.nw;
		int sum[4] = {0, 0, 0, 0};
		for (int m = r; m < k.mm; m += nslice) {
			const int4 par = k.s_par[m];
			const unsigned f = (unsigned)par.x & 0xffu;
			uint2 o = make_uint2(0, 0);
			if ((f & MI_MIX_LINKED) && (f & MI_MIX_ACTIVE)) {
				const uint2 cur = k.rows[m * k.row_w + j];
				int x[4] = {lo16(cur.x), hi16(cur.x), lo16(cur.y), hi16(cur.y)};
				if (GAIN) apply_gain(x, par);
				const float gn = __int_as_float(par.w);
				if (gn != 1.0f) {
#pragma unroll
					for (int i = 0; i < 4; ++i) x[i] = sat16((int)(gn * (float)x[i]));
				}
#pragma unroll
				for (int i = 0; i < 4; ++i) sum[i] += x[i];
				o = make_uint2(pack16(x[0], x[1]), pack16(x[2], x[3]));
			}
			k.rows[m * k.row_w + j] = o;
		}
#pragma unroll
		for (int i = 0; i < 4; ++i) atomicAdd(&k.s_sum[4 * j + i], sum[i]);
	}
}

// ---- (D) lane = (member, eight columns), for every pin with its output enabled: saturate(sum - own)
// (channel_process_out) to the leg's store or encoder, consecutive lanes, consecutive bytes -- or, for a member with an
// out_resampler, over its own row: that resampler's input.  out: the legs' rows, `pitch` code units each (store_group)
template <int FORMS, int OUT>
__device__ __forceinline__ void mix_minus(const Conf &k, uint8_t *out, int pitch) {
	for (int item = k.t; item < k.mm * k.ng; item += BT) {
		const int m = item / k.ng, g = item - m * k.ng;
		if (!((unsigned)k.s_par[m].x & MI_MIX_OUTPUT)) continue;
		const uint2 own0 = k.rows[m * k.row_w + 2 * g], own1 = k.rows[m * k.row_w + 2 * g + 1];
		const int4 sa = *reinterpret_cast<const int4 *>(k.s_sum + 8 * g), sb = *reinterpret_cast<const int4 *>(k.s_sum + 8 * g + 4);
		const int o[8] = {sat16(sa.x - lo16(own0.x)), sat16(sa.y - hi16(own0.x)), sat16(sa.z - lo16(own0.y)), sat16(sa.w - hi16(own0.y)),
		                  sat16(sb.x - lo16(own1.x)), sat16(sb.y - hi16(own1.x)), sat16(sb.z - lo16(own1.y)), sat16(sb.w - hi16(own1.y))};
		if (FORMS != F_SAME && k.s_rt[m] != 1) store_group<ON_ROW>(reinterpret_cast<uint8_t *>(k.rows + m * k.row_w), 0, g, o);
		else store_group<OUT>(out, (size_t)(k.s0 + m) * pitch, g, o, OUT == BY_KIND ? k.s_cd[m] >> 2 : OUT);
	}
}

// ---- the resamplers, one wavefront running one member's: the steps of resample_steps.hpp, which mi_resampler's batch
// kernels (resample.hip) are composed of as well -- the same shares from zero accumulators, added in the same order.  Here a
// member's tick is read from the head of its row in LDS and its history from HBM, a loop of quads over the 64 lanes, and the
// tables arrive as the lanes read them (build_tables, bridge.hip).

// An up-sampler by `den`: out[m * den + p] = sum_j table[p][j] * x[m + j], one share per output, the result written over the
// row.  x: [rs_flat_len(in_len)] floats.
__device__ __forceinline__ void rated_up(float *x, int16_t *row, int16_t *hist, const float *tab, int den, int in_len, int lane) {
	constexpr int HIST = RS_FILT - 1, HQ = RS_FILT / 4;
	for (int q = lane; q < HQ + (in_len >> 2); q += 64) {
		const short4 v = q < HQ ? *reinterpret_cast<const short4 *>(hist + 4 * q) : *reinterpret_cast<const short4 *>(row + 4 * (q - HQ));
		scatter_quad<1>(x, v, q, HQ, HIST, 1, 0);
	}
	for (int i = HIST + in_len + lane; i < rs_flat_len(in_len); i += 64) x[i] = 0.f;
	wave_sync(); // the whole tick is staged before the first output lands on the row
	const int nlanes = den * (in_len >> 3);
	for (int base = 0; base < nlanes; base += 64) {
		const int l = base + lane;
		const bool on = l < nlanes;
		const int tile = on ? l / den : 0, p = on ? l - tile * den : 0;
		f2 t2[RS_FILT / 2], acc2[RS_R / 2];
		load_taps<RS_FILT>(tab + p * RS_FILT, t2);
		fir_share<RS_FILT>(x + tile * RS_R, t2, acc2);
		if (on) {
#pragma unroll
			for (int q = 0; q < RS_R / 2; ++q) {
				row[(tile * RS_R + 2 * q) * den + p] = rs_word2int(acc2[q].x);
				row[(tile * RS_R + 2 * q + 1) * den + p] = rs_word2int(acc2[q].y);
			}
		}
	}
	// history_quad(x, lane, HIST, in_len, 1, 0) written out, the pad slot taking the zero slack instead of a test: with the
	// step's select bridge_ratios_kernel, which sits at its 128 VGPRs, spills one (profiles/resample_steps.md)
	if (lane < HQ) {
		const float *hx = x + in_len + 4 * lane;
		short4 h;
		h.x = (int16_t)hx[0], h.y = (int16_t)hx[1], h.z = (int16_t)hx[2], h.w = (int16_t)hx[3];
		*reinterpret_cast<short4 *>(hist + 4 * lane) = h;
	}
	wave_sync(); // x is read out before the wave's next member stages over it
}

// A down-sampler by `num` (a run-time count): lane (tile, phase) computes its phase's share of eight outputs, the shares meet
// in LDS; the in_len / num outputs leave through store_group<OUT> at `at` of `sink`, eight per lane: a leg's row behind a pin,
// the head of the row itself (ON_ROW) in front of one.  tab: phase-major [num][48].  xp: [num][plen] ++ [in_len] floats.
// `kind` is the same in every lane of the wave.
template <int OUT>
__device__ __forceinline__ void resample_down(float *xp, const int16_t *row, int16_t *hist, const float *tab, int num, int in_len, int plen,
                                              int lane, uint8_t *sink, size_t at, int kind = OUT) {
	const int HIST = num * RS_FILT - 1, hq = (num * RS_FILT) >> 2, nq = hq + (in_len >> 2);
	const int out_len = in_len / num;
	float *part = xp + num * plen; // [out_len][num] partial sums
	for (int i = lane; i < num * plen; i += 64) xp[i] = 0.f;
	wave_sync();
	for (int q = lane; q < nq; q += 64) { // (a 287-sample history is more than one pass of the 64 lanes)
		const short4 v = q < hq ? *reinterpret_cast<const short4 *>(hist + 4 * q) : *reinterpret_cast<const short4 *>(row + 4 * (q - hq));
		scatter_quad<1>(xp, v, q, hq, HIST, num, plen);
	}
	wave_sync(); // the whole tick is staged before the first output lands on the row
	const int nlanes = num * (out_len >> 3);
	for (int base = 0; base < nlanes; base += 64) {
		const int l = base + lane;
		const bool on = l < nlanes;
		const int tile = on ? l / num : 0, p = on ? l - tile * num : 0;
		f2 t2[RS_FILT / 2], acc2[RS_R / 2];
		load_taps<RS_FILT>(tab + p * RS_FILT, t2);
		fir_share<RS_FILT>(xp + p * plen + tile * RS_R, t2, acc2);
		if (on) {
			float *d = part + (tile * RS_R) * num + p;
#pragma unroll
			for (int q = 0; q < RS_R / 2; ++q) d[(2 * q) * num] = acc2[q].x, d[(2 * q + 1) * num] = acc2[q].y;
		}
	}
	wave_sync();
	for (int g = lane; g < (out_len >> 3); g += 64) {
		int o[8];
		gather_group(part + g * 8 * num, num, o);
		store_group<OUT>(sink, at, g, o, kind);
	}
	for (int q = lane; q < hq; q += 64) *reinterpret_cast<short4 *>(hist + 4 * q) = history_quad(xp, q, HIST, in_len, num, plen);
	wave_sync(); // xp is read out before the wave's next member stages over it
}

// One member's rational resampler, L / M = 3/2 or 2/3 (resample_split_kernel's head has the indices).  tab: rearranged on the
// host per (r, p'), [r * M + p'][24].  Lane (tile, r) computes the M shares of its eight outputs one after the other into
// accumulators of their own and adds them upward from 0.f: the bits of the batch kernel's partial-sum array without the
// array.  The in_len samples at the head of `row` are the input, the in_len / M * L outputs are written back over the row
// once the whole tick is staged -- the in_resampler in front of a pin as it stands, the out_resampler behind it with
// store_row after it.  xp: [2][M][plen] floats.
template <int L, int M>
__device__ __forceinline__ void rational_run(float *xp, int16_t *row, int16_t *hist, const float *tab, int in_len, int lane) {
	constexpr int NT = RQ_FT * M, HIST = NT - 1, HQ = NT / 4;
	static_assert((L - 1) * M / L + M - 1 < 2 * M, "u / M is 0 or 1: two copies of the phase arrays");
	const int plen = rs_plen_odd(RQ_FT, M, in_len), periods = in_len / M;
	for (int i = lane; i < 2 * M * plen; i += 64) xp[i] = 0.f;
	wave_sync();
	for (int q = lane; q < HQ + (in_len >> 2); q += 64) {
		const short4 v = q < HQ ? *reinterpret_cast<const short4 *>(hist + 4 * q) : *reinterpret_cast<const short4 *>(row + 4 * (q - HQ));
		scatter_quad<2>(xp, v, q, HQ, HIST, M, plen);
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
			load_taps<RQ_FT>(tab + (r * M + pp) * RQ_FT, t2);
			fir_share<RQ_FT>(xp + u * plen + tile * RS_R, t2, acc2[pp]);
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
	if (lane < HQ) *reinterpret_cast<short4 *>(hist + 4 * lane) = history_quad(xp, lane, HIST, in_len, M, plen);
	wave_sync(); // xp is read out before the wave's next member stages over it
}


// One member's resampler at num : den (in : out, lowest terms) in mi_resampler's GENERIC order: resample_generic_kernel's
// arithmetic (resample.hip) with a direct table.  History ++ tick staged as floats; output k is ONE __builtin_fmaf chain from
// 0.f over taps j = 0 .. filt - 1 of table row (k * num) % den against x[(k * num) / den + j], then rs_word2int; the last
// filt - 1 samples of history ++ tick are the new history (a tick shorter than the history keeps part of the old one).  A
// tick is whole periods of `num` samples, so mi_resampler's position state is (0, 0) at every tick's start and the bridge
// keeps none.  The in_len samples at the head of `row` are the input, the in_len / num * den outputs go back over the row
// once the whole tick is staged, as rational_run's.  The taps are read from LDS: the `den` rows of the table, staged per
// member behind x at a pitch of filt + 1 floats (lanes of different phases would meet on one bank at a pitch of 48 .. 128);
// generic_scratch (bridge_plan.hpp) budgets both.  x reads run at a stride of num / den floats across the lanes.
__device__ __forceinline__ void generic_run(float *x, int16_t *row, int16_t *hist, const float *tab, int num, int den, int filt, int in_len,
                                            int lane) {
	const int hl = filt - 1, pitch = filt + 1, out_len = in_len / num * den;
	float *taps = x + generic_xlen(filt, in_len);
	for (int i = lane; i < hl; i += 64) x[i] = (float)hist[i];
	for (int i = lane; i < in_len; i += 64) x[hl + i] = (float)row[i];
	for (int i = lane; i < den * filt; i += 64) {
		const int r = i / filt;
		taps[r * pitch + (i - r * filt)] = tab[i];
	}
	wave_sync(); // the whole tick is staged before the first output lands on the row
	for (int k = lane; k < out_len; k += 64) {
		const int t = k * num, last = t / den, frac = t - last * den;
		const float *sc = taps + frac * pitch, *ip = x + last;
		float sum = 0.f;
#pragma unroll 8
		for (int j = 0; j < filt; ++j) sum = __builtin_fmaf(sc[j], ip[j], sum);
		row[k] = rs_word2int(sum);
	}
	for (int i = lane; i < hl; i += 64) hist[i] = (int16_t)x[in_len + i];
	wave_sync(); // x is read out before the wave's next member stages over it
}

// One member's resampler at num : den (in : out, lowest terms) in mi_resampler's generic order on the PER-PHASE table, which
// stays in memory: the 44 100 Hz legs' (mi_bridge_create_offgrid).  generic_run's arithmetic to the bit -- output k is ONE
// __builtin_fmaf chain from 0.f over taps j = 0 .. filt - 1 of table row (k * num) % den against x[(k * num) / den + j], then
// rs_word2int; the last filt - 1 samples of history ++ tick are the new history -- but nothing of the table is staged: it is 28
// to 92 KB, no wavefront's scratch holds it, and a tick uses every row of it about once (441 rows for 441 outputs, 160 for
// 160), so a staged copy would be read once as well.  Each lane reads ITS output's row, filt floats (a multiple of eight, the
// row 16-byte aligned), in 16-byte loads, two in flight per step; the rows are the same for every such leg of the launch and
// stay in L2.  x: [generic_xlen(filt, in_len)] floats.  A tick is whole periods of `num` samples: no position state.
__device__ __forceinline__ void offgrid_run(float *x, int16_t *row, int16_t *hist, const float *tab, int num, int den, int filt, int in_len,
                                            int lane) {
	const int hl = filt - 1, out_len = in_len / num * den;
	for (int i = lane; i < hl; i += 64) x[i] = (float)hist[i];
	for (int i = lane; i < in_len; i += 64) x[hl + i] = (float)row[i];
	wave_sync(); // the whole tick is staged before the first output lands on the row
	for (int k = lane; k < out_len; k += 64) {
		const int t = k * num, last = t / den, frac = t - last * den;
		const float4 *sc = reinterpret_cast<const float4 *>(tab + (size_t)frac * filt);
		const float *ip = x + last;
		float sum = 0.f;
		for (int j = 0; j < (filt >> 3); ++j) {
			const float4 a = sc[2 * j], b = sc[2 * j + 1];
			const float *w = ip + 8 * j;
			sum = __builtin_fmaf(a.x, w[0], sum);
			sum = __builtin_fmaf(a.y, w[1], sum);
			sum = __builtin_fmaf(a.z, w[2], sum);
			sum = __builtin_fmaf(a.w, w[3], sum);
			sum = __builtin_fmaf(b.x, w[4], sum);
			sum = __builtin_fmaf(b.y, w[5], sum);
			sum = __builtin_fmaf(b.z, w[6], sum);
			sum = __builtin_fmaf(b.w, w[7], sum);
		}
		row[k] = rs_word2int(sum);
	}
	for (int i = lane; i < hl; i += 64) hist[i] = (int16_t)x[in_len + i];
	wave_sync(); // x is read out before the wave's next member stages over it
}

// what an up-sampler behind a pin left on the member's row -- its out_resampler's `len` leg-rate samples -- through the leg's
// store or encoder, 16 bytes of PCM or 8 code words per lane
__device__ __forceinline__ void store_row(const int16_t *row, uint8_t *out, int kind, int len, int lane) {
	for (int g = lane; g < (len >> 3); g += 64) {
		const uint2 *r = reinterpret_cast<const uint2 *>(row + 8 * g);
		const uint2 w0 = r[0], w1 = r[1];
		const int o[8] = {lo16(w0.x), hi16(w0.x), lo16(w0.y), hi16(w0.y), lo16(w1.x), hi16(w1.x), lo16(w1.y), hi16(w1.y)};
		store_group<BY_KIND>(out, 0, g, o, kind);
	}
}

// the REM < 8 samples behind the `groups` whole groups store_row has stored, one store each and not a byte past them: the
// row's tail in the host buffers stays as it is
template <int REM>
__device__ __forceinline__ void store_tail(const int16_t *row, uint8_t *out, int kind, int groups, int lane) {
	if (lane >= REM) return;
	const int i = 8 * groups + lane, x = row[i];
	if (kind == MI_SESSION_PCM16) reinterpret_cast<int16_t *>(out)[i] = (int16_t)x;
	else out[i] = (uint8_t)(kind == MI_SESSION_PCMU ? lin2ulaw(x) : lin2alaw(x));
}

// a wavefront's resampler scratch in the dynamic LDS
__device__ __forceinline__ float *wave_scratch(char *smem, const RatedArgs &ra, int t) {
	return reinterpret_cast<float *>(smem + ra.scratch_off + (t >> 6) * ra.scratch_per_wave);
}

// a member's ratio byte in (U) and (W), where one wavefront runs the member.  Uniform over the wave by construction; the
// kernels with legs above the mix say so to the compiler, those without keep the per-lane read their register figures
// were settled with
template <int FORMS>
__device__ __forceinline__ int wave_ratio(const Conf &k, int m) {
	return FORMS >= F_ABOVE ? __builtin_amdgcn_readfirstlane(k.s_rt[m]) : (int)k.s_rt[m];
}

// ---- (U) one wavefront per member, the four waves taking members in turn: the in_resampler of a present, plumbed leg (the
// run mask present & linked of mi_resampler_process_masked; any other keeps its history), from the head of the row back over
// it -- rated_up for a leg below the mix, resample_down for one above it, rational_run (x 3/2 below, x 2/3 above) for
// UD_R32, generic_run for UD_GEN, offgrid_run for UD_OFF (loops of their own as well).  ua, qa, ga, oa: null in a kernel without
// those forms.
// The legs at 3/2 and 2/3 have a loop of their own, here and in (W): what a helper keeps per lane stays live over its own
// loop only, and one loop over all forms is how a kernel goes past 128 VGPRs.
template <int FORMS>
__device__ __forceinline__ void resample_in(const Conf &k, const RatedArgs &ra, const UpdownArgs *ua, const RationalArgs *qa, float *scr,
                                            const RatiosArgs *ga = nullptr, const OffgridArgs *oa = nullptr) {
	const int wave = k.t >> 6, lane = k.t & 63, ns = k.ns;
	const int hin = FORMS >= F_ABOVE ? ua->hin_stride : RS_FILT;
	for (int m = wave; m < k.mm; m += BT / 64) {
		const int r = wave_ratio<FORMS>(k, m), n = FORMS >= F_ABOVE ? r & 7 : r;
		if (r == 1 || (FORMS >= F_R32 && (r & UD_R32)) || (FORMS >= F_GEN && (r & UD_GEN)) || (FORMS >= F_OFF && (r & UD_OFF)) || !k.s_on[m] ||
		    !((unsigned)k.s_par[m].x & MI_MIX_LINKED))
			continue;
		int16_t *row = reinterpret_cast<int16_t *>(k.rows + m * k.row_w), *hist = ra.hist_in + (size_t)(k.s0 + m) * hin;
		if (FORMS >= F_ABOVE && (r & UD_ABOVE))
			resample_down<ON_ROW>(scr, row, hist, ra.tab + ua->tab_down_in[n], n, ns * n, rs_plen_odd(RS_FILT, n, ns * n), lane, reinterpret_cast<uint8_t *>(row), 0);
		else rated_up(scr, row, hist, ra.tab + ra.tab_up[n], n, ns / n, lane);
	}
	if (FORMS < F_R32) return;
	for (int m = wave; m < k.mm; m += BT / 64) {
		const int r = __builtin_amdgcn_readfirstlane(k.s_rt[m]);
		if (!(r & UD_R32) || (FORMS >= F_GEN && (r & UD_GEN)) || !k.s_on[m] || !((unsigned)k.s_par[m].x & MI_MIX_LINKED)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(k.rows + m * k.row_w), *hist = ra.hist_in + (size_t)(k.s0 + m) * hin;
		if (r & UD_ABOVE) rational_run<2, 3>(scr, row, hist, ra.tab + qa->tab_above_in, ns / 2 * 3, lane);
		else rational_run<3, 2>(scr, row, hist, ra.tab + qa->tab_below_in, ns / 3 * 2, lane);
	}
	if (FORMS < F_GEN) return;
	for (int m = wave; m < k.mm; m += BT / 64) { // (a : b: leg -> conference is a : b, in : out)
		const int r = __builtin_amdgcn_readfirstlane(k.s_rt[m]);
		if (!(r & UD_GEN) || !k.s_on[m] || !((unsigned)k.s_par[m].x & MI_MIX_LINKED)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(k.rows + m * k.row_w), *hist = ra.hist_in + (size_t)(k.s0 + m) * hin;
		const int la = gen_a(r), cb = gen_b(r);
		generic_run(scr, row, hist, ra.tab + ga->gen_tab[gen_code(r)].x, la, cb, filter_rule(la, cb).filt_len, ns / cb * la, lane);
	}
	if (FORMS < F_OFF) return;
	for (int m = wave; m < k.mm; m += BT / 64) { // (44 100 Hz: leg -> conference is num : den, 441 samples in)
		const int r = __builtin_amdgcn_readfirstlane(k.s_rt[m]);
		if (!is_offgrid(r) || !k.s_on[m] || !((unsigned)k.s_par[m].x & MI_MIX_LINKED)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(k.rows + m * k.row_w), *hist = ra.hist_in + (size_t)(k.s0 + m) * hin;
		offgrid_run(scr, row, hist, ra.tab + oa->tab_in, oa->num, oa->den, oa->filt_in, OFFGRID_LEN, lane);
	}
}

// ---- (W) one wavefront per member: the out_resampler of a pin with its output on, then the leg's store or encoder --
// resample_down for a leg below the mix; for one above it rated_up, for UD_R32 rational_run the other way, from the head of
// the row back over the row (which held the leg's input, so it is wide enough), for UD_GEN generic_run and for UD_OFF
// offgrid_run likewise, then store_row (and store_tail for the 441st sample).  OUT as in (D).
template <int FORMS, int OUT>
__device__ __forceinline__ void resample_out(const Conf &k, const RatedArgs &ra, const UpdownArgs *ua, const RationalArgs *qa, float *scr,
                                             uint8_t *out, int pitch, const RatiosArgs *ga = nullptr, const OffgridArgs *oa = nullptr) {
	const int wave = k.t >> 6, lane = k.t & 63, ns = k.ns;
	for (int m = wave; m < k.mm; m += BT / 64) {
		const int r = wave_ratio<FORMS>(k, m), n = FORMS >= F_ABOVE ? r & 7 : r;
		if (r == 1 || (FORMS >= F_R32 && (r & UD_R32)) || (FORMS >= F_GEN && (r & UD_GEN)) || (FORMS >= F_OFF && (r & UD_OFF)) ||
		    !((unsigned)k.s_par[m].x & MI_MIX_OUTPUT))
			continue;
		int16_t *row = reinterpret_cast<int16_t *>(k.rows + m * k.row_w), *hist = ra.hist_out + (size_t)(k.s0 + m) * ra.hout_stride;
		const int kind = OUT == BY_KIND ? __builtin_amdgcn_readfirstlane(k.s_cd[m] >> 2) : OUT;
		const size_t at = (size_t)(k.s0 + m) * pitch;
		if (FORMS >= F_ABOVE && (r & UD_ABOVE)) {
			rated_up(scr, row, hist, ra.tab + ua->tab_up_out[n], n, ns, lane);
			store_row(row, out + at, kind, ns * n, lane);
		} else {
			resample_down<OUT>(scr, row, hist, ra.tab + ra.tab_down[n], n, ns, rs_plen(RS_FILT, n, ns), lane, out, at, kind);
		}
	}
	if (FORMS < F_R32) return;
	for (int m = wave; m < k.mm; m += BT / 64) {
		const int r = __builtin_amdgcn_readfirstlane(k.s_rt[m]);
		if (!(r & UD_R32) || (FORMS >= F_GEN && (r & UD_GEN)) || !((unsigned)k.s_par[m].x & MI_MIX_OUTPUT)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(k.rows + m * k.row_w), *hist = ra.hist_out + (size_t)(k.s0 + m) * ra.hout_stride;
		if (r & UD_ABOVE) rational_run<3, 2>(scr, row, hist, ra.tab + qa->tab_above_out, ns, lane);
		else rational_run<2, 3>(scr, row, hist, ra.tab + qa->tab_below_out, ns, lane);
		store_row(row, out + (size_t)(k.s0 + m) * pitch, __builtin_amdgcn_readfirstlane(k.s_cd[m] >> 2), leg_span<FORMS>(r, ns), lane);
	}
	if (FORMS < F_GEN) return;
	for (int m = wave; m < k.mm; m += BT / 64) { // (conference -> leg is b : a)
		const int r = __builtin_amdgcn_readfirstlane(k.s_rt[m]);
		if (!(r & UD_GEN) || !((unsigned)k.s_par[m].x & MI_MIX_OUTPUT)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(k.rows + m * k.row_w), *hist = ra.hist_out + (size_t)(k.s0 + m) * ra.hout_stride;
		const int la = gen_a(r), cb = gen_b(r);
		generic_run(scr, row, hist, ra.tab + ga->gen_tab[gen_code(r)].y, cb, la, filter_rule(cb, la).filt_len, ns, lane);
		store_row(row, out + (size_t)(k.s0 + m) * pitch, __builtin_amdgcn_readfirstlane(k.s_cd[m] >> 2), leg_span<FORMS>(r, ns), lane);
	}
	if (FORMS < F_OFF) return;
	for (int m = wave; m < k.mm; m += BT / 64) { // (conference -> 44 100 Hz is den : num, 441 samples out: 55 groups and the tail)
		const int r = __builtin_amdgcn_readfirstlane(k.s_rt[m]);
		if (!is_offgrid(r) || !((unsigned)k.s_par[m].x & MI_MIX_OUTPUT)) continue;
		int16_t *row = reinterpret_cast<int16_t *>(k.rows + m * k.row_w), *hist = ra.hist_out + (size_t)(k.s0 + m) * ra.hout_stride;
		uint8_t *dst = out + (size_t)(k.s0 + m) * pitch;
		const int kind = __builtin_amdgcn_readfirstlane(k.s_cd[m] >> 2);
		offgrid_run(scr, row, hist, ra.tab + oa->tab_out, oa->den, oa->num, oa->filt_out, ns, lane);
		store_row(row, dst, kind, OFFGRID_LEN, lane);
		store_tail<OFFGRID_TAIL>(row, dst, kind, OFFGRID_LEN >> 3, lane);
	}
}

} // namespace
