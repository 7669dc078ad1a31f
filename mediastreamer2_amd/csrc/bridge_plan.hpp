// bridge_plan.hpp -- what creating an mi_bridge decides before anything is allocated, as plain C++ with no HIP in it: the
// refusals, the kernel family, the LDS layout, the pitches and strides, every leg's ratio byte.  bridge.hip's constructors
// plan, then allocate what the plan says, then tick by it; tests/host/bridge_plan_check.cpp runs the plan alone on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/msmi355x.h"
#include "../../include/msmi355x_bridge.h"
#include "seat_changes.hpp"

#ifdef __HIPCC__
#define MI_PLAN_HD __host__ __device__
#else
#define MI_PLAN_HD
#endif

namespace mi { void set_error(const char *fmt, ...); }
// plc.hip: what the concealer cannot serve, said for one rate without a device
int mi_plc_check_rate(const char *fn, const char *what, int index, int rate);

namespace {

constexpr int BT = 256, BMAX = MI_MIXER_MAX_CHANNELS;
constexpr size_t BRIDGE_LDS_MAX = 64 * 1024;
constexpr size_t RATED_STATIC_LDS = 2048; // bound on a kernel's static LDS (tests/test_bridge_rates_cpu.py holds it)

// ---- the resamplers' constants and lengths, one wavefront running one member's (under hipcc: their steps as well).  A
// down-sampler's phase arrays are rs_plen(RS_FILT, num, ..) floats behind a pin and rs_plen_odd in FRONT of one; a rational
// resampler's rs_plen_odd(RQ_FT, M, ..): lanes (tile, r) and (tile, r + 1) read neighbouring arrays at one offset.
#include "resample_steps.hpp"
// bytes of a wavefront's scratch for a rational resampler: two copies of M phase arrays
MI_PLAN_HD inline size_t rational_scratch(int m, int in_len) { return (size_t)2 * m * rs_plen_odd(RQ_FT, m, in_len) * sizeof(float); }

// of a resampler in mi_resampler's generic order (generic_run, bridge_phases.hpp): history ++ tick as floats, then the `den`
// polyphase rows of `filt` taps at a pitch of filt + 1 floats -- the filters are 48 .. 128 taps, multiples of 8, and rows at
// that pitch would all start on one LDS bank
MI_PLAN_HD inline int generic_xlen(int filt, int in_len) { return (filt - 1 + in_len + 3) & ~3; }
MI_PLAN_HD inline size_t generic_scratch(int filt, int den, int in_len) {
	return ((size_t)generic_xlen(filt, in_len) + (size_t)den * (filt + 1)) * sizeof(float);
}

// design_filter's rule (resample.hip) at quality 3 for in : out = num : den in lowest terms: 48 taps, stretched by num / den
// and rounded up to eight where the resampler goes down, the table's oversampling halved past every power of two of that
// ratio; the table is direct -- den rows of filt_len taps -- where filt_len * den <= filt_len * oversample + 8
struct FilterRule { int filt_len; bool direct; };
MI_PLAN_HD inline FilterRule filter_rule(int num, int den) {
	int len = RS_FILT, over = 8;
	if (num > den) len = ((RS_FILT * num / den - 1) & ~7) + 8;
	for (int k = 2; k <= 16 && num > den; k *= 2) over = k * den < num ? over >> 1 : over;
	return {len, len * den <= len * (over < 1 ? 1 : over) + 8};
}
constexpr int GENERIC_MAX_FILT = 128, GENERIC_MAX_TERM = 8; // the longest filter generic_run takes; a and b of a : b in the byte

// ---- the one rate off the 800 Hz grid (mi_bridge_create_offgrid): 44 100 Hz, a tick of 441 samples = 55 groups of eight and
// one sample.  Against a mix at 100 n Hz that is 441 / g : n / g with g = gcd(441, n) -- whole periods either way, so
// mi_resampler's position state is (0, 0) at every tick.  Its resamplers run in the generic order on the PER-PHASE table
// (design_filter blends an interpolated design once per phase, up to 256 KB), read from memory by offgrid_run
// (bridge_phases.hpp): the tables are 28 to 92 KB, more than a wavefront's scratch.
constexpr int OFFGRID_RATE = 44100, OFFGRID_LEN = OFFGRID_RATE / 100;
constexpr int OFFGRID_GROUPS = (OFFGRID_LEN + 7) / 8, OFFGRID_WORDS = (OFFGRID_LEN + 3) / 4; // the tail group holds one sample
constexpr int OFFGRID_MAX_FILT = 264;                 // 44.1 -> 8 kHz
constexpr size_t PHASE_TABLE_MAX = 256 * 1024;        // bytes: design_filter's bound on a per-phase table
// whether design_filter has a per-phase table for in : out = num : den, direct or blended
MI_PLAN_HD inline bool has_phase_table(int num, int den) {
	const FilterRule f = filter_rule(num, den);
	return f.direct || (size_t)den * f.filt_len * sizeof(float) <= PHASE_TABLE_MAX;
}

// ---- a member's ratio byte.  Conference rate / leg rate (1, 2, 3 or 6; 4 under mi_bridge_create_ratios) for a leg at or
// below the mix; with UD_ABOVE the leg is above it and the low three bits are leg rate / conference rate; with UD_R32 the
// ratio is 3/2 (the whole part: 1), UD_ABOVE still giving the direction.  With UD_GEN the leg stands a : b to the mix, any
// other non-whole ratio of mi_bridge_create_ratios: a - 1 in bits 0-2, b - 1 in bits 3, 4 and 6, UD_ABOVE where a > b.  The
// kernels read it through leg_span (bridge_phases.hpp).
// With UD_OFF, and neither UD_GEN nor UD_R32, the leg is at 44 100 Hz (mi_bridge_create_offgrid): the byte says no more than
// that and UD_ABOVE -- the one pair num : den, its filters and tables are the bridge's, not the leg's (OffgridArgs).
constexpr unsigned UD_ABOVE = 0x80, UD_R32 = 0x40, UD_GEN = 0x20, UD_OFF = 0x10;
MI_PLAN_HD inline bool is_offgrid(int rb) { return (rb & (int)(UD_GEN | UD_R32 | UD_OFF)) == (int)UD_OFF; }
constexpr int NO_WHOLE_RATIO = -1, RATIO_NOT_SERVED = -2;
MI_PLAN_HD inline int gen_a(int rb) { return (rb & 7) + 1; }
MI_PLAN_HD inline int gen_b(int rb) { return ((rb >> 3) & 3) + ((rb >> 4) & 4) + 1; }
MI_PLAN_HD inline int gen_code(int rb) { return (gen_a(rb) - 1) | (gen_b(rb) - 1) << 3; } // 0 .. 63: the index of its tables
inline int gen_byte(int a, int b) {
	return (int)(UD_GEN | (a > b ? UD_ABOVE : 0u) | (unsigned)(a - 1) | ((unsigned)(b - 1) & 3u) << 3 | ((unsigned)(b - 1) & 4u) << 4);
}

// The one place where two rates become a ratio byte, or one of the two reasons why there is none.  3/2 or 2/3, both rates
// multiples of 800: leg and mix are 2400 k and 1600 k Hz, their ticks 24 k and 16 k samples -- 8 k periods of 3 samples against
// 2: whole periods and whole eight-period tiles, eight-sample groups, both ways
inline int ratio_byte(int leg, int conf) {
	if ((int64_t)2 * leg == (int64_t)3 * conf) return (int)(UD_R32 | UD_ABOVE | 1u);
	if ((int64_t)3 * leg == (int64_t)2 * conf) return (int)(UD_R32 | 1u);
	const int hi = std::max(leg, conf), lo = std::min(leg, conf);
	if (hi % lo != 0) return NO_WHOLE_RATIO;
	const int r = hi / lo;
	if (r != 1 && r != 2 && r != 3 && r != 6) return RATIO_NOT_SERVED;
	return leg > conf ? (int)(UD_ABOVE | (unsigned)r) : r;
}

// ---- a public constructor's rules.  fn: its name, in the texts about the legs' codecs; rates_fn: the name in the texts about
// rates of a bridge without the per-leg concealer, which is the older constructor's bridge and speaks as that one
struct Rules {
	const char *fn, *rates_fn;
	// above: a leg may be above the mix (and brings the codecs as data and byte rows); leg_plc: cfg->plc with legs that differ in
	// rate or codec is served by the per-leg concealer, not refused; rational: a leg may be at 3/2 or 2/3 of the mix
	// ratios: a leg may be at 4 or 1/4 of the mix, or stand a : b to it wherever both its resamplers have a direct table of at
	// most 128 taps
	// offgrid: a leg may be at 44 100 Hz wherever both its resamplers have a per-phase table of at most 264 taps
	bool above, leg_plc, rational, ratios, offgrid = false;
};
constexpr Rules RULES_RATED = {"mi_bridge_create_rated", "mi_bridge_create_rated", false, false, false};
constexpr Rules RULES_LEGS = {"mi_bridge_create_legs", "mi_bridge_create_rated", false, false, false};
constexpr Rules RULES_ENDPOINTS = {"mi_bridge_create_endpoints", "mi_bridge_create_endpoints", true, false, false};
constexpr Rules RULES_CONCEALED = {"mi_bridge_create_concealed", "mi_bridge_create_endpoints", true, true, false};
constexpr Rules RULES_RATIONAL = {"mi_bridge_create_rational", "mi_bridge_create_rational", true, true, true};
constexpr Rules RULES_RATIOS = {"mi_bridge_create_ratios", "mi_bridge_create_ratios", true, true, true, true};
constexpr Rules RULES_OFFGRID = {"mi_bridge_create_offgrid", "mi_bridge_create_offgrid", true, true, true, true, true};

struct Plan {
	// which kernel a tick launches, chosen once: compile-time codecs without and with resamplers, per-leg codecs without and
	// with them, a leg above the mix, a leg at 3/2 or 2/3 of it, a leg at 4, 1/4 or a : b, a leg at 44 100 Hz
	enum Family { TICK, RATED, LEGS, LEGS_RATED, UPDOWN, RATIONAL, RATIOS, OFFGRID } family = TICK;
	mi_bridge_config cfg = {}; // in_codec, out_codec: leg 0's where the legs were given
	int n = 0, nconf = 0, mm = 0, len = 0;
	// a leg not at the conference's rate (ratio bytes, resamplers, tables); one above the mix by a whole ratio; one at 3/2 or 2/3 of
	// it; the concealer is the per-leg one, behind every leg's own decoder
	bool rated = false, updown = false, rational = false, leg_plc = false;
	bool ratios = false;          // a leg at 4 or 1/4 of the mix, or at a : b: only mi_bridge_create_ratios plans one
	std::vector<uint8_t> generic; // the distinct UD_GEN ratio bytes of the legs: a pair of tables each (gen_code)
	// a leg at 44 100 Hz: only mi_bridge_create_offgrid plans one.  off_num : off_den is leg : mix in lowest terms, off_fin and
	// off_fout the taps of its in_resampler (leg -> mix, off_den rows) and its out_resampler (mix -> leg, off_num rows)
	bool offgrid = false;
	int off_num = 0, off_den = 0, off_fin = 0, off_fout = 0;
	bool used[7] = {}, above[7] = {};         // the whole ratios of legs below the mix, and of legs above it
	bool r32_above = false, r32_below = false; // a leg at 3/2 of the mix, a leg at 2/3
	int max_ratio = 1, common = 0; // common: the first leg's rate, the one concealer batch's
	int wide = 0;   // samples per LDS row: the widest leg's tick where one is above the mix
	int row_w = 0, sum_off = 0, nslice = 0; // 8-byte words per row (odd), the sum row's byte offset, member slices of (C)
	size_t lds = 0;                         // dynamic LDS of a launch
	int scratch_off = 0, scratch_per_wave = 0; // bytes: each wavefront's resampler scratch in it
	int pitch = 0;                          // samples per row of the host buffers: the widest leg's tick
	// samples per row of the PCM the per-leg concealer hands the kernel: whole groups of eight (448 for a 441-sample tick)
	int pcm_pitch() const { return (pitch + 7) & ~7; }
	size_t in_bytes = 0, out_bytes = 0;     // per stream and tick, on the host side; byte rows' pitch where the codecs are data
	int hin_stride = RS_FILT, hout_stride = 0; // samples per member of the in_resamplers' and out_resamplers' histories
	std::vector<int32_t> leg_rate;  // [n], empty: every leg at cfg.rate
	std::vector<uint8_t> leg_codec; // [n] in_codec | out_codec << 2 where the codecs are the kernel's data; empty: cfg's pair
	std::vector<uint8_t> ratio;     // [n] ratio bytes, empty unless `rated`
	// the codecs are the kernel's data (a row on the device) and the host rows byte rows.  On a closed bridge: leg_codec is there
	bool data = false;
	// plan_open with admitted kinds: the seats may change hands.  Everything above that is not per seat was planned for `kinds`,
	// the distinct (rate, in_codec, out_codec) of the initial legs and the admitted ones; the three per-seat vectors always exist
	bool open = false;
	std::vector<mi_bridge_leg> kinds;
	std::vector<uint8_t> kind_ratio; // [kinds.size()] the ratio byte of each (1 without resamplers)
};

#define MI_PLAN_ARG(cond) if (!(cond)) return mi::set_error("%s:%d invalid argument: %s", __FILE__, __LINE__, #cond), (int)MI_EINVAL
#define MI_REFUSE(...) return mi::set_error(__VA_ARGS__), (int)MI_ENOTSUP

inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }

// rates [nstreams] or null: every leg at cfg->rate.  codec [nstreams] in_codec | out_codec << 2 (plan_legs has checked them)
// or null: cfg's pair on every leg.  MI_OK, or the refusal with its text set; *p is whole only with MI_OK.  own: the legs from
// `own` on are no seats but stand for admitted kinds, a conference of members_per_conference each (plan_open), and a refusal
// names them so; < 0: every leg is a seat.
inline int plan_bridge(const Rules &rules, const mi_bridge_config *cfg, const int32_t *rates, const uint8_t *codec, Plan *p, int own = -1) {
	MI_PLAN_ARG(cfg && p);
	MI_PLAN_ARG(cfg->nstreams > 0 && cfg->members_per_conference > 0 && cfg->members_per_conference <= MI_MIXER_MAX_CHANNELS &&
	            cfg->nstreams % cfg->members_per_conference == 0);
	MI_PLAN_ARG(cfg->rate > 0);
	MI_PLAN_ARG(cfg->in_codec >= MI_SESSION_PCM16 && cfg->in_codec <= MI_SESSION_PCMU && cfg->out_codec >= MI_SESSION_PCM16 &&
	            cfg->out_codec <= MI_SESSION_PCMU);
	if (cfg->rate % 800 != 0)
		MI_REFUSE("mi_bridge_create: rate %d is no multiple of 800 (a 10 ms tick must be whole groups of 8 samples)", cfg->rate);
	*p = Plan(), p->cfg = *cfg;
	const int n = p->n = cfg->nstreams, mm = p->mm = cfg->members_per_conference, len = p->len = cfg->rate / 100;
	p->nconf = n / mm;
	const auto who = [&](int s) { return own >= 0 && s >= own ? "admitted kind" : "leg"; };
	const auto idx = [&](int s) { return own >= 0 && s >= own ? (s - own) / mm : s; };
	bool mixed = false, differ = false; // the legs' pairs differ: the codecs are the kernel's data; they or the rates do
	for (int s = 1; codec && s < n; ++s) mixed |= codec[s] != codec[0], differ |= codec[s] != codec[0] || (rates && rates[s] != rates[0]);
	// (a 44 100 Hz leg's tick is no whole groups of eight: only the per-leg concealer, behind the legs' decoders, takes it)
	for (int s = 0; rules.offgrid && rates && s < n; ++s) differ |= rates[s] == OFFGRID_RATE;
	p->leg_plc = rules.leg_plc && cfg->plc && differ;
	const char *fn = p->leg_plc ? rules.fn : rules.rates_fn;
	// ---- the legs' rates
	int widest = 0;
	bool data = mixed || p->leg_plc; // the codecs are the kernel's data and the host rows byte rows
	for (int s = 0; rates && s < n; ++s) {
		const int lr = rates[s];
		MI_PLAN_ARG(lr > 0);
		const bool up = lr > cfg->rate;
		if (rules.offgrid && lr % 800 != 0) { // the one rate off the grid that is a whole tick and has its tables, or the reason
			if (lr % 100 != 0)
				MI_REFUSE("%s: %s %d at %d Hz in a %d Hz conference: %d.%02d samples are no 10 ms tick; off the 800 Hz grid only %d Hz is served",
				          fn, who(s), idx(s), lr, cfg->rate, lr / 100, lr % 100, OFFGRID_RATE);
			if (lr != OFFGRID_RATE)
				MI_REFUSE("%s: %s %d at %d Hz in a %d Hz conference: the rate is no multiple of 800 (a 10 ms tick must be whole groups of 8 "
				          "samples); off that grid only %d Hz is served", fn, who(s), idx(s), lr, cfg->rate, OFFGRID_RATE);
			int g = OFFGRID_LEN, h = len;
			while (h) { const int t = g % h; g = h, h = t; }
			const int la = OFFGRID_LEN / g, cb = len / g; // leg : mix
			const FilterRule in = filter_rule(la, cb), out = filter_rule(cb, la);
			if (!has_phase_table(la, cb) || !has_phase_table(cb, la) || in.filt_len > OFFGRID_MAX_FILT || out.filt_len > OFFGRID_MAX_FILT)
				MI_REFUSE("%s: %s %d at %d Hz in a %d Hz conference is %d : %d, a ratio whose resamplers have no per-phase table of at most "
				          "%zu KB and %d taps (%d taps in %d rows one way, %d in %d the other)", fn, who(s), idx(s), lr, cfg->rate, la, cb,
				          PHASE_TABLE_MAX / 1024, OFFGRID_MAX_FILT, in.filt_len, cb, out.filt_len, la);
			if (cfg->plc && !p->leg_plc && p->common && lr != p->common)
				MI_REFUSE("%s: plc with legs at %d Hz and %d Hz: the concealer batch has one rate", fn, p->common, lr);
			if (!p->common) p->common = lr;
			widest = std::max(widest, lr);
			p->offgrid = true, p->off_num = la, p->off_den = cb, p->off_fin = in.filt_len, p->off_fout = out.filt_len;
			data |= codec != nullptr; // (such a leg brings the codecs as data, whether they differ or not)
			p->ratio.push_back((uint8_t)(UD_OFF | (up ? UD_ABOVE : 0u)));
			continue;
		}
		int rb = ratio_byte(lr, cfg->rate);
		if (rb >= 0 && (rb & UD_R32) && !rules.rational) rb = NO_WHOLE_RATIO;
		bool added = false; // a form only mi_bridge_create_ratios plans
		if (rules.ratios && rb == RATIO_NOT_SERVED && std::max(lr, cfg->rate) / std::min(lr, cfg->rate) == 4)
			rb = (int)((up ? UD_ABOVE : 0u) | 4u), added = true;
		if (rules.ratios && rb == NO_WHOLE_RATIO) {
			int g = lr, h = cfg->rate;
			while (h) { const int t = g % h; g = h, h = t; }
			const int la = lr / g, cb = cfg->rate / g; // a : b
			const FilterRule in = filter_rule(la, cb), out = filter_rule(cb, la);
			if (la > GENERIC_MAX_TERM || cb > GENERIC_MAX_TERM || !in.direct || !out.direct || in.filt_len > GENERIC_MAX_FILT || out.filt_len > GENERIC_MAX_FILT)
				MI_REFUSE("%s: %s %d at %d Hz in a %d Hz conference is %d : %d (%.3f), a ratio whose resamplers have no direct table "
				          "of at most %d taps (%d taps%s one way, %d%s the other); supported: whole ratios 1, 2, 3, 4, 6 either way, and a : b "
				          "with a, b <= %d and a ratio of at most 8/3",
				          fn, who(s), idx(s), lr, cfg->rate, la, cb, (double)std::max(la, cb) / std::min(la, cb), GENERIC_MAX_FILT, in.filt_len,
				          in.direct ? "" : ", interpolated,", out.filt_len, out.direct ? "" : ", interpolated,", GENERIC_MAX_TERM);
			rb = gen_byte(la, cb), added = true;
		}
		if (up && !rules.above)
			MI_REFUSE("mi_bridge_create_rated: %s %d at %d Hz is above its conference's %d Hz (only legs at or below the mix are resampled)",
			          who(s), idx(s), lr, cfg->rate);
		const int hi = up ? lr : cfg->rate, lo = up ? cfg->rate : lr;
		if (rb == NO_WHOLE_RATIO)
			MI_REFUSE("%s: %s %d at %d Hz in a %d Hz conference is no whole ratio (%.3f); supported: 1, 2, 3, 6%s", fn, who(s), idx(s), lr, cfg->rate,
			          (double)hi / lo, rules.rational ? ", and 3/2 either way" : "");
		if (rb == RATIO_NOT_SERVED)
			MI_REFUSE("%s: %s %d at %d Hz in a %d Hz conference is ratio %d; supported: 1, 2, 3, %s6%s", fn, who(s), idx(s), lr, cfg->rate, hi / lo,
			          rules.ratios ? "4, " : "", rules.ratios ? ", and a : b with a, b <= 8 up to 8/3 either way" : rules.rational ? ", and 3/2 either way" : "");
		// what holds for a leg of any ratio, checked once that ratio is known to be served: a tick of whole groups, and one rate
		// for the one concealer batch
		if (lr % 800 != 0)
			MI_REFUSE("%s: %s %d's rate %d is no multiple of 800 (a 10 ms tick must be whole groups of 8 samples)", fn, who(s), idx(s), lr);
		if (cfg->plc && !p->leg_plc && p->common && lr != p->common)
			MI_REFUSE("%s: plc with legs at %d Hz and %d Hz: the concealer batch has one rate", fn, p->common, lr);
		if (!p->common) p->common = lr;
		widest = std::max(widest, lr);
		p->ratios |= added;
		if (rb & UD_GEN) {
			if (std::find(p->generic.begin(), p->generic.end(), (uint8_t)rb) == p->generic.end()) p->generic.push_back((uint8_t)rb);
		} else if (rb & UD_R32) {
			(up ? p->r32_above : p->r32_below) = true;
		} else {
			(up ? p->above : p->used)[rb & 7] = true;
			p->updown |= up;
			p->max_ratio = std::max(p->max_ratio, rb & 7);
		}
		data |= codec && ((rb & (UD_ABOVE | UD_R32 | UD_GEN)) || added); // (such a leg brings the codecs as data, whether they differ or not)
		p->ratio.push_back((uint8_t)rb);
	}
	p->rational = p->r32_above || p->r32_below; // without such a leg: mi_bridge_create_concealed's bridge exactly
	p->rated = p->max_ratio > 1 || p->rational || !p->generic.empty() || p->offgrid;
	if (!p->rated) p->ratio.clear();
	// ---- the LDS of a launch.  Samples per row: the widest leg's tick where one is above the mix
	p->wide = p->updown ? widest / 100 : p->rational || !p->generic.empty() ? std::max(len, widest / 100) : len;
	// a 441-sample tick is staged, levelled and stored in whole groups of eight, the tail group's other seven zero: 448 samples
	if (p->offgrid) p->wide = std::max(len, (widest / 100 + 7) & ~7);
	p->row_w = (p->wide >> 2) | 1;
	p->sum_off = (int)up16((size_t)mm * p->row_w * 8);
	p->nslice = std::max(1, std::min(mm, BT / (len >> 2)));
	size_t lds = p->sum_off + (size_t)len * 4;
	if (p->rated) {
		size_t scratch = 0;
		for (int r = 2; r < 7; ++r) {
			// each wavefront's scratch: the larger of the forms per used ratio -- up-sampler and down-sampler of a leg below the
			// mix (in front of the pin, behind it), down-sampler and up-sampler of a leg above it
			size_t up = 0, down = 0;
			if (p->used[r]) {
				up = (size_t)rs_flat_len(len / r) * 4;
				down = ((size_t)r * rs_plen(RS_FILT, r, len) + (size_t)len) * 4;
			}
			if (p->above[r]) {
				up = std::max(up, (size_t)rs_flat_len(len) * 4);
				down = std::max(down, ((size_t)r * rs_plen_odd(RS_FILT, r, r * len) + (size_t)r * len) * 4);
			}
			scratch = std::max(scratch, up16(std::max(up, down)));
		}
		// a leg at 3/2 of the mix: x 2/3 from its tick in front of the pin, x 3/2 from the mix's behind it; one at 2/3: x 3/2 from
		// its tick, x 2/3 from the mix's
		if (p->r32_above) scratch = std::max(scratch, std::max(rational_scratch(3, len / 2 * 3), rational_scratch(2, len)));
		if (p->r32_below) scratch = std::max(scratch, std::max(rational_scratch(2, len / 3 * 2), rational_scratch(3, len)));
		// a leg at a : b in mi_resampler's generic order: leg -> mix from its tick in front of the pin (b rows of taps), mix -> leg
		// from the mix's behind it (a rows); its histories are filt_len - 1 samples, kept at mi_resampler's stride
		int generic_hist = 0;
		for (const uint8_t rb : p->generic) {
			const int la = gen_a(rb), cb = gen_b(rb), fin = filter_rule(la, cb).filt_len, fout = filter_rule(cb, la).filt_len;
			scratch = std::max(scratch, up16(std::max(generic_scratch(fin, cb, len / cb * la), generic_scratch(fout, la, len))));
			generic_hist = std::max(generic_hist, (std::max(fin, fout) - 1 + 7) & ~7);
		}
		// a leg at 44 100 Hz: history ++ tick as floats either way, nothing else -- the tables stay in memory (offgrid_run)
		if (p->offgrid) {
			scratch = std::max(scratch, up16(sizeof(float) * (size_t)std::max(generic_xlen(p->off_fin, OFFGRID_LEN), generic_xlen(p->off_fout, len))));
			generic_hist = std::max(generic_hist, (std::max(p->off_fin, p->off_fout) - 1 + 7) & ~7); // up to 263 samples
		}
		const size_t scratch_off = up16(lds);
		lds = scratch_off + (BT / 64) * scratch;
		if (lds + RATED_STATIC_LDS > BRIDGE_LDS_MAX)
			MI_REFUSE("%s: a conference's tick and its resamplers' scratch must fit %zu bytes of LDS (%d members x %d samples "
			          "= %zu, + %d wavefronts x %zu for ratio %d%s, + %zu of the kernel's own: %zu)",
			          fn, BRIDGE_LDS_MAX, mm, p->wide, scratch_off, BT / 64, scratch, p->max_ratio,
			          p->offgrid ? " and 44100 Hz" : !p->generic.empty() ? " and a : b" : p->rational ? " and 3/2" : "", RATED_STATIC_LDS,
			          lds + RATED_STATIC_LDS);
		p->scratch_off = (int)scratch_off, p->scratch_per_wave = (int)scratch;
		p->hout_stride = p->max_ratio * RS_FILT; // mi_resampler's round_up(filt_len - 1, 8) of the longest filter
		if (p->rational) p->hout_stride = std::max(p->hout_stride, 3 * RQ_FT); // x 2/3 keeps 71 samples (x 3/2: 47)
		p->hout_stride = std::max(p->hout_stride, generic_hist);               // up to 127 samples
		if (p->updown || p->rational || generic_hist) p->hin_stride = p->hout_stride; // a down-sampler's history on either side of the pin
	} else if (lds > BRIDGE_LDS_MAX)
		MI_REFUSE("mi_bridge_create: a conference's tick must fit %zu bytes of LDS (%d members x %d samples need %zu)", BRIDGE_LDS_MAX, mm, len, lds);
	p->lds = lds;
	// ---- the host rows
	p->pitch = p->rated ? widest / 100 : len;
	p->in_bytes = (size_t)p->pitch * (cfg->in_codec ? 1 : 2), p->out_bytes = (size_t)p->pitch * (cfg->out_codec ? 1 : 2);
	p->data = data;
	if (data) { // byte rows: the widest leg's tick in bytes, rounded up to the 16 bytes a lane loads
		p->in_bytes = p->out_bytes = 0;
		for (int s = 0; s < n; ++s) {
			const size_t ll = (size_t)(rates ? rates[s] : cfg->rate) / 100;
			p->in_bytes = std::max(p->in_bytes, ll * ((codec[s] & 3) ? 1 : 2));
			p->out_bytes = std::max(p->out_bytes, ll * ((codec[s] >> 2) ? 1 : 2));
		}
		p->in_bytes = up16(p->in_bytes), p->out_bytes = up16(p->out_bytes);
		p->leg_codec.assign(codec, codec + n);
	}
	if (rates) p->leg_rate.assign(rates, rates + n);
	// the widest form a leg needs: the order matters
	p->family = p->offgrid ? Plan::OFFGRID : p->ratios ? Plan::RATIOS : p->rational ? Plan::RATIONAL : p->updown ? Plan::UPDOWN : data ? (p->rated ? Plan::LEGS_RATED : Plan::LEGS)
	            : p->rated  ? Plan::RATED : Plan::TICK;
	return MI_OK;
}

// mi_bridge_create_legs and its successors: the legs' codecs checked, the concealer asked about every rate where it will be
// the per-leg one, then plan_bridge under the same rules with the first leg's pair as the bridge's.  A uniform bridge is
// mi_bridge_create_rated's, its one pair compile-time in the kernels.
inline int plan_legs(const Rules &rules, const mi_bridge_config *cfg, const mi_bridge_leg *legs, Plan *p, int own = -1) {
	MI_PLAN_ARG(cfg && legs && p);
	MI_PLAN_ARG(cfg->nstreams > 0);
	const size_t n = (size_t)cfg->nstreams;
	const int per = std::max(1, cfg->members_per_conference);
	const auto who = [&](size_t s) { return own >= 0 && (int)s >= own ? "admitted kind" : "leg"; };
	const auto idx = [&](size_t s) { return own >= 0 && (int)s >= own ? ((int)s - own) / per : (int)s; };
	std::vector<int32_t> rate(n);
	std::vector<uint8_t> codec(n);
	int differs = -1; // the first leg whose pair is not leg 0's
	for (size_t s = 0; s < n; ++s) {
		const mi_bridge_leg &l = legs[s];
		for (int v : {l.in_codec, l.out_codec})
			if (v < MI_SESSION_PCM16 || v > MI_SESSION_PCMU)
				MI_REFUSE("%s: %s %d names codec %d; supported: MI_SESSION_PCM16 (0), MI_SESSION_PCMA (1), MI_SESSION_PCMU (2)", rules.fn, who(s), idx(s), v);
		rate[s] = l.rate;
		codec[s] = (uint8_t)(l.in_codec | l.out_codec << 2);
		if (differs < 0 && codec[s] != codec[0]) differs = (int)s;
	}
	if (rules.leg_plc && cfg->plc) {
		for (size_t s = 0; s < n; ++s) // what the concealer cannot serve
			if (const int rc = mi_plc_check_rate(rules.fn, who(s), idx(s), rate[s])) return rc;
	} else if (differs >= 0 && cfg->plc)
		MI_REFUSE("%s: plc with leg %d's codecs (in %d, out %d) unlike leg 0's (in %d, out %d): the concealer batch "
		          "sits behind one decoder", rules.fn, differs, legs[differs].in_codec, legs[differs].out_codec, legs[0].in_codec, legs[0].out_codec);
	mi_bridge_config c = *cfg;
	c.in_codec = legs[0].in_codec, c.out_codec = legs[0].out_codec;
	return plan_bridge(rules, &c, rate.data(), codec.data(), p, own);
}

// ---- seats that change hands (mi_bridge_create_open, mi_bridge_change_members)

constexpr int PLAN_MAX_RATE_CLASSES = 7; // the concealer's PLC_MAX_CLASSES (common.hpp; bridge.hip holds the two equal)

inline bool same_kind(const mi_bridge_leg &a, const mi_bridge_leg &b) {
	return a.rate == b.rate && a.in_codec == b.in_codec && a.out_codec == b.out_codec;
}

// mi_bridge_create_open: ONE plan for the union -- the kinds of `legs` and the admitted ones.  It is the plan of the closed
// bridge that holds the legs followed by one whole conference of each admitted kind (so every refusal, the LDS one included,
// can come from an admitted kind alone, and names it so), cut back to the seats there are: the per-seat vectors are the
// union's first nstreams entries, and a kind's ratio byte is the one plan_bridge wrote for it.  nadmit == 0: plan_legs exactly.
inline int plan_open(const Rules &rules, const mi_bridge_config *cfg, const mi_bridge_leg *legs, const mi_bridge_leg *admit, int nadmit, Plan *p) {
	MI_PLAN_ARG(cfg && legs && p && nadmit >= 0 && (admit || nadmit == 0));
	if (nadmit == 0) return plan_legs(rules, cfg, legs, p);
	MI_PLAN_ARG(cfg->nstreams > 0 && cfg->members_per_conference > 0 && cfg->members_per_conference <= MI_MIXER_MAX_CHANNELS &&
	            cfg->nstreams % cfg->members_per_conference == 0);
	const int n = cfg->nstreams, mm = cfg->members_per_conference;
	MI_PLAN_ARG(nadmit <= (INT32_MAX - n) / mm);
	std::vector<mi_bridge_leg> all(legs, legs + n);
	for (int k = 0; k < nadmit; ++k) all.insert(all.end(), (size_t)mm, admit[k]);
	mi_bridge_config c = *cfg;
	c.nstreams = (int32_t)all.size();
	const int rc = plan_legs(rules, &c, all.data(), p, n);
	if (rc != MI_OK) return rc;
	std::vector<int32_t> rates;
	for (size_t i = 0; i < all.size(); ++i) {
		const mi_bridge_leg &l = all[i];
		if (std::find(rates.begin(), rates.end(), l.rate) == rates.end()) rates.push_back(l.rate);
		if (std::find_if(p->kinds.begin(), p->kinds.end(), [&](const mi_bridge_leg &k) { return same_kind(k, l); }) == p->kinds.end())
			p->kinds.push_back(l), p->kind_ratio.push_back(p->ratio.empty() ? 1 : p->ratio[i]);
	}
	if (cfg->plc && (int)rates.size() > PLAN_MAX_RATE_CLASSES)
		MI_REFUSE("mi_bridge_create_open: plc with %zu distinct rates among the legs and the admitted kinds: the concealer holds %d rate classes",
		          rates.size(), PLAN_MAX_RATE_CLASSES);
	p->open = true;
	p->cfg.nstreams = p->n = n, p->nconf = n / mm;
	p->leg_rate.resize((size_t)n); // (plan_bridge keeps the rates it was given)
	if (p->ratio.empty()) p->ratio.assign(all.size(), 1); // no resamplers: every kind at the mix
	p->ratio.resize((size_t)n);
	p->leg_codec.resize((size_t)n);
	for (int s = 0; s < n; ++s) p->leg_codec[(size_t)s] = (uint8_t)(legs[s].in_codec | legs[s].out_codec << 2);
	return MI_OK;
}

inline mi_bridge_leg seat_kind(const Plan &p, int s) {
	const int pair = p.leg_codec.empty() ? p.cfg.in_codec | p.cfg.out_codec << 2 : p.leg_codec[(size_t)s];
	return {p.leg_rate.empty() ? p.cfg.rate : p.leg_rate[(size_t)s], pair & 3, pair >> 2};
}

// mi_bridge_change_members' rules, without a device.  flags [p.n]: the pins' MI_MIX_* as the roster has them.  MI_OK with
// ratio [count] -- the ratio byte of every JOIN's kind, 0 for a LEAVE --, or the refusal naming the entry; nothing is applied
// here.  An open plan admits its `kinds` on every seat; any other plan admits on a seat that seat's own kind only.  scratch:
// mi::check_seat_list's
inline int check_changes(const Plan &p, const uint8_t *flags, const mi_bridge_change *ch, int count, std::vector<uint8_t> *ratio,
                         std::vector<int32_t> *scratch = nullptr) {
	MI_PLAN_ARG(flags && ratio && count >= 0 && (ch || count == 0));
	const char *fn = "mi_bridge_change_members";
	static_assert(MI_BRIDGE_JOIN == MI_SEAT_JOIN && MI_BRIDGE_LEAVE == MI_SEAT_LEAVE, "the public ops are the command's");
	const int rc = mi::check_seat_list(fn, "MI_BRIDGE_JOIN (1) or MI_BRIDGE_LEAVE (2)", p.n, ch, count, scratch);
	if (rc != MI_OK) return rc;
	ratio->assign((size_t)count, 0);
	for (int i = 0; i < count; ++i) {
		const mi_bridge_change &c = ch[i];
		if (c.op == MI_BRIDGE_LEAVE) {
			if (!(flags[c.stream] & MI_MIX_LINKED)) return mi::set_error("%s: entry %d: stream %d is no member", fn, i, c.stream), (int)MI_EINVAL;
			continue;
		}
		const mi_bridge_leg own = seat_kind(p, c.stream);
		const size_t kind = (size_t)(std::find_if(p.kinds.begin(), p.kinds.end(), [&](const mi_bridge_leg &k) { return same_kind(k, c.leg); }) - p.kinds.begin());
		const bool ok = p.open ? kind < p.kinds.size() : same_kind(own, c.leg);
		if (!ok && p.open)
			MI_REFUSE("%s: entry %d: seat %d cannot take an endpoint at %d Hz with codecs in %d, out %d: the bridge admits %zu kinds, "
			          "those of its initial legs and of mi_bridge_create_open's h_admit", fn, i, c.stream, c.leg.rate, c.leg.in_codec, c.leg.out_codec,
			          p.kinds.size());
		if (!ok)
			MI_REFUSE("%s: entry %d: seat %d cannot take an endpoint at %d Hz with codecs in %d, out %d: 1 kind is admitted there, the "
			          "seat's own (%d Hz, in %d, out %d); mi_bridge_create_open plans a bridge for more", fn, i, c.stream, c.leg.rate,
			          c.leg.in_codec, c.leg.out_codec, own.rate, own.in_codec, own.out_codec);
		(*ratio)[(size_t)i] = p.open ? p.kind_ratio[kind] : p.ratio.empty() ? 1 : p.ratio[(size_t)c.stream];
	}
	return MI_OK;
}

} // namespace
