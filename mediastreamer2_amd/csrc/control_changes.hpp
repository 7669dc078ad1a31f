// control_changes.hpp -- control changes on their way to the device, next to seat_changes.hpp: mi_ctl_cmd, the one place that
// says how the device unpacks it (load_ctl), the list checks, and mi::ControlChanges, which mi::ConferenceBook
// (conference_book.hpp) drives for mi_bridge_change_controls and mi_session_change_controls alike.  But for load_ctl, host code
// only, plain C++ with no HIP in it (tests/host/controls_check.cpp runs it alone on the CPU).  A change -- mute, listen-only, input gain, a seat's
// mi_volume_params -- is applied by the tick submitted next, so between the call and that submit it is bookkeeping: the host's
// mirrors of what the device will hold (mi::Roster::flags, and the gains and parameters here), which every setter updates at
// once, the waiting ones too; per seat the fields that a call has touched since the last submit, merged; and the command row
// the tick carries, staged AT SUBMIT from the mirrors -- so whoever spoke last before the submit has the last word, field by
// field.  Also here: the threshold the device's election compares with (report_threshold).
#pragma once
#include <cmath>
#include <cstring>
#include <type_traits>
#include <utility>

#include "seat_changes.hpp"

// One control change as the device applies it (controls.hip): a pinned row of these per pipe slot, uploaded with the tick they
// take effect in.  MI_CTL_JOINED is the library's own: the seat's place in its conference's joining order, which the report
// kernel's election reads -- it rides here because mi_seat_cmd has no room for it.
// (the three public bits as msmi355x_bridge.h and msmi355x_session_controls.h spell them, token for token)
#define MI_CTL_FLAGS 1u
#define MI_CTL_GAIN 2u
#define MI_CTL_VOLUME 4u
#define MI_CTL_JOINED 8u
struct mi_ctl_cmd {
	int32_t stream;
	uint8_t what;  // MI_CTL_*
	uint8_t flags; // FLAGS: the pin's MI_MIX_*, whole
	uint8_t pad[2];
	float gain;      // GAIN
	uint32_t joined; // JOINED
	mi_volume_params params; // VOLUME
	uint32_t pad2;
};
static_assert(sizeof(mi_volume_params) == 60, "fifteen words");
static_assert(sizeof(mi_ctl_cmd) == 80, "a command is five 16-byte loads");
// (load_ctl's shifts: the word at 4 is what | flags << 8; controls.hip copies the fifteen words from 16 on)
static_assert(offsetof(mi_ctl_cmd, stream) == 0 && offsetof(mi_ctl_cmd, what) == 4 && offsetof(mi_ctl_cmd, flags) == 5 &&
                  offsetof(mi_ctl_cmd, gain) == 8 && offsetof(mi_ctl_cmd, joined) == 12 && offsetof(mi_ctl_cmd, params) == 16,
              "load_ctl unpacks these offsets");

#ifdef __HIPCC__
// the head of command i of a row as controls_kernel reads it: the first 16-byte load, named
struct CtlFields { int stream; unsigned what, flags; float gain; unsigned joined; };
__device__ __forceinline__ CtlFields load_ctl(const mi_ctl_cmd *row, int i) {
	const uint4 c = reinterpret_cast<const uint4 *>(row + i)[0];
	return {(int)c.x, c.y & 0xffu, (c.y >> 8) & 0xffu, __uint_as_float(c.z), c.w};
}
#endif

namespace mi {

// audioconference.c:31 compares dBm0 floats (max_db > -30); the device compares linear values.  The smallest float whose
// 10 * log10f is above -30.0f, found with the host's own libm, makes `lin >= thr` the very same predicate
// (tests/test_controls_cpu.py holds it for every float within 64 ulp)
inline float report_threshold() {
	auto above = [](float x) { return 10 * log10f(x) > -30.0f; };
	float x = 1e-3f;
	for (int i = 0; i < 1024 && above(x); ++i) x = nextafterf(x, 0.f);
	for (int i = 0; i < 2048 && !above(x); ++i) x = nextafterf(x, 1.f);
	return x;
}

// what holds of every control list before anything is applied.  Control: { int32_t stream; uint32_t what, flags; ... };
// allowed: the MI_CTL_* bits the object serves; flags [n]: the roster's MI_MIX_*, earlier membership changes included; seen:
// check_named_once's
template <class Control>
inline int check_controls(const char *fn, int n, const uint8_t *flags, unsigned allowed, const Control *ch, int count, std::vector<int32_t> &seen) {
	if (count < 0 || (count > 0 && !ch)) return set_error("%s: %d changes at %s", fn, count, ch ? "h_changes" : "a null h_changes"), (int)MI_EINVAL;
	seen.clear();
	for (int i = 0; i < count; ++i) {
		const Control &c = ch[i];
		if (c.stream < 0 || c.stream >= n) return set_error("%s: entry %d names stream %d of %d", fn, i, c.stream, n), (int)MI_EINVAL;
		if (!c.what || (c.what & ~allowed))
			return set_error("%s: entry %d (stream %d) has what 0x%x; a non-empty mask within 0x%x", fn, i, c.stream, c.what, allowed), (int)MI_EINVAL;
		if ((c.what & MI_CTL_FLAGS) && (c.flags & ~(uint32_t)(MI_MIX_ACTIVE | MI_MIX_OUTPUT)))
			return set_error("%s: entry %d (stream %d) has flags 0x%x; MI_MIX_ACTIVE | MI_MIX_OUTPUT only, MI_MIX_LINKED is membership's", fn, i,
			                 c.stream, c.flags), (int)MI_EINVAL;
		if ((c.what & MI_CTL_FLAGS) && !(flags[c.stream] & MI_MIX_LINKED))
			return set_error("%s: entry %d: MI_CTL_FLAGS on stream %d, which is no member", fn, i, c.stream), (int)MI_EINVAL;
		seen.push_back(c.stream);
	}
	return check_named_once(fn, ch, count, seen);
}

// a public control record with a `params` field (mi_bridge_control; not mi_session_control: the two readers below are empty)
template <class Control, class = void>
struct carries_params : std::false_type {};
template <class Control>
struct carries_params<Control, std::void_t<decltype(std::declval<Control>().params)>> : std::true_type {};

// MI_CTL_VOLUME's own rule (mi_bridge_set_volume_params'): a bridge has no far end to limit against
template <class Control>
inline int check_control_params(const char *fn, const Control *ch, int count) {
	if constexpr (carries_params<Control>::value)
		for (int i = 0; i < count; ++i)
			if ((ch[i].what & MI_CTL_VOLUME) && ch[i].params.peer != -1)
				return set_error("%s: entry %d (stream %d) names an echo-limiter peer (%d); a bridge has no far end to limit against", fn, i,
				                 ch[i].stream, ch[i].params.peer), (int)MI_ENOTSUP;
	return MI_OK;
}

struct ControlChanges {
	std::vector<float> gain;              // [n] the pins' input gains as the device will hold them
	std::vector<mi_volume_params> params; // [n] the seats' MSVolume parameters likewise; empty: the object has no setter for them
	std::vector<uint8_t> what;            // [n] the fields a call has touched since the last submit
	std::vector<int32_t> changed;         // the seats with what[s] != 0
	std::vector<int32_t> scratch;         // the list checks' (check_named_once), the membership lists' too

	void init(int n, const mi_volume_params *initial) { // initial: every seat's parameters at creation, or null
		gain.assign((size_t)n, 1.0f);                   // mi_mixer_create's
		if (initial) params.assign((size_t)n, *initial);
		what.assign((size_t)n, 0);
		changed.clear();
		changed.reserve((size_t)n), scratch.reserve((size_t)n); // a call never grows them
	}

	// the waiting setters' part: the device is written by their own blocking copies, the mirrors follow
	void set_gains(const float *h_gain) { std::copy(h_gain, h_gain + gain.size(), gain.begin()); }
	void set_params(int first, int count, const mi_volume_params *h) {
		if (!params.empty()) std::copy(h, h + count, params.begin() + first);
	}

	// a seat is listed once, when its first field is touched: `changed` never holds more than n seats, the row's length
	void note(int32_t stream, uint8_t bits) {
		if (!bits) return;
		if (!what[(size_t)stream]) changed.push_back(stream);
		what[(size_t)stream] |= bits;
	}

	// one entry of a call that has been checked: the mirrors at once, the fields noted.  roster_flags [n]: mi::Roster::flags
	template <class Control>
	void apply(const Control &c, uint8_t *roster_flags) {
		const size_t s = (size_t)c.stream;
		if (c.what & MI_CTL_FLAGS) roster_flags[s] = (uint8_t)((roster_flags[s] & MI_MIX_LINKED) | (c.flags & (MI_MIX_ACTIVE | MI_MIX_OUTPUT)));
		if (c.what & MI_CTL_GAIN) gain[s] = c.gain;
		note(c.stream, (uint8_t)(c.what & (MI_CTL_FLAGS | MI_CTL_GAIN)));
	}
	template <class Control>
	void apply_params(const Control &c) {
		if constexpr (carries_params<Control>::value)
			if (c.what & MI_CTL_VOLUME) params[(size_t)c.stream] = c.params, note(c.stream, MI_CTL_VOLUME);
	}

	// the command row of the tick about to be submitted, into the slot's pinned staging: every touched field as the mirrors hold
	// it NOW.  roster_flags, joined [n]: mi::Roster's.  Returns the row's length, <= n
	int stage(mi_ctl_cmd *row, const uint8_t *roster_flags, const uint32_t *joined) const {
		int k = 0;
		for (const int32_t s : changed) {
			if ((size_t)k == what.size()) break; // (the row holds n commands; `changed` lists a seat once)
			mi_ctl_cmd &c = row[k++];
			memset(&c, 0, sizeof(c));
			c.stream = s, c.what = what[(size_t)s], c.flags = roster_flags[(size_t)s], c.gain = gain[(size_t)s], c.joined = joined[(size_t)s];
			if (c.what & MI_CTL_VOLUME) c.params = params[(size_t)s];
		}
		return k;
	}

	// the tick is on its way
	void submitted() {
		for (const int32_t s : changed) what[(size_t)s] = 0;
		changed.clear();
	}
};

} // namespace mi
