// seat_changes.hpp -- membership changes on their way to the device: mi_seat_cmd, the one place that says how the device
// unpacks it (load_seat), the list checks, and mi::SeatChanges, which mi::ConferenceBook (conference_book.hpp) drives for
// mi_bridge_change_members and mi_session_change_members alike.  But for load_seat, host code only, plain C++ with no HIP in it
// (tests/host/session_open_check.cpp runs it alone on the CPU).  A change is applied by the tick submitted next, so between
// the call and that submit it is bookkeeping: what the calls since the last submit left per seat, merged; the command row the
// tick carries; and the seats whose output row is still to be cleared in slots to come.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/msmi355x.h"

namespace mi { void set_error(const char *fmt, ...); }

// One membership change as the device applies it: a pinned row of these per pipe slot, uploaded with the tick they take effect
// in.  bridge_roster.hip applies the bridge's part, session_roster.hip the session's, plc.hip the concealer's.
enum : uint8_t { MI_SEAT_JOIN = 1, MI_SEAT_LEAVE = 2, MI_SEAT_CLEAR = 4 }; // CLEAR: zero the seat's output row in this tick's slot
struct mi_seat_cmd {
	int32_t stream;
	uint8_t op;    // MI_SEAT_*
	uint8_t ratio; // JOIN: the kind's ratio byte (bridge_plan.hpp)
	uint8_t codec; // JOIN: in_codec | out_codec << 2
	uint8_t cls;   // JOIN: the kind's rate class in the concealer
	int32_t len;   // JOIN: the kind's rate / 100
	uint8_t flags; // JOIN, LEAVE: the pin's MI_MIX_* as the roster has them when the tick is submitted
	uint8_t pad[3];
};
static_assert(sizeof(mi_seat_cmd) == 16, "a command is one 16-byte load");
// (load_seat's shifts: the word at 4 is op | ratio << 8 | codec << 16 | cls << 24, the one at 12 starts with flags)
static_assert(offsetof(mi_seat_cmd, stream) == 0 && offsetof(mi_seat_cmd, op) == 4 && offsetof(mi_seat_cmd, ratio) == 5 && offsetof(mi_seat_cmd, codec) == 6 &&
                  offsetof(mi_seat_cmd, cls) == 7 && offsetof(mi_seat_cmd, len) == 8 && offsetof(mi_seat_cmd, flags) == 12, "load_seat unpacks these offsets");

#ifdef __HIPCC__
// command i of a row as the kernels read it (bridge_roster.hip, session_roster.hip, plc.hip): the one 16-byte load, named
struct SeatFields { int stream, len; unsigned op, ratio, codec, cls, flags; };
__device__ __forceinline__ SeatFields load_seat(const mi_seat_cmd *row, int i) {
	const uint4 c = reinterpret_cast<const uint4 *>(row)[i];
	return {(int)c.x, (int)c.z, c.y & 0xffu, (c.y >> 8) & 0xffu, (c.y >> 16) & 0xffu, c.y >> 24, c.w & 0xffu};
}
#endif

namespace mi {

// no seat twice in one call, or the refusal naming the later entry.  seen: every entry's stream, gathered by the caller's own
// pass into scratch with room for n (mi::ControlChanges::scratch), so that a call of up to n entries allocates nothing
template <class Entry>
inline int check_named_once(const char *fn, const Entry *ch, int count, std::vector<int32_t> &seen) {
	std::sort(seen.begin(), seen.end());
	const auto twice = std::adjacent_find(seen.begin(), seen.end());
	if (twice == seen.end()) return MI_OK;
	int at = count - 1;
	while (at > 0 && ch[at].stream != *twice) --at;
	return set_error("%s: entry %d names stream %d a second time in one call", fn, at, *twice), (int)MI_EINVAL;
}

// what holds of every change list before any entry is looked at for itself: each names a seat that exists and one of the two
// ops (MI_SEAT_JOIN and MI_SEAT_LEAVE are the public values), and no seat twice.  Change: { int32_t stream, op; ... }.
// names: the ops as the entry point's header spells them, for the message; scratch: check_named_once's, or null: the call's own
template <class Change>
inline int check_seat_list(const char *fn, const char *names, int n, const Change *ch, int count, std::vector<int32_t> *scratch = nullptr) {
	std::vector<int32_t> own, &seen = scratch ? *scratch : own;
	seen.clear();
	for (int i = 0; i < count; ++i) {
		const Change &c = ch[i];
		if (c.stream < 0 || c.stream >= n) return set_error("%s: entry %d names stream %d of %d", fn, i, c.stream, n), (int)MI_EINVAL;
		if (c.op != MI_SEAT_JOIN && c.op != MI_SEAT_LEAVE)
			return set_error("%s: entry %d (stream %d) has op %d; %s", fn, i, c.stream, c.op, names), (int)MI_EINVAL;
		seen.push_back(c.stream);
	}
	return check_named_once(fn, ch, count, seen);
}

// a list of uniform seats (mi_session_change_members): the above, and a LEAVE names a member.  flags [n]: the roster's MI_MIX_*
template <class Change>
inline int check_uniform_changes(const char *fn, const char *names, int n, const uint8_t *flags, const Change *ch, int count,
                                 std::vector<int32_t> *scratch = nullptr) {
	if (count < 0 || (count > 0 && !ch)) return set_error("%s: %d changes at %s", fn, count, ch ? "h_changes" : "a null h_changes"), (int)MI_EINVAL;
	const int rc = check_seat_list(fn, names, n, ch, count, scratch);
	if (rc != MI_OK) return rc;
	for (int i = 0; i < count; ++i)
		if (ch[i].op == MI_SEAT_LEAVE && !(flags[ch[i].stream] & MI_MIX_LINKED))
			return set_error("%s: entry %d: stream %d is no member", fn, i, ch[i].stream), (int)MI_EINVAL;
	return MI_OK;
}

struct SeatChanges {
	// what the calls since the last submit left for one seat, merged -- op 0: nothing.  clear: the seat was a member when one of
	// them came, so what it last heard is to be zeroed
	struct Pending { uint8_t op = 0, ratio = 0, codec = 0, cls = 0; bool clear = false; int32_t len = 0; };
	int slots = 0;
	std::vector<Pending> pending;    // [n]
	std::vector<int32_t> changed;    // the seats with pending[s].op != 0
	std::vector<uint8_t> clear_left; // [n] submits in which the seat's row is still to be cleared
	std::vector<int32_t> clearing;   // the seats with clear_left[s] != 0

	void init(int n, int pipe_slots) {
		slots = pipe_slots;
		pending.assign((size_t)n, Pending());
		clear_left.assign((size_t)n, 0);
		changed.clear(), clearing.clear();
		changed.reserve((size_t)n), clearing.reserve((size_t)n); // a call never grows them
	}

	// one entry of a call that has been checked: the last one before a submit wins, a member met on the way is remembered.  The
	// caller fills in what a JOIN brings (ratio, codec, cls, len)
	Pending &note(int32_t stream, uint8_t op, bool was_member) {
		Pending &p = pending[(size_t)stream];
		if (!p.op) changed.push_back(stream);
		p.clear |= was_member;
		p.op = op;
		return p;
	}

	// the seats a NEW endpoint has taken since the last submit: its filters are fresh, whatever the device still holds there
	std::vector<int32_t> joining() const {
		std::vector<int32_t> out;
		for (const int32_t s : changed)
			if (pending[(size_t)s].op & MI_SEAT_JOIN) out.push_back(s);
		return out;
	}

	// the command row of the tick about to be submitted, into the slot's pinned staging (acquire has waited for the slot's last
	// use): the merged changes, each with MI_SEAT_CLEAR where the seat's row is to be zeroed, then a bare MI_SEAT_CLEAR for every
	// seat that left within the last slots - 1 submits -- a slot's device row is cleared only by the tick that runs in that slot,
	// so the clear repeats until every slot has had it.  flags [n]: the pins' flags as the roster has them NOW -- a waiting call
	// since the change (set_controls, add_member, remove_member) has had the last word on them.  Returns the row's length, <= n
	int stage(mi_seat_cmd *row, const uint8_t *flags) const {
		int k = 0;
		for (const int32_t s : changed) {
			const Pending &p = pending[(size_t)s];
			const bool clear = p.clear || clear_left[(size_t)s];
			row[k++] = {s, (uint8_t)(p.op | (clear ? MI_SEAT_CLEAR : 0)), p.ratio, p.codec, p.cls, p.len, flags[(size_t)s], {0, 0, 0}};
		}
		for (const int32_t s : clearing)
			if (!pending[(size_t)s].op) row[k++] = {s, MI_SEAT_CLEAR, 0, 0, 0, 0, 0, {0, 0, 0}};
		return k;
	}

	// the tick is on its way
	void submitted() {
		for (const int32_t s : clearing) clear_left[(size_t)s]--;
		clearing.erase(std::remove_if(clearing.begin(), clearing.end(), [&](int32_t s) { return !clear_left[(size_t)s]; }), clearing.end());
		for (const int32_t s : changed) {
			if (pending[(size_t)s].clear && slots > 1) { // (a pipe of one slot has no other slot to clear)
				if (!clear_left[(size_t)s]) clearing.push_back(s);
				clear_left[(size_t)s] = (uint8_t)(slots - 1);
			}
			pending[(size_t)s] = Pending();
		}
		changed.clear();
	}
};

} // namespace mi
