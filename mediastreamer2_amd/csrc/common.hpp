// common.hpp -- shared host-side plumbing of libmsmi355x (error reporting,
// context object, small RAII helpers).  gfx950 only; no CUDA/other-backend paths.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/msmi355x.h"

namespace mi {

void set_error(const char *fmt, ...);

#define MI_HIP(expr)                                                                        \
	do {                                                                                    \
		hipError_t e__ = (expr);                                                            \
		if (e__ != hipSuccess) {                                                            \
			mi::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
			return MI_ENODEV;                                                               \
		}                                                                                   \
	} while (0)

#define MI_CHECK_ARG(cond)                                                           \
	do {                                                                             \
		if (!(cond)) {                                                               \
			mi::set_error("%s:%d invalid argument: %s", __FILE__, __LINE__, #cond);  \
			return MI_EINVAL;                                                        \
		}                                                                            \
	} while (0)

#define MI_LAUNCH_CHECK()                                                                  \
	do {                                                                                   \
		hipError_t e__ = hipGetLastError();                                                \
		if (e__ != hipSuccess) {                                                           \
			mi::set_error("%s:%d kernel launch -> %s", __FILE__, __LINE__, hipGetErrorString(e__)); \
			return MI_ENODEV;                                                              \
		}                                                                                  \
	} while (0)

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
// Workgroups are observed to be dealt round-robin to the 8 XCDs (block b runs on XCD b % 8), each with its own L2.  A
// kernel whose neighbouring work items touch the same cache lines (rows of 960 bytes are not multiples of the 128-byte
// line) launches xcd_grid(n) blocks and turns blockIdx.x into its work item with xcd_item(): every XCD then owns one
// contiguous run of items, and a line two neighbours share is fetched into one L2 instead of two.  Speed only -- any
// placement computes the same thing.  Items >= n (the padding of the last run) return at once.
inline unsigned xcd_grid(unsigned n) { return (n + 7u) / 8u * 8u; }
__device__ __forceinline__ unsigned xcd_item(unsigned block, unsigned grid) { return (block & 7u) * (grid >> 3) + (block >> 3); }
inline size_t round_up(size_t a, size_t b) { return (a + b - 1) / b * b; }
// One kernel per translation unit, registered at load time: mi_warmup (ctx.hip) asks the runtime for its attributes, which makes it load
// the unit's code object on the context's device THEN -- not under the first launch of a ticker's first tick (HIP loads a code object
// lazily, behind one process-wide lock: sixteen ticker threads' first ticks waited 0.1 - 0.3 s for it).
void warm_register(const void *kernel);
struct WarmEntry {
	explicit WarmEntry(const void *k) { warm_register(k); }
};

} // namespace mi

struct mi_graph {
	struct mi_ctx *ctx = nullptr;
	hipGraph_t graph = nullptr;
	hipGraphExec_t exec = nullptr;
};

// MSBufferizer for a batch of streams on the device (fifo.hip).  Defined here because the canceller and the volume
// kernel read / write the rings directly (no separate pop / push launch).
struct mi_fifo {
	struct mi_ctx *ctx = nullptr;
	int nstreams = 0, capacity = 0;
	int16_t *d_ring = nullptr; // [nstreams][capacity]
	int2 *d_pos = nullptr;     // x = head (index of the oldest sample, < capacity), y = level (samples held)
	int32_t *d_overflow = nullptr;
};
// what a kernel needs of one
struct FifoView {
	int16_t *ring;
	int2 *pos;
	int32_t *overflow;
	int cap;
};
inline FifoView fifo_view(const mi_fifo *f) {
	FifoView v;
	v.ring = f ? f->d_ring : nullptr;
	v.pos = f ? f->d_pos : nullptr;
	v.overflow = f ? f->d_overflow : nullptr;
	v.cap = f ? f->capacity : 0;
	return v;
}

// Stream s's share of `phases` re-framing phases (mi_fifo_push_lead, mi_aec_stagger_fifos): a multiplicative hash (a bijection
// of the 32-bit slot index) decides, so that ANY regular arrangement of slots -- consecutive legs of a conference, every eighth
// slot, one bank -- gets every phase equally often.  Host and device use the same function.
__host__ __device__ inline unsigned fifo_phase_of(unsigned s, unsigned phases) { return ((s * 0x9E3779B1u) >> 16) % phases; }

// What the canceller's tick kernel needs of an up-sampling mi_resampler to run it as its own first phase (MSResample folded
// into MSSpeexEC's launch, mi_aec_process_fifos_resampled).  Filled by mi_resampler_view (resample.hip); ok = the resampler
// is an integer up-sampler with the 48-tap direct table whose streams all sit on a whole output period.
struct ResamplerView {
	int16_t *hist = nullptr;     // [nstreams][hist_stride] the last filt-1 input samples of every stream
	const float *table = nullptr; // [den][filt] polyphase rows
	int hist_stride = 0, den = 0, filt = 0, nstreams = 0;
	int device = -1;
	bool ok = false;
};
struct mi_resampler;
void mi_resampler_view(mi_resampler *r, ResamplerView *v);
// The table mi_resampler's generic kernel runs as a direct one, [den][filt_len] floats: the direct design, or an interpolated
// design blended once per phase (resample.hip's Design::phase_table, which mi_resampler_get_table does not hand out).  Returns
// its length, copying where cap allows; 0 for a design that has neither.  For the bridge's 44 100 Hz legs (bridge.hip).
int mi_resampler_get_phase_table(const mi_resampler *r, float *h_dst, int cap);

// What the fused volume + conference mix kernel (volume.hip) needs of an mi_mixer: its per-pin controls
struct MixerView {
	const uint8_t *flags = nullptr; // [nconf][mm] MI_MIX_*
	const float *gain = nullptr;    // [nconf][mm]
	int nconf = 0, mm = 0, ns = 0, device = -1;
};
struct mi_mixer;
void mi_mixer_view(const mi_mixer *m, MixerView *v);

// What the bridge's fused tick kernel (bridge.hip) needs of an mi_volume: parameters, running state and the one-second
// maximum windows of its streams (x = current maximum, y = ms since the window started, < 0: not started)
struct VolumeView {
	const mi_volume_params *params = nullptr;
	mi_volume_state *state = nullptr;
	float2 *win = nullptr;
	int nstreams = 0, sample_rate = 0, device = -1;
};
void mi_volume_view(const mi_volume *v, VolumeView *out);

// What the bridge's roster kernel (bridge_roster.hip) WRITES of an mi_volume and an mi_mixer when a new endpoint takes a seat,
// in stream order ahead of a tick: the meter as conference.hpp's reset_meters leaves it -- the state record, both halves of the
// energy mirror, the one-second window -- and the pin's flags.  The arrays are those of mi_volume_view / mi_mixer_view.
struct VolumeEdit {
	mi_volume_state *state = nullptr;
	float2 *win = nullptr;
	float *energy[2] = {nullptr, nullptr};
};
void mi_volume_edit(mi_volume *v, VolumeEdit *out);
// seat s's meter as a NEW MSVolume has it (one lane; both roster kernels)
__device__ __forceinline__ void fresh_meter(const VolumeEdit &v, int s) {
	mi_volume_state st = {};
	st.gain = st.target_gain = 1; // volume_init msvolume.c:92
	st.ng_gain = 1;               // :112
	v.state[s] = st;
	v.energy[0][s] = v.energy[1][s] = 0.f;
	v.win[s] = make_float2(0.f, -1.f); // the one-second window not started
}
struct MixerEdit {
	uint8_t *flags = nullptr; // [nconf][mm] MI_MIX_*
};
void mi_mixer_edit(mi_mixer *m, MixerEdit *out);

// One membership change as the device applies it (mi_bridge_change_members, mi_session_change_members): mi_seat_cmd, with the
// host's bookkeeping around it
#include "seat_changes.hpp"

// What the session's roster kernel (session_roster.hip) WRITES when a new endpoint takes a seat, besides the meter and the pin
// above: a fresh canceller, fresh resamplers.  The canceller's layout stays aec.hip's: the kernel is told which byte ranges of
// a stream are zero in a fresh speex_echo_state (both filter halves, the X history) and handed a template of the rest -- the
// `small` row and the scalar record as init_state writes them, built once on the device when the canceller is created.
struct AecEdit {
	float *X = nullptr, *WF = nullptr;   // [nstreams] x_bytes / wf_bytes each, multiples of 16
	size_t x_bytes = 0, wf_bytes = 0;
	float *small = nullptr;              // [nstreams] small_bytes each, a multiple of 16
	void *scal = nullptr;                // [nstreams] scal_bytes each, a multiple of 16
	const float *small_tpl = nullptr;    // small_bytes
	const void *scal_tpl = nullptr;      // scal_bytes
	int small_bytes = 0, scal_bytes = 0;
};
void mi_aec_edit(mi_aec *a, AecEdit *out);
struct ResamplerEdit {
	int16_t *hist = nullptr; // [nstreams][hist_stride], hist_stride a multiple of 8
	int2 *pos = nullptr;     // [nstreams] (last_sample, frac)
	int hist_stride = 0;
};
void mi_resampler_edit(mi_resampler *r, ResamplerEdit *out);

// The concealer batch whose streams each have a rate and a decoder of their own (plc.hip), for the bridge's legs:
// h_rate [nstreams] in Hz (multiples of 800), h_kind [nstreams] MI_SESSION_PCM16 | PCMA | PCMU: what the stream's byte row
// holds, pitch: samples per PCM row.  MI_ENOTSUP, stream and rate in the message: a rate outside 8 - 48 kHz, or one whose
// transforms need a radix above 17 (mi_plc_check_rate says so for one rate, naming `what` `index`, without a device).
// mi_plc_reset / _info / _destroy take the object as they take mi_plc_create's.
// mi_plc_process_legs: a tick of rate / 100 samples for every stream -- d_in byte rows at in_pitch (a multiple of 16; a
// stream fills the first rate / 100 x 1 or 2 bytes), d_pcm the int16 rows out at `pitch` samples, d_mode the MI_PLC_*
// event bytes -- in three launches, the decoders inside the RECEIVED pass.
// Seats that change hands (mi_bridge_create_open): h_open_rate [nopen] are the rates of EVERY kind that may come, the
// streams' own among them.  Each is a class from the start, built with room for every stream at rank = stream -- any class
// may come to hold all of them, so a change never allocates.  nopen == 0: classes for the rates present, sized by their
// streams, as ever.
// mi_plc_class_of: the class a NEW endpoint at `rate` on `stream` would sit in, nothing changed; MI_ENOTSUP for a rate that
// has none (a batch that is not open serves the stream's own rate only); mi_plc_create's batch: class 0 for every rate.
// mi_plc_seat: that endpoint, whose row holds `kind`, takes the stream in class `cls`, on the host's mirrors at once.  mi_plc_apply_seats: the device's part, one launch on the context's stream over d_cmd
// [count] -- for every JOIN the stream's tag and length rewritten and its class state at its rank zeroed (class_reset's four
// arrays).
constexpr int PLC_MAX_CLASSES = 7;
int mi_plc_check_rate(const char *fn, const char *what, int index, int rate);
int mi_plc_create_legs(mi_ctx *c, int nstreams, const int32_t *h_rate, const uint8_t *h_kind, int pitch, mi_plc **out,
                       const int32_t *h_open_rate = nullptr, int nopen = 0);
int mi_plc_process_legs(mi_plc *p, const uint8_t *d_in, size_t in_pitch, int16_t *d_pcm, size_t pitch, const uint8_t *d_mode);
int mi_plc_class_of(const mi_plc *p, int stream, int rate);
void mi_plc_seat(mi_plc *p, int stream, int cls, int kind);
int mi_plc_apply_seats(mi_plc *p, const mi_seat_cmd *d_cmd, int count);

struct mi_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	bool own_stream = false;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	int cu_count = 0;
	size_t hbm_bytes = 0;
	char name[128] = {0};
	// scratch for *_host entry points (grown on demand)
	void *scratch[4] = {nullptr, nullptr, nullptr, nullptr};
	size_t scratch_bytes[4] = {0, 0, 0, 0};
	int ensure_scratch(int slot, size_t bytes, void **out);
	int activate() const;
};
