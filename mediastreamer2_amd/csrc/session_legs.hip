// session_legs.hip -- the ingress and egress of a session whose legs differ in rate or codec (mi_session_create_legs): what
// plumb_to_conf hangs on an endpoint's pin around the canceller -- its decoder and in_resampler in front, its out_resampler and
// encoder behind (audioconference.c:226-251) -- as two launches for the whole batch, one wavefront running one leg, four legs
// per workgroup:
//   session_ingress_kernel  the leg's own groups from its byte row through its codec (or the concealer's PCM row); a leg at
//                           the canceller's rate goes straight to the microphone tick, one below it onto the wavefront's row
//                           in LDS, through rated_up with its 47-sample history and the shared table, and from the row out;
//   session_egress_kernel   the leg's mix at the canceller's rate through resample_down by its ratio with its
//                           ratio * 48 - 1 sample history, store_group with its out codec into its byte row; ratio 1: store_row.
// Both run every leg every tick, unmasked, as the uniform session's resamplers and encoder do.  The steps are the bridge's
// (bridge_phases.hpp, resample_steps.hpp) -- the arithmetic of mi_resampler's batch kernels and mi_g711's, bit for bit --; the
// waves of a workgroup share nothing, so there is no barrier: wave_sync orders a wave's own LDS traffic.
#include "session_legs.hpp"

#include "bridge_phases.hpp"
#include "resample_tables.hpp"

namespace {

constexpr int LT = 256, LEG_WAVES = LT / 64;

struct IngressArgs {
	LegSrc src;           // the byte rows, their pitch, every leg's codec pair (its low two bits: what the row holds)
	const uint8_t *ratio; // [n]
	int16_t *hist;        // [n][hist_stride]
	const float *tab;
	int tab_up[7];
	int16_t *mic;         // [n][mic_stride]
	int n, len, hist_stride, mic_stride;
	int row_bytes, wave_bytes; // the wavefront's row in LDS; row + scratch
};

struct EgressArgs {
	const int16_t *mix;   // [n][len]
	const uint8_t *ratio, *codec;
	int16_t *hist;        // [n][hist_stride]
	const float *tab;
	int tab_down[7];
	uint8_t *out;         // [n][out_pitch] bytes
	int n, len, hist_stride, out_pitch;
	int wave_bytes;
};

__global__ __launch_bounds__(LT) void session_ingress_kernel(IngressArgs a) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
	const int s = (int)blockIdx.x * LEG_WAVES + wave;
	if (s >= a.n) return; // (the last workgroup: no barrier follows)
	const int r = __builtin_amdgcn_readfirstlane(a.ratio[s]), kind = __builtin_amdgcn_readfirstlane(a.src.kind(s));
	const int ll = a.len / r; // the leg's own tick
	int16_t *row = reinterpret_cast<int16_t *>(smem + wave * a.wave_bytes);
	int16_t *mic = a.mic + (size_t)s * a.mic_stride;
	for (int g = lane; g < (ll >> 3); g += 64) {
		const uint4 d = a.src.decoded(a.src.fetch(s, kind, g), kind, g);
		*reinterpret_cast<uint4 *>((r == 1 ? mic : row) + 8 * g) = d;
	}
	if (r == 1) return;
	wave_sync();
	rated_up(reinterpret_cast<float *>(smem + wave * a.wave_bytes + a.row_bytes), row, a.hist + (size_t)s * a.hist_stride, a.tab + a.tab_up[r], r, ll, lane);
	for (int g = lane; g < (a.len >> 3); g += 64) *reinterpret_cast<uint4 *>(mic + 8 * g) = *reinterpret_cast<const uint4 *>(row + 8 * g);
}

__global__ __launch_bounds__(LT) void session_egress_kernel(EgressArgs a) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
	const int s = (int)blockIdx.x * LEG_WAVES + wave;
	if (s >= a.n) return;
	const int r = __builtin_amdgcn_readfirstlane(a.ratio[s]), kind = __builtin_amdgcn_readfirstlane(a.codec[s] >> 2);
	const int16_t *mix = a.mix + (size_t)s * a.len;
	const size_t at = (size_t)s * a.out_pitch;
	if (r == 1) store_row(mix, a.out + at, kind, a.len, lane);
	else
		resample_down<BY_KIND>(reinterpret_cast<float *>(smem + wave * a.wave_bytes), mix, a.hist + (size_t)s * a.hist_stride, a.tab + a.tab_down[r], r,
		                       a.len, rs_plen(RS_FILT, r, a.len), lane, a.out, at, kind);
}

} // namespace

void mi_session_legs_destroy(SessionLegs *g) {
	if (!g) return;
	void *const dv[] = {g->d_ratio, g->d_codec, g->d_hist_in, g->d_hist_out, g->d_tab};
	for (void *p : dv)
		if (p) mi_dev_free(g->ctx, p);
	delete g;
}

int mi_session_legs_reset(SessionLegs *g, int first, int count) {
	MI_CHECK_ARG(g && first >= 0 && count >= 0 && first + count <= g->z.n);
	if (count == 0) return MI_OK;
	const SessionLegsSizes &z = g->z;
	MI_HIP(hipMemsetAsync(g->d_hist_in + (size_t)first * z.hin_stride, 0, (size_t)count * z.hin_stride * sizeof(int16_t), g->ctx->stream));
	MI_HIP(hipMemsetAsync(g->d_hist_out + (size_t)first * z.hout_stride, 0, (size_t)count * z.hout_stride * sizeof(int16_t), g->ctx->stream));
	return MI_OK;
}

int mi_session_legs_create(mi_ctx *ctx, const SessionLegsSizes &z, SessionLegs **out) {
	MI_CHECK_ARG(ctx && out && z.n > 0 && z.len > 0 && z.len % 8 == 0 && z.used && z.ratio && z.codec);
	MI_CHECK_ARG(z.hin_stride >= RS_FILT && z.hin_stride % 8 == 0 && z.hout_stride % 8 == 0 && z.in_row % 16 == 0 && z.in_scratch % 16 == 0 &&
	             z.out_scratch % 16 == 0 && z.in_row >= z.len * 2);
	*out = nullptr;
	SessionLegs *g = new SessionLegs();
	g->ctx = ctx, g->z = z;
	g->z.used = nullptr, g->z.ratio = g->z.codec = nullptr; // the caller's: not kept
	auto fail = [&](int code) { return mi_session_legs_destroy(g), code; };
	const size_t n = (size_t)z.n;
	for (size_t s = 0; s < n; ++s) { // every leg's resamplers fit what the plan sized: no store past a history row or the scratch
		const int r = z.ratio[s];
		if (!(r == 1 || ((r == 2 || r == 3 || r == 6) && z.used[r] && z.len % (8 * r) == 0 && r * RS_FILT <= z.hout_stride &&
		                 rs_flat_len(z.len / r) * (int)sizeof(float) <= z.in_scratch &&
		                 (r * rs_plen(RS_FILT, r, z.len) + z.len) * (int)sizeof(float) <= z.out_scratch)))
			return mi::set_error("mi_session_legs_create: leg %zu's ratio %d is not what the plan sized", s, r), fail(MI_EINVAL);
	}
	std::vector<uint8_t> codec(z.codec, z.codec + n);
	for (size_t s = 0; s < n; ++s) codec.push_back((uint8_t)(z.codec[s] & ~3u)); // behind the concealer the row holds PCM
	g->d_ratio = (uint8_t *)mi_dev_alloc(ctx, n);
	g->d_codec = (uint8_t *)mi_dev_alloc(ctx, 2 * n);
	g->d_hist_in = (int16_t *)mi_dev_alloc(ctx, n * z.hin_stride * sizeof(int16_t));
	g->d_hist_out = (int16_t *)mi_dev_alloc(ctx, n * z.hout_stride * sizeof(int16_t));
	if (!g->d_ratio || !g->d_codec || !g->d_hist_in || !g->d_hist_out) return fail(MI_ENOMEM);
	if (hipMemcpy(g->d_ratio, z.ratio, n, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(g->d_codec, codec.data(), 2 * n, hipMemcpyHostToDevice) != hipSuccess)
		return fail(MI_ENODEV);
	int rc;
	if ((rc = mi_session_legs_reset(g, 0, z.n)) != MI_OK) return fail(rc);
	// the shared tables, one pair per ratio in use: the up-sampler's polyphase rows [r][48] as designed, the down-sampler's
	// phase-major (resample_tables.hpp)
	std::vector<float> all, t;
	for (int r = 2; r < 7; ++r) {
		if (!z.used[r]) continue;
		if ((rc = design_table(ctx, z.rate / r, z.rate, t)) != MI_OK) return fail(rc);
		if (t.size() != (size_t)r * RS_FILT) return fail(MI_ENOTSUP);
		g->tab_up[r] = (int)all.size();
		all.insert(all.end(), t.begin(), t.end());
		if ((rc = design_table(ctx, z.rate, z.rate / r, t)) != MI_OK) return fail(rc);
		if (t.size() != (size_t)r * RS_FILT) return fail(MI_ENOTSUP);
		g->tab_down[r] = (int)all.size();
		append_phase_major(all, t, r, RS_FILT);
	}
	if (all.empty()) all.push_back(0.f); // (codecs alone differ: no table is read)
	if (!(g->d_tab = (float *)mi_dev_alloc(ctx, all.size() * sizeof(float)))) return fail(MI_ENOMEM);
	if (hipMemcpy(g->d_tab, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return fail(MI_ENODEV);
	*out = g;
	return MI_OK;
}

int mi_session_legs_ingress(SessionLegs *g, const uint8_t *d_in, size_t in_pitch, bool pcm, int16_t *d_mic, int mic_stride) {
	MI_CHECK_ARG(g && d_in && d_mic && in_pitch % 16 == 0 && mic_stride % 8 == 0 && mic_stride >= g->z.len);
	const SessionLegsSizes &z = g->z;
	IngressArgs a = {};
	a.src = {d_in, (int)in_pitch, pcm ? g->d_codec + z.n : g->d_codec};
	a.ratio = g->d_ratio, a.hist = g->d_hist_in, a.tab = g->d_tab;
	for (int r = 0; r < 7; ++r) a.tab_up[r] = g->tab_up[r];
	a.mic = d_mic, a.n = z.n, a.len = z.len, a.hist_stride = z.hin_stride, a.mic_stride = mic_stride;
	a.row_bytes = z.in_row, a.wave_bytes = z.in_row + z.in_scratch;
	hipLaunchKernelGGL(session_ingress_kernel, dim3((unsigned)((z.n + LEG_WAVES - 1) / LEG_WAVES)), dim3(LT), (size_t)LEG_WAVES * a.wave_bytes,
	                   g->ctx->stream, a);
	MI_LAUNCH_CHECK();
	return MI_OK;
}

int mi_session_legs_egress(SessionLegs *g, const int16_t *d_mix, uint8_t *d_out, size_t out_pitch) {
	MI_CHECK_ARG(g && d_mix && d_out && out_pitch % 16 == 0);
	const SessionLegsSizes &z = g->z;
	EgressArgs a = {};
	a.mix = d_mix, a.ratio = g->d_ratio, a.codec = g->d_codec, a.hist = g->d_hist_out, a.tab = g->d_tab;
	for (int r = 0; r < 7; ++r) a.tab_down[r] = g->tab_down[r];
	a.out = d_out, a.n = z.n, a.len = z.len, a.hist_stride = z.hout_stride, a.out_pitch = (int)out_pitch;
	a.wave_bytes = z.out_scratch;
	hipLaunchKernelGGL(session_egress_kernel, dim3((unsigned)((z.n + LEG_WAVES - 1) / LEG_WAVES)), dim3(LT), (size_t)LEG_WAVES * a.wave_bytes,
	                   g->ctx->stream, a);
	MI_LAUNCH_CHECK();
	return MI_OK;
}
