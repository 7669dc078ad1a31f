// bridge_ratios.hip -- the sixth kernel of mi_bridge (bridge.hip, whose head describes a tick's phases): a conference with a leg
// at 4 or 1/4 of the mix's rate, or at a : b of it in mi_resampler's generic order (mi_bridge_create_ratios).  A unit of its
// own: bridge.hip keeps mi_bridge, the plan's constructors, the tables and the dispatch, and calls mi_bridge_ratios_launch.
// Built with -ffp-contract=off like bridge.hip: MSVolume's control chain is float32 evaluated unfused in source order; the
// generic resampler's sums are __builtin_fmaf chains, fused where resample.hip fuses them.
#include "common.hpp"

#include "bridge_phases.hpp"

#pragma clang fp contract(off)

namespace {

// bridge_rational_kernel with the generic-order form as well: a 12 kHz member of a 16 kHz room, a 32 kHz member of an 8, 12
// or 24 kHz one.  A leg at 4 or 1/4 runs rated_up / resample_down with that ratio as the number it already is; a leg at a : b
// runs generic_run, one wavefront per member, in loops of its own in (U) and (W).  Only a bridge with such a leg runs this
// kernel.  Four waves per SIMD asked for: left to itself the allocator takes 141 VGPRs and a CU holds three conferences; held
// to 128 like bridge_rational_kernel it spills nothing (tests/test_bridge_ratios_cpu.py).
__global__ __launch_bounds__(BT) __attribute__((amdgpu_waves_per_eu(4))) void bridge_ratios_kernel(RatiosArgs ga) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	__shared__ unsigned char s_rt[BMAX], s_on[BMAX], s_cd[BMAX];
	const RationalArgs &qa = ga.q;
	const UpdownArgs &ua = qa.u;
	const LegsArgs &la = ua.l;
	const RatedArgs &ra = la.r;
	const BridgeArgs &a = ra.b;
	const Conf k = conf_view(a, smem, s_pk, s_dc, s_par, s_rt, s_on, s_cd);
	uint8_t *out = static_cast<uint8_t *>(a.out);
	float *scr = wave_scratch(smem, ra, k.t);
	mi_volume_params p;
	mi_volume_state st;
	Member me = load_member<F_GEN, true>(k, a, ra.ratio, la.codec, p, st);
	stage_rows<F_GEN>(k, a.present, ra.ratio, LegSrc{static_cast<const uint8_t *>(a.in), la.in_pitch, la.codec});
	__syncthreads();
	meter<F_GEN>(k, a, me, p, st);
	__syncthreads();
	level_legs<F_GEN>(k, ua.wide >> 2);
	__syncthreads();
	resample_in<F_GEN>(k, ra, &ua, &qa, scr, &ga);
	__syncthreads();
	mix<false>(k, a.nslice);
	__syncthreads();
	mix_minus<F_GEN, BY_KIND>(k, out, la.out_pitch);
	__syncthreads();
	resample_out<F_GEN, BY_KIND>(k, ra, &ua, &qa, scr, out, la.out_pitch, &ga);
}

} // namespace

// bridge.hip's dispatch for Plan::RATIOS.  The argument struct lives in each unit's anonymous namespace, so it crosses as
// bytes whose size both units check
int mi_bridge_ratios_launch(const void *args, size_t bytes, int nconf, size_t lds, hipStream_t stream) {
	MI_CHECK_ARG(args && bytes == sizeof(RatiosArgs) && nconf > 0);
	RatiosArgs ga;
	memcpy(&ga, args, sizeof(ga));
	hipLaunchKernelGGL(bridge_ratios_kernel, dim3((unsigned)nconf), dim3(BT), lds, stream, ga);
	MI_LAUNCH_CHECK();
	return MI_OK;
}

// (mi_warmup, ctx.hip: this unit's code object is loaded when the library is, not under a tick's first launch)
static const mi::WarmEntry g_warm_bridge_ratios(reinterpret_cast<const void *>(&bridge_ratios_kernel));
