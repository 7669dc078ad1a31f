// bridge_offgrid.hip -- the seventh kernel of mi_bridge (bridge.hip, whose head describes a tick's phases): a conference with a
// leg at 44 100 Hz (mi_bridge_create_offgrid) -- an L16 / 44 100 member (RTP payload types 10 and 11), AAC-ELD at 44.1 kHz, a
// sound card -- beside legs of every older form.  A unit of its own like bridge_ratios.hip: bridge.hip keeps mi_bridge, the
// plan's constructors, the tables and the dispatch, and calls mi_bridge_offgrid_launch.  Built with -ffp-contract=off like
// bridge.hip: MSVolume's control chain is float32 evaluated unfused in source order; the resampler's sums are __builtin_fmaf
// chains, fused where resample.hip fuses them.
//
// What 44 100 Hz brings, each step written once in bridge_phases.hpp:
//   a tick of 441 samples = 55 groups of eight and ONE sample.  (A) reads that sample alone (LegSrc::fetch_tail) and puts the
//   tail group on the row with seven zeros (keep_head), so the meter's words and the peak / DC reduction run over whole words
//   whose padding adds nothing; (G) keeps the padding zero; (W) stores 55 groups and then the one sample (store_tail).  The
//   tail group's load and store touch no byte past the leg's 882 or 441, and no store at all does: the row's tail in the host
//   buffers stays as it is.  (A G.711 leg's group 54 arrives, as every even group does, in the aligned 16-byte load that also
//   spans the next group's place -- inside the row's pitch, and only its own eight code bytes are decoded.)
//   resamplers at 441 : 80 .. 147 : 160 (offgrid_run): mi_resampler's generic order on the per-phase table, 48 to 264 taps in
//   80 to 441 rows, 28 to 92 KB -- more than the 64 KB of a workgroup's LDS can give a wavefront.
// Where the table is read from.  The choice was between each lane reading its own row from memory in 16-byte loads, and
// staging slices of rows through LDS for the conference's four waves to share.  A tick uses every row about once per member
// and direction (160 outputs from 160 rows, 441 from 441), and the four waves run different members, in (W) mostly of other
// kinds: a slice staged in LDS would be read as often as it was written, behind a barrier that the one-wavefront-per-member
// loops of (U) and (W) do not otherwise have.  Read from memory, a lane's row is contiguous, so every load is a full 16 bytes
// -- the width at which L1 and L2 serve a lane at their full rate; 8-byte accesses run at 0.54 to 0.70 of it -- and the rows
// are the same 28 to 92 KB for every such leg of every conference of the launch: they stay in each XCD's 4 MiB L2, the case the
// microarchitecture notes measure at 17 to 19 TB/s for rows shared by every workgroup.  So: own row, 16-byte loads, two in
// flight per step of eight taps; the LDS holds history ++ tick as floats only.
#include "common.hpp"

#include "bridge_phases.hpp"

#pragma clang fp contract(off)

namespace {

// bridge_ratios_kernel with the 44 100 Hz form as well: every older form's loops in (U) and (W) as they are, the new one's
// behind them.  Only a bridge with such a leg or admitted kind runs this kernel.  NO occupancy hint, unlike
// bridge_ratios_kernel: held to 128 VGPRs (four waves per SIMD) the composition spills one register to 8 bytes of scratch per
// lane; left to itself the allocator takes 142 and spills nothing: three conferences per CU instead of four.  A 16 kHz
// conference of 32 with 441-sample rows takes 39 KB of LDS, four to a CU, so below about 40 members the registers are the
// bound and above it the LDS is (tests/test_bridge_offgrid_cpu.py holds the kernel to no spill and no scratch).
__global__ __launch_bounds__(BT) void bridge_offgrid_kernel(OffgridArgs oa) {
	extern __shared__ __attribute__((aligned(16))) char smem[];
	__shared__ int s_pk[BMAX], s_dc[BMAX];
	__shared__ int4 s_par[BMAX];
	__shared__ unsigned char s_rt[BMAX], s_on[BMAX], s_cd[BMAX];
	const RatiosArgs &ga = oa.g;
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
	Member me = load_member<F_OFF, true>(k, a, ra.ratio, la.codec, p, st);
	stage_rows<F_OFF>(k, a.present, ra.ratio, LegSrc{static_cast<const uint8_t *>(a.in), la.in_pitch, la.codec});
	__syncthreads();
	meter<F_OFF>(k, a, me, p, st);
	__syncthreads();
	level_legs<F_OFF>(k, ua.wide >> 2);
	__syncthreads();
	resample_in<F_OFF>(k, ra, &ua, &qa, scr, &ga, &oa);
	__syncthreads();
	mix<false>(k, a.nslice);
	__syncthreads();
	mix_minus<F_OFF, BY_KIND>(k, out, la.out_pitch);
	__syncthreads();
	resample_out<F_OFF, BY_KIND>(k, ra, &ua, &qa, scr, out, la.out_pitch, &ga, &oa);
}

} // namespace

// bridge.hip's dispatch for Plan::OFFGRID.  The argument struct lives in each unit's anonymous namespace, so it crosses as
// bytes whose size both units check
int mi_bridge_offgrid_launch(const void *args, size_t bytes, int nconf, size_t lds, hipStream_t stream) {
	MI_CHECK_ARG(args && bytes == sizeof(OffgridArgs) && nconf > 0);
	OffgridArgs oa;
	memcpy(&oa, args, sizeof(oa));
	// a lane's row starts on 16 bytes: both offsets whole float4s, both filters whole groups of eight taps
	MI_CHECK_ARG(oa.tab_in % 4 == 0 && oa.tab_out % 4 == 0 && oa.filt_in % 8 == 0 && oa.filt_out % 8 == 0 && oa.num > 0 && oa.den > 0);
	hipLaunchKernelGGL(bridge_offgrid_kernel, dim3((unsigned)nconf), dim3(BT), lds, stream, oa);
	MI_LAUNCH_CHECK();
	return MI_OK;
}

// (mi_warmup, ctx.hip: this unit's code object is loaded when the library is, not under a tick's first launch)
static const mi::WarmEntry g_warm_bridge_offgrid(reinterpret_cast<const void *>(&bridge_offgrid_kernel));
