// aec_tick.hpp -- the AEC kernels in their per-TICK form (included by aec.hip after aec_wave.hpp, whose FFT / ordered-sum
// helpers they use, and aec_steps.hpp, whose steps of a frame they compose with Wave<F> as the lanes policy).  One launch
// serves every frame a stream has ready in this 10 ms tick: at 48 kHz the filter's 256-sample frames (speexec.c:171-180)
// make that one or two frames (15 per 8 ticks).  What is written here is what only this form has: the FIFOs and the folded
// resampler, the leg lists, the streaming passes and their two-frame machinery, the state parked in LDS, the barriers.
//
// Why per tick: the canceller is HBM-bound, and with both frames of a tick inside one wavefront
//   * the per-stream "small" state (error spectrum, step sizes, power / Eh / Yh, post-filter estimates: ~40 KB moved per
//     frame by the per-frame kernels) is read once and written once per TICK -- it lives in registers in between;
//   * the foreground filter is streamed ONCE for both frames: frame 2's foreground response sum_j X'(j) FG(j) uses the
//     same FG blocks as frame 1's (X'(j) = X(j-1)), so it is accumulated in frame 1's pass -- "speculatively": if frame
//     1 decides to copy the background into the foreground (update_foreground), frame 2's response is instead
//     sum_j X'(j) W1(j), which frame 2's own pass over W yields for free (W1(j) is what it loads before updating it),
//     and the copy itself degenerates into stores of the blocks that pass already holds (no second read of W);
//   * nothing else changes: every sum keeps the library's operand order, so results are bit-identical to the per-frame
//     kernels (tests/test_gpu_aec.py compares both with the oracle).
//   * the residual-echo / noise post-filter (speex_preprocess_run) runs as the TAIL PHASE of the same wavefront: the
//     canceller is HBM-bound and the post-filter VALU-bound, so waves in their post-filter phase leave the memory system
//     to the waves that are streaming -- the overlap two launches on two HIP streams only approximated (a separate
//     post-filter launch kept HBM idle for 17 % of the tick); the canceller's output frames and echo estimates reach the
//     post-filter through LDS instead of HBM.
// Cost: the second frame's far-end spectrum is needed early, and ~50 more live registers: 2 waves per SIMD at F = 256
// instead of 3 (measured on the per-frame kernel: 1.5 % slower per launch at that occupancy; the bytes saved are ~20 %).

// The per-stream small-state block, offsets in floats: written ONCE, as a function of the frame size that the host calls
// too (mi_aec_create sizes the block with it, init_state and mi_aec_get find the arrays with it).
struct SmallLayout {
	int XPREV;   // F   pre-emphasised far end of the last frame (first half of the next FFT input)
	int E;       // 2F  error spectrum of the last frame, bin-interleaved
	int POWER;   // F   (+1 in TAIL)
	int POWER1, EH, YH;
	int LASTY;   // 2F  echo estimate of the last two frames [older | newest] (3F reserved)
	int ECHON, INBUF, OUTBUF, NOISE, OLDPS, ZETA, S_, SMIN, STMP; // post-filter, F each
	int MISC;
	int PROP;    // M <= 64
	int WNORM;   // M
	int TAIL;    // POWER[F], POWER1[F], EH[F], YH[F]
	int OLDPS_B; // 24 Bark bands
	int ZETA_B;
	int FGNORM;  // M: |foreground block|^2, what WNORM becomes when the background is reset to it
	int TOTAL;
};
__host__ __device__ constexpr SmallLayout small_layout(int F) {
	SmallLayout l{};
	l.XPREV = 0, l.E = F, l.POWER = 3 * F, l.POWER1 = 4 * F, l.EH = 5 * F, l.YH = 6 * F, l.LASTY = 7 * F;
	l.ECHON = 10 * F, l.INBUF = 11 * F, l.OUTBUF = 12 * F, l.NOISE = 13 * F, l.OLDPS = 14 * F, l.ZETA = 15 * F;
	l.S_ = 16 * F, l.SMIN = 17 * F, l.STMP = 18 * F, l.MISC = 19 * F;
	l.PROP = l.MISC, l.WNORM = l.MISC + 64, l.TAIL = l.MISC + 128, l.OLDPS_B = l.MISC + 136, l.ZETA_B = l.MISC + 160, l.FGNORM = l.MISC + 192;
	l.TOTAL = 19 * F + 256;
	return l;
}
template <int F>
struct TickLayout { // the same as compile-time constants of a kernel
	static constexpr SmallLayout L = small_layout(F);
	static constexpr int XPREV = L.XPREV, E = L.E, POWER = L.POWER, POWER1 = L.POWER1, EH = L.EH, YH = L.YH, LASTY = L.LASTY;
	static constexpr int ECHON = L.ECHON, INBUF = L.INBUF, OUTBUF = L.OUTBUF, NOISE = L.NOISE, OLDPS = L.OLDPS, ZETA = L.ZETA;
	static constexpr int S_ = L.S_, SMIN = L.SMIN, STMP = L.STMP, PROP = L.PROP, WNORM = L.WNORM, TAIL = L.TAIL;
	static constexpr int OLDPS_B = L.OLDPS_B, ZETA_B = L.ZETA_B, FGNORM = L.FGNORM, TOTAL = L.TOTAL;
};

// LDS of the canceller kernel: FFT work space + tables and the per-bin state parked while the blocks stream (none of the
// post-filter's arrays): 16.3 KB at F = 256.  (Tables read from global memory instead cost 24 % of the kernel at 2 waves
// per SIMD: 6.35 against 5.14 ms per tick of 65 536 legs.)
template <int F>
struct alignas(16) TLds {
	float2 zbuf[F];      // complex FFT work
	float tbuf[2 * F];   // time-domain exchange / inverse-transform staging
	float spec[2 * F];   // bin-interleaved spectrum exchange
	float2 tw[F], super[F];
	uint16_t perm[F];
	float prop[64], wnorm[64];
	// per-bin state that is not needed while the blocks stream: parked here instead of in registers
	float pw[F], eh[F], yh[F], input[F];
	// canceller -> post-filter hand-over: echo estimates [before the tick | after frame 1 | after frame 2], output frames
	float ly[3][F];
	int16_t outf[2][F];
	// the post-filter phase reuses the parked arrays (their contents are in HBM by then)
	__device__ float *vec() { return pw; }        // F
	__device__ float *band() { return eh; }       // 4 * NB_BANDS + 8
};


// ---- buffer addressing: one 128-bit descriptor (SGPRs) per per-stream array + ONE per-lane byte offset + a scalar
// offset, instead of a 64-bit per-lane address (two VGPRs) per array and block: the canceller touches ~25 arrays
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef unsigned int u2v __attribute__((ext_vector_type(2)));
using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t mk_rsrc(const void *p, unsigned bytes) {
	return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float u2f(unsigned v) { return __uint_as_float(v); }
__device__ __forceinline__ unsigned f2u(float v) { return __float_as_uint(v); }
template <typename T>
__device__ __forceinline__ T mk2(float x, float y) {
	T t;
	t.x = x, t.y = y;
	return t;
}
// T = float2, or v2f: a 64-bit register pair per bin, so that whole bins move with one v_mov_b64 / feed v_pk_* directly
template <int K, typename T>
__device__ __forceinline__ void bload_bins(rsrc_t r, unsigned voff, unsigned soff, T (&v)[K]) {
	if constexpr (K == 1) {
		const u2v t = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
		v[0] = mk2<T>(u2f(t.x), u2f(t.y));
	} else {
#pragma unroll
		for (int k = 0; k < K; k += 2) {
			const u4v t = __builtin_amdgcn_raw_buffer_load_b128(r, voff + 8 * k, soff, 0);
			v[k] = mk2<T>(u2f(t.x), u2f(t.y));
			v[k + 1] = mk2<T>(u2f(t.z), u2f(t.w));
		}
	}
}
template <int K, typename T>
__device__ __forceinline__ void bstore_bins(rsrc_t r, unsigned voff, unsigned soff, const T (&v)[K]) {
	if constexpr (K == 1) {
		u2v t = {f2u(v[0].x), f2u(v[0].y)};
		__builtin_amdgcn_raw_buffer_store_b64(t, r, voff, soff, 0);
	} else {
#pragma unroll
		for (int k = 0; k < K; k += 2) {
			u4v t = {f2u(v[k].x), f2u(v[k].y), f2u(v[k + 1].x), f2u(v[k + 1].y)};
			__builtin_amdgcn_raw_buffer_store_b128(t, r, voff + 8 * k, soff, 0);
		}
	}
}
template <int K>
__device__ __forceinline__ void bload_vec(rsrc_t r, unsigned voff, unsigned soff, float (&v)[K]) {
	if constexpr (K == 4) {
		const u4v t = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
		v[0] = u2f(t.x), v[1] = u2f(t.y), v[2] = u2f(t.z), v[3] = u2f(t.w);
	} else if constexpr (K == 2) {
		const u2v t = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
		v[0] = u2f(t.x), v[1] = u2f(t.y);
	} else if constexpr (K == 8) {
		const u4v t = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0), u = __builtin_amdgcn_raw_buffer_load_b128(r, voff + 16, soff, 0);
		v[0] = u2f(t.x), v[1] = u2f(t.y), v[2] = u2f(t.z), v[3] = u2f(t.w);
		v[4] = u2f(u.x), v[5] = u2f(u.y), v[6] = u2f(u.z), v[7] = u2f(u.w);
	} else {
		v[0] = u2f(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
	}
}
template <int K>
__device__ __forceinline__ void bstore_vec(rsrc_t r, unsigned voff, unsigned soff, const float (&v)[K]) {
	if constexpr (K == 4) {
		u4v t = {f2u(v[0]), f2u(v[1]), f2u(v[2]), f2u(v[3])};
		__builtin_amdgcn_raw_buffer_store_b128(t, r, voff, soff, 0);
	} else if constexpr (K == 2) {
		u2v t = {f2u(v[0]), f2u(v[1])};
		__builtin_amdgcn_raw_buffer_store_b64(t, r, voff, soff, 0);
	} else if constexpr (K == 8) {
		u4v t = {f2u(v[0]), f2u(v[1]), f2u(v[2]), f2u(v[3])}, u = {f2u(v[4]), f2u(v[5]), f2u(v[6]), f2u(v[7])};
		__builtin_amdgcn_raw_buffer_store_b128(t, r, voff, soff, 0);
		__builtin_amdgcn_raw_buffer_store_b128(u, r, voff + 16, soff, 0);
	} else {
		__builtin_amdgcn_raw_buffer_store_b32(f2u(v[0]), r, voff, soff, 0);
	}
}

// the post-filter's per-bin state of a leg (aec_steps.hpp: PfState) from / to its small-state block, its tables alongside
// (vb4: this lane's byte offset into a per-bin array; the Bark-band entries are the kernel's: one lane per band or two)
template <typename P>
__device__ __forceinline__ void pf_load(rsrc_t rS, unsigned vb4, const AecTables &t, PfState<P> &pf) {
	using SL = TickLayout<P::F>;
	constexpr int K = P::K, F = P::F;
	const int e0 = P::lane() * K;
	bload_vec<K>(rS, vb4, SL::ECHON * 4, pf.en);
	bload_vec<K>(rS, vb4, SL::INBUF * 4, pf.inb);
	bload_vec<K>(rS, vb4, SL::S_ * 4, pf.S);
	bload_vec<K>(rS, vb4, SL::SMIN * 4, pf.Smin);
	bload_vec<K>(rS, vb4, SL::STMP * 4, pf.Stmp);
	bload_vec<K>(rS, vb4, SL::NOISE * 4, pf.noise);
	bload_vec<K>(rS, vb4, SL::OLDPS * 4, pf.old_ps);
	bload_vec<K>(rS, vb4, SL::ZETA * 4, pf.zeta);
	bload_vec<K>(rS, vb4, SL::OUTBUF * 4, pf.ob);
	load_vec<K>(t.bfl + e0, pf.wl);
	load_vec<K>(t.bfr + e0, pf.wr);
	load_vec<K>(t.hann + e0, pf.h0);
	load_vec<K>(t.hann + F + e0, pf.h1);
	load_vec<K>(t.pwin + e0, pf.w0);
	load_vec<K>(t.pwin + F + e0, pf.w1);
}
template <typename P>
__device__ __forceinline__ void pf_store(rsrc_t rS, unsigned vb4, const PfState<P> &pf) {
	using SL = TickLayout<P::F>;
	constexpr int K = P::K;
	bstore_vec<K>(rS, vb4, SL::ECHON * 4, pf.en);
	bstore_vec<K>(rS, vb4, SL::INBUF * 4, pf.inb);
	bstore_vec<K>(rS, vb4, SL::S_ * 4, pf.S);
	bstore_vec<K>(rS, vb4, SL::SMIN * 4, pf.Smin);
	bstore_vec<K>(rS, vb4, SL::STMP * 4, pf.Stmp);
	bstore_vec<K>(rS, vb4, SL::NOISE * 4, pf.noise);
	bstore_vec<K>(rS, vb4, SL::OLDPS * 4, pf.old_ps);
	bstore_vec<K>(rS, vb4, SL::ZETA * 4, pf.zeta);
	bstore_vec<K>(rS, vb4, SL::OUTBUF * 4, pf.ob);
}

// acc += x w, bin by bin; bin 0 (lane 0's first) holds (DC, Nyquist): two real products there
template <int K, typename TA, typename TX, typename TW>
__device__ __forceinline__ void cmac_bins(TA (&acc)[K], const TX (&x)[K], const TW (&w)[K], int e0) {
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const v2f xv = {x[k].x, x[k].y}, wv = {w[k].x, w[k].y};
		v2f pr = pk_cmul(xv, wv); // (x.x w.x - x.y w.y, x.y w.x + x.x w.y)
		if (k == 0) {
			const v2f dc = xv * wv; // (x.x w.x, x.y w.y)
			if (e0 == 0) pr = dc;
		}
		const v2f a = (v2f){acc[k].x, acc[k].y} + pr;
		acc[k] = mk2<TA>(a.x, a.y);
	}
}

// words of AecArgs::ctl (the list hand-over between consecutive launches of the FIFO entry)
// Eight lists (classes), one per XCD (workgroup b runs on XCD b % 8), in two sets: the set of parity p is served by this
// launch, the set of parity p ^ 1 is filled by it for the next one.  A list has room for cap8 entries: legs that will run
// two frames are entered from the front, the others from the back, the slots in between stay empty (their workgroups leave
// at once).  Every class has its own 128-byte line of control words (the atomics of different classes do not queue up behind
// each other) and a ninth line is shared:
//   PLACED  [parity] 64 bits: entries of this class's list of that parity, front | back << 32 -- counted up by the atomics of
//           the launch that fills the list, read as the list's lengths by the launch that serves it
//   global line: PARITY (which set of lists the next launch serves)
// Nothing inside a launch depends on another workgroup's progress: a launch only READS the parity and its own set's lengths
// and only ADDS to the other set's.  The turn-over -- the served set's counts back to zero, the parity flipped -- is a
// launch of its own right behind (aec_tick_advance_kernel: one wavefront, stream order does the rest).  (Rounds 2-3 had the
// last wave of the tick kernel do it, found through per-class completion counts: a class whose list was empty never
// completed -- batches of fewer than 8 legs froze on their first lists, and the counts grew past the lists -- and workgroups
// on empty slots read words the turn-over might already have rewritten.)
struct TickOrder {
	static constexpr int STRIDE = 32, PLACED = 0, GLOBAL = 8 * STRIDE, PARITY = 0, WORDS = 9 * STRIDE;
	// a class's share of the legs wanders by fewer than 16 around nstreams / 8 (the mixing rule below deals every list out
	// over all eight: sixteen roundings of an eighth of a front or back run), whatever the history
	static constexpr int SLACK = 32;
};

__global__ __launch_bounds__(64) void aec_tick_advance_kernel(int *ctl) {
	const int par = ctl[TickOrder::GLOBAL + TickOrder::PARITY];
	if (threadIdx.x < 8) *reinterpret_cast<unsigned long long *>(ctl + threadIdx.x * TickOrder::STRIDE + TickOrder::PLACED + 2 * par) = 0ull;
	if (threadIdx.x == 0) ctl[TickOrder::GLOBAL + TickOrder::PARITY] = par ^ 1;
}

// MODE: where the frames come from and go to -- decided at compile time, so that each form carries only its own addressing,
// scalars and code (the three forms in one kernel cost the headline's form ~1.5 KB of instruction cache and a dozen scalar
// registers it never used):
//   TICK_ROWS     rows of frames handed in by the caller (mi_aec_process / mi_aec_process_frames);
//   TICK_FIFO     the three device FIFOs, the tick's microphone block from the caller's row (mi_aec_process_fifos);
//   TICK_FIFO_RS  the same with the leg's MSResample folded in: the block is up-sampled by this wave (.._resampled).
enum { TICK_ROWS = 0, TICK_FIFO = 1, TICK_FIFO_RS = 2 };

// (Round 5 built a form that keeps frame 1's updated background W1 -- 48 KB at M = 24 -- in LDS instead of redoing it from W0 in frame
// 2's pass: bit-equal and 2.9x slower, two wavefronts per CU where this form runs eight.  profiles/r05_w_in_lds.txt holds the
// measurement; the form is no longer in the source.)
template <int F, int MODE>
__global__ __launch_bounds__(64, F == 512 ? 1 : (F == 256 ? 2 : (F == 128 ? 3 : 4))) void aec_tick_kernel(AecArgs a) {
	__shared__ TLds<F> L;
	using SL = TickLayout<F>;
	using WP = Wave<F>; // the lanes policy of the shared steps (aec_steps.hpp): the leg is the wavefront
	constexpr int N = 2 * F, K = F / 64;
	// ---- which leg this wavefront serves.  Rows / per-frame entries: leg = block.  FIFO entry: the leg comes out of a list
	// the PREVIOUS tick's launch sorted (TickOrder above) -- legs that will run two frames first, the short ones last, one
	// list per class b % 8: every XCD gets the same mix whatever pattern the legs' phases follow, and the long legs are
	// started first.
	constexpr bool sched = MODE != TICK_ROWS; // (the leg lists belong to the FIFO entries: aec_launch sets them for those)
	int s = a.first + blockIdx.x, par = 0;
	if (sched) {
		const unsigned c = blockIdx.x & 7u, i = blockIdx.x >> 3;
		par = a.ctl[TickOrder::GLOBAL + TickOrder::PARITY];
		const int front = a.ctl[c * TickOrder::STRIDE + TickOrder::PLACED + 2 * par], back = a.ctl[c * TickOrder::STRIDE + TickOrder::PLACED + 2 * par + 1];
		if (i >= (unsigned)front && i < (unsigned)(a.cap8 - back)) return; // an empty slot between the two ends of the list
		s = a.order[(size_t)par * 8 * a.cap8 + c * a.cap8 + i];
	}
	const int lane = threadIdx.x;
	const int e0 = lane * K; // first element (sample / bin) this lane owns
	// ---- where the frames come from and go to: rows (per-frame / per-tick entries) or the three FIFOs
	constexpr bool fifo = MODE != TICK_ROWS, folded = MODE == TICK_FIFO_RS;
	int nf, ref_frames = 0;
	int2 qm = make_int2(0, 0), qr = make_int2(0, 0), qo = make_int2(0, 0); // (head, level) before this tick
	bool mic_new = false, ref_new = false;                                 // the tick's blocks were taken
	if (fifo) {
		qm = a.fmic.pos[s], qr = a.fref.pos[s], qo = a.fout.pos[s];
		// ms_bufferizer_put of the tick's blocks (a block that does not fit is refused and counted, like mi_fifo_push)
		auto append = [&](const FifoView &q, int2 p, const int16_t *row, int len) -> bool {
			if (len <= 0) return false;
			if (p.y + len > q.cap) {
				if (lane == 0) atomicAdd(q.overflow, 1);
				return false;
			}
			int16_t *ring = q.ring + (size_t)s * q.cap;
			unsigned tail = (unsigned)p.x + (unsigned)p.y;
			if (tail >= (unsigned)q.cap) tail -= (unsigned)q.cap;
			if (((tail | (unsigned)len) & 7u) == 0 && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
				// whole 16-byte groups (capacities are multiples of the frame size, so of 8): one per lane, 60 lanes at 480 samples
				for (int i = lane; i < (len >> 3); i += 64) {
					unsigned w = tail + 8u * (unsigned)i;
					if (w >= (unsigned)q.cap) w -= (unsigned)q.cap;
					*reinterpret_cast<uint4 *>(ring + w) = *reinterpret_cast<const uint4 *>(row + 8 * i);
				}
			} else {
				for (int i = lane; i < len; i += 64) {
					unsigned w = tail + (unsigned)i;
					if (w >= (unsigned)q.cap) w -= (unsigned)q.cap;
					ring[w] = row[i];
				}
			}
			return true;
		};
		// ---- MSResample folded in (msresample.c:122-179 for this leg's block): out[m den + p] = sum_j table[p][j] x[m + j] over
		// history ++ input, lane (tile, phase) = 8 consecutive input positions of one polyphase row (resample_tile.hpp: the
		// resampler kernel's own tile FIR, so the samples are bit for bit what mi_resampler_process delivers).  Window, table
		// and output staging live in the transform work space, which nothing uses yet.
		const int16_t *mic_row = folded ? nullptr : a.mic_tick + (size_t)s * a.mic_tick_stride;
		// a.run (the *_masked forms): 0 = this leg has no microphone block in this launch (nothing is queued, the resampler's
		// state stays; whatever frames its queue still holds run all the same)
		const int mlen = (a.run && !a.run[s]) ? 0 : a.tick_len;
		if (folded && mlen) {
			constexpr int RS_FILT = 48, RS_R = 8, RS_HIST = RS_FILT - 1;
			const int den = a.rs_den, in_len = a.rs_in_len;
			float *x = reinterpret_cast<float *>(L.zbuf);                    // [xn] history ++ input ++ zero slack
			const int xn = ((RS_HIST + in_len + RS_R + 1) + 3) & ~3;
			int16_t *obuf = reinterpret_cast<int16_t *>(x + xn);             // [in_len * den]
			float4 *tab4 = reinterpret_cast<float4 *>(obuf + ((in_len * den + 7) & ~7));
			const int hq = a.rs_hist_stride >> 2, nq = hq + (in_len >> 2);
			int16_t *hist = a.rs_hist + (size_t)s * a.rs_hist_stride;
			short4 v0 = make_short4(0, 0, 0, 0);
			if (lane < nq)
				v0 = *reinterpret_cast<const short4 *>(lane < hq ? hist + 4 * lane : a.rs_in + (size_t)s * a.rs_in_stride + 4 * (lane - hq));
			for (int i = lane; i < den * RS_FILT / 4; i += 64) tab4[i] = reinterpret_cast<const float4 *>(a.rs_table)[i];
			for (int i = RS_HIST + in_len + lane; i < xn; i += 64) x[i] = 0.f;
			if (lane < nq) {
				const int b = 4 * lane - (lane < hq ? 0 : 4 * hq - RS_HIST);
				if (lane < hq) {
					if (b + 0 < RS_HIST) x[b + 0] = (float)v0.x;
					if (b + 1 < RS_HIST) x[b + 1] = (float)v0.y;
					if (b + 2 < RS_HIST) x[b + 2] = (float)v0.z;
					if (b + 3 < RS_HIST) x[b + 3] = (float)v0.w;
				} else {
					x[b + 0] = (float)v0.x, x[b + 1] = (float)v0.y, x[b + 2] = (float)v0.z, x[b + 3] = (float)v0.w;
				}
			}
			wave_sync();
			const int nlanes = den * ((in_len + RS_R - 1) / RS_R);
			const bool on = lane < nlanes;
			const int tile = on ? lane / den : 0, ph = on ? lane - tile * den : 0, m0 = tile * RS_R;
			f2 acc2[RS_R / 2];
#pragma unroll
			for (int q = 0; q < RS_R / 2; ++q) acc2[q] = (f2){0.f, 0.f};
			fir_tile_rolled<RS_FILT, RS_R>(x + m0, reinterpret_cast<const float *>(tab4 + ph * (RS_FILT / 4)), acc2);
			if (on) {
#pragma unroll
				for (int r = 0; r < RS_R; ++r)
					if (m0 + r < in_len) obuf[(m0 + r) * den + ph] = rs_word2int((r & 1) ? acc2[r / 2].y : acc2[r / 2].x);
			}
			if (lane < hq) { // new history = the last 47 samples of (history ++ input); the pad slot takes the zero slack
				const float *hx = x + in_len + 4 * lane;
				short4 h;
				h.x = (int16_t)hx[0], h.y = (int16_t)hx[1], h.z = (int16_t)hx[2], h.w = (int16_t)hx[3];
				*reinterpret_cast<short4 *>(hist + 4 * lane) = h;
			}
			wave_sync();
			mic_row = obuf;
		}
		int rlen = a.ref_len ? a.ref_len[s] : a.tick_len; // the far end's block may be missing or short this tick
		rlen = rlen < 0 ? 0 : (rlen > a.tick_len ? a.tick_len : rlen);
		mic_new = append(a.fmic, qm, mic_row, mlen);
		ref_new = append(a.fref, qr, a.ref_tick + (size_t)s * a.ref_tick_stride, rlen);
		if (!ref_new) rlen = 0;
		nf = (qm.y + (mic_new ? a.tick_len : 0)) / F;
		if (nf > a.max_frames) nf = a.max_frames;
		ref_frames = (qr.y + rlen) / F; // frames the far end can supply; the rest is silence
		if (ref_frames > nf) ref_frames = nf;
		if (qo.y + nf * F > a.fout.cap) { // no room for the results: nothing runs (counted), the inputs stay queued
			if (lane == 0) atomicAdd(a.fout.overflow, 1);
			nf = 0;
		}
		if (sched && lane == 0) {
			// This leg's place in the NEXT tick's lists: every leg is handed a block every tick, so the frames it will then have
			// follow from what it keeps now (a wrong guess -- a refused block -- only costs placement).  WHICH list: class
			// (c + i) % 8 for the leg at position i of class c -- a class's legs are dealt out over all eight classes every
			// tick, so legs that share a phase cannot stay together on one XCD however the slots were arranged (phase =
			// slot % 8 kept every tick's light legs on ONE XCD with per-class lists that never mixed: +4 % on the launch), and
			// every class keeps nstreams / 8 legs give or take fewer than 16.  Front of the list for two frames, back for
			// fewer: one 64-bit atomic on the destination class's line.
			const int keep = qm.y + (mic_new ? a.tick_len : 0) - nf * F;
			int next = (keep + a.tick_len) / F;
			if (next > a.max_frames) next = a.max_frames;
			const unsigned c = blockIdx.x & 7u, i = blockIdx.x >> 3, d = (c + i) & 7u;
			int *dst = a.order + (size_t)(par ^ 1) * 8 * a.cap8 + d * a.cap8;
			unsigned long long *placed = reinterpret_cast<unsigned long long *>(a.ctl + d * TickOrder::STRIDE + TickOrder::PLACED + 2 * (par ^ 1));
			const unsigned long long old = atomicAdd(placed, next >= 2 ? 1ull : (1ull << 32));
			const unsigned at = next >= 2 ? (unsigned)old : (unsigned)a.cap8 - 1u - (unsigned)(old >> 32);
			if (at < (unsigned)a.cap8) dst[at] = s; // (it always is: the bound at TickOrder::SLACK)
		}
		if (lane == 0) {
			if (a.count_out) a.count_out[s] = (uint8_t)nf;
			const int rf = nf ? ref_frames : 0;
			a.fmic.pos[s] = make_int2((qm.x + nf * F) % a.fmic.cap, qm.y + (mic_new ? a.tick_len : 0) - nf * F);
			a.fref.pos[s] = make_int2((qr.x + rf * F) % a.fref.cap, qr.y + rlen - rf * F);
			a.fout.pos[s] = make_int2(qo.x, qo.y + nf * F);
		}
	} else {
		nf = a.count ? (int)a.count[s] : ((a.run && !a.run[s]) ? 0 : 1);
		if (nf > a.max_frames) nf = a.max_frames;
	}
	if (nf <= 0) return;
	// sample e (< F) of frame f.  FIFO: position f * F + e of the queue = the ring while it is inside what was queued
	// before this tick, the tick's own block after that (read from the caller's row: nothing this wave wrote is read back)
	// Position p of a queue: the ring while p lies inside what was queued before this tick, the tick's own block after
	// that.  (No integer division: one add and two conditional subtractions, p < 2 F <= capacity.)
	auto ring_at = [&](const FifoView &q, int head, int p) -> int {
		unsigned at = (unsigned)head + (unsigned)p;
		if (at >= (unsigned)q.cap) at -= (unsigned)q.cap;
		if (at >= (unsigned)q.cap) at -= (unsigned)q.cap;
		return q.ring[(size_t)s * q.cap + at];
	};
	auto mic_at = [&](int f, int e) -> int {
		if (!fifo) return a.mic[(size_t)s * a.stride + f * F + e];
		const int p = f * F + e;
		// (up-sampled in this launch: the block exists nowhere but in the ring it was queued in)
		if (folded || p < qm.y) return ring_at(a.fmic, qm.x, p);
		return a.mic_tick[(size_t)s * a.mic_tick_stride + (p - qm.y)];
	};
	auto ref_at = [&](int f, int e) -> int {
		if (!fifo) return a.ref[(size_t)s * a.stride + f * F + e];
		if (f >= ref_frames) return 0; // speexec.c:261-272: a frame of zeros when the far end runs short
		const int p = f * F + e;
		if (p < qr.y) return ring_at(a.fref, qr.x, p);
		return a.ref_tick[(size_t)s * a.ref_tick_stride + (p - qr.y)];
	};
	auto out_ptr = [&](int f) -> int16_t * { // where this lane's K cleaned samples of frame f go
		if (!fifo) return a.out + (size_t)s * a.stride + f * F + e0;
		unsigned tail = (unsigned)(qo.x + qo.y) + (unsigned)(f * F); // the output FIFO is popped in ticks: its tail is what is F-aligned
		while (tail >= (unsigned)a.fout.cap) tail -= (unsigned)a.fout.cap;
		return a.fout.ring + (size_t)s * a.fout.cap + tail + e0; // K samples never wrap
	};
	const int M = a.M;
	float *sm = a.small + (size_t)s * a.small_stride;
	const rsrc_t rS = mk_rsrc(sm, (unsigned)a.small_stride * 4u);
	const rsrc_t rX = mk_rsrc(a.X + (size_t)s * (M + 1) * N, (unsigned)((M + 1) * N) * 4u);
	// The two filters of a stream lie back to back in two equal halves: ONE descriptor, a half is chosen by a scalar offset.
	// Which half holds the background and which the foreground is per-stream state (sc.wsel): it is how the library's two
	// filter copies cost nothing here (see pendingFG below).
	const rsrc_t rWF = mk_rsrc(a.WF + (size_t)s * 2 * M * N, (unsigned)(2 * M * N) * 4u);
	const unsigned HALF = (unsigned)(M * N) * 4u;
	const unsigned vb4 = (unsigned)e0 * 4u, vb8 = (unsigned)e0 * 8u; // this lane's byte offset into a float / a bin array
	AecScalars sc = a.scal[s];
	unsigned wo = sc.wsel ? HALF : 0u, fo = HALF - wo; // byte offset of the background / foreground half

	// ---- tables, per-block step / norm, the per-bin state that stays in registers for the whole tick
#pragma unroll
	for (int k = 0; k < K; ++k) {
		L.tw[e0 + k] = a.t.tw[e0 + k];
		L.super[e0 + k] = a.t.super[e0 + k];
		L.perm[e0 + k] = a.t.perm[e0 + k];
	}
	if (lane < M) {
		L.prop[lane] = sm[SL::PROP + lane];
		L.wnorm[lane] = sm[SL::WNORM + lane];
	}
	float2 Eprev[K];
	float p1[K];
	bload_bins<K>(rS, vb8, SL::E * 4, Eprev);
	bload_vec<K>(rS, vb4, SL::POWER1 * 4, p1);
	{ // each lane parks and later fetches its own K elements: no cross-lane traffic, program order suffices
		float t[K];
		bload_vec<K>(rS, vb4, SL::POWER * 4, t);
		store_vec<K>(L.pw + e0, t);
		bload_vec<K>(rS, vb4, SL::EH * 4, t);
		store_vec<K>(L.eh + e0, t);
		bload_vec<K>(rS, vb4, SL::YH * 4, t);
		store_vec<K>(L.yh + e0, t);
		bload_vec<K>(rS, vb4, (SL::LASTY + F) * 4, t);
		store_vec<K>(L.ly[0] + e0, t);
	}
	float pw_F = sm[SL::TAIL + 0], p1_F = sm[SL::TAIL + 1], eh_F = sm[SL::TAIL + 2], yh_F = sm[SL::TAIL + 3];
	bool prop_dirty = false;

	// far end of frame f: pre-emphasis, energy, spectrum of [previous frame | this frame]
	auto prep_far = [&](int f, const float (&xp)[K], float (&xn)[K], float2 (&X0)[K], float &Sxx) {
		float far[K];
#pragma unroll
		for (int k = 0; k < K; ++k) far[k] = (float)ref_at(f, e0 + k);
		far_end<WP>(L, a.t, far, xp, sc.memX, xn, X0, Sxx);
	};

	float2 X0[K], X0B[K]; // far-end spectrum of the frame at hand / of the frame behind it
	float Sxx = 0, SxxB = 0;
	{
		float xp[K], xa[K], xb[K];
		bload_vec<K>(rS, vb4, SL::XPREV * 4, xp);
		prep_far(0, xp, xa, X0, Sxx);
		if (nf > 1) {
			prep_far(1, xa, xb, X0B, SxxB);
			bstore_vec<K>(rS, vb4, SL::XPREV * 4, xb);
		} else {
			bstore_vec<K>(rS, vb4, SL::XPREV * 4, xa);
#pragma unroll
			for (int k = 0; k < K; ++k) X0B[k] = make_float2(0, 0);
		}
	}

	float2 spec2[K]; // frame 2's foreground response, accumulated over frame 1's pass
#pragma unroll
	for (int k = 0; k < K; ++k) spec2[k] = make_float2(0, 0);
	// The library's two filter copies are never passes of their own, and neither moves a byte that was not moving anyway:
	//  * foreground := background (update_foreground).  The NEXT pass over the filter -- this tick's second frame's, or the
	//    first frame's of the next tick (the request then waits in the scalars) -- reads the background's half, which IS the
	//    foreground from now on, and writes the updated background into the OTHER half: the halves swap roles (sc.wsel).
	//    That pass reads one filter instead of two; nothing is copied.  (A pass of its own cost 98 KB per request and made the
	//    ticks in which many legs ask at once -- every ~12th with SURVEY 8(d)'s scene -- 10 % longer than the others.)
	//  * background := foreground (reset_background).  The next pass reads the foreground's half as the background too and
	//    writes the updated blocks to the background's half as it always does.  The block norms the proportional step needs
	//    in between are the foreground's, kept alongside (fgnorm: taken from wnorm whenever the foreground is set).
	// Until that pass one half in HBM is stale; fg_pending / bg_pending say so (mi_aec_get / export_state resolve it).
	bool pendingFG = sc.fg_pending != 0, pendingBG = sc.bg_pending != 0;
	float fgnorm = lane < M ? sm[SL::FGNORM + lane] : 0.f; // lane j: |foreground block j|^2 (one register for the whole tick)
	const bool postfilter = (a.flags & 1) != 0; // MI_AEC_POSTFILTER
	float leakf[2] = {sc.leak_estimate, sc.leak_estimate}; // leak estimate after each frame (post-filter input)
	bool resetf[2] = {false, false};                       // the frame reset the canceller: its echo estimate is zero
	// Frame 1 of a two-frame tick does not write its updated background: frame 2's pass reads W0(j) again and redoes frame
	// 1's gradient step on it (same operands, same operations: the same bits) before its own -- a block read and a few
	// multiply-adds instead of a block written and read (a written byte costs the memory system 1.75 read ones).  What
	// frame 1 still writes: the blocks it constrained (0 and jc) and the last one, whose far-end block leaves the ring.
	bool lazy1 = false;
	int jc1 = -1;
	float2 E1s[K];
	float p1s[K], p1s_F = 0.f;
#pragma unroll
	for (int k = 0; k < K; ++k) E1s[k] = make_float2(0, 0), p1s[k] = 0.f;

	for (int f = 0; f < nf; ++f) {
		// Frame 2's first blocks are asked for NOW (frame 1's pass wrote them long ago): the notch and the proportional step
		// below -- 5 us of serial chains that touch no HBM -- cover their round trip.  (Not frame 1's: with the far-end
		// spectra of both frames and the speculation accumulators live, the 24 registers spill; measured, no gain.)
		const int head = (sc.xhead + M) % (M + 1);
		auto xoff = [&](int j) { return (unsigned)((head + j) % (M + 1)) * (unsigned)(F * 8); };
		v2f pre0[K], pre1[K], pre2[K], pre3[K]; // frame 2's pass takes them over as its first far-end and background blocks
		if (f == 0) {
#pragma unroll
			for (int k = 0; k < K; ++k) pre0[k] = pre1[k] = pre2[k] = pre3[k] = (v2f){0.f, 0.f};
		} else {
			bload_bins<K>(rX, vb8, xoff(1), pre0);
			bload_bins<K>(rX, vb8, xoff(2 < M ? 2 : M), pre1);
			const unsigned wpre = pendingBG ? fo : wo; // frame 1 reset the background: its blocks are the foreground's
			bload_bins<K>(rWF, vb8, wpre, pre2);
			bload_bins<K>(rWF, vb8, wpre + (unsigned)(1 < M ? 1 : 0) * (unsigned)(F * 8), pre3);
		}
		// ---- near end: saturation flag, DC notch (serial IIR), pre-emphasis
		int any_sat;
		{
			float input[K], fin[K];
#pragma unroll
			for (int k = 0; k < K; ++k) fin[k] = (float)mic_at(f, e0 + k);
			any_sat = near_end<WP>(fin, a.notch_radius, sc, input);
			store_vec<K>(L.input + e0, input);
		}
		sc.cancel_count++;
		sc.frames++;

		// ---- newest far-end spectrum into the ring; its power spectrum is all the rest of the frame needs of it
		sc.xhead = head;
		bstore_bins<K>(rX, vb8, (unsigned)head * (F * 8), X0);
		float Xf[K], Xf_F;
		bin_power<WP>(X0, Xf, Xf_F);

		// ---- proportional step
		if (sc.adapted) {
			// mdf_adjust_prop, one block per lane: prop = sqrt(1 + |W_j|^2); the maximum is exact in any order; the sum
			// 1 + prop_0 + prop_1 + .. is the library's serial loop, run as a systolic chain over the first M lanes
			WSYNC();
			float p = sqrt_via_double(1.0f + (lane < M ? L.wnorm[lane] : 0.f));
			const float max_sum = wave_tree(lane < M ? p : 1.f, [](float x, float y) { return y > x ? y : x; });
			p = p + .1f * max_sum;
			float run = 1.f;
			for (int i = 0; i < M; ++i) run = dpp_shr1(1.f, run) + p;
			const float prop_sum = rdlane(run, M - 1);
			WSYNC();
			if (lane < M) L.prop[lane] = (.99f * p) / prop_sum;
			prop_dirty = true;
		}
		WSYNC();
		const bool do_grad = (sc.saturated == 0);
		if (!do_grad) sc.saturated--;

		// ---- one streaming pass over the blocks (next block's loads in flight).  Block 0 and the round-robin block jc get
		// the AUMDF constraint (IFFT, zero the second half, FFT) where the pass meets them: the blocks are independent of each
		// other, only the sums over j have an order, and it stays ascending.
		const int jc = (M > 1) ? (sc.cancel_count % (M - 1)) + 1 : -1;
		float2 yfg[K], ybgs[K];
#pragma unroll
		for (int k = 0; k < K; ++k) yfg[k] = ybgs[k] = make_float2(0, 0);
		auto norm_of = [&](const auto (&w)[K], int j) {
			float nn = 0;
#pragma unroll
			for (int k = 0; k < K; ++k) nn += w[k].x * w[k].x + w[k].y * w[k].y;
			nn = wave_tree(nn, [](float x, float y) { return x + y; });
			if (lane == 0) L.wnorm[j] = nn; // feeds the NEXT frame's proportional step
		};
		if (f == 0) {
			// frame 1: X, foreground and background; with a second frame behind it also that frame's foreground response
			const bool spec = nf > 1;
			v2f xj[K], xn[K], fg[K], wl[K], xm1[K]; // xm1: the block before xj = frame 2's block at this position (register pairs)
#pragma unroll
			for (int k = 0; k < K; ++k) xj[k] = (v2f){X0[k].x, X0[k].y}, xm1[k] = (v2f){X0B[k].x, X0B[k].y};
			// a filter copy the previous tick's last frame asked for (see pendingFG above): which half is read as what, and where
			// the updated background goes
			const bool carryFG = pendingFG, carryBG = pendingBG;
			pendingFG = pendingBG = false;
			const unsigned fsrc = carryFG ? wo : fo, wsrc = carryBG ? fo : wo, wdst = carryFG ? fo : wo;
			const bool lazy = spec && do_grad && !carryBG && !carryFG && M <= 32; // (the block weights wait in L.prop[32..])
			bload_bins<K>(rX, vb8, xoff(1), xn);
			bload_bins<K>(rWF, vb8, fsrc, fg);
			bload_bins<K>(rWF, vb8, wsrc, wl);
			for (int j = 0; j < M; ++j) {
				v2f xn2[K], fg2[K], wl2[K];
				{ // (behind the last block: its own again, dropped)
					const int jn = j + 1 < M ? j + 1 : j;
					bload_bins<K>(rX, vb8, xoff(jn + 1), xn2);
					bload_bins<K>(rWF, vb8, fsrc + (unsigned)jn * (F * 8), fg2);
					bload_bins<K>(rWF, vb8, wsrc + (unsigned)jn * (F * 8), wl2);
				}
				const bool aumdf = (j == 0 || j == jc);
				if (do_grad) gradient<WP>(wl, xn, L.prop[j], Eprev, p1, p1_F);
				if (aumdf) constrain<WP>(L, a.t, wl);
				if (lazy ? (aumdf || j == M - 1) : (do_grad || aumdf || carryBG || carryFG)) bstore_bins<K>(rWF, vb8, wdst + (unsigned)j * (F * 8), wl);
				cmac_bins<K>(yfg, xj, fg, e0);
				cmac_bins<K>(ybgs, xj, wl, e0);
				if (spec) cmac_bins<K>(spec2, xm1, fg, e0);
				norm_of(wl, j);
#pragma unroll
				for (int k = 0; k < K; ++k) xm1[k] = xj[k], xj[k] = xn[k], xn[k] = xn2[k], fg[k] = fg2[k], wl[k] = wl2[k];
			}
			if (carryFG) { // the halves have swapped roles
				const unsigned t = wo;
				wo = fo, fo = t;
				sc.wsel ^= 1;
			}
			if (lazy) { // what frame 2's pass needs to redo this frame's step: the error spectrum, the steps, the block weights
				lazy1 = true;
				jc1 = jc;
				p1s_F = p1_F;
#pragma unroll
				for (int k = 0; k < K; ++k) E1s[k] = Eprev[k], p1s[k] = p1[k];
				WSYNC();
				if (lane < M) L.prop[32 + lane] = L.prop[lane];
				WSYNC();
			}
		} else {
			// frame 2: X and the background only.  alt = sum_j X(j) W1(j) with W1 the background as frame 1 left it: the
			// foreground response when frame 1 updated the foreground (its half then stays behind as the foreground and the
			// updated blocks go to the other half).
			// Two blocks per iteration: every iteration ends in ONE wait for everything in flight (loads and stores share a
			// counter and may complete out of order with each other, so with a store in flight the only wait is vmcnt(0)), a
			// full memory round trip that the iteration's arithmetic does not cover.  This pass has no foreground blocks in
			// flight, so it has the registers to take the blocks in pairs: half as many round trips.
			v2f xj[K], xn3[K]; // register pairs: a bin moves with one instruction
			v2f(&xn)[K] = pre0, (&xn2)[K] = pre1, (&wl)[K] = pre2, (&wl2)[K] = pre3;
#pragma unroll
			for (int k = 0; k < K; ++k) xj[k] = (v2f){X0[k].x, X0[k].y};
			auto xclamp = [&](int i) { return xoff(i < M ? i : M); };
			auto wclamp = [&](int i) { return (unsigned)(i < M ? i : M - 1) * (unsigned)(F * 8); };
			const bool carryBG = pendingBG, carryFG = pendingFG; // frame 1 reset the background / updated the foreground
			pendingBG = false;
			if (carryFG) { // the speculated foreground response is void: its registers take alt
#pragma unroll
				for (int k = 0; k < K; ++k) spec2[k] = make_float2(0, 0);
			}
			const unsigned wsrc = carryBG ? fo : wo, wdst = carryFG ? fo : wo;
			// a block's redo needs the far-end block two places on: four landed far-end blocks per pair, the next two in flight.
			// The fourth of the first pair is waited for HERE, once, so that no iteration waits in its middle.
			bload_bins<K>(rX, vb8, xclamp(3), xn3);
			__builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)
			const bool redo = lazy1 && !carryBG; // frame 1 left its updated blocks unwritten (all but 0, jc1 and the last)
			const bool keepW1 = redo && carryFG;  // ... and then made them the foreground: they must exist in that half
			auto block = [&](int j, v2f (&w)[K], const v2f (&xa)[K], const v2f (&xb)[K], const v2f (&xc)[K]) { // X(j), X(j+1), X(j+2)
				if (redo && j != 0 && j != jc1 && j != M - 1) {
					gradient<WP>(w, xc, L.prop[32 + j], E1s, p1s, p1s_F);
					if (keepW1) bstore_bins<K>(rWF, vb8, wo + (unsigned)j * (F * 8), w);
				}
				if (carryFG) cmac_bins<K>(spec2, xa, w, e0);
				const bool aumdf = (j == 0 || j == jc);
				if (do_grad) gradient<WP>(w, xb, L.prop[j], Eprev, p1, p1_F);
				if (aumdf) constrain<WP>(L, a.t, w);
				if (do_grad || aumdf || carryBG || carryFG || lazy1) bstore_bins<K>(rWF, vb8, wdst + (unsigned)j * (F * 8), w);
				cmac_bins<K>(ybgs, xa, w, e0);
				norm_of(w, j);
			};
			if constexpr (F == 512) {
				// one block per iteration (64 bytes per lane and block, twice the 256-sample form's): a second copy of `block` would
				// take the form past the instruction cache
				for (int j = 0; j < M; ++j) {
					v2f xa[K], wa[K]; // the next block's: X(j+4), W(j+2) (clamped at the end: dropped)
					bload_bins<K>(rX, vb8, xclamp(j + 4), xa);
					bload_bins<K>(rWF, vb8, wsrc + wclamp(j + 2), wa);
					block(j, wl, xj, xn, xn2);
#pragma unroll
					for (int k = 0; k < K; ++k) xj[k] = xn[k], xn[k] = xn2[k], xn2[k] = xn3[k], xn3[k] = xa[k], wl[k] = wl2[k], wl2[k] = wa[k];
				}
			} else {
			for (int j = 0; j < M; j += 2) { // an odd block count: the last round serves one block (no third copy of `block` in the code)
				v2f xa[K], xb[K], wa[K], wb[K]; // the next pair: X(j+3), X(j+4), W(j+2), W(j+3) (clamped at the end: dropped)
				bload_bins<K>(rX, vb8, xclamp(j + 4), xa);
				bload_bins<K>(rX, vb8, xclamp(j + 5), xb);
				bload_bins<K>(rWF, vb8, wsrc + wclamp(j + 2), wa);
				bload_bins<K>(rWF, vb8, wsrc + wclamp(j + 3), wb);
				block(j, wl, xj, xn, xn2);
				if (j + 1 < M) block(j + 1, wl2, xn, xn2, xn3);
#pragma unroll
				for (int k = 0; k < K; ++k) xj[k] = xn2[k], xn[k] = xn3[k], xn2[k] = xa[k], xn3[k] = xb[k], wl[k] = wa[k], wl2[k] = wb[k];
			}
			}
#pragma unroll
			for (int k = 0; k < K; ++k) yfg[k] = spec2[k];
			pendingFG = false;
			lazy1 = false;
			if (carryFG) {
				const unsigned t = wo;
				wo = fo, fo = t;
				sc.wsel ^= 1;
			}
		}

		// ---- time-domain responses
		float efg[K], ybg[K], e1[K], e2[K], dresp[K], input[K];
		w_rfft_inverse<F>(L, a.t, yfg);
		load_vec<K>(w_time(L) + F + e0, efg);
		load_vec<K>(L.input + e0, input);
#pragma unroll
		for (int k = 0; k < K; ++k) e1[k] = input[k] - efg[k];
		w_rfft_inverse<F>(L, a.t, ybgs);
		load_vec<K>(w_time(L) + F + e0, ybg);
#pragma unroll
		for (int k = 0; k < K; ++k) {
			e2[k] = input[k] - ybg[k];
			dresp[k] = efg[k] - ybg[k];
		}
		float Sff, Dbf, See;
		WSeq<K>::inner_prod3(e1, e1, dresp, dresp, e2, e2, Sff, Dbf, See);
		Dbf = 10 + Dbf;

		// ---- two-path control
		if (two_path_update(sc, Sff, See, Dbf)) {
			pendingFG = true; // the next pass over the filter (this tick's or the next one's) carries the copy out
			WSYNC();
			if (lane < M) fgnorm = L.wnorm[lane];
			blend_foreground<WP>(a.t.hann, efg, ybg);
		} else if (two_path_reset(sc, Sff, See, Dbf)) {
			pendingBG = true; // the next pass reads the foreground's blocks as the background's
			WSYNC();
			if (lane < M) L.wnorm[lane] = fgnorm;
			take_foreground<WP>(efg, input, Sff, ybg, e2, See);
		}

		int out_i[K];
		float Sey, Syy, Sdd;
		output_and_correlations<WP>(sc, input, efg, e2, ybg, any_sat, out_i, Sey, Syy, Sdd);

		float2 Ecur[K], Ycur[K];
		error_spectra<WP>(L, a.t, e2, ybg, Ecur, Ycur);
		float Rf[K], Yf[K], Rf_F, Yf_F;
		bin_power<WP>(Ecur, Rf, Rf_F);
		bin_power<WP>(Ycur, Yf, Yf_F);
#pragma unroll
		for (int k = 0; k < K; ++k) Eprev[k] = Ecur[k];

		sanity_checks<WP>(sc, Sff, See, Sxx, Syy, Sdd, out_i);
		int16_t *op = out_ptr(f);
		auto emit = [&](const int (&o)[K]) { // to the post-filter phase through LDS, else straight out
#pragma unroll
			for (int k = 0; k < K; ++k) {
				if (postfilter) L.outf[f][e0 + k] = (int16_t)o[k];
				else op[k] = (int16_t)o[k];
			}
		};
		if (sc.screwed_up >= 50) { // speex_echo_state_reset
			float z[K];
			float2 z2[K];
#pragma unroll
			for (int k = 0; k < K; ++k) z[k] = 0.f, z2[k] = make_float2(0, 0);
			for (int j = 0; j < M; ++j) {
				bstore_bins<K>(rWF, vb8, (unsigned)j * (F * 8), z2);
				bstore_bins<K>(rWF, vb8, HALF + (unsigned)j * (F * 8), z2);
			}
			for (int j = 0; j <= M; ++j) bstore_bins<K>(rX, vb8, (unsigned)j * (F * 8), z2);
#pragma unroll
			for (int k = 0; k < K; ++k) {
				p1[k] = 1.0f;
				Eprev[k] = make_float2(0, 0);
				spec2[k] = make_float2(0, 0);
			}
			lazy1 = false; // both halves are zero in HBM: nothing of frame 1's step is left to redo
			store_vec<K>(L.pw + e0, z);
			store_vec<K>(L.eh + e0, z);
			store_vec<K>(L.yh + e0, z);
			store_vec<K>(L.ly[f + 1] + e0, z);
			pw_F = eh_F = yh_F = 0.f;
			p1_F = 1.0f;
			WSYNC();
			if (lane < M) L.wnorm[lane] = 0;
			fgnorm = 0.f;
			bstore_vec<K>(rS, vb4, SL::LASTY * 4, z);
			bstore_vec<K>(rS, vb4, (SL::LASTY + F) * 4, z);
			bstore_vec<K>(rS, vb4, (SL::LASTY + (2) * F) * 4, z);
			reset_scalars(sc);
			pendingFG = pendingBG = false;
			if (f) resetf[1] = true, leakf[1] = sc.leak_estimate;
			else resetf[0] = true, leakf[0] = sc.leak_estimate;
			emit(out_i);
			if (f + 1 < nf) { // the next frame starts from the reset far-end state
				float xn[K];
				prep_far(f + 1, z, xn, X0, Sxx);
				bstore_vec<K>(rS, vb4, SL::XPREV * 4, xn);
			} else {
				bstore_vec<K>(rS, vb4, SL::XPREV * 4, z);
			}
			continue;
		}
		if (See < (float)(N * 100)) See = (float)(N * 100);
		float Sxx2 = Sxx + Sxx; // sic: the library accumulates the far-end energy a second time here

		// ---- far-end power, leak estimate
		float pw[K];
		load_vec<K>(L.pw + e0, pw);
		far_power<WP>(a, Xf, Xf_F, pw, pw_F);
		store_vec<K>(L.pw + e0, pw);
		float Ehd[K], Yhd[K], Ehd_F, Yhd_F;
		{
			float eh[K], yh[K];
			load_vec<K>(L.eh + e0, eh);
			load_vec<K>(L.yh + e0, yh);
			spectral_averages<WP>(a, Rf, Rf_F, Yf, Yf_F, eh, eh_F, yh, yh_F, Ehd, Ehd_F, Yhd, Yhd_F);
			store_vec<K>(L.eh + e0, eh);
			store_vec<K>(L.yh + e0, yh);
		}
		int m_here = M; // (converted by the step, HERE: hoisted to the kernel's entry the float lived -- spilled to scratch -- through the whole tick)
		asm volatile("" : "+s"(m_here));
		leak_and_steps<WP>(a, sc, m_here, Sxx2, See, Syy, Sey, Ehd, Ehd_F, Yhd, Yhd_F, Rf, Rf_F, Yf, Yf_F, pw, pw_F, p1, p1_F);

		// ---- echo estimate of this frame for the residual-echo stage (ring of three frames)
		{
			float ln[K], lprev[K];
			load_vec<K>(L.ly[f] + e0, lprev);
#pragma unroll
			for (int k = 0; k < K; ++k) ln[k] = sc.adapted ? (float)(mic_at(f, e0 + k) - out_i[k]) : lprev[k];
			store_vec<K>(L.ly[f + 1] + e0, ln);
		}
		if (f) leakf[1] = sc.leak_estimate;
		else leakf[0] = sc.leak_estimate;
		emit(out_i);
#pragma unroll
		for (int k = 0; k < K; ++k) X0[k] = X0B[k]; // the frame behind this one, if any
		Sxx = SxxB;
	}

	// ---- the tick's state back to HBM, once
	bstore_bins<K>(rS, vb8, SL::E * 4, Eprev);
	bstore_vec<K>(rS, vb4, SL::POWER1 * 4, p1);
	{
		float t[K];
		load_vec<K>(L.pw + e0, t);
		bstore_vec<K>(rS, vb4, SL::POWER * 4, t);
		load_vec<K>(L.eh + e0, t);
		bstore_vec<K>(rS, vb4, SL::EH * 4, t);
		load_vec<K>(L.yh + e0, t);
		bstore_vec<K>(rS, vb4, SL::YH * 4, t);
	}
	WSYNC();
	if (lane < M) {
		sm[SL::WNORM + lane] = L.wnorm[lane];
		sm[SL::FGNORM + lane] = fgnorm;
		if (prop_dirty) sm[SL::PROP + lane] = L.prop[lane];
	}
	{ // echo estimate of the last frame's pair [older | newest]
		float lo[K], ln[K];
		load_vec<K>(L.ly[nf - 1] + e0, lo);
		load_vec<K>(L.ly[nf] + e0, ln);
		if (nf > 1 ? resetf[1] : resetf[0]) {
#pragma unroll
			for (int k = 0; k < K; ++k) lo[k] = 0.f;
		}
		bstore_vec<K>(rS, vb4, SL::LASTY * 4, lo);
		bstore_vec<K>(rS, vb4, (SL::LASTY + F) * 4, ln);
	}
	if (lane == 0) {
		sm[SL::TAIL + 0] = pw_F;
		sm[SL::TAIL + 1] = p1_F;
		sm[SL::TAIL + 2] = eh_F;
		sm[SL::TAIL + 3] = yh_F;
	}
	if (!postfilter) {
		sc.fg_pending = pendingFG ? 1 : 0, sc.bg_pending = pendingBG ? 1 : 0;
		if (lane == 0) a.scal[s] = sc;
		return;
	}
	WSYNC(); // the parked arrays are re-used from here on

	// ---- the tail phase: the residual-echo / noise post-filter of the tick's frames, per-bin state in registers, band b in lane b
	PfState<WP> pf;
	pf_load<WP>(rS, vb4, a.t, pf);
	pf.old_ps_b[0] = pf.zeta_b[0] = 0;
	if (lane < NB_BANDS) {
		pf.old_ps_b[0] = sm[SL::OLDPS_B + lane];
		pf.zeta_b[0] = sm[SL::ZETA_B + lane];
	}
	for (int f = 0; f < nf; ++f) {
		{
			float lo[K], ln[K];
			load_vec<K>(L.ly[f] + e0, lo);
			load_vec<K>(L.ly[f + 1] + e0, ln);
			residual_echo<WP>(L, a.t, pf, lo, ln, f ? resetf[1] : resetf[0], f ? leakf[1] : leakf[0]);
		}
		float xcur[K];
#pragma unroll
		for (int k = 0; k < K; ++k) xcur[k] = (float)L.outf[f][e0 + k];
		int out_f[K];
		postfilter_frame<WP>(L, a.t, a.t, L.vec(), L.band(), sc, pf, xcur, out_f);
		int16_t *op = out_ptr(f);
#pragma unroll
		for (int k = 0; k < K; ++k) op[k] = (int16_t)out_f[k];
		WSYNC();
	}
	pf_store<WP>(rS, vb4, pf);
	if (lane < NB_BANDS) {
		sm[SL::OLDPS_B + lane] = pf.old_ps_b[0];
		sm[SL::ZETA_B + lane] = pf.zeta_b[0];
	}

	sc.fg_pending = pendingFG ? 1 : 0, sc.bg_pending = pendingBG ? 1 : 0;
	if (lane == 0) a.scal[s] = sc;
}
