// resample_steps.hpp -- the quality-3 polyphase resampler, written ONCE: the lengths of its LDS arrays in plain C++ (the
// host's plans include this file without HIP) and, under hipcc, the steps that the batch kernels of resample.hip and the
// one-member-per-wave resamplers of bridge_phases.hpp are composed of.  Included INSIDE the includer's anonymous namespace,
// as resample_tile.hpp is.  A caller keeps what is its own: which lane takes which (tile, row), where its loads are issued
// and how deep, and where eight results go.
//
// The arithmetic, in one place.  X = history ++ input is split into m phases, X_p[j] = X[j * m + p] (m = 1: X itself), each
// an array of `plen` floats with zero slack behind it.  A lane computes one SHARE: fir_tile<FT, 8> from zero accumulators
// over one row of FT taps at a window of one phase array.  An up-sampler's output is one share; a down-sampler's (L = 1) or
// a rational resampler's (L / M) is the sum of m shares added upward from 0.f.  Then rs_word2int.  The last taps - 1
// samples of X are the next tick's history.
#pragma once

#ifdef __HIPCC__
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

constexpr int RS_FILT = 48, RS_R = 8; // quality 3: 48 taps per polyphase row, fir_tile's eight positions
constexpr int RQ_FT = 24;             // taps per lane of the rational resamplers: filt_len / M, 48 / 2 and 72 / 3

// floats of an up-sampler's flat window: history ++ input ++ the last tile's look-ahead, zero
RS_HD inline int rs_flat_len(int in_len) { return (RS_FILT - 1 + in_len + RS_R + 1 + 3) & ~3; }
// floats per phase array of a resampler that splits its input into m phases, ft taps per phase: its share of history ++
// input + the tile FIR's look-ahead
RS_HD inline int rs_plen(int ft, int m, int in_len) { return ((ft * m - 1 + in_len + m - 1) / m + RS_R + 8 + 3) & ~3; }
// the same with plen / 4 odd, for a caller whose neighbouring lanes read neighbouring arrays at one offset.  Lane l of the
// tile FIR reads 16 bytes at array (l % m) * plen + 8 * (l / m): the tiles fall on the even 16-byte slots of the 256-byte
// bank row, an odd plen / 4 puts the neighbouring array on the odd ones (an even one -- 144, 224 -- stacks them on one
// slot).  The two stay apart: they decide the LDS bank placement of each form and the scratch its caller budgets.
RS_HD inline int rs_plen_odd(int ft, int m, int in_len) { return rs_plen(ft, m, in_len) | 4; }

#ifdef __HIPCC__
#include "resample_tile.hpp"

__device__ __forceinline__ unsigned pack16(int lo, int hi) { return (unsigned)(lo & 0xffff) | ((unsigned)hi << 16); }

// a polyphase row of FT taps (16-byte aligned) into register pairs: v_pk_fma_f32 broadcasts either half through op_sel
template <int FT>
__device__ __forceinline__ void load_taps(const float *row, f2 (&t2)[FT / 2]) {
	const float4 *tp = reinterpret_cast<const float4 *>(row);
#pragma unroll
	for (int j = 0; j < FT / 4; ++j) {
		const float4 v = tp[j];
		t2[2 * j] = (f2){v.x, v.y}, t2[2 * j + 1] = (f2){v.z, v.w};
	}
}

// Quad q of history ++ input, as loaded -- quads [0, hq) are the history row, hist = 4 * hq - 1 samples (the taps are a
// multiple of four) and a pad slot, the row's last, that is no sample; the rest is the input -- into the m phase arrays as
// floats.  COPIES == 2 stages every array a second time behind the first m, one float early (X_p[j] at j - 1): a window
// that starts one sample on, on 16 bytes again.
template <int COPIES>
__device__ __forceinline__ void scatter_quad(float *xp, const short4 v, int q, int hq, int hist, int m, int plen) {
	static_assert(COPIES == 1 || COPIES == 2, "one window offset, or two");
	const bool h = q < hq;
	const int b = h ? 4 * q : hist + 4 * (q - hq); // index in history ++ input
	const short e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const int i = b + k;
		if (k < 3 || !h || i < hist) {
			const int ph = i % m, j = i / m;
			const float f = (float)e[k];
			xp[ph * plen + j] = f;
			if (COPIES == 2 && j >= 1) xp[(m + ph) * plen + j - 1] = f;
		}
	}
}

// one share: R = 8 consecutive positions of one row of taps from zero accumulators, the window 16-byte aligned
template <int FT>
__device__ __forceinline__ void fir_share(const float *win, const f2 (&t2)[FT / 2], f2 (&acc2)[RS_R / 2]) {
#pragma unroll
	for (int q = 0; q < RS_R / 2; ++q) acc2[q] = (f2){0.f, 0.f};
	fir_tile<FT, RS_R>(win, t2, acc2);
}

// eight consecutive outputs, each the sum of its m shares ps[k * m + p] added upward from 0.f
__device__ __forceinline__ void gather_group(const float *ps, int m, int (&o)[8]) {
#pragma unroll
	for (int k = 0; k < 8; ++k) {
		float sum = 0.f;
		for (int p = 0; p < m; ++p) sum += ps[k * m + p];
		o[k] = rs_word2int(sum);
	}
}

// quad q of the new history row: the last `hist` = taps - 1 samples of history ++ input out of the phase arrays, samples
// in_len + 4q on; the pad slot zero
__device__ __forceinline__ short4 history_quad(const float *xp, int q, int hist, int in_len, int m, int plen) {
	short4 h;
	short *hp = &h.x;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const int i = in_len + 4 * q + k;
		hp[k] = (4 * q + k < hist) ? (short)xp[(i % m) * plen + i / m] : (short)0;
	}
	return h;
}
#endif
