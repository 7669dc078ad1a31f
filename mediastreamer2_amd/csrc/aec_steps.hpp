// aec_steps.hpp -- the steps of one libspeexdsp frame (speex_echo_cancellation, then speex_preprocess_run), each written
// ONCE for both canceller kernels (included by aec.hip after aec_wave.hpp; aec_tick.hpp and aec_group.hpp compose them).
//
// A step is the library's arithmetic in the library's operand order (the unit is built with -ffp-contract=off and the tests
// compare bits); what it does not know is which lanes hold a leg.  That is the lanes policy P:
//   Wave<F>  the leg is the whole wavefront, K = F / 64 bins per lane          (aec_tick_kernel, below)
//   Grp<F>   the leg is G = F / 4 lanes of it, 4 bins per lane                 (aec_group_kernel, aec_group.hpp)
// with the members  F, K, G, NBL (Bark bands per lane)  lane()  first / last (a value of the leg's first / last lane, in
// all of them)  shr1 (lane l <- lane l - 1, the first <- head)  any  tree  Seq (the ordered sums)  dc_notch  deemphasis
// rfft_forward  rfft_inverse  band_total (the ascending sum over the 24 bands).
// A step takes its state by reference -- arrays, AecScalars -- and never branches for the kernel: the two-path control
// hands back its decisions and the kernel keeps its own if / else (one function with a three-way code moved the tick
// kernel's register allocation: 12 bytes of scratch at F = 256).  Addressing, LDS layout, the streaming passes over the
// filter blocks and every barrier between steps belong to the kernels.

template <int F_>
struct Wave { // the 64 lanes of the wavefront: exactly the instructions aec_tick_kernel has always used
	static constexpr int F = F_, K = F / 64, G = 64, NBL = 1;
	using Seq = WSeq<K>;
	__device__ static __forceinline__ int lane() { return threadIdx.x; }
	__device__ static __forceinline__ float first(float v) { return rdlane(v, 0); }
	__device__ static __forceinline__ float last(float v) { return rdlane(v, 63); }
	__device__ static __forceinline__ float shr1(float head, float v) {
		float t = __shfl_up(v, 1);
		if (threadIdx.x == 0) t = head;
		return t;
	}
	__device__ static __forceinline__ int any(bool p) { return __any(p); }
	template <typename Op>
	__device__ static __forceinline__ float tree(float v, Op op) { return wave_tree(v, op); }
	__device__ static __forceinline__ void dc_notch(const float (&in)[K], float radius, float den2, float &m0, float &m1, float (&out)[K]) {
		w_dc_notch<K>(in, radius, den2, m0, m1, out);
	}
	__device__ static __forceinline__ void deemphasis(const float (&d)[K], float &mem, float (&out)[K]) { w_deemphasis<K>(d, mem, out); }
	template <typename LL, typename LT>
	__device__ static __forceinline__ void rfft_forward(LL &L, const LT &T, float2 (&out)[K], const float *src = nullptr) {
		w_rfft_forward<F>(L, T, out, src);
	}
	template <typename LL, typename LT>
	__device__ static __forceinline__ void rfft_inverse(LL &L, const LT &T, const float2 (&in)[K]) { w_rfft_inverse<F>(L, T, in); }
	// lane b < 24 holds band b's value: the library's ascending sum over the bands
	__device__ static __forceinline__ float band_total(const float (&vb)[NBL], float *) {
		float sum = 0;
#pragma unroll
		for (int i = 0; i < NB_BANDS; ++i) sum = sum + rdlane(vb[0], i);
		return sum;
	}
};

// ---- far end: pre-emphasis (memX: the last sample of the frame before), energy, spectrum of [previous frame | this frame]
template <typename P, typename LL, typename LT>
__device__ __forceinline__ void far_end(LL &L, const LT &T, const float (&far)[P::K], const float (&xp)[P::K], float &memX, float (&xn)[P::K],
                                        float2 (&X0)[P::K], float &Sxx) {
	constexpr int K = P::K, F = P::F;
	const int e0 = P::lane() * K;
	float prev = P::shr1(memX, far[K - 1]);
#pragma unroll
	for (int k = 0; k < K; ++k) {
		xn[k] = far[k] - .9f * prev;
		prev = far[k];
	}
	memX = P::last(far[K - 1]);
	Sxx = P::Seq::inner_prod(xn, xn);
	WSYNC();
	store_vec<K>(L.tbuf + e0, xp);
	store_vec<K>(L.tbuf + F + e0, xn);
	P::rfft_forward(L, T, X0);
}

// ---- near end: saturation flag (returned: some sample of the leg's frame is at the rails), DC notch (serial IIR), pre-emphasis
template <typename P>
__device__ __forceinline__ auto near_end(const float (&fin)[P::K], float radius, AecScalars &sc, float (&input)[P::K]) {
	constexpr int K = P::K;
	bool satl = false;
#pragma unroll
	for (int k = 0; k < K; ++k) satl |= (fin[k] <= -32000.f || fin[k] >= 32000.f);
	const auto any_sat = P::any(satl);
	const float den2 = (float)(radius * radius + .7 * (1 - radius) * (1 - radius));
	float v[K];
	P::dc_notch(fin, radius, den2, sc.notch0, sc.notch1, v);
	float vprev = P::shr1(sc.memD, v[K - 1]);
#pragma unroll
	for (int k = 0; k < K; ++k) {
		input[k] = v[k] - .9f * vprev;
		vprev = v[k];
	}
	sc.memD = P::last(v[K - 1]);
	return any_sat;
}

// ---- |X|^2 bin by bin; bin 0 holds (DC, Nyquist): the Nyquist power goes to every lane of the leg (the ordered sums need it)
template <typename P>
__device__ __forceinline__ void bin_power(const float2 (&X)[P::K], float (&pw)[P::K], float &pw_F) {
	constexpr int K = P::K;
	const int e0 = P::lane() * K;
	float nyq = 0;
#pragma unroll
	for (int k = 0; k < K; ++k) {
		if (e0 + k == 0) {
			pw[k] = X[k].x * X[k].x;
			nyq = X[k].y * X[k].y;
		} else {
			pw[k] = X[k].x * X[k].x + X[k].y * X[k].y;
		}
	}
	pw_F = P::first(nyq);
}

// ---- W += prop p1 conj(X) E, bin by bin (weighted_spectral_mul_conj); bin 0 = (DC, Nyquist): real products with their own steps
template <typename P, typename TW, typename TX>
__device__ __forceinline__ void gradient(TW (&w)[P::K], const TX (&x)[P::K], float prop, const float2 (&E)[P::K], const float (&pp)[P::K], float pp_F) {
	constexpr int K = P::K;
	const int e0 = P::lane() * K;
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const v2f xv = {x[k].x, x[k].y}, ev = {E[k].x, E[k].y};
		const float Wt = prop * pp[k];
		v2f st = pk_cmul_conj(xv, ev) * (v2f){Wt, Wt}; // Wt (x.x E.x + x.y E.y), Wt ((-x.y) E.x + x.x E.y)
		if (k == 0) {
			const v2f dc = (xv * ev) * (v2f){Wt, prop * pp_F}; // W0 (x.x E.x), WN (x.y E.y)
			if (e0 == 0) st = dc;
		}
		const v2f r = (v2f){w[k].x, w[k].y} + st;
		w[k].x = r.x, w[k].y = r.y;
	}
}

// ---- AUMDF constraint of one block: IFFT, zero the second half, FFT.  The transforms need every lane of the wavefront: a
// wavefront of several legs runs it whenever one of them asks and keeps the result for the legs that did
template <typename P, typename LL, typename LT, typename TW>
__device__ __forceinline__ void constrain(LL &L, const LT &T, TW (&wv)[P::K]) {
	constexpr int K = P::K, F = P::F;
	const int e0 = P::lane() * K;
	float2 w[K];
#pragma unroll
	for (int k = 0; k < K; ++k) w[k] = make_float2(wv[k].x, wv[k].y);
	P::rfft_inverse(L, T, w);
	float z[K];
#pragma unroll
	for (int k = 0; k < K; ++k) z[k] = 0.f;
	store_vec<K>(w_time(L) + F + e0, z);
	P::rfft_forward(L, T, w, w_time(L));
#pragma unroll
	for (int k = 0; k < K; ++k) wv[k].x = w[k].x, wv[k].y = w[k].y;
}

// ---- two-path control.  The kernel branches: if (two_path_update) { its filter copy; blend_foreground }
// else if (two_path_reset) { its filter copy; take_foreground }.
// the running statistics and the test "the background does better": true = foreground := background (its scalars are done)
__device__ __forceinline__ bool two_path_update(AecScalars &sc, float Sff, float See, float Dbf) {
	sc.Davg1 = .6f * sc.Davg1 + .4f * (Sff - See);
	sc.Davg2 = .85f * sc.Davg2 + .15f * (Sff - See);
	sc.Dvar1 = .36f * sc.Dvar1 + (.4f * Sff) * (.4f * Dbf);
	sc.Dvar2 = .7225f * sc.Dvar2 + (.15f * Sff) * (.15f * Dbf);
	bool update_foreground = false;
	if ((Sff - See) * fabsf(Sff - See) > Sff * Dbf) update_foreground = true;
	else if (sc.Davg1 * fabsf(sc.Davg1) > .5f * sc.Dvar1) update_foreground = true;
	else if (sc.Davg2 * fabsf(sc.Davg2) > .25f * sc.Dvar2) update_foreground = true;
	if (update_foreground) {
		sc.fg_updates++;
		sc.Davg1 = sc.Davg2 = 0;
		sc.Dvar1 = sc.Dvar2 = 0;
	}
	return update_foreground;
}
// the output of a frame that updated the foreground: the two responses cross-faded under the Hann window
template <typename P>
__device__ __forceinline__ void blend_foreground(const float *hann, float (&efg)[P::K], const float (&ybg)[P::K]) {
	constexpr int K = P::K, F = P::F;
	const int e0 = P::lane() * K;
	float h0[K], h1[K];
	load_vec<K>(hann + e0, h0);
	load_vec<K>(hann + F + e0, h1);
#pragma unroll
	for (int k = 0; k < K; ++k) efg[k] = h1[k] * efg[k] + h0[k] * ybg[k];
}
// the test "the background has diverged": true = background := foreground (its scalars are done)
__device__ __forceinline__ bool two_path_reset(AecScalars &sc, float Sff, float See, float Dbf) {
	bool reset_background = false;
	if ((-(Sff - See)) * fabsf(Sff - See) > 4.f * (Sff * Dbf)) reset_background = true;
	if ((-sc.Davg1) * fabsf(sc.Davg1) > 4.f * sc.Dvar1) reset_background = true;
	if ((-sc.Davg2) * fabsf(sc.Davg2) > 4.f * sc.Dvar2) reset_background = true;
	if (reset_background) {
		sc.bg_resets++;
		sc.Davg1 = sc.Davg2 = 0;
		sc.Dvar1 = sc.Dvar2 = 0;
	}
	return reset_background;
}
// ... the background's response, error and error energy become the foreground's
template <typename P>
__device__ __forceinline__ void take_foreground(const float (&efg)[P::K], const float (&input)[P::K], float Sff, float (&ybg)[P::K], float (&e2)[P::K],
                                                float &See) {
#pragma unroll
	for (int k = 0; k < P::K; ++k) {
		ybg[k] = efg[k];
		e2[k] = input[k] - efg[k];
	}
	See = Sff;
}

// ---- output (serial de-emphasis) and the frame's correlations
template <typename P, typename TS>
__device__ __forceinline__ void output_and_correlations(AecScalars &sc, const float (&input)[P::K], const float (&efg)[P::K], const float (&e2)[P::K],
                                                        const float (&ybg)[P::K], TS any_sat, int (&out_i)[P::K], float &Sey, float &Syy, float &Sdd) {
	constexpr int K = P::K;
	{
		float d[K], tout[K];
#pragma unroll
		for (int k = 0; k < K; ++k) d[k] = input[k] - efg[k];
		P::deemphasis(d, sc.memE, tout);
#pragma unroll
		for (int k = 0; k < K; ++k) out_i[k] = word2int(tout[k]);
	}
	P::Seq::inner_prod3(e2, ybg, ybg, ybg, input, input, Sey, Syy, Sdd);
	if (any_sat && sc.saturated == 0) sc.saturated = 1;
}

// ---- error / response spectra: transforms of [0 | e2] and [0 | ybg]
template <typename P, typename LL, typename LT>
__device__ __forceinline__ void error_spectra(LL &L, const LT &T, const float (&e2)[P::K], const float (&ybg)[P::K], float2 (&Ecur)[P::K],
                                              float2 (&Ycur)[P::K]) {
	constexpr int K = P::K, F = P::F;
	const int e0 = P::lane() * K;
	float z[K];
#pragma unroll
	for (int k = 0; k < K; ++k) z[k] = 0.f;
	WSYNC();
	store_vec<K>(L.tbuf + e0, z);
	store_vec<K>(L.tbuf + F + e0, e2);
	P::rfft_forward(L, T, Ecur);
	store_vec<K>(L.tbuf + e0, z);
	store_vec<K>(L.tbuf + F + e0, ybg);
	P::rfft_forward(L, T, Ycur);
}

// ---- sanity checks: the frame's output is zeroed when the energies are not numbers; screwed_up >= 50 asks for the reset
template <typename P>
__device__ __forceinline__ void sanity_checks(AecScalars &sc, float Sff, float See, float Sxx, float Syy, float Sdd, int (&out_i)[P::K]) {
	constexpr int N = 2 * P::F;
	bool zero_out = false;
	if (!(Syy >= 0 && Sxx >= 0 && See >= 0) || !(Sff < N * 1e9 && Syy < N * 1e9 && Sxx < N * 1e9)) {
		sc.screwed_up += 50;
		zero_out = true;
	} else if (Sff > Sdd + (float)(N * 10000)) {
		sc.screwed_up++;
	} else {
		sc.screwed_up = 0;
	}
	if (zero_out) {
#pragma unroll
		for (int k = 0; k < P::K; ++k) out_i[k] = 0;
	}
}

// ---- the scalar part of speex_echo_state_reset (the arrays are the kernel's: it knows where they live)
__device__ __forceinline__ void reset_scalars(AecScalars &sc) {
	sc.state_resets++;
	sc.cancel_count = 0;
	sc.screwed_up = 0;
	sc.notch0 = sc.notch1 = 0;
	sc.memD = sc.memE = sc.memX = 0;
	sc.saturated = 0;
	sc.adapted = 0;
	sc.sum_adapt = 0;
	sc.Pey = sc.Pyy = 1.0f;
	sc.Davg1 = sc.Davg2 = sc.Dvar1 = sc.Dvar2 = 0;
}

// ---- far-end power, smoothed
template <typename P>
__device__ __forceinline__ void far_power(const AecArgs &a, const float (&Xf)[P::K], float Xf_F, float (&pw)[P::K], float &pw_F) {
#pragma unroll
	for (int k = 0; k < P::K; ++k) pw[k] = a.ss_1 * pw[k] + 1 + a.ss * Xf[k];
	pw_F = a.ss_1 * pw_F + 1 + a.ss * Xf_F;
}

// ---- error / response power against their averages (the leak estimate's inputs), the averages moved on
template <typename P>
__device__ __forceinline__ void spectral_averages(const AecArgs &a, const float (&Rf)[P::K], float Rf_F, const float (&Yf)[P::K], float Yf_F,
                                                  float (&eh)[P::K], float &eh_F, float (&yh)[P::K], float &yh_F, float (&Ehd)[P::K], float &Ehd_F,
                                                  float (&Yhd)[P::K], float &Yhd_F) {
#pragma unroll
	for (int k = 0; k < P::K; ++k) {
		Ehd[k] = Rf[k] - eh[k];
		Yhd[k] = Yf[k] - yh[k];
		eh[k] = (1 - a.spec_average) * eh[k] + a.spec_average * Rf[k];
		yh[k] = (1 - a.spec_average) * yh[k] + a.spec_average * Yf[k];
	}
	Ehd_F = Rf_F - eh_F;
	Yhd_F = Yf_F - yh_F;
	eh_F = (1 - a.spec_average) * eh_F + a.spec_average * Rf_F;
	yh_F = (1 - a.spec_average) * yh_F + a.spec_average * Yf_F;
}

// ---- leak estimate, residual-to-error ratio, the adaptation flag and the per-bin step sizes p1 of the NEXT frame
// (M: the filter's block count; Sxx2: the far-end energy as the library has it by then)
template <typename P>
__device__ __forceinline__ void leak_and_steps(const AecArgs &a, AecScalars &sc, int M, float Sxx2, float See, float Syy, float Sey,
                                               const float (&Ehd)[P::K], float Ehd_F, const float (&Yhd)[P::K], float Yhd_F, const float (&Rf)[P::K],
                                               float Rf_F, const float (&Yf)[P::K], float Yf_F, const float (&pw)[P::K], float pw_F, float (&p1)[P::K],
                                               float &p1_F) {
	constexpr int K = P::K, N = 2 * P::F;
	float Pey = 1.0f, Pyy = 1.0f;
	Pey = Pey + Ehd_F * Yhd_F;
	Pyy = Pyy + Yhd_F * Yhd_F;
	P::Seq::dot_desc2(Pey, Ehd, Yhd, Pyy, Yhd, Yhd, Pey, Pyy);
	Pyy = sqrt_via_double(Pyy);
	Pey = Pey / Pyy;
	float tmp32 = a.beta0 * Syy;
	if (tmp32 > a.beta_max * See) tmp32 = a.beta_max * See;
	const float alpha = tmp32 / See;
	const float alpha_1 = 1.0f - alpha;
	sc.Pey = alpha_1 * sc.Pey + alpha * Pey;
	sc.Pyy = alpha_1 * sc.Pyy + alpha * Pyy;
	if (sc.Pyy < 1.0f) sc.Pyy = 1.0f;
	if (sc.Pey < .005f * sc.Pyy) sc.Pey = .005f * sc.Pyy;
	if (sc.Pey > sc.Pyy) sc.Pey = sc.Pyy;
	sc.leak_estimate = sc.Pey / sc.Pyy;
	float RER = (float)((.0001 * Sxx2 + 3. * (sc.leak_estimate * Syy)) / See);
	if (RER < Sey * Sey / (1 + See * Syy)) RER = Sey * Sey / (1 + See * Syy);
	if (RER > .5) RER = .5;
	if (!sc.adapted && sc.sum_adapt > (float)M && sc.leak_estimate * Syy > .03f * Syy) sc.adapted = 1;

	auto step = [&](float Yfv, float Rfv, float pwv) -> float {
		float r = sc.leak_estimate * Yfv;
		const float e = Rfv + 1;
		if (r > .5 * e) r = (float)(.5 * e);
		r = .7f * r + .3f * (float)(RER * e);
		return r / (e * (pwv + 10));
	};
	if (sc.adapted) {
#pragma unroll
		for (int k = 0; k < K; ++k) p1[k] = step(Yf[k], Rf[k], pw[k]);
		p1_F = step(Yf_F, Rf_F, pw_F);
	} else {
		float adapt_rate = 0;
		if (Sxx2 > (float)(N * 1000)) {
			tmp32 = .25f * Sxx2;
			if (tmp32 > .25 * See) tmp32 = (float)(.25 * See);
			adapt_rate = tmp32 / See;
		}
#pragma unroll
		for (int k = 0; k < K; ++k) p1[k] = adapt_rate / (pw[k] + 10);
		p1_F = adapt_rate / (pw_F + 10);
		sc.sum_adapt = sc.sum_adapt + adapt_rate;
	}
}

// ---- the post-filter (speex_preprocess_run).  Its per-bin state and tables, in registers for as long as the kernel runs
// frames; one or two of the 24 Bark bands per lane (lane l of the leg: bands l, l + G)
template <typename P>
struct PfState {
	static constexpr int K = P::K, NBL = P::NBL;
	float en[K], inb[K], S[K], Smin[K], Stmp[K], noise[K], old_ps[K], zeta[K], ob[K]; // state
	float wl[K], wr[K], h0[K], h1[K], w0[K], w1[K];                                   // filterbank weights, Hann and analysis windows
	float old_ps_b[NBL], zeta_b[NBL];
};

// residual echo spectrum (speex_echo_get_residual) of the echo estimates [lo | ln] into the smoothed estimate pf.en; its
// filterbank products wait in L.spec for postfilter_frame's band sums
template <typename P, typename LL, typename LT>
__device__ __forceinline__ void residual_echo(LL &L, const LT &T, PfState<P> &pf, const float (&lo_in)[P::K], const float (&ln_in)[P::K], bool was_reset,
                                              float leak) {
	constexpr int K = P::K, F = P::F;
	const int e0 = P::lane() * K;
	float *pl = L.spec, *pr = L.spec + F;
	{
		float lo[K], ln[K];
#pragma unroll
		for (int k = 0; k < K; ++k) lo[k] = pf.h0[k] * (was_reset ? 0.f : lo_in[k]), ln[k] = pf.h1[k] * ln_in[k];
		WSYNC();
		store_vec<K>(L.tbuf + e0, lo);
		store_vec<K>(L.tbuf + F + e0, ln);
	}
	float2 Yr[K];
	P::rfft_forward(L, T, Yr);
	const float leak2 = (leak > .5) ? 1.f : 2 * leak;
	float res[K];
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const float r = (e0 + k == 0) ? Yr[k].x * Yr[k].x : Yr[k].x * Yr[k].x + Yr[k].y * Yr[k].y;
		res[k] = (float)(int32_t)(leak2 * r);
	}
	const float res0 = P::first(res[0]);
	const bool bad = !(res0 >= 0 && res0 < F * 1e9f);
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const float rr = bad ? 0.f : res[k];
		const float c = .6f * pf.en[k];
		pf.en[k] = c > rr ? c : rr;
		pl[e0 + k] = pf.wl[k] * pf.en[k];
		pr[e0 + k] = pf.wr[k] * pf.en[k];
	}
}

__device__ __forceinline__ void pf_snr(float psv, float noisev, float echov, float oldps, float &post, float &prior) {
	const float tot_noise = 1.f + noisev + echov + 0.f;
	post = psv / tot_noise - 1.f;
	if (post > 100.f) post = 100.f;
	const float t = oldps / (oldps + tot_noise);
	const float gamma = .1f + .89f * (t * t);
	prior = gamma * (post > 0 ? post : 0) + (1.0f - gamma) * (oldps / tot_noise);
	if (prior > 100.f) prior = 100.f;
}

// the rest of the frame: analysis of the cancelled frame xcur, noise estimate, the gains per band and per bin, synthesis
// -> the K output samples.  lvec: F floats, bandv: 4 * 24 floats of the leg's LDS; t: the filterbank's tables.
template <typename P, typename LL, typename LT>
__device__ __forceinline__ void postfilter_frame(LL &L, const LT &T, const AecTables &t, float *lvec, float *bandv, AecScalars &sc, PfState<P> &pf,
                                                 const float (&xcur)[P::K], int (&out)[P::K]) {
	constexpr int K = P::K, F = P::F, G = P::G, NBL = P::NBL;
	const int lane = P::lane(), e0 = lane * K;
	sc.nb_adapt++;
	if (sc.nb_adapt > 20000) sc.nb_adapt = 20000;
	sc.min_count++;
	float beta = 1.0f / sc.nb_adapt;
	if (beta < .03f) beta = .03f;
	const float beta_1 = 1.0f - beta;
	// analysis frame [inbuf, x] * window
	{
		float a0[K], a1[K];
#pragma unroll
		for (int k = 0; k < K; ++k) {
			a0[k] = pf.inb[k] * pf.w0[k];
			a1[k] = xcur[k] * pf.w1[k];
			pf.inb[k] = xcur[k];
		}
		store_vec<K>(L.tbuf + e0, a0);
		store_vec<K>(L.tbuf + F + e0, a1);
	}
	float2 ft[K];
	P::rfft_forward(L, T, ft);
	float ps[K];
#pragma unroll
	for (int k = 0; k < K; ++k) {
		ps[k] = (e0 + k == 0) ? ft[k].x * ft[k].x : ft[k].x * ft[k].x + ft[k].y * ft[k].y;
		lvec[e0 + k] = ps[k];
		L.tbuf[e0 + k] = pf.wl[k] * ps[k];     // the analysis transform is done with its input: the frame's filterbank
		L.tbuf[F + e0 + k] = pf.wr[k] * ps[k]; // products wait there (left halves, right halves) for the fused band sums
	}
	WSYNC();
	// update_noise_prob
	int min_range;
	if (sc.nb_adapt < 100) min_range = 15;
	else if (sc.nb_adapt < 1000) min_range = 50;
	else if (sc.nb_adapt < 10000) min_range = 150;
	else min_range = 300;
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const int b = e0 + k;
		if (b == 0 || b == F - 1) pf.S[k] = .8f * pf.S[k] + .2f * ps[k];
		else pf.S[k] = .8f * pf.S[k] + .05f * lvec[b - 1] + .1f * ps[k] + .05f * lvec[b + 1];
		if (sc.nb_adapt == 1) pf.Smin[k] = pf.Stmp[k] = 0;
		if (sc.min_count > min_range) {
			pf.Smin[k] = pf.Stmp[k] < pf.S[k] ? pf.Stmp[k] : pf.S[k];
			pf.Stmp[k] = pf.S[k];
		} else {
			pf.Smin[k] = pf.Smin[k] < pf.S[k] ? pf.Smin[k] : pf.S[k];
			pf.Stmp[k] = pf.Stmp[k] < pf.S[k] ? pf.Stmp[k] : pf.S[k];
		}
		const int update_prob = (.4f * pf.S[k] > pf.Smin[k]) ? 1 : 0;
		if (!update_prob || ps[k] < pf.noise[k]) {
			const float v = beta_1 * pf.noise[k] + beta * ps[k];
			pf.noise[k] = v > 0 ? v : 0;
		}
	}
	if (sc.min_count > min_range) sc.min_count = 0;
	{
		float *np = w_time(L); // free between the analysis and the synthesis transform
#pragma unroll
		for (int k = 0; k < K; ++k) {
			np[e0 + k] = pf.wl[k] * pf.noise[k];
			np[F + e0 + k] = pf.wr[k] * pf.noise[k];
		}
		WSYNC();
		// echo estimate (products in L.spec since residual_echo), frame, noise: three band sums in one loop
#pragma unroll
		for (int bi = 0; bi < NBL; ++bi) {
			const int b = lane + bi * G;
			if (b < NB_BANDS) band_sum3<F>(t, b, L.spec, L.tbuf, np, bandv[b], bandv[NB_BANDS + b], bandv[2 * NB_BANDS + b]);
		}
	}
	WSYNC();

	float post[K], prior[K];
#pragma unroll
	for (int k = 0; k < K; ++k) {
		if (sc.nb_adapt == 1) pf.old_ps[k] = ps[k];
		pf_snr(ps[k], pf.noise[k], pf.en[k], pf.old_ps[k], post[k], prior[k]);
		lvec[e0 + k] = prior[k];
	}
	float post_b[NBL], prior_b[NBL], ps_b[NBL];
#pragma unroll
	for (int bi = 0; bi < NBL; ++bi) {
		const int b = lane + bi * G;
		post_b[bi] = prior_b[bi] = ps_b[bi] = 0;
		if (b < NB_BANDS) {
			ps_b[bi] = bandv[NB_BANDS + b];
			if (sc.nb_adapt == 1) pf.old_ps_b[bi] = ps_b[bi];
			pf_snr(ps_b[bi], bandv[2 * NB_BANDS + b], bandv[b], pf.old_ps_b[bi], post_b[bi], prior_b[bi]);
		}
	}
	WSYNC();
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const int b = e0 + k;
		if (b == 0 || b >= F - 1) pf.zeta[k] = .7f * pf.zeta[k] + .3f * prior[k];
		else pf.zeta[k] = .7f * pf.zeta[k] + .15f * prior[k] + .075f * lvec[b - 1] + .075f * lvec[b + 1];
	}
#pragma unroll
	for (int bi = 0; bi < NBL; ++bi)
		if (lane + bi * G < NB_BANDS) pf.zeta_b[bi] = .7f * pf.zeta_b[bi] + .3f * prior_b[bi];
	const float Zframe = P::band_total(pf.zeta_b, bandv + 3 * NB_BANDS);
	const float Pframe = .1f + .899f * qcurve(Zframe / NB_BANDS);
	const int eff_echo = (int)((1.0f - Pframe) * -40 + Pframe * -15);
	// (a lane reads and writes its own bands' entries only: the gains take the band energies' place as they are made)
#pragma unroll
	for (int bi = 0; bi < NBL; ++bi) {
		const int b = lane + bi * G;
		if (b < NB_BANDS) {
			const float noise_floor = (float)exp((double)(.2302585f * -15));
			const float echo_floor = (float)exp((double)(.2302585f * eff_echo));
			const float nb = bandv[2 * NB_BANDS + b], eb = bandv[b];
			const float gfloor = (float)(sqrt((double)(noise_floor * nb + echo_floor * eb)) / sqrt((double)(1 + nb + eb)));
			const float prior_ratio = prior_b[bi] / (prior_b[bi] + 1.f);
			const float theta = prior_ratio * (1.f + post_b[bi]);
			const float MM = hypergeom_gain(theta);
			float g = prior_ratio * MM;
			if (g > 1.f) g = 1.f;
			pf.old_ps_b[bi] = .2f * pf.old_ps_b[bi] + (.8f * (g * g)) * ps_b[bi];
			const float P1 = .199f + .8f * qcurve(pf.zeta_b[bi]);
			const float q = 1.0f - Pframe * P1;
			const float g2 = (float)(1 / (1.f + (q / (1.f - q)) * (1 + prior_b[bi]) * exp((double)(-theta))));
			bandv[b] = g2;
			bandv[NB_BANDS + b] = g;
			bandv[2 * NB_BANDS + b] = gfloor;
		}
	}
	WSYNC();
	float gain2[K];
#pragma unroll
	for (int k = 0; k < K; ++k) {
		const int bl = t.bleft[e0 + k], br = bl + 1;
		auto psd = [&](const float *mel) -> float {
			float v = mel[bl] * pf.wl[k];
			v += mel[br] * pf.wr[k];
			return v;
		};
		const float p = psd(bandv);
		const float gain_bark = psd(bandv + NB_BANDS);
		const float gfl = psd(bandv + 2 * NB_BANDS);
		const float prior_ratio = prior[k] / (prior[k] + 1.f);
		const float theta = prior_ratio * (1.f + post[k]);
		const float MM = hypergeom_gain(theta);
		float g = prior_ratio * MM;
		if (g > 1.f) g = 1.f;
		if (.333f * g > gain_bark) g = 3 * gain_bark;
		float gain = g;
		pf.old_ps[k] = .2f * pf.old_ps[k] + (.8f * (gain * gain)) * ps[k];
		if (gain < gfl) gain = gfl;
		const float tmp = p * sqrt_via_double(gain) + (1.0f - p) * sqrt_via_double(gfl);
		gain2[k] = tmp * tmp;
	}
	const float g_last = P::last(gain2[K - 1]); // gain2[F-1] scales the Nyquist term
#pragma unroll
	for (int k = 0; k < K; ++k) {
		if (e0 + k == 0) {
			ft[k].x = gain2[k] * ft[k].x;
			ft[k].y = g_last * ft[k].y;
		} else {
			ft[k].x = gain2[k] * ft[k].x;
			ft[k].y = gain2[k] * ft[k].y;
		}
	}
	P::rfft_inverse(L, T, ft);
	{
		float lo[K], hi[K];
		load_vec<K>(w_time(L) + e0, lo);
		load_vec<K>(w_time(L) + F + e0, hi);
#pragma unroll
		for (int k = 0; k < K; ++k) {
			out[k] = word2int(pf.ob[k] + lo[k] * pf.w0[k]);
			pf.ob[k] = hi[k] * pf.w1[k];
		}
	}
}
