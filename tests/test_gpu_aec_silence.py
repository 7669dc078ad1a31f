"""The echo canceller through digital silence: exact zeros on one or both pins for a second or more, which a muted
microphone, a held call or an empty conference gives it on every real call -- and which no other GPU test feeds it.

About a quarter of a second after both pins go quiet the whole error spectrum E of the library's canceller is subnormal,
Davg1/2 and Dvar1/2 follow, and the in-LDS FFT, the packed multiplies and the DPP chains all work on subnormal operands
for the rest of the span.  The oracle restates the reference's x86 float build, which keeps subnormals; the kernels must
too (hipcc's default float mode does; one flush-to-zero flag in the build would not be noticed by any other test).

The `both`- and `far`-silent scenes never reach `adapted`, so the project's contract -- bit for bit until adaptation --
holds through all of them: every output sample and every state word as uint32, in every kernel form.  (A leg that keeps
its far end -- the never-silent one, and the one with only its microphone muted -- does adapt, after 1 to 2 s on these
scenes: from the frame the oracle sets `adapted` such a leg is held to the project's bar after adaptation, 1e-4 RMS of
full scale and the same decisions.)  tests/test_aec_silence_scene_cpu.py pins the premise on the oracle alone; every
test here re-asserts it on its own oracle run, and on the GPU's own E, so none of them can compare a flushed zero with a
flushed zero.  After adaptation (3 s active, 8 s of zeros, 3 s active) the bar is the suite's 1e-4 RMS, over the whole
run and in every second of it."""
import numpy as np
import pytest

import mediastreamer2_amd as ms
import aec_silence as sil
from aec_silence import make_echo_scene
from test_gpu_pipeline import NpFifo

pytestmark = pytest.mark.gpu
FULL_SCALE = 32768.0
U32 = np.uint32
TOTAL_ACTIVE = max(sil.ONSETS) + sil.BACK_FRAMES   # every leg of a batch runs the same number of frames
REASONS = ("first_silent", "first_subnormal", "most_subnormal_E", "last_silent", "last")

# (mode, active frames before the zeros).  Neighbours differ, so the four / two legs of a wavefront in the group form
# (8 / 16 kHz) never run the same scene; "masked" is gated off by the run mask for the whole silent span.
LEGS = [("both", 6), ("both", 10), ("none", 0), ("mic", 6), ("far", 10), ("masked", 6),
        ("both", 10), ("both", 6), ("mic", 10), ("far", 6), ("both", 10)]


class Leg:
    """One leg's oracle (canceller, optionally + post-filter), the record of what the zeros do to its state, and the
    comparison of a GPU leg with it: bit for bit while `adapted` is 0, the squared error kept for the 1e-4 bar after."""

    def __init__(self, oracle, rate, F, tail_ms, mode):
        self.F, self.M, self.mode = F, sil.blocks(rate, F, tail_ms), mode
        self.ec = oracle.Echo(F, tail_ms * rate // 1000, rate)
        self.frames, self.exact, self.state = 0, True, None
        self.sub, self.sub_E, self.bad, self.adapted = [], [], [], []
        self.best_E, self.want, self.verified, self.gpu_E_sub = 0, set(), {}, 0
        self.sq, self.n = 0.0, 0

    def feed(self, m, r):
        """one frame through the oracle -> its output; notes the reasons to compare the whole state after this launch"""
        o = self.ec.cancel(m, r)
        st = {what: self.ec.get(what, n) for what, n in sil.state_list(self.F, self.M)}
        counts = {what: sil.count_words(a) for what, a in st.items()}
        sub = sum(c[0] for c in counts.values())
        if sub and not any(self.sub):
            self.want.add("first_subnormal")
        if counts["E"][0] > self.best_E:
            self.best_E = counts["E"][0]
            self.want.add("most_subnormal_E")
        self.sub.append(sub)
        self.sub_E.append(counts["E"][0])
        self.bad.append(sum(c[1] for c in counts.values()))
        self.adapted.append(int(st["scalars"][8]))
        if st["scalars"][8] != 0:
            self.exact = False
        self.state, self.frames = st, self.frames + 1
        return o

    def check_output(self, got, ref, label):
        if self.exact:
            np.testing.assert_array_equal(got, ref, err_msg=label)
        else:
            d = (got.astype(np.float64) - ref.astype(np.float64)) / FULL_SCALE
            self.sq += float((d * d).sum())
            self.n += d.size

    def check_state(self, aec, s, label, force=()):
        """the GPU leg's whole state == the oracle's, as uint32, if this launch held a checkpoint (and the leg is still
        inside the bit-for-bit contract)"""
        why = self.want | set(force)
        self.want = set()
        if not why or not self.exact:
            return
        for what, n in sil.state_list(self.F, self.M):
            g = aec.get(s, what, n)
            np.testing.assert_array_equal(g.view(U32), self.state[what].view(U32), err_msg=f"{label} frame {self.frames - 1} ({', '.join(sorted(why))}): {what}")
            if what == "E" and "most_subnormal_E" in why:
                self.gpu_E_sub = sil.count_words(g)[0]
        for w in why:
            self.verified[w] = self.frames - 1

    def run(self):
        return {k: np.array(getattr(self, k)) for k in ("sub", "sub_E", "adapted")} | {"nonfinite": np.array(self.bad)}

    def finish(self, aec, s, label):
        sg, so = aec.get(s, "scalars", 16), self.ec.get("scalars", 16)
        assert sg[8] == so[8] and sg[11] == so[11], f"{label}: adapted / frame counter {sg[8]}, {sg[11]} vs the oracle's {so[8]}, {so[11]}"
        assert np.isfinite(np.concatenate([aec.get(s, what, n) for what, n in sil.state_list(self.F, self.M)])).all(), label
        if self.n:
            rms = np.sqrt(self.sq / self.n)
            assert rms <= 1e-4, f"{label}: {rms:.3e} RMS of full scale after adaptation"
        if self.mode == "both":
            sil.assert_premise(self.run(), self.F, label)
            assert set(self.verified) == set(REASONS), f"{label}: state compared at {self.verified}"
            assert self.gpu_E_sub > self.F, f"{label}: the GPU's own E holds {self.gpu_E_sub} subnormal words at its checkpoint"
        if self.mode == "far":
            assert self.exact and "last" in self.verified, label


def leg_frames(rate, F, s, mode, onset):
    """-> (mic [T, F], far [T, F], span in the leg's own frames or None)"""
    nsil = sil.silent_frames(rate, F, sil.SILENT_S)
    act = onset or min(sil.ONSETS)
    mic, far, span = sil.silence_scene(300 + s, rate, F, act, sil.SILENT_S, TOTAL_ACTIVE - act,
                                       mode if mode in ("both", "mic", "far") else "none")
    mic, far = mic.reshape(-1, F), far.reshape(-1, F)
    if mode == "masked":   # it sits the others' silent span out: the frames it is handed are the ones around it
        keep = list(range(min(sil.ONSETS))) + list(range(max(sil.ONSETS) + nsil, len(mic)))
        mic, far = mic[keep], far[keep]
    return mic, far, (span if mode in ("both", "mic", "far") else None)


def note_frame(leg, span, idx, last):
    if span is not None and idx == span[0]:
        leg.want.add("first_silent")
    if span is not None and idx == span[1] - 1:
        leg.want.add("last_silent")
    if idx == last:
        leg.want.add("last")


def run_rows(ctx, oracle, rate, F, tail_ms, tick_form):
    """LEGS through mi_aec_process (one frame per launch, host rows, a run mask) or mi_aec_process_frames (up to two frames
    per launch, device rows, per-leg counts), flags = 0, against one oracle per leg"""
    torch = pytest.importorskip("torch")
    n = len(LEGS)
    nsil = sil.silent_frames(rate, F, sil.SILENT_S)
    aec = ms.AecBatch(ctx, n, rate, frame_size=F, filter_length=tail_ms * rate // 1000)
    legs = [Leg(oracle, rate, F, tail_ms, m) for m, _ in LEGS]
    data = [leg_frames(rate, F, s, m, o) for s, (m, o) in enumerate(LEGS)]
    pos = np.zeros(n, int)
    per = 2 if tick_form else 1
    m_lo, m_hi = min(sil.ONSETS), max(sil.ONSETS) + nsil   # the masked leg is gated off over these frames of the batch
    onset_slot = set()
    step = 0
    while any(pos[s] < len(data[s][0]) for s in range(n)):
        cnt = np.zeros(n, np.uint8)
        for s, (mode, _) in enumerate(LEGS):
            left = len(data[s][0]) - pos[s]
            k = min(per, left)
            if tick_form and step == 0 and s % 2:
                k = 1   # odd legs: their even frames are the second of a launch from here on
            if mode == "masked" and m_lo <= step * per < m_hi:
                k = 0
            cnt[s] = k
        m2, f2 = np.zeros((n, per * F), np.int16), np.zeros((n, per * F), np.int16)
        for s in range(n):
            for j in range(int(cnt[s])):
                m2[s, j * F:(j + 1) * F] = data[s][0][pos[s] + j]
                f2[s, j * F:(j + 1) * F] = data[s][1][pos[s] + j]
        if tick_form:
            dm, df, dc = torch.from_numpy(m2).cuda(), torch.from_numpy(f2).cuda(), torch.from_numpy(cnt).cuda()
            out = torch.full_like(dm, 777)
            torch.cuda.synchronize()
            aec.process_frames(dm, df, out, dc, max_frames=2, flags=0)
            ctx.sync()
            got = out.cpu().numpy()
        else:
            got = aec.process(m2, f2, out=np.full((n, F), 777, np.int16), run=cnt, flags=0)
        for s, (mode, _) in enumerate(LEGS):
            leg, (mic, far, span), k = legs[s], data[s], int(cnt[s])
            label = f"{rate}/{F}/{tail_ms} launch {step} leg {s} ({mode})"
            assert (got[s, k * F:] == 777).all(), f"{label}: rows of frames that did not run were written"
            for j in range(k):
                idx = pos[s] + j
                note_frame(leg, span, idx, len(mic) - 1)
                if span is not None and idx == span[0]:
                    onset_slot.add((mode, j))
                leg.check_output(got[s, j * F:(j + 1) * F], leg.feed(mic[idx], far[idx]), f"{label} frame {idx}")
            pos[s] += k
            last_masked = mode == "masked" and k == 0 and not (m_lo <= (step + 1) * per < m_hi)
            if k or last_masked:   # (a gated leg: its state equals the oracle's that was not called)
                leg.check_state(aec, s, label, force=("masked_span_end",) if last_masked else ())
        step += 1
    for s, (mode, _) in enumerate(LEGS):
        legs[s].finish(aec, s, f"{rate}/{F}/{tail_ms} leg {s} ({mode})")
    masked = legs[[m for m, _ in LEGS].index("masked")]
    assert "masked_span_end" in masked.verified and masked.frames == TOTAL_ACTIVE - (max(sil.ONSETS) - min(sil.ONSETS))
    if tick_form:
        assert {("both", 0), ("both", 1)} <= onset_slot, f"the zeros must start on either frame of a launch: {onset_slot}"
    aec.close()
    return legs


@pytest.mark.parametrize("rate,F,tail_ms", sil.GEOMETRIES)
def test_silence_bit_exact_frame_by_frame(ctx, oracle, rate, F, tail_ms):
    """mi_aec_process, 11 legs: zeros on both pins from frame 6 or 10 on, on the microphone or the far end alone, never, and
    one leg gated off for the whole span -- neighbours differ, so at 8 / 16 kHz silent and active legs share a wavefront.
    Every output sample of every frame and the whole state at the checkpoints == the oracle's as uint32."""
    run_rows(ctx, oracle, rate, F, tail_ms, tick_form=False)


@pytest.mark.parametrize("rate,F,tail_ms", [(8000, 64, 128), (16000, 128, 128), (48000, 256, 128), (48000, 512, 128)])
def test_silence_bit_exact_tick_form(ctx, oracle, rate, F, tail_ms):
    """mi_aec_process_frames, two frames per launch: the same scenes against the same oracle, the zeros starting on the first
    frame of a launch for the even legs and on the second for the odd ones"""
    run_rows(ctx, oracle, rate, F, tail_ms, tick_form=True)


# (mode, active frames before the zeros, the far end's silent blocks are MISSING: the canceller injects the silence itself)
FIFO_LEGS = [("both", 6, False), ("both", 10, True), ("none", 0, False), ("mic", 6, False), ("far", 10, False), ("far", 6, True),
             ("both", 10, False), ("both", 6, True), ("mic", 10, False), ("both", 6, False), ("both", 10, True)]


def run_fifos(ctx, oracle, rate, F, tail_ms, in_rate=None):
    """FIFO_LEGS through mi_aec_process_fifos (in_rate None) or mi_aec_process_fifos_resampled, 10 ms ticks, flags = 0: the
    framing modelled as tests/test_gpu_pipeline.py models it (NpFifo: MSBufferizer for a batch; a far end that cannot supply
    a frame gives zeros and keeps what it holds), one oracle per leg fed the frames the model pops.  Folded resampler: the
    model continues from the block the launch itself queued (<= 1 LSB from the oracle's resampler)."""
    torch = pytest.importorskip("torch")
    n, ns = len(FIFO_LEGS), rate // 100
    nin = ns if in_rate is None else in_rate // 100
    nsil = int(round(sil.SILENT_S * 100))
    nticks = (TOTAL_ACTIVE * F + ns - 1) // ns + nsil
    cap = 6 * F
    aec = ms.AecBatch(ctx, n, rate, frame_size=F, filter_length=tail_ms * rate // 1000)
    rs = ms.ResamplerBatch(ctx, n, in_rate, rate) if in_rate else None
    o_rs = [oracle.Resampler(in_rate, rate) for _ in range(n)] if in_rate else None
    fm, fr, fo = (ms.FifoBatch(ctx, n, cap) for _ in range(3))
    m_mic, m_ref, m_out = NpFifo(n), NpFifo(n), NpFifo(n)
    legs = [Leg(oracle, rate, F, tail_ms, m) for m, _, _ in FIFO_LEGS]
    mic, far, rlen, pend = np.zeros((n, nticks * nin), np.int16), np.zeros((n, nticks * ns), np.int16), np.full((n, nticks), ns, np.int32), []
    for s, (mode, onset, missing) in enumerate(FIFO_LEGS):
        t0 = (onset or min(sil.ONSETS)) * F // ns
        mic_s, far_s = make_echo_scene(400 + s, rate, nticks * ns)
        mic[s] = mic_s if in_rate is None else make_echo_scene(400 + s, in_rate, nticks * nin)[0]
        far[s] = far_s
        if mode in ("both", "mic"):
            mic[s, t0 * nin:(t0 + nsil) * nin] = 0
        if mode in ("both", "far"):
            if missing:
                rlen[s, t0:t0 + nsil] = 0    # (the block handed in keeps its samples: they must not be read)
            else:
                far[s, t0 * ns:(t0 + nsil) * ns] = 0
        # whole state compared at the first launch that runs a frame made of the zeros alone, and at the end of the span (at
        # 48 kHz / 512 a tick in sixteen runs no frame: the next one that does)
        pend.append({"first_silent": t0 + (F + ns - 1) // ns, "last_silent": t0 + nsil - 2} if mode != "none" else {})
    z = lambda *sh, dt=torch.int16: torch.zeros(sh, dtype=dt, device="cuda")
    cnt, tick, ok = z(n, dt=torch.uint8), z(n, ns), z(n, dt=torch.uint8)
    lv = z(n, dt=torch.int32)
    up_worst, tick_sq, tick_n = 0, np.zeros(n), np.zeros(n)
    for t in range(nticks):
        dm = torch.from_numpy(np.ascontiguousarray(mic[:, t * nin:(t + 1) * nin])).cuda()
        dr = torch.from_numpy(np.ascontiguousarray(far[:, t * ns:(t + 1) * ns])).cuda()
        rc = torch.from_numpy(np.ascontiguousarray(rlen[:, t])).cuda()
        torch.cuda.synchronize()
        if in_rate:
            aec.process_fifos_resampled(rs, dm, fm, fr, dr, fo, max_frames=2, flags=0, count_out=cnt, ref_len=rc)
            ctx.sync()
            rings, head, level = fm.snapshot()
            blk = np.zeros((n, ns), np.int16)
            for s in range(n):   # (the consumed frames still lie in the ring behind the read position: the tick's block is the last ns queued)
                end = int(head[s]) + int(level[s])
                blk[s] = rings[s, np.arange(end - ns, end) % cap]
                want = o_rs[s].process(mic[s, t * nin:(t + 1) * nin])[:ns]
                up_worst = max(up_worst, int(np.abs(blk[s].astype(int) - want.astype(int)).max()))
        else:
            aec.process_fifos(fm, dm, fr, dr, fo, tick_len=ns, max_frames=2, flags=0, count_out=cnt, ref_len=rc)
            blk = mic[:, t * ns:(t + 1) * ns]
        fo.pop(ns, tick, ok=ok, zero_fill=True)
        ctx.sync()
        g_cnt, g_tick, g_ok = cnt.cpu().numpy(), tick.cpu().numpy(), ok.cpu().numpy()
        m_mic.push(blk)
        m_ref.push(far[:, t * ns:(t + 1) * ns], rlen[:, t])
        w_cnt = np.zeros(n, np.uint8)
        for _ in range(2):
            a, aok = m_mic.pop(F)
            b, _ = m_ref.pop(F, gate=aok)
            clean = np.zeros((n, F), np.int16)
            for s in range(n):
                if aok[s]:
                    clean[s] = legs[s].feed(a[s], b[s])
                    w_cnt[s] += 1
            m_out.push(clean, aok.astype(np.int32) * F)
        np.testing.assert_array_equal(g_cnt, w_cnt, err_msg=f"tick {t}: frames run")
        w_tick, w_ok = m_out.pop(ns)
        np.testing.assert_array_equal(g_ok, w_ok, err_msg=f"tick {t}")
        for s, (mode, _, missing) in enumerate(FIFO_LEGS):
            leg, label = legs[s], f"{rate}/{F} tick {t} leg {s} ({mode}{', far-end blocks missing' if missing else ''})"
            if leg.exact:
                np.testing.assert_array_equal(g_tick[s], w_tick[s], err_msg=label)
            else:   # after adaptation: the model's queue holds the oracle's samples, the GPU's are within the tolerance
                d = (g_tick[s].astype(np.float64) - w_tick[s]) / FULL_SCALE
                tick_sq[s] += float((d * d).sum())
                tick_n[s] += d.size
            force = []
            if w_cnt[s]:
                for why in [w for w, at in pend[s].items() if t >= at]:
                    force.append(why)
                    del pend[s][why]
                if t % 25 == 24:
                    force.append("every_25")
            if t == nticks - 1:
                force.append("last")
            leg.check_state(aec, s, label, force=force)
        for f, m in ((fm, m_mic), (fr, m_ref), (fo, m_out)):
            f.levels(lv)
            ctx.sync()
            np.testing.assert_array_equal(lv.cpu().numpy(), [len(q) for q in m.q], err_msg=f"tick {t}: FIFO levels")
    assert up_worst <= 1, up_worst
    for s, (mode, _, missing) in enumerate(FIFO_LEGS):
        label = f"{rate}/{F} leg {s} ({mode})"
        legs[s].verified.pop("every_25", None)
        legs[s].finish(aec, s, label)
        if tick_n[s]:
            assert np.sqrt(tick_sq[s] / tick_n[s]) <= 1e-4, (label, np.sqrt(tick_sq[s] / tick_n[s]))
    assert fm.overflows() + fr.overflows() + fo.overflows() == 0
    for o in (aec, fm, fr, fo) + ((rs,) if rs else ()):
        o.close()


@pytest.mark.parametrize("rate,F", [(8000, 64), (16000, 128), (48000, 256), (48000, 512)])
def test_silence_bit_exact_fifo_entry(ctx, oracle, rate, F):
    """mi_aec_process_fifos: the zeros arrive as 10 ms blocks of zeros, or -- the far end of four legs -- as no blocks at
    all, where the canceller injects the silence itself (speexec.c:261-272).  What the output queue delivers every tick, the
    three queues' levels and the canceller's state == the oracle fed the frames the framing model pops."""
    run_fifos(ctx, oracle, rate, F, 128)


@pytest.mark.parametrize("in_rate,rate,F", [(16000, 48000, 256), (8000, 16000, 128)])
def test_silence_bit_exact_resampler_folded_launch(ctx, oracle, in_rate, rate, F):
    """mi_aec_process_fifos_resampled: the microphone's zeros arrive at the resampler's input rate and reach the canceller
    as exact zeros once its 47 samples of history have drained (re-asserted: the oracle's E goes subnormal)"""
    run_fifos(ctx, oracle, rate, F, 128, in_rate=in_rate)


def test_silence_at_4096_legs(ctx, oracle):
    """4 096 legs at 48 kHz / 256, device-resident, seven scenes tiled over the batch (three of them silent on both pins
    from frame 6 / 8 / 10 on, one on the microphone, one on the far end, two never): legs on the same scene give the same
    bytes wherever they sit, frame after frame, and sampled legs -- first, last, one per XCD stride and more -- equal the
    oracle bit for bit, outputs every frame and the whole state at the checkpoints"""
    torch = pytest.importorskip("torch")
    rate, F, tail_ms, n, nsc = 48000, 256, 128, 4096, 7
    scenes = [("both", 6), ("none", 0), ("both", 8), ("mic", 6), ("both", 10), ("far", 10), ("none", 0)]
    nsil = sil.silent_frames(rate, F, sil.SILENT_S)
    aec = ms.AecBatch(ctx, n, rate, frame_size=F, filter_length=tail_ms * rate // 1000)
    data, legs = [], [Leg(oracle, rate, F, tail_ms, m) for m, _ in scenes]
    for k, (mode, onset) in enumerate(scenes):
        act = onset or min(sil.ONSETS)
        mic, far, span = sil.silence_scene(500 + k, rate, F, act, sil.SILENT_S, TOTAL_ACTIVE - act, mode)
        data.append((mic.reshape(-1, F), far.reshape(-1, F), span if mode != "none" else None))
    total = TOTAL_ACTIVE + nsil
    idx = torch.from_numpy(np.arange(n) % nsc).cuda()
    d_mic = torch.from_numpy(np.stack([d[0] for d in data])).cuda()   # [scene, frame, F]
    d_far = torch.from_numpy(np.stack([d[1] for d in data])).cuda()
    picks = (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 512, 1001, 1024, 1536, 2050, 2560, 3072, 3333, 3584, 4088, 4094, 4095)
    assert {p % nsc for p in picks} == set(range(nsc))
    out = torch.zeros((n, F), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for f in range(total):
        m, r = d_mic[:, f][idx].contiguous(), d_far[:, f][idx].contiguous()
        torch.cuda.synchronize()   # torch cuts the frames out on ITS stream; the canceller runs on the context's
        aec.process(m, r, out=out, flags=0)
        ctx.sync()
        o = out.cpu().numpy()
        for k in range(nsc):
            rows = o[k::nsc]
            assert (rows == rows[:1]).all(), f"frame {f}: legs on scene {k} differ"
            note_frame(legs[k], data[k][2], f, total - 1)
            ref = legs[k].feed(data[k][0][f], data[k][1][f])
            why = set(legs[k].want)
            for p in picks:
                if p % nsc == k:
                    legs[k].want = set(why)
                    legs[k].check_output(o[p], ref, f"frame {f} leg {p} (scene {k}: {scenes[k][0]})")
                    legs[k].check_state(aec, p, f"leg {p} (scene {k}: {scenes[k][0]})")
    for k, (mode, _) in enumerate(scenes):
        legs[k].finish(aec, k, f"scene {k} ({mode})")
    aec.close()


# ---- after adaptation: 3 s active, 8 s of zeros, 3 s active

AFTER = [(rate, F, mode, pf) for rate, F in ((16000, 128), (48000, 256)) for mode in ("both", "mic", "far") for pf in (False, True)]
AFTER += [(48000, 512, "both", True), (8000, 64, "both", True)]


@pytest.mark.parametrize("rate,F,mode,postfilter", AFTER)
def test_silence_after_adaptation_within_tolerance(ctx, oracle, rate, F, mode, postfilter):
    """Four legs adapt for 3 s, get 8 s of exact zeros on the pins `mode` names, and talk again for 3 s: <= 1e-4 RMS of full
    scale against the oracle over the whole run AND in every one-second window of it (a divergence that starts at the return
    from silence must not hide behind eleven quiet seconds), the same `adapted` flag and frame counter, every GPU state word
    finite at the end of the zeros and at the end of the run, ERLE over the last half second within 0.1 dB of the oracle's.
    The worst window per case is in DESIGN 3."""
    tail_ms, ns = 128, 4
    flen = tail_ms * rate // 1000
    M = sil.blocks(rate, F, tail_ms)
    act = int(3.0 * rate / F)
    nsil = sil.silent_frames(rate, F, 8.0)
    scenes = [sil.silence_scene(600 + s, rate, F, act, 8.0, act, mode) for s in range(ns)]
    mic = np.stack([m for m, _, _ in scenes])
    far = np.stack([f for _, f, _ in scenes])
    nframes = mic.shape[1] // F
    assert nframes == 2 * act + nsil
    aec = ms.AecBatch(ctx, ns, rate, frame_size=F, filter_length=flen)
    ecs = [oracle.Echo(F, flen, rate) for _ in range(ns)]
    pps = [oracle.Preproc(F, rate, e) for e in ecs] if postfilter else None
    got, ref = np.zeros_like(mic), np.zeros_like(mic)
    flags = ms.MI_AEC_POSTFILTER if postfilter else 0
    finite = lambda s: np.isfinite(np.concatenate([aec.get(s, what, k) for what, k in sil.state_list(F, M)])).all()
    adapted_before = None
    for f in range(nframes):
        sl = slice(f * F, (f + 1) * F)
        got[:, sl] = aec.process(np.ascontiguousarray(mic[:, sl]), np.ascontiguousarray(far[:, sl]), flags=flags)
        for s in range(ns):
            o = ecs[s].cancel(mic[s, sl], far[s, sl])
            ref[s, sl] = pps[s].run(o) if postfilter else o
        if f == act - 1:
            adapted_before = [e.get("scalars", 16)[8] for e in ecs]
        if f == act + nsil - 1:
            assert all(finite(s) for s in range(ns)), "non-finite GPU state at the end of the zeros"
    if rate > 8000:   # (the 64-sample frames of 8 kHz take longer than 3 s to reach `adapted` on this scene)
        assert all(v == 1.0 for v in adapted_before), "the scene must be adapted before the zeros"
    worst = 0.0
    for s in range(ns):
        d = (got[s].astype(np.float64) - ref[s].astype(np.float64)) / FULL_SCALE
        rms = np.sqrt(np.mean(d ** 2))
        per_s = np.sqrt(np.mean(d[:len(d) // rate * rate].reshape(-1, rate) ** 2, axis=1))
        worst = max(worst, float(per_s.max()))
        print(f"\n{rate}/{F} {mode} postfilter={postfilter} leg {s}: whole run {rms:.3e}, worst second {per_s.max():.3e} (second {int(per_s.argmax())})")
        assert rms <= 1e-4, f"stream {s}: rms {rms:.3e}, max {np.abs(d).max() * FULL_SCALE}"
        assert per_s.max() <= 1e-4, f"stream {s}: second {int(per_s.argmax())}: {per_s.max():.3e} (whole run {rms:.3e})"
        sg, so = aec.get(s, "scalars", 16), ecs[s].get("scalars", 16)
        assert sg[8] == so[8], "same adaptation decision"
        assert sg[11] == so[11], "same frame counter"
        assert finite(s), "non-finite GPU state at the end of the run"
        assert ref[s, -3 * rate:].any(), "the output is not silence after the return"
        tail = slice(-rate // 2, None)
        pw = lambda v: np.mean(v[tail].astype(np.float64) ** 2) + 1e-9
        erle, erle_ref = 10 * np.log10(pw(mic[s]) / pw(got[s])), 10 * np.log10(pw(mic[s]) / pw(ref[s]))
        assert abs(erle - erle_ref) < 0.1, f"stream {s}: ERLE {erle:.2f} dB vs oracle {erle_ref:.2f} dB"
    aec.close()
