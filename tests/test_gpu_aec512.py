"""The canceller at 512-sample frames: what MSSpeexEC's 2^k sizing (speexec.c:171-180) gives at 48 kHz with a frame-size
setting of 86 to 170 (MS_ECHO_CANCELLER_SET_FRAMESIZE, e.g. 128) and at 96 kHz with the default 64.  The kernel is
aec_tick_kernel<512, MODE> (one wavefront per leg, 8 bins and 8 samples per lane); it is held to the oracle's restatement of
the library (generic kiss FFT 4.4.4.4.2) as tests/test_gpu_aec.py holds the 256-sample form, then through the FIFO entries,
the state blob, a batch of 4 096 legs and the plugin (MSSpeexEC on its own bank, and inside the fused sending leg)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import mediastreamer2_amd as ms
from mediastreamer2_amd import _lib
from conftest import synth_pcm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fused_graph as fg  # noqa: E402
from test_gpu_aec import _run_pair, make_echo_scene  # noqa: E402

pytestmark = pytest.mark.gpu
F = 512
FULL_SCALE = 32768.0
PKG = os.path.join(fg.ROOT, "mediastreamer2_amd")
EC_SET_FRAMESIZE = fg.IDS["MS_ECHO_CANCELLER_SET_FRAMESIZE"]


def test_fft_1024_point_bit_exact(ctx, oracle):
    """the in-LDS real transform of 1 024 points (complex 512 = 2 x 4 x 4 x 4 x 4, the two deepest stages in registers) ==
    the kiss_fft float build restated in the oracle, forward and inverse, impulse and zero frames included"""
    torch = pytest.importorskip("torch")
    L = _lib.load()
    L.mi_debug_fft.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    aec = ms.AecBatch(ctx, 1, 48000, frame_size=F, filter_length=4 * F)
    N, nfr = 2 * F, 6
    x = np.random.default_rng(3).normal(0, 3000, (nfr, N)).astype(np.float32)
    x[1] = 0
    x[2, :] = 0
    x[2, 5] = 1.0
    d = torch.from_numpy(x).cuda()
    o = torch.zeros_like(d)
    assert L.mi_debug_fft(aec.h, d.data_ptr(), o.data_ptr(), nfr, 0) == 0
    ctx.sync()
    spec = o.cpu().numpy()
    for i in range(nfr):
        ref = oracle.ms_fft(x[i])
        got = np.empty(N, np.float32)
        got[0], got[N - 1] = spec[i, 0], spec[i, 1]
        got[1:N - 1] = spec[i, 2:]
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=f"fwd frame {i}")
    t = torch.zeros_like(d)
    assert L.mi_debug_fft(aec.h, o.data_ptr(), t.data_ptr(), nfr, 1) == 0
    ctx.sync()
    back = t.cpu().numpy()
    for i in range(nfr):
        ref = oracle.ms_ifft(oracle.ms_fft(x[i]))
        np.testing.assert_array_equal(back[i].view(np.uint32), ref.view(np.uint32), err_msg=f"inv frame {i}")
    aec.close()


@pytest.mark.parametrize("rate,tail_ms", [(48000, 128), (96000, 128), (48000, 682)])  # 682 ms at 48 kHz: M = 64 blocks
def test_mdf_512_bit_exact_before_adaptation(ctx, oracle, rate, tail_ms):
    nframes = 12
    aec, ecs, mic, far, got, ref = _run_pair(ctx, oracle, rate, F, tail_ms, 3, nframes, postfilter=False)
    M = (tail_ms * rate // 1000 + F - 1) // F
    if tail_ms == 682:
        assert M == 64
    N = 2 * F
    for s in range(3):
        sc_g, sc_o = aec.get(s, "scalars", 16), ecs[s].get("scalars", 16)
        assert sc_o[8] == 0, "scene adapted too early for this test"
        np.testing.assert_array_equal(got[s], ref[s], err_msg=f"stream {s} output")
        np.testing.assert_array_equal(sc_g.view(np.uint32), sc_o.view(np.uint32), err_msg=f"scalars {s}")
        for what, n in (("W", M * N), ("foreground", M * N), ("X", (M + 1) * N), ("E", N), ("power", F + 1),
                        ("power_1", F + 1), ("Eh", F + 1), ("Yh", F + 1), ("last_y", N)):
            np.testing.assert_array_equal(aec.get(s, what, n).view(np.uint32), ecs[s].get(what, n).view(np.uint32),
                                          err_msg=f"stream {s} {what}")
    assert not np.array_equal(got, mic)
    aec.close()


@pytest.mark.parametrize("rate,postfilter", [(48000, False), (48000, True), (96000, False), (96000, True)])
def test_aec_512_two_seconds_within_tolerance(ctx, oracle, rate, postfilter):
    """2 s from zero state: RMS error <= 1e-4 of full scale (the bar the 256-sample form is held to), the same adaptation
    decisions, and the canceller cancels"""
    nframes = int(2.0 * rate / F)
    ns = 3
    aec, ecs, mic, far, got, ref = _run_pair(ctx, oracle, rate, F, 128, ns, nframes, postfilter)
    for s in range(ns):
        d = got[s].astype(np.float64) - ref[s].astype(np.float64)
        rms = np.sqrt(np.mean(d ** 2)) / FULL_SCALE
        assert rms <= 1e-4, f"stream {s}: rms {rms:.3e}, max {np.abs(d).max()}"
        sg, so = aec.get(s, "scalars", 16), ecs[s].get("scalars", 16)
        assert sg[8] == so[8] == 1.0, "both must have reached the adapted state"
        assert sg[11] == so[11] == nframes
        tail = slice(-rate // 2, None)
        pw = lambda v: np.mean(v[tail].astype(np.float64) ** 2) + 1e-9
        erle, erle_ref = 10 * np.log10(pw(mic[s]) / pw(got[s])), 10 * np.log10(pw(mic[s]) / pw(ref[s]))
        assert erle > (12.0 if postfilter else 6.0), f"stream {s}: ERLE {erle:.1f} dB"
        assert abs(erle - erle_ref) < 0.1, f"stream {s}: ERLE {erle:.2f} dB vs oracle {erle_ref:.2f} dB"
    aec.close()


def test_tick_form_512_equals_frame_by_frame(ctx):
    """mi_aec_process_frames at F = 512 (0, 1 or 2 frames per leg and launch: 96 kHz ticks carry 1 or 2) == the same frames
    through mi_aec_process one by one: outputs and every state array bit for bit, through adaptation, a saturating burst
    and far-end overloads that reset the canceller in the first or the second frame of a launch"""
    torch = pytest.importorskip("torch")
    rate, n, nticks, tail_ms = 96000, 5, 120, 128
    flen = tail_ms * rate // 1000
    a_tick = ms.AecBatch(ctx, n, rate, frame_size=F, filter_length=flen)
    a_ref = ms.AecBatch(ctx, n, rate, frame_size=F, filter_length=flen)
    rng = np.random.default_rng(17)
    total = 2 * nticks
    scenes = [make_echo_scene(40 + s, rate, F * total) for s in range(n)]
    mic = np.stack([m for m, _ in scenes]).reshape(n, total, F)
    far = np.stack([f for _, f in scenes]).reshape(n, total, F)
    mic[2, 40:43] = 32767
    far[3, 60] = np.where(np.arange(F) % 2 == 0, 32767, -32767)
    far[4, 81] = np.where(np.arange(F) % 2 == 0, 32767, -32767)
    pos = np.zeros(n, int)
    M = (flen + F - 1) // F
    for t in range(nticks):
        cnt = rng.integers(0, 3, n).astype(np.uint8)
        cnt[0], cnt[1] = 2, 1
        m2 = np.zeros((n, 2 * F), np.int16)
        f2 = np.zeros((n, 2 * F), np.int16)
        for s in range(n):
            for k in range(int(cnt[s])):
                m2[s, k * F:(k + 1) * F] = mic[s, pos[s] + k]
                f2[s, k * F:(k + 1) * F] = far[s, pos[s] + k]
        dm, df, dc = torch.from_numpy(m2).cuda(), torch.from_numpy(f2).cuda(), torch.from_numpy(cnt).cuda()
        out_t = torch.zeros_like(dm)
        torch.cuda.synchronize()
        a_tick.process_frames(dm, df, out_t, dc, max_frames=2)
        out_r = torch.zeros_like(dm)
        torch.cuda.synchronize()
        for k in range(2):
            run = torch.from_numpy((cnt > k).astype(np.uint8)).cuda()
            mk, fk = dm[:, k * F:(k + 1) * F].contiguous(), df[:, k * F:(k + 1) * F].contiguous()
            ok = torch.zeros_like(mk)
            torch.cuda.synchronize()
            a_ref.process(mk, fk, out=ok, run=run)
            ctx.sync()
            out_r[:, k * F:(k + 1) * F] = torch.where(run[:, None].bool(), ok, out_r[:, k * F:(k + 1) * F])
        ctx.sync()
        torch.cuda.synchronize()
        got, ref = out_t.cpu().numpy(), out_r.cpu().numpy()
        for s in range(n):
            w = int(cnt[s]) * F
            assert np.array_equal(got[s, :w], ref[s, :w]), f"tick {t} stream {s} ({cnt[s]} frames)"
        pos += cnt.astype(int)
        if t % 30 == 29:
            for s in range(n):
                for what, ln in (("W", M * 2 * F), ("foreground", M * 2 * F), ("X", (M + 1) * 2 * F), ("E", 2 * F), ("power", F + 1),
                                 ("power_1", F + 1), ("Eh", F + 1), ("Yh", F + 1), ("last_y", 2 * F), ("prop", M), ("scalars", 16)):
                    x, y = a_tick.get(s, what, ln), a_ref.get(s, what, ln)
                    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"tick {t} stream {s}: {what}"
    assert any(a_tick.get(s, "scalars", 16)[8] == 1.0 for s in range(n)), "the scene should take a stream through adaptation"
    assert a_tick.get(3, "counters", 4)[2] >= 1, "the far-end overload must have reset stream 3"
    a_tick.close()
    a_ref.close()


@pytest.mark.parametrize("rate", [48000, 96000])
def test_fifo_entry_512_equals_the_separate_launches(ctx, rate):
    """mi_aec_process_fifos at F = 512 (48 kHz: 0 or 1 frame per 480-sample tick; 96 kHz: 1 or 2 per 960-sample tick) ==
    mi_fifo_push x 2, mi_fifo_pop_frames x 2, mi_aec_process_frames, mi_fifo_push_frames: FIFO levels, what the output FIFO
    delivers and the canceller's state, bit for bit -- far-end blocks missing or short of any length, a delay line of silence"""
    torch = pytest.importorskip("torch")
    n, ns, nticks, tail = 12, rate // 100, 60, 128
    cap = 4 * F
    flen = tail * rate // 1000
    M = (flen + F - 1) // F
    rng = np.random.default_rng(rate + 512)
    mic = np.stack([synth_pcm(200 + s, ns * nticks, rate=rate, sigma=2500.0) for s in range(n)])
    ref = np.stack([synth_pcm(300 + s, ns * nticks, rate=rate, sigma=3000.0) for s in range(n)])
    z = lambda *sh, dt=torch.int16: torch.zeros(sh, dtype=dt, device="cuda")

    def rig():
        a = ms.AecBatch(ctx, n, rate, frame_size=F, filter_length=flen)
        fm, fr, fo = (ms.FifoBatch(ctx, n, cap) for _ in range(3))
        delay = z(n, 2 * F)
        gate = torch.from_numpy((np.arange(n) % 3 == 0).astype(np.uint8)).cuda()
        torch.cuda.synchronize()
        fr.push(delay, nsamples=F + 32, gate=gate)
        return a, fm, fr, fo

    a1, fm1, fr1, fo1 = rig()
    a2, fm2, fr2, fo2 = rig()
    micf, reff, clean, cnt = z(n, 2 * F), z(n, 2 * F), z(n, 2 * F), z(n, dt=torch.uint8)
    cnt2 = z(n, dt=torch.uint8)
    t1, t2, ok1, ok2 = z(n, ns), z(n, ns), z(n, dt=torch.uint8), z(n, dt=torch.uint8)
    lv1, lv2 = z(n, dt=torch.int32), z(n, dt=torch.int32)
    seen = set()
    for t in range(nticks):
        dm = torch.from_numpy(np.ascontiguousarray(mic[:, t * ns:(t + 1) * ns])).cuda()
        dr = torch.from_numpy(ref[:, t * ns:(t + 1) * ns].copy()).cuda()
        skip = rng.random(n) < 0.15
        short = rng.integers(1, ns, n)
        rc = torch.from_numpy(np.where(skip, 0, np.where(rng.random(n) < 0.2, short, ns)).astype(np.int32)).cuda()
        torch.cuda.synchronize()
        fm1.push(dm)
        fr1.push(dr, nsamples=ns, count=rc)
        fm1.pop_frames(F, 2, micf, nframes_out=cnt)
        fr1.pop_frames(F, 2, reff, wanted=cnt, zero_fill=True)
        a1.process_frames(micf, reff, clean, cnt, max_frames=2)
        fo1.push_frames(clean, F, 2, cnt)
        fo1.pop(ns, t1, ok=ok1, zero_fill=True)
        a2.process_fifos(fm2, dm, fr2, dr, fo2, tick_len=ns, max_frames=2, count_out=cnt2, ref_len=rc)
        fo2.pop(ns, t2, ok=ok2, zero_fill=True)
        for f1, f2 in ((fm1, fm2), (fr1, fr2), (fo1, fo2)):
            f1.levels(lv1)
            f2.levels(lv2)
            ctx.sync()
            np.testing.assert_array_equal(lv1.cpu().numpy(), lv2.cpu().numpy(), err_msg=f"rate {rate} tick {t}")
        ctx.sync()
        c = cnt.cpu().numpy()
        seen.update(int(v) for v in c)
        np.testing.assert_array_equal(c, cnt2.cpu().numpy())
        np.testing.assert_array_equal(ok1.cpu().numpy(), ok2.cpu().numpy())
        np.testing.assert_array_equal(t1.cpu().numpy(), t2.cpu().numpy(), err_msg=f"rate {rate} tick {t}")
    assert seen == ({0, 1} if rate == 48000 else {1, 2}), seen
    assert t2.cpu().numpy().any()
    for s_ in range(n):
        for what, ln in (("W", M * 2 * F), ("foreground", M * 2 * F), ("X", (M + 1) * 2 * F), ("E", 2 * F), ("power_1", F + 1), ("scalars", 16)):
            x, y = a1.get(s_, what, ln), a2.get(s_, what, ln)
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"rate {rate} stream {s_}: {what}"
    assert fm2.overflows() + fr2.overflows() + fo2.overflows() == 0
    for o in (a1, a2, fm1, fr1, fo1, fm2, fr2, fo2):
        o.close()


def test_resampler_folded_launch_512_equals_the_two_launches(ctx):
    """mi_aec_process_fifos_resampled at F = 512 (16 kHz -> 48 kHz: the fused sending leg's launch) == mi_resampler_process
    followed by mi_aec_process_fifos, the legs staggered as the plugin staggers them (leads below one frame)"""
    torch = pytest.importorskip("torch")
    in_rate, rate = 16000, 48000
    n, nticks, nin, ns = 37, 40, in_rate // 100, rate // 100
    flen = 128 * rate // 1000
    mic = np.stack([synth_pcm(900 + s, nin * (nticks + 2), rate=in_rate, sigma=2500.0) for s in range(n)])
    ref = np.stack([synth_pcm(950 + s, ns * nticks, rate=rate, sigma=3000.0) for s in range(n)])
    z = lambda *sh, dt=torch.int16: torch.zeros(sh, dtype=dt, device="cuda")

    def rig():
        return (ms.ResamplerBatch(ctx, n, in_rate, rate), ms.AecBatch(ctx, n, rate, frame_size=F, filter_length=flen),
                *(ms.FifoBatch(ctx, n, 4 * F) for _ in range(3)))

    (rs1, a1, fm1, fr1, fo1), (rs2, a2, fm2, fr2, fo2) = rig(), rig()
    L = _lib.load()
    unit, phases = C.c_int(), C.c_int()
    assert L.mi_aec_stagger_info(a1.h, ns, C.byref(unit), C.byref(phases)) == 0
    assert (unit.value, phases.value) == (64, 8) and unit.value * (phases.value - 1) < F
    for a, fm, fr in ((a1, fm1, fr1), (a2, fm2, fr2)):
        a.stagger_fifos(fm, fr, ns)
    up = z(n, (ns + 8 + 7) & ~7)
    t1, t2, lv1, lv2 = z(n, ns), z(n, ns), z(n, dt=torch.int32), z(n, dt=torch.int32)
    for t in range(nticks):
        dm = torch.from_numpy(np.ascontiguousarray(mic[:, t * nin:(t + 1) * nin])).cuda()
        dr = torch.from_numpy(np.ascontiguousarray(ref[:, t * ns:(t + 1) * ns])).cuda()
        torch.cuda.synchronize()
        rs1.process(dm, out=up)
        a1.process_fifos(fm1, up, fr1, dr, fo1, tick_len=ns, max_frames=2)
        a2.process_fifos_resampled(rs2, dm, fm2, fr2, dr, fo2, max_frames=2)
        fo1.pop(ns, t1, zero_fill=True)
        fo2.pop(ns, t2, zero_fill=True)
        fm1.levels(lv1)
        fm2.levels(lv2)
        ctx.sync()
        np.testing.assert_array_equal(t1.cpu().numpy(), t2.cpu().numpy(), err_msg=f"tick {t}")
        np.testing.assert_array_equal(lv1.cpu().numpy(), lv2.cpu().numpy())
    assert t1.cpu().numpy().any()
    for t in range(nticks, nticks + 2):   # the folded resampler's state went along
        dm = torch.from_numpy(np.ascontiguousarray(mic[:, t * nin:(t + 1) * nin])).cuda()
        torch.cuda.synchronize()
        o1, _ = rs1.process(dm)
        o2, _ = rs2.process(dm)
        ctx.sync()
        np.testing.assert_array_equal(o1.cpu().numpy()[:, :ns], o2.cpu().numpy()[:, :ns])
    assert fm2.overflows() + fr2.overflows() + fo2.overflows() == 0
    for o in (rs1, a1, fm1, fr1, fo1, rs2, a2, fm2, fr2, fo2):
        o.close()


def test_aec_512_state_blob_resumes_bit_for_bit(ctx):
    rate = 48000
    flen = 128 * rate // 1000
    nfr = 70
    mic, far = make_echo_scene(3, rate, F * nfr)
    a = ms.AecBatch(ctx, 2, rate, frame_size=F, filter_length=flen)
    m2, f2 = np.stack([mic, mic]), np.stack([far, far])
    fl = ms.MI_AEC_POSTFILTER
    for f in range(45):
        sl = slice(f * F, (f + 1) * F)
        a.process(np.ascontiguousarray(m2[:, sl]), np.ascontiguousarray(f2[:, sl]), flags=fl)
    blob = a.export_state(1)
    assert len(blob) == a.state_bytes() + 32
    b = ms.AecBatch(ctx, 3, rate, frame_size=F, filter_length=flen)
    b.import_state(2, blob)
    m3, f3 = np.stack([mic] * 3), np.stack([far] * 3)
    for f in range(45, nfr):
        sl = slice(f * F, (f + 1) * F)
        oa = a.process(np.ascontiguousarray(m2[:, sl]), np.ascontiguousarray(f2[:, sl]), flags=fl)
        ob = b.process(np.ascontiguousarray(m3[:, sl]), np.ascontiguousarray(f3[:, sl]), flags=fl)
        np.testing.assert_array_equal(ob[2], oa[1], err_msg=f"frame {f}")
    # a 256-sample canceller's blob does not load into a 512 one
    c = ms.AecBatch(ctx, 1, rate, frame_size=256, filter_length=flen)
    with pytest.raises(ms.MiError):
        c.import_state(0, blob)
    for x in (a, b, c):
        x.close()


def test_aec_512_at_4096_legs(ctx, oracle):
    """4 096 legs at 48 kHz / F = 512, device-resident: identical scenes give identical bytes across the batch, and legs spread
    over the batch (first, last, strides across the eight XCDs) equal the oracle"""
    torch = pytest.importorskip("torch")
    rate, n, nframes = 48000, 4096, 5
    flen = 128 * rate // 1000
    aec = ms.AecBatch(ctx, n, rate, frame_size=F, filter_length=flen)
    scenes = [make_echo_scene(s, rate, F * nframes) for s in range(8)]
    mic = np.stack([scenes[s % 8][0] for s in range(n)])
    far = np.stack([scenes[s % 8][1] for s in range(n)])
    picks = (0, 1, 7, 8, 13, 1001, 2050, 3333, 4088, 4095)
    ecs = {s: oracle.Echo(F, flen, rate) for s in picks}
    for f in range(nframes):
        sl = slice(f * F, (f + 1) * F)
        dm = torch.from_numpy(np.ascontiguousarray(mic[:, sl])).cuda()
        dr = torch.from_numpy(np.ascontiguousarray(far[:, sl])).cuda()
        o = aec.process(dm, dr, flags=0)
        ctx.sync()
        out = o.cpu().numpy()
        grp = out.reshape(n // 8, 8, F)
        assert (grp == grp[:1]).all()
        for s, e in ecs.items():
            np.testing.assert_array_equal(out[s], e.cancel(mic[s, sl], far[s, sl]), err_msg=f"frame {f} stream {s}")
    aec.close()


# ---- the plugin

@pytest.fixture(scope="module")
def host():
    import torch  # noqa: F401  (one HIP runtime per process, see mediastreamer2_amd/_lib.py)
    return fg.Host(PKG)


def speexec_512(oracle, rate, far, mic, tail_ms):
    """MSSpeexEC restated (speexec.c:188-305) at F = 512 over 10 ms ticks on both pins: reference blocks are dropped until the
    first microphone frame has been processed, every full microphone frame is cancelled against the delay line or against
    injected silence when that runs short, then the post-filter (modelled on speexec_core, tests/test_aec_tester_scenarios.py)"""
    ns = rate // 100
    e = oracle.Echo(F, tail_ms * rate // 1000, rate)
    p = oracle.Preproc(F, rate, e)
    echo_fifo, dref_fifo = np.zeros(0, np.int16), np.zeros(0, np.int16)
    started, outs = False, []
    for t in range(len(mic) // ns):
        if started:
            dref_fifo = np.concatenate([dref_fifo, far[t * ns:(t + 1) * ns]])
        echo_fifo = np.concatenate([echo_fifo, mic[t * ns:(t + 1) * ns]])
        while len(echo_fifo) >= F:
            fr, echo_fifo = echo_fifo[:F], echo_fifo[F:]
            started = True
            if len(dref_fifo) < F:
                dref_fifo = np.concatenate([dref_fifo, np.zeros(F, np.int16)])
            r, dref_fifo = dref_fifo[:F], dref_fifo[F:]
            outs.append(p.run(e.cancel(fr, r)))
    return np.concatenate(outs)


@pytest.mark.parametrize("rate,framesize", [(48000, 128), (96000, None)])
def test_speex_ec_facade_cancels_at_512(host, oracle, rate, framesize):
    """far-end + microphone sources -> MSSpeexEC -> sinks at 48 kHz with MS_ECHO_CANCELLER_SET_FRAMESIZE 128, and at 96 kHz
    with the default: both give 512-sample frames, which the filter used to pass through untouched.  The cleaned microphone
    equals the restated framing over the oracle (1e-4 RMS of full scale, as the other sizes) and is not the microphone."""
    S, tail_ms = host.S, 128
    ec = S.ms_factory_create_filter(host.fac, fg.MS_SPEEX_EC_ID)
    assert host.call_int(ec, fg.IDS["MS_FILTER_SET_SAMPLE_RATE"], rate) == 0
    assert host.call_int(ec, fg.EC_SET_TAIL, tail_ms) == 0
    assert host.call_int(ec, fg.EC_SET_DELAY, 0) == 0
    if framesize is not None:
        assert host.call_int(ec, EC_SET_FRAMESIZE, framesize) == 0
    s_ref, s_mic, k_ref, k_mic = S.ms2shim_new_source(host.fac), S.ms2shim_new_source(host.fac), S.ms2shim_new_sink(host.fac), S.ms2shim_new_sink(host.fac)
    for a, pa, b, pb in ((s_ref, 0, ec, 0), (s_mic, 0, ec, 1), (ec, 0, k_ref, 0), (ec, 1, k_mic, 0)):
        assert S.ms_filter_link(a, pa, b, pb) == 0
    ticker = S.ms_ticker_new()
    S.ms_ticker_attach(ticker, ec)
    ns = rate // 100
    nt = 200
    mic, far = make_echo_scene(11, rate, ns * nt)
    for t in range(nt):
        host.push(s_ref, far[t * ns:(t + 1) * ns])
        host.push(s_mic, mic[t * ns:(t + 1) * ns])
    for _ in range(nt + 3):
        S.ms_ticker_step(ticker)
    got, spk = host.drain(k_mic), host.drain(k_ref)
    S.ms_ticker_detach(ticker, ec)
    S.ms_ticker_destroy(ticker)
    for f in (ec, s_ref, s_mic, k_ref, k_mic):
        S.ms_filter_destroy(f)
    ref = speexec_512(oracle, rate, far, mic, tail_ms)
    assert len(got) == len(ref) > 0 and len(got) % F == 0
    assert len(spk) == len(ref)
    d = got.astype(np.float64) - ref.astype(np.float64)
    assert np.sqrt(np.mean(d ** 2)) / FULL_SCALE <= 1e-4
    assert not np.array_equal(got, mic[:len(got)])
    tail = slice(-len(got) // 4, None)
    assert np.mean(got[tail].astype(np.float64) ** 2) < 0.5 * np.mean(mic[:len(got)][tail].astype(np.float64) ** 2), "it cancels"


def run_legs_512(h, fuse, mixer, nticks=120, nconf=2, members=4):
    """MSResample 16k -> 48k -> MSSpeexEC (frame size setting 128: 512-sample frames) -> MSVolume -> [mixer] for every leg,
    run fused (the device-resident leg batch) or with MSMI355X_NO_FUSE=1 (every facade on its own bank)"""
    if fuse:
        os.environ.pop("MSMI355X_NO_FUSE", None)
    else:
        os.environ["MSMI355X_NO_FUSE"] = "1"
    os.environ.pop("MSMI355X_NO_EARLY_LAUNCH", None)
    os.environ["MSMI355X_CHECK_LEVELS"] = "1"
    try:
        conf = fg.Conferences(h, nconf, members, 16000, 48000, 128, 0, mixer=mixer, agc=mixer)
        for leg in conf.legs:
            assert h.call_int(leg["ec"], EC_SET_FRAMESIZE, 128) == 0
        n, ni, ns = nconf * members, 160, 480
        mic, far = fg.scene(n, nticks, 16000, 48000, seed=29)
        late0 = h.P.ms_mi355x_late_events()
        conf.attach()
        stats = None
        for t in range(nticks):
            for s, leg in enumerate(conf.legs):
                h.push(leg["mic"], mic[s, t * ni:(t + 1) * ni])
                h.push(leg["far"], far[s, t * ns:(t + 1) * ns])
            conf.step()
            if t == nticks // 2:
                stats = h.fused_stats()
        res = {"out": [h.drain(leg["out"]) for leg in conf.legs], "spk": [h.drain(leg["spk"]) for leg in conf.legs], "stats": stats,
               "late": h.P.ms_mi355x_late_events() - late0}
        conf.close()
        return res
    finally:
        os.environ.pop("MSMI355X_NO_FUSE", None)
        os.environ.pop("MSMI355X_CHECK_LEVELS", None)


@pytest.mark.parametrize("mixer", [True, False])
def test_fused_sending_leg_at_512_equals_its_facades(host, mixer):
    """the fused sending leg (conference members, and a plain AudioStream sending side without a mixer) with 512-sample frames:
    it really fuses (the legs are in the batch) and equals the same graph on its facades bit for bit"""
    fused = run_legs_512(host, True, mixer)
    plain = run_legs_512(host, False, mixer)
    assert fused["stats"]["legs"] > 0, fused["stats"]
    assert plain["stats"]["legs"] == 0
    assert fg.compare(fused, plain, 0, 480) == []
    assert sum(len(x) for x in fused["out"]) > 0 and any(x.any() for x in fused["out"])
    assert fused["late"] == 0 and plain["late"] == 0
