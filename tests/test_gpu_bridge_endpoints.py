"""GPU parity of bridges whose endpoints sit on either side of the mix (mi_bridge_create_endpoints,
include/msmi355x_bridge.h): a leg ABOVE its conference's rate -- a 48 kHz PCM member of a 16 kHz room -- gets plumb_to_conf's
down-sampler in front of its pin and the up-sampler behind it, inside the bridge's one launch per tick, next to legs at and
below the mix.

The yardstick is the parts on the C ABI -- mi_g711_decode once per law -> mi_volume_process (a batch per leg rate) ->
mi_resampler_process_masked (leg -> conference) -> mi_mixer_process -> mi_resampler_process_masked (conference -> leg) ->
mi_g711_encode once per law -- and every comparison with it is BIT-EXACT over all legs, samples and ticks: output bytes,
mi_volume_state bytes, meter maxima.  Against the oracle chain the meters are bit-exact and the audio is held to the float
resampler path's tolerance (tests/test_gpu_resample.py): 1e-4 RMS of full scale and at most 1 LSB."""
import os
import subprocess

import numpy as np
import pytest

import mediastreamer2_amd as ms
from bridge_parts import FLOAT_STATE, INT_STATE, Parts, mk  # noqa: F401 (mk: a fixture)
from bridge_parts import bits as _bits
from bridge_parts import one_tick as _one_tick
from bridge_parts import pair as _pair
from conftest import synth_pcm
from mediastreamer2_amd import _lib

pytestmark = pytest.mark.gpu

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


MIXED16 = [(8000, PCMU, PCMU), (8000, PCMA, PCMA), (16000, PCM16, PCM16), (48000, PCM16, PCM16)]  # in a 16 kHz conference
CASES = {
    "16k-in-8k": (8000, [(16000, PCM16, PCM16)]),
    "48k-in-16k": (16000, [(48000, PCM16, PCM16)]),
    "48k-in-8k": (8000, [(48000, PCM16, PCM16)]),
    "mixed-in-16k": (16000, MIXED16),
    "16k-alaw-ulaw-in-8k": (8000, [(16000, PCMA, PCMU)]),
}


def _legs(case, n):
    conf, turn = CASES[case]
    return conf, [turn[s % len(turn)] for s in range(n)]


@pytest.mark.parametrize("nconf", [1, 9])
@pytest.mark.parametrize("mm", [3, 9])
@pytest.mark.parametrize("case", list(CASES))
def test_equal_to_the_parts(ctx, mk, case, mm, nconf):
    """ratios 2, 3 and 6 above the mix (the 287-sample in-history of ratio 6 takes a wave more than one staging pass); legs
    below, at and above one 16 kHz mix with both laws; the up-sampler's result through an encoder.  3 members leave a wave
    idle, 9 give a wave a second and a third member on one scratch.  8 ticks reuse every staging slot and carry the
    histories; AGC and DC removal on, an inactive pin, an input gain != 1, a pin with its output off (moved to another pin
    half way: both out_resamplers must have kept their state while off), a seeded fifth of the legs absent per tick"""
    n, nticks = mm * nconf, 8
    conf, legs = _legs(case, n)
    br = mk(ms.Bridge, n, members=mm, rate=conf, endpoints=legs)
    parts = _pair(br, ctx, mk, mm, conf, legs)
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    br.set_volume_params([p] * n)
    parts.set_params([p] * n)
    parts.flags[1] = L | O
    parts.flags[2] = L | A
    parts.gain[0] = 0.7
    parts.gain[n - 1] = 1.6
    br.set_controls(flags=parts.flags, gain=parts.gain)
    parts.set_controls()
    rng = np.random.default_rng(0xE2D90 + mm)
    for t in range(nticks):
        if t == nticks // 2:
            parts.flags[2], parts.flags[0] = L | A | O, L | A
            br.set_controls(flags=parts.flags)
            parts.set_controls()
        x = parts.rows(rng)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        got, want = _one_tick(br, x, present), parts.tick(x, present)
        np.testing.assert_array_equal(got, want, err_msg=f"tick {t}")
    parts.check_state(br)


def test_membership_and_reset(ctx, mk):
    """a 48 kHz member of a 16 kHz conference removed at tick 2 and added back at tick 5, reset_streams on another at tick 4:
    the parts with both resamplers and the meter restarted at those ticks; the removed row reads zeros over the whole pitch"""
    mm, conf = 3, 16000
    legs = [MIXED16[3], MIXED16[0], MIXED16[3], MIXED16[2], MIXED16[3], MIXED16[1]]
    n = len(legs)
    br = mk(ms.Bridge, n, members=mm, rate=conf, endpoints=legs)
    parts = _pair(br, ctx, mk, mm, conf, legs)
    rng = np.random.default_rng(0x3E3C)
    gone, off, on = 2, 2, 5
    for t in range(9):
        present = np.ones(n, np.uint8)
        if t == 4:
            br.reset_streams(4, 1)
            parts.restart(4)
        if t == off:
            br.remove_member(gone)
            parts.flags[gone] = 0
            parts.set_controls()
            parts.held[:, gone] = 0
            assert br.member_count(gone // mm) == mm - 1
        if off <= t < on:
            present[gone] = 0  # nobody sends on a pin that is not plumbed
        if t == on:
            br.add_member(gone)
            parts.flags[gone] = L | A | O
            parts.set_controls()
            parts.restart(gone)
        x = parts.rows(rng)
        got = _one_tick(br, x, present)
        np.testing.assert_array_equal(got, parts.tick(x, present), err_msg=f"tick {t}")
        assert got.shape[1] == 960 and got[gone].any() == (not off <= t < on), t
    parts.check_state(br)


def test_three_ticks_in_flight(ctx, mk):
    """the mixed bridge submitted three deep returns the rows of the same ticks submitted one at a time"""
    mm, n, nticks = 4, 8, 7
    conf, legs = _legs("mixed-in-16k", n)
    deep, single = mk(ms.Bridge, n, members=mm, rate=conf, endpoints=legs), mk(ms.Bridge, n, members=mm, rate=conf, endpoints=legs)
    rng = np.random.default_rng(11)
    xs = [rng.integers(0, 256, (n, 960), dtype=np.uint8) for _ in range(nticks)]
    want = [_one_tick(single, x) for x in xs]
    got = []
    for x in xs:
        if deep.in_flight() == 3:
            got.append(deep.collect().copy())
        h_in, _ = deep.acquire()
        h_in[:] = x
        deep.submit()
    assert deep.in_flight() == 3
    while deep.in_flight():
        got.append(deep.collect().copy())
    for t in range(nticks):
        np.testing.assert_array_equal(got[t], want[t], err_msg=f"tick {t}")
    assert bytes(deep.volume_state()) == bytes(single.volume_state())


@pytest.mark.parametrize("leg,conf", [(48000, 16000), (16000, 8000)])
def test_against_the_oracle_chain(ctx, mk, oracle, leg, conf):
    """per leg g711_decode -> Volume.chunk -> Resampler(leg, conf) -> mixer_tick -> Resampler(conf, leg); three members,
    mu-law in, PCM16 out, 12 ticks: the meters bit-exact, the audio within 1e-4 RMS of full scale and 1 LSB.
    Measured: 48 kHz in 16 kHz and 16 kHz in 8 kHz are printed by this test and kept in LOG.md"""
    n, ll, ns, nticks = 3, leg // 100, conf // 100, 12
    br = mk(ms.Bridge, n, members=n, rate=conf, endpoints=[(leg, PCMU, PCM16)] * n)
    vol = [oracle.Volume(leg) for _ in range(n)]
    mx = [oracle.Extremum(1000) for _ in range(n)]
    res_in = [oracle.Resampler(leg, conf) for _ in range(n)]
    res_out = [oracle.Resampler(conf, leg) for _ in range(n)]
    sig = np.stack([synth_pcm(40 + s, ll * nticks, sigma=3000.0, rate=leg) for s in range(n)])
    err2, cnt, worst = 0.0, 0, 0
    for t in range(nticks):
        x = oracle.g711_encode(ms.MI_LAW_PCMU, sig[:, t * ll:(t + 1) * ll])
        got = np.ascontiguousarray(_one_tick(br, x)[:, :2 * ll]).view(np.int16)
        pcm = oracle.g711_decode(ms.MI_LAW_PCMU, x)
        narrow = np.zeros((n, ns), np.int16)
        for s in range(n):
            lev = vol[s].chunk(pcm[s])
            mx[s].record_max(10 * t, vol[s].v.energy)
            narrow[s] = res_in[s].process(lev)[:ns]
        mix, _ = oracle.mixer_tick(narrow)
        want = np.stack([res_out[s].process(mix[s])[:ll] for s in range(n)])
        d = got.astype(np.float64) - want
        err2, cnt, worst = err2 + float((d * d).sum()), cnt + d.size, max(worst, int(np.abs(d).max()))
    rms = np.sqrt(err2 / cnt) / 32768.0
    print(f"bridge {leg} in {conf} vs oracle chain: rms {rms:.3e} of full scale, max |diff| {worst}")
    assert rms <= 1e-4 and worst <= 1, f"rms {rms:.3e} of full scale, max |diff| {worst} LSB"
    st, bmx = br.volume_state(), br.volume_max()
    for s in range(n):
        for name in FLOAT_STATE:
            assert _bits(getattr(st[s], name)) == _bits(getattr(vol[s].v, name)), (s, name)
        for name in INT_STATE:
            assert getattr(st[s], name) == getattr(vol[s].v, name), (s, name)
        assert _bits(bmx[s]) == _bits(mx[s].current), (s, "max")


def test_geometry(ctx, mk):
    """the pitch is the widest leg's tick in bytes and may exceed the conference's own; a leg's own bytes are audio, the
    tails past them stay the zeros of creation on the device rows (what collect() hands out is their download)"""
    legs = [(8000, PCMU, PCMU), (16000, PCM16, PCM16), (48000, PCM16, PCM16)] * 2
    br = mk(ms.Bridge, 6, members=3, rate=16000, endpoints=np.array(legs, np.int32))
    assert br.tick_bytes() == (960, 960)
    assert [br.leg_bytes(s) for s in range(3)] == [(80, 80), (320, 320), (960, 960)]
    assert [br.leg_rate(s) for s in range(6)] == [l[0] for l in legs]
    assert [br.leg_codec(s) for s in range(6)] == [l[1:] for l in legs]
    with pytest.raises(ms.MiError):
        br.leg_rate(6)
    parts = Parts(ctx, mk, 3, 16000, legs)
    rng = np.random.default_rng(0x6E0)
    for t in range(4):
        x = parts.rows(rng)
        got = _one_tick(br, x)
        np.testing.assert_array_equal(got, parts.tick(x), err_msg=f"tick {t}")
        for s in range(6):
            own = br.leg_bytes(s)[1]
            assert got[s, :own].any() and not got[s, own:].any(), (t, s)
            assert br.leg_out(got, s).shape == (legs[s][0] // 100,)


@pytest.mark.parametrize("conf,legs", [(16000, [(8000, PCMA, PCMU)] * 6),
                                       (16000, [(8000, PCMU, PCMU), (8000, PCMA, PCMA), (16000, PCM16, PCM16), (8000, PCMA, PCMU),
                                                (16000, PCM16, PCMA), (16000, PCM16, PCM16)])], ids=["uniform", "mixed-codecs"])
def test_no_leg_above_is_the_legs_bridge(ctx, mk, conf, legs):
    """endpoints= with no leg above the mix is legs=: the same tick_bytes, 6 ticks and the meter state bit for bit (the
    uniform shape runs mi_bridge_create_rated's kernel, the other bridge_legs_kernel)"""
    n, mm = 6, 3
    old, new = mk(ms.Bridge, n, members=mm, rate=conf, legs=legs), mk(ms.Bridge, n, members=mm, rate=conf, endpoints=legs)
    assert new.tick_bytes() == old.tick_bytes()
    assert [new.leg_bytes(s) for s in range(n)] == [old.leg_bytes(s) for s in range(n)]
    p = ms.VolumeBatch.default_params()
    p.agc_enabled = 1
    old.set_volume_params([p] * n)
    new.set_volume_params([p] * n)
    rng = np.random.default_rng(0x5A3E)
    for t in range(6):
        x = rng.integers(0, 256, (n, old.tick_bytes()[0]), dtype=np.uint8)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        np.testing.assert_array_equal(_one_tick(new, x, present), _one_tick(old, x, present), err_msg=f"tick {t}")
    assert bytes(new.volume_state()) == bytes(old.volume_state())
    np.testing.assert_array_equal(new.volume_max().view(np.uint32), old.volume_max().view(np.uint32))


def test_endpoints_none_is_the_plain_bridge(ctx, mk):
    kw = dict(members=3, rate=8000, in_codec=PCMA, out_codec=PCMU)
    plain, none = mk(ms.Bridge, 6, **kw), mk(ms.Bridge, 6, endpoints=None, **kw)
    assert none.tick_bytes() == plain.tick_bytes() == (80, 80)
    rng = np.random.default_rng(5)
    for t in range(3):
        x = rng.integers(0, 256, (6, 80), dtype=np.uint8)
        np.testing.assert_array_equal(_one_tick(none, x), _one_tick(plain, x), err_msg=f"tick {t}")
    assert bytes(none.volume_state()) == bytes(plain.volume_state())


def test_refusals(ctx, mk):
    def refused(values, *a, **kw):
        with pytest.raises(ms.MiError) as e:
            mk(ms.Bridge, *a, **kw)
        assert e.value.code == _lib.MI_ENOTSUP, str(e.value)
        for v in values:
            assert str(v) in str(e.value), str(e.value)

    ok8, ok16 = [(8000, PCMU, PCMU)] * 6, [(16000, PCM16, PCM16)] * 6
    refused(["leg 5 at 32000", "ratio 4"], 6, members=3, rate=8000, endpoints=ok8[:5] + [(32000, PCM16, PCM16)])
    refused(["leg 2 at 24000", "1.5"], 6, members=3, rate=16000, endpoints=ok16[:2] + [(24000, PCM16, PCM16)] + ok16[3:])
    refused(["leg 5 at 44100"], 6, members=3, rate=8000, endpoints=ok8[:5] + [(44100, PCM16, PCM16)])
    refused(["leg 4's rate 4400"], 6, members=3, rate=8800, endpoints=[(8800, PCM16, PCM16)] * 4 + [(4400, PCM16, PCM16)] * 2)
    refused(["leg 5 names codec 7"], 6, members=3, rate=8000, endpoints=ok8[:5] + [(16000, PCMU, 7)])
    refused([16000, 48000], 6, members=3, rate=8000, endpoints=[(16000, PCM16, PCM16)] * 5 + [(48000, PCM16, PCM16)], plc=True)
    refused(["LDS", "50 members x 480 samples"], 50, members=50, rate=8000, endpoints=[(48000, PCM16, PCM16)] * 50)
    with pytest.raises(ms.MiError) as e:  # the older constructor keeps its refusal
        mk(ms.Bridge, 6, members=3, rate=8000, legs=ok8[:5] + [(16000, PCM16, PCM16)])
    assert e.value.code == _lib.MI_ENOTSUP and "leg 5 at 16000 Hz is above" in str(e.value)
    br = mk(ms.Bridge, 6, members=3, rate=8000, endpoints=ok8[:5] + [(16000, PCM16, PCM16)])  # the context is usable afterwards
    assert _one_tick(br, np.zeros((6, 320), np.uint8)).shape == (6, 320)


def test_plc_with_one_rate_above_the_mix(ctx, mk):
    """plc with every leg at one rate and one pair, 16 kHz mu-law in and A-law out in an 8 kHz conference: mi_plc_process at
    the legs' rate behind the decoder, in front of the parts; lost ticks concealed"""
    mm, n, conf, nticks = 3, 6, 8000, 8
    legs = [(16000, PCMU, PCMA)] * n
    br = mk(ms.Bridge, n, members=mm, rate=conf, endpoints=legs, plc=True)
    parts = _pair(br, ctx, mk, mm, conf, legs, plc=True)
    lost = {1: {2}, 4: {4, 5, 6}}
    rng = np.random.default_rng(21)
    for t in range(nticks):
        x = parts.rows(rng)
        present = np.array([0 if t in lost.get(s, ()) else 1 for s in range(n)], np.uint8)
        np.testing.assert_array_equal(_one_tick(br, x, present), parts.tick(x, present), err_msg=f"tick {t}")
    parts.check_state(br)


def test_wideband_room_example_runs(tmp_path):
    """300 ticks of 384 legs -- mu-law trunks, 16 kHz and 48 kHz PCM members in 16 kHz conferences -- through the plain-C
    example; it checks its own row sizes and return codes"""
    pkg, exe = os.path.join(ROOT, "mediastreamer2_amd"), tmp_path / "wideband_room"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "wideband_room.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", (run.stdout, run.stderr)
