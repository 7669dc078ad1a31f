"""mi_session_create_legs (include/msmi355x_session.h): legs at their own rate and codec around one canceller rate.

The yardstick is tests/session_legs_parts.py: a twin mi_session_create session at the canceller's rate with PCM in and out,
wrapped in per-kind class batches of the existing C ABI (decoder, concealer and up-sampler in front, down-sampler and encoder
behind).  Every leg's first leg_bytes of every tick's output equals it BIT FOR BIT -- the same arithmetic on the same device,
so no tolerance applies --, a seat that has left included: the egress runs every leg every tick, as the yardstick's class
batches do.  The legs session keeps three ticks in flight; the twin runs one at a time.

The first shape is 2 conferences x 5 members with six kinds.  Five seats cannot hold six kinds, so no conference holds them
all: conference 0 holds five of them, conference 1 the sixth beside four of the others, and both mix every ratio."""
import os
import subprocess

import numpy as np
import pytest

import mediastreamer2_amd as ms
from mediastreamer2_amd import _lib
from bridge_parts import mk  # noqa: F401  (a fixture)
from session_legs_parts import JOIN, LEAVE, PCM16, PCMA, PCMU, Shape, Yardstick, fill, signals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_U8, K_A8, K_16, K_24, K_A48, K_48 = ((8000, PCMU, PCMU), (8000, PCMA, PCM16), (16000, PCM16, PCM16), (24000, PCM16, PCMU),
                                       (48000, PCMA, PCM16), (48000, PCM16, PCM16))
FIRST = dict(rate=48000, members=5, legs=[K_U8, K_A8, K_16, K_24, K_A48, K_48, K_U8, K_16, K_24, K_A8])  # ten legs: the last workgroup is partly empty
SECOND = dict(rate=16000, members=3, legs=[(8000, PCMU, PCMU), (8000, PCMA, PCMA), (16000, PCM16, PCM16)])  # 128-sample frames do not divide the tick
NT = 40


def _run(ctx, mk, oracle, shape_cfg, nticks=NT, lost=None, schedule=None, waiting=None, **cfg):
    """the legs session, three ticks in flight, against the yardstick.  schedule: {tick: [(seat, op), ...]} through
    change_members with three ticks in flight; waiting: {tick: fn(session or yardstick)} with everything collected first.
    Returns the session's ticks; asserts each equal to the yardstick's on every leg's own bytes"""
    shape = Shape(shape_cfg["legs"], shape_cfg["rate"])
    plc = lost is not None
    se = mk(ms.Session, shape.n, members=shape_cfg["members"], rate=shape.rate, tail_ms=32, legs=shape.legs, plc=plc, **cfg)
    yard = Yardstick(ctx, mk, shape, shape_cfg["members"], plc=plc, **cfg)
    assert se.tick_bytes()[0] == shape.mic_pitch and se.tick_bytes()[2] == shape.out_pitch
    sig = signals(oracle, shape, nticks, echo=not cfg.get("ref_loopback"))
    rng = np.random.default_rng(3)
    want, got = [], []
    for t in range(nticks):
        if waiting and t in waiting:
            while se.in_flight():
                got.append(se.collect().copy())
            waiting[t](se)
            waiting[t](yard)
        if schedule and t in schedule:
            assert se.in_flight() == 3
            se.change_members(schedule[t])
            yard.change_members(schedule[t])
        if se.in_flight() == 3:
            got.append(se.collect().copy())
        x, ref = fill(se, shape, sig, t, rng, None if lost is None else lost[t])
        want.append(yard.tick(x, ref, None if lost is None else lost[t]))
        se.submit()
    while se.in_flight():
        got.append(se.collect().copy())
    assert len(got) == len(want) == nticks
    for t in range(nticks):
        for s in range(shape.n):
            b = int(shape.out_bytes[s])
            np.testing.assert_array_equal(got[t][s, :b], want[t][s, :b], err_msg=f"tick {t}, leg {s} {tuple(shape.legs[s])}")
            assert not got[t][s, b:].any(), f"tick {t}, leg {s}: bytes of its out row past its {b} were written"
    return shape, got


def _hears(shape, tick):
    """every leg's own bytes of a late tick are no constant row"""
    for s in range(shape.n):
        assert len(np.unique(tick[s, :int(shape.out_bytes[s])])) > 8, f"leg {s} hears nothing"


def test_six_kinds_in_a_48k_session(ctx, mk, oracle):
    shape, got = _run(ctx, mk, oracle, FIRST, agc=True, stagger=True, use_graphs=False)
    assert (shape.mic_pitch, shape.out_pitch) == (960, 960)
    _hears(shape, got[-1])


def test_three_kinds_in_a_16k_session(ctx, mk, oracle):
    shape, got = _run(ctx, mk, oracle, SECOND, agc=True, stagger=True, use_graphs=True)
    assert (shape.mic_pitch, shape.out_pitch) == (320, 320)
    _hears(shape, got[-1])


def test_one_kind_is_the_uniform_session(ctx, mk, oracle):
    """all legs 16 kHz mu-law in a 48 kHz session: mi_session_create's session bit for bit, equal tick bytes"""
    n, mm, kind = 8, 4, (16000, PCMU, PCMU)
    cfg = dict(members=mm, rate=48000, tail_ms=32, agc=True, stagger=True, use_graphs=False)
    a = mk(ms.Session, n, legs=[kind] * n, **cfg)
    b = mk(ms.Session, n, in_rate=16000, out_rate=16000, mic_codec=PCMU, out_codec=PCMU, **cfg)
    assert a.tick_bytes() == b.tick_bytes() == (160, 960, 160)
    shape = Shape([kind] * n, 48000)
    mic, ref = signals(oracle, shape, 30)
    for t in range(30):
        for se in (a, b):
            h_mic, h_ref = se.acquire()
            assert h_mic.shape == (n, 160) and h_mic.dtype == np.uint8
            h_mic[:] = np.stack([m[t * 160:(t + 1) * 160] for m in mic])
            h_ref[:] = ref[:, t * 480:(t + 1) * 480]
            se.submit()
        np.testing.assert_array_equal(a.collect(), b.collect(), err_msg=f"tick {t}")
    assert a.leg_rate(3) == 16000 and a.leg_codec(3) == (PCMU, PCMU) and a.leg_bytes(3) == (160, 160)


def test_loopback_reference_behind_a_delay_line(ctx, mk, oracle):
    shape, got = _run(ctx, mk, oracle, FIRST, agc=True, stagger=True, use_graphs=False, ref_loopback=True, ref_delay_ms=20)
    _hears(shape, got[-1])


def test_host_reference_with_graphs(ctx, mk, oracle):
    _run(ctx, mk, oracle, FIRST, agc=False, stagger=False, use_graphs=True)


def test_concealer_at_every_legs_rate(ctx, mk, oracle):
    """single losses, three in a row on an 8 kHz leg (0) and on a 48 kHz leg (5), and a loss in the first tick"""
    nt = 45
    lost = np.zeros((nt, len(FIRST["legs"])), bool)
    lost[0, 2] = lost[0, 6] = True
    for t, s in ((5, 1), (9, 3), (12, 4), (17, 7), (23, 8), (30, 9), (31, 2)):
        lost[t, s] = True
    lost[14:17, 0] = True
    lost[20:23, 5] = True
    shape, got = _run(ctx, mk, oracle, FIRST, nticks=nt, lost=lost, agc=True, stagger=True, use_graphs=False)
    _hears(shape, got[-1])


@pytest.mark.parametrize("plc, graphs", [(False, False), (True, False), (False, True)], ids=["no-plc", "plc", "graphs"])
def test_membership_with_three_ticks_in_flight_then_the_waiting_calls(ctx, mk, oracle, plc, graphs):
    """JOIN and LEAVE on legs of three kinds (8 kHz mu-law 0, 16 kHz PCM 2, 48 kHz A-law 4) through change_members, then
    remove_member / add_member / reset_streams; the seats that have left are compared like every other, unmasked"""
    schedule = {4: [(0, LEAVE)], 6: [(2, JOIN), (4, LEAVE)], 9: [(0, JOIN)], 12: [(4, JOIN), (2, LEAVE)], 15: [(2, JOIN)]}
    waiting = {20: lambda x: x.remove_member(3), 24: lambda x: (x.remove_member(7), x.add_member(3)), 28: lambda x: x.reset_streams(8, 2),
               31: lambda x: x.add_member(7)}
    lost = None
    if plc:  # (a re-seated leg's concealer starts over: losses around the changes)
        lost = np.zeros((50, len(FIRST["legs"])), bool)
        for t, s in ((3, 0), (8, 2), (10, 0), (13, 4), (16, 2), (25, 3), (29, 8), (33, 7)):
            lost[t, s] = True
    shape, got = _run(ctx, mk, oracle, FIRST, nticks=50, lost=lost, schedule=schedule, waiting=waiting, agc=True, stagger=True, use_graphs=graphs,
                      ref_loopback=True, ref_delay_ms=20)
    _hears(shape, got[-1])


def test_leg_queries(ctx, mk):
    shape = Shape(FIRST["legs"], 48000)
    se = mk(ms.Session, shape.n, members=5, rate=48000, tail_ms=32, legs=shape.legs, use_graphs=False)
    for s in range(shape.n):
        assert se.leg_rate(s) == shape.rates[s] and se.leg_codec(s) == (shape.ic[s], shape.oc[s])
        assert se.leg_bytes(s) == (shape.mic_bytes[s], shape.out_bytes[s])
    L = ctx.L
    for bad in (-1, shape.n):
        assert L.mi_legs_session_rate(se.h, bad) == _lib.MI_EINVAL
        assert L.mi_legs_session_codec(se.h, bad, None, None) == _lib.MI_EINVAL
        assert L.mi_legs_session_bytes(se.h, bad, None, None) == _lib.MI_EINVAL
    with pytest.raises(ms.MiError) as e:
        ms.Session(ctx, 2, members=2, rate=48000, tail_ms=32, legs=[(8000, PCMU, PCMU), (44100, PCM16, PCM16)])
    assert e.value.code == _lib.MI_ENOTSUP and "leg 1" in str(e.value) and "44100" in str(e.value) and "48000" in str(e.value)


def test_mixed_rate_session_example_runs(tmp_path):
    """mu-law and A-law trunks and 16 kHz members in one 48 kHz session with cancellers and a looped-back reference, through
    the plain-C example: no error, every leg hears the conference, `ok`"""
    pkg, exe = os.path.join(ROOT, "mediastreamer2_amd"), tmp_path / "mixed_rate_session"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mixed_rate_session.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines[-1] == "ok", (run.stdout, run.stderr)
