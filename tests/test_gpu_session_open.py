"""mi_session_change_members (include/msmi355x_session.h): legs join and leave a running session without a drain, the
changes applied on the device ahead of the tick that carries them.

The yardstick is the waiting path of the same build on the same device: session A collects everything in flight and calls
remove_member / add_member (a replacement is remove followed by add), session B calls change_members and keeps three ticks in
flight throughout.  Every collected tick of B equals A's bit for bit, every row; right after each call and at the end the
meters' levels, the member counts and the election agree.  40 ticks of seeded noise plus a tone per leg: at least 25 ticks
follow the last change, the cancellers are adapting, and a stale or half-written state of a seat shows in the output.

A row whose seat has left reads silence: zeros as 16-bit PCM, the code word of zero behind an encoder (mi_g711_encode writes
every row of the tick, so with out_codec the row is 0xff / 0xd5, not 0x00 -- on the waiting path too).  Behind the
down-sampler (out_rate) the first tick after the leave still carries the tail of the down-sampler's history -- on the waiting
path too, whose remove_member does not touch it; the row is compared with A's there and held to silence from the next tick on."""
import os
import subprocess

import numpy as np
import pytest

import mediastreamer2_amd as ms
from mediastreamer2_amd import _lib
from conftest import synth_pcm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOIN, LEAVE = ms.MI_SESSION_JOIN, ms.MI_SESSION_LEAVE
N, MM, NT = 16, 4, 40  # 4 conferences of 4: every stagger phase of 480-in-256 framing is occupied (checked below)

SHAPES = {
    # (a) 48 kHz in and out, AGC, stagger on, graphs on
    "a-48k-agc-stagger-graphs": dict(in_rate=48000, rate=48000, agc=True, stagger=True, use_graphs=True),
    # (b) the up-sampler folded into the canceller's launch, A-law in, mu-law out behind the down-sampler, the far end looped
    # back behind a 20 ms delay line, the concealer with lost ticks
    "b-16k-48k-pcma-8k-pcmu-loopback-plc-graphs": dict(in_rate=16000, rate=48000, agc=True, mic_codec=ms.MI_SESSION_PCMA, out_rate=8000,
                                                       out_codec=ms.MI_SESSION_PCMU, ref_loopback=True, ref_delay_ms=20, plc=True, stagger=True,
                                                       use_graphs=True),
    # (c) F = 64, mu-law both ways, the concealer, no graphs
    "c-8k-pcmu-plc-eager": dict(in_rate=8000, rate=8000, agc=True, mic_codec=ms.MI_SESSION_PCMU, out_codec=ms.MI_SESSION_PCMU, plc=True,
                                stagger=True, use_graphs=False),
    # (d) F = 128, no stagger
    "d-8k-16k-no-stagger": dict(in_rate=8000, rate=16000, agc=True, stagger=False, use_graphs=True),
    # (e) 16 -> 44.1 kHz: the resampler's own launch and its position word (tests/test_gpu_pipeline.py runs the session there)
    "e-16k-44k1-own-resampler": dict(in_rate=16000, rate=44100, agc=True, stagger=True, use_graphs=False),
}

# tick -> calls made for that tick, each (when, [(seat, op), ...]).  "filling": between acquire and submit; "full": with three
# ticks in flight and none of them collected
SCHEDULE = {
    0: [("filling", [(1, JOIN)])],                       # a JOIN on a taken seat before the first submit: no graph captured yet
    3: [("filling", [(5, LEAVE)])],
    4: [("filling", [(5, JOIN)])],                       # a CLEAR is still owed while the seat is plumbed again
    6: [("filling", [(9, LEAVE)])],                      # one seat in three consecutive ticks
    7: [("filling", [(9, JOIN)])],
    8: [("filling", [(9, LEAVE)])],                      # ... and it stays away: its row is silence to the end
    10: [("filling", [(2, LEAVE)]), ("filling", [(2, JOIN)])],  # two calls before one submit: the last one wins
    11: [("filling", [(s, LEAVE) for s in range(12, 16)])],     # every seat of conference 3 in one call
    13: [("filling", [(s, JOIN) for s in range(12, 16)])],      # ... and back two ticks later
    14: [("full", [(7, JOIN), (0, LEAVE)])],
}
assert max(SCHEDULE) + 25 < NT


def _mk(ctx, cfg):
    return ms.Session(ctx, N, members=MM, tail_ms=32, **cfg)


def _signals(oracle, cfg, seed=0):
    in_len, ln = cfg["in_rate"] // 100, cfg["rate"] // 100
    mic = np.stack([synth_pcm(seed + 40 + s, in_len * NT, rate=cfg["in_rate"], sigma=2500.0, tone_hz=400.0 + 60 * s) for s in range(N)])
    ref = np.stack([synth_pcm(seed + 500 + s, ln * NT, rate=cfg["rate"], sigma=3000.0) for s in range(N)])
    if cfg.get("mic_codec"):
        mic = oracle.g711_encode(ms.MI_LAW_PCMA if cfg["mic_codec"] == ms.MI_SESSION_PCMA else ms.MI_LAW_PCMU, mic)
    lost = np.random.default_rng(9 + seed).random((NT, N)) < (0.1 if cfg.get("plc") else 0.0)
    lost[:3] = False
    return mic, ref, lost


def _fill(se, cfg, sig, t):
    mic, ref, lost = sig
    in_len, ln = cfg["in_rate"] // 100, cfg["rate"] // 100
    h_mic, h_ref = se.acquire()
    h_mic[:] = mic[:, t * in_len:(t + 1) * in_len]
    if h_ref is not None:
        h_ref[:] = ref[:, t * ln:(t + 1) * ln]
    if cfg.get("plc"):
        se.events()[lost[t]] = ms.MI_PLC_CONCEAL


def _silence(oracle, cfg):
    if not cfg.get("out_codec"):
        return 0
    law = ms.MI_LAW_PCMA if cfg["out_codec"] == ms.MI_SESSION_PCMA else ms.MI_LAW_PCMU
    return int(oracle.g711_encode(law, np.zeros((1, 1), np.int16))[0, 0])


def _same_answers(a, b, where):
    assert [a.member_count(c) for c in range(N // MM)] == [b.member_count(c) for c in range(N // MM)], where
    np.testing.assert_array_equal(a.levels(), b.levels(), err_msg=f"get_levels {where}")
    (wa, da), (wb, db) = a.active_speakers(0), b.active_speakers(0)
    np.testing.assert_array_equal(wa, wb, err_msg=f"active_speakers {where}")
    np.testing.assert_array_equal(da, db, err_msg=f"active_speakers' level {where}")


class Waiting:
    """the yardstick's side of a change list: remove_member / add_member on a session with nothing in flight"""

    def __init__(self, se):
        self.se, self.members = se, set(range(N))

    def apply(self, changes):
        assert self.se.in_flight() == 0
        for seat, op in changes:
            if seat in self.members:
                self.se.remove_member(seat)
                self.members.discard(seat)
            if op == JOIN:
                self.se.add_member(seat)
                self.members.add(seat)


def _run_pair(ctx, oracle, cfg, schedule):
    """A by the waiting calls, one tick at a time; B by change_members, three ticks in flight.  Returns both sessions' ticks and,
    per tick, {seat: ticks since it left} for the seats that are no members in it"""
    sig = _signals(oracle, cfg)
    a, b = _mk(ctx, cfg), _mk(ctx, cfg)
    wa = Waiting(a)
    got_a, got_b, away, left_at = [], [], [], {}

    def call(changes, t):
        wa.apply(changes)
        b.change_members(changes)
        for seat, op in changes:
            if op == LEAVE:
                left_at[seat] = t
            else:
                left_at.pop(seat, None)
        _same_answers(a, b, f"after the call for tick {t}: {changes}")

    for t in range(NT):
        calls = schedule.get(t, [])
        for when, changes in calls:
            if when == "full":
                assert b.in_flight() == 3
                call(changes, t)
        if b.in_flight() == 3:
            got_b.append(b.collect().copy())
        _fill(b, cfg, sig, t)
        for when, changes in calls:
            if when == "filling":
                call(changes, t)
        b.submit()
        assert b.in_flight() == min(t + 1, 3)
        _fill(a, cfg, sig, t)
        a.submit()
        got_a.append(a.collect().copy())
        away.append({s: t - at for s, at in left_at.items()})
    while b.in_flight():
        got_b.append(b.collect().copy())
    _same_answers(a, b, "at the end")
    a.close()
    b.close()
    return got_a, got_b, away


def test_every_stagger_phase_is_occupied(ctx):
    L = ctx.L
    assert sorted({L.mi_fifo_phase_of(s, 8) for s in range(N)}) == list(range(8))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_seats_change_hands_with_three_ticks_in_flight(ctx, oracle, shape):
    cfg = SHAPES[shape]
    got_a, got_b, away = _run_pair(ctx, oracle, cfg, SCHEDULE)
    assert len(got_a) == len(got_b) == NT
    silence, tail = _silence(oracle, cfg), (1 if cfg.get("out_rate") else 0)
    for t in range(NT):
        np.testing.assert_array_equal(got_b[t], got_a[t], err_msg=f"{shape}: tick {t}")
        for seat, since in away[t].items():
            if since >= tail:
                assert (got_b[t][seat] == silence).all(), f"{shape}: tick {t}: seat {seat} left {since} ticks ago and its row is not silence"
    assert away[-1].keys() == {0, 9}
    # the members hear each other to the end, the replaced seats among them
    for seat in (1, 2, 5, 7, 12):
        assert len(np.unique(got_b[-1][seat])) > 8, f"{shape}: seat {seat} hears nothing"


def test_no_changes_change_nothing(ctx, oracle):
    cfg = SHAPES["a-48k-agc-stagger-graphs"]
    sig = _signals(oracle, cfg)
    p, q = _mk(ctx, cfg), _mk(ctx, cfg)
    for t in range(8):
        _fill(p, cfg, sig, t)
        p.change_members([])
        p.submit()
        _fill(q, cfg, sig, t)
        q.submit()
        np.testing.assert_array_equal(p.collect(), q.collect(), err_msg=f"tick {t}")
    _same_answers(p, q, "count == 0")
    p.close()
    q.close()


def test_refusals_apply_nothing(ctx, oracle):
    """each refusal returns MI_EINVAL, names the entry point, and applies nothing: the host's answers and the following ticks
    equal those of a session that never got the call -- the good entries around the bad one included"""
    cfg = SHAPES["d-8k-16k-no-stagger"]
    sig = _signals(oracle, cfg)
    p, q = _mk(ctx, cfg), _mk(ctx, cfg)
    for se in (p, q):
        se.remove_member(6)
    L = ctx.L
    t = 0

    def ticks(k):
        nonlocal t
        for _ in range(k):
            for se in (p, q):
                _fill(se, cfg, sig, t)
                se.submit()
            np.testing.assert_array_equal(p.collect(), q.collect(), err_msg=f"tick {t}")
            t += 1

    ticks(3)
    bad = [
        ([(1, JOIN), (N, LEAVE), (2, LEAVE)], f"stream {N} of {N}"),
        ([(1, JOIN), (-1, JOIN)], "stream -1"),
        ([(1, JOIN), (2, 3)], "op 3"),
        ([(2, 0), (1, JOIN)], "op 0"),
        ([(1, JOIN), (6, LEAVE), (2, LEAVE)], "stream 6 is no member"),
        ([(1, JOIN), (2, LEAVE), (1, LEAVE)], "stream 1 a second time"),
    ]
    for changes, text in bad:
        with pytest.raises(ms.MiError) as e:
            p.change_members(changes)
        assert e.value.code == _lib.MI_EINVAL and "mi_session_change_members" in str(e.value) and text in str(e.value), str(e.value)
        _same_answers(p, q, f"after the refused {changes}")
        ticks(2)
    one = np.array([[1, JOIN]], np.int32)
    assert L.mi_session_change_members(None, one.ctypes.data, 1) == _lib.MI_EINVAL
    assert L.mi_session_change_members(p.h, one.ctypes.data, -1) == _lib.MI_EINVAL
    assert L.mi_session_change_members(p.h, None, 1) == _lib.MI_EINVAL and b"mi_session_change_members" in L.mi_last_error()
    assert L.mi_session_change_members(p.h, None, 0) == _lib.MI_OK
    ticks(3)
    _same_answers(p, q, "at the end")
    p.close()
    q.close()


def test_a_waiting_call_has_the_last_word(ctx, oracle):
    """a waiting remove_member between a JOIN and the submit that carries it leaves the seat unplumbed on device and roster
    alike; a waiting add_member after a LEAVE leaves it plumbed.  Against a twin driven by the waiting calls alone"""
    cfg = SHAPES["a-48k-agc-stagger-graphs"]
    sig = _signals(oracle, cfg)
    p, q = _mk(ctx, cfg), _mk(ctx, cfg)

    def tick(t, between=lambda: None):
        _fill(p, cfg, sig, t)
        between()
        p.submit()
        _fill(q, cfg, sig, t)
        q.submit()
        out = p.collect().copy()
        np.testing.assert_array_equal(out, q.collect(), err_msg=f"tick {t}")
        return out

    for t in range(4):
        tick(t)

    def join_then_remove():
        p.change_members([(3, JOIN)])
        assert p.member_count(0) == MM
        p.remove_member(3)
        assert p.member_count(0) == MM - 1

    q.remove_member(3)
    q.add_member(3)
    q.remove_member(3)
    for t in range(4, 10):
        out = tick(t, join_then_remove if t == 4 else (lambda: None))
        assert not out[3].any() and p.member_count(0) == MM - 1
    _same_answers(p, q, "after JOIN + remove_member")

    def leave_then_add():
        p.change_members([(10, LEAVE)])
        p.add_member(10)
        assert p.member_count(2) == MM

    q.remove_member(10)
    q.add_member(10)
    for t in range(10, 16):
        out = tick(t, leave_then_add if t == 10 else (lambda: None))
    assert out[10].any() and p.member_count(2) == MM
    _same_answers(p, q, "after LEAVE + add_member")
    p.close()
    q.close()


def test_churning_session_example_runs(tmp_path):
    """a 64-leg session whose seats change hands every few ticks with three ticks in flight, through the plain-C example, which
    checks itself against a second session driven by the waiting calls and prints ok"""
    pkg, exe = os.path.join(ROOT, "mediastreamer2_amd"), tmp_path / "churning_session"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "churning_session.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines[-1] == "ok", (run.stdout, run.stderr)
