"""mi_bridge_change_controls, mi_bridge_set_reports and mi_bridge_collected_report (include/msmi355x_bridge.h): a running bridge
is steered -- mute, listen-only, input gain, a seat's mi_volume_params -- and observed -- levels, the elected speaker -- without
ever waiting for the device.

The yardstick is the waiting path of the same build on the same device (tests/controls_pair.py): the SUBJECT keeps three ticks
in flight across every call, the TWIN is fed the same rows, driven by mi_bridge_set_controls / _set_volume_params /
_remove_member / _add_member one tick at a time and polled after every tick.  Output rows, the meters' mi_volume_state words
and every report are compared bit for bit.  Two shapes: 2 conferences x 4 members of 8 kHz mu-law, and an open bridge of 8 kHz
mu-law, 16 kHz PCM and 48 kHz PCM seats in a 16 kHz mix with the concealer, so that the ratios kernel and plc are in the tick."""
import os
import subprocess

import numpy as np
import pytest

import mediastreamer2_amd as ms
from controls_pair import A, L, O, ON, Pair, ambiguous_maxima, words
from mediastreamer2_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCM16, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMU
K8U, K16, K48 = (8000, PCMU, PCMU), (16000, PCM16, PCM16), (48000, PCM16, PCM16)
N, MM = 8, 4
MIXED = [K8U, K16, K48, K8U, K48, K8U, K16, K16]


def _bridges(ctx, shape):
    if shape == "g711":
        return [ms.Bridge(ctx, N, members=MM) for _ in range(2)], [K8U] * N
    return [ms.Bridge(ctx, N, members=MM, rate=16000, plc=True, open=MIXED, admit=[K8U]) for _ in range(2)], MIXED


def _pair(ctx, shape, rows, present=None):
    """rows [ticks][N][pitch] uint8, present [ticks][N] or None"""
    (b, a), kinds = _bridges(ctx, shape)

    def fill(br, t):
        h_in, h_present = br.acquire()
        h_in[:] = rows[t]
        if present is not None:
            h_present[:] = present[t]

    return Pair(b, a, fill, kinds)


def _noise(shape, nticks, seed, lossy=0.0):
    rng = np.random.default_rng(seed)
    pitch = 80 if shape == "g711" else 960
    return rng.integers(0, 256, (nticks, N, pitch), dtype=np.uint8), (rng.random((nticks, N)) >= lossy).astype(np.uint8)


def _same_meters(b, a, t):
    assert bytes(b.volume_state()) == bytes(a.volume_state()), f"the meters after tick {t}"


def _finish(p, what):
    p.drain()
    p.assert_same_rows(what)
    _same_meters(p.b, p.a, "last")
    np.testing.assert_array_equal(words(p.b.volume_max()), words(p.a.volume_max()))
    p.close()


@pytest.mark.parametrize("shape", ["g711", "mixed-plc"])
def test_a_churn_of_mute_listen_only_and_gain(ctx, shape):
    """40 ticks; mute, un-mute, listen-only and gain on a seeded seat in most of them, between acquire and submit or with three
    ticks in flight and none collected; in_flight stays 3 across every call (Pair.tick asserts it)"""
    nticks = 40
    rows, present = _noise(shape, nticks, 0xC0, lossy=0.15)
    p = _pair(ctx, shape, rows, present)
    rng = np.random.default_rng(0xC1)
    heard = False
    for t in range(nticks):
        acts = []
        if t % 4 != 3:
            s1, s2 = (int(v) for v in rng.choice(N, 2, replace=False))
            fl = int(rng.choice([0, A, O, A | O]))
            ch = [(s1, {"flags": fl}), (s2, {"gain": float(rng.choice([0.25, 0.5, 1.0, 1.5, 2.0]))})]
            if t % 5 == 0:
                ch[1][1]["flags"] = A | O
            acts = [lambda q, ch=ch: q.ctl(ch)]
        when = "full" if t >= 3 and t % 3 == 0 else "filling"
        p.tick(state=_same_meters, **{when: acts})
        heard = heard or bool(p.got_a[-1].any())
    assert heard and (p.flags != ON).any() and (p.gain != 1).any()
    _finish(p, shape)


def test_volume_params_switch_mid_run(ctx, oracle):
    """MI_CTL_VOLUME: AGC, static gain and the noise gate switched on and off over 60 ticks, with gain and flags in the same
    entries now and then"""
    nticks = 60
    rng = np.random.default_rng(0xC2)
    # speech-like level, with a quiet stretch for the gate
    pcm = (rng.normal(0, 1, (nticks, N, 80)) * np.where((np.arange(nticks) // 10) % 2, 60.0, 4000.0)[:, None, None]).round().clip(-32767, 32767)
    rows = np.stack([oracle.g711_encode(ms.MI_LAW_PCMU, pcm[t].astype(np.int16)) for t in range(nticks)])
    p = _pair(ctx, "g711", rows)

    def params(**kw):
        v = ms.VolumeBatch.default_params()
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    script = {
        2: [(0, {"volume": params(agc_enabled=1)}), (5, {"volume": params(static_gain=0.5)})],
        9: [(1, {"volume": params(noise_gate_enabled=1, ng_threshold=0.05), "gain": 1.5})],
        15: [(0, {"volume": params(agc_enabled=1, remove_dc=1)}), (2, {"volume": params(static_gain=2.0), "flags": O})],
        24: [(0, {"volume": params()}), (6, {"volume": params(agc_enabled=1, noise_gate_enabled=1)})],
        33: [(5, {"volume": params(static_gain=1.25, noise_gate_enabled=1)}), (2, {"flags": A | O})],
        47: [(s, {"volume": params(agc_enabled=s & 1, static_gain=1.0 + 0.1 * s)}) for s in range(N)],
    }
    for t in range(nticks):
        acts = [lambda q, ch=script[t]: q.ctl(ch)] if t in script else []
        p.tick(state=_same_meters, **{("full" if t == 24 else "filling"): acts})
    _finish(p, "volume")


def test_ordering_inside_a_tick(ctx):
    """a join that arrives muted; a LEAVE and a control on one seat before the same submit, either way round; several calls
    merged per seat and field; a waiting setter between a change and its submit"""
    nticks = 30
    rows, _ = _noise("g711", nticks, 0xC3)
    p = _pair(ctx, "g711", rows)

    def arrives_muted(q):
        q.members(leaves=[2])

    def rejoins_muted(q):
        q.members(joins=[2])
        q.ctl([(2, {"flags": O})])

    def control_then_leave(q):
        q.ctl([(5, {"flags": A, "gain": 0.5})])
        q.members(leaves=[5])

    def leave_then_gain(q):
        q.members(leaves=[6])
        q.ctl([(6, {"gain": 2.0})])  # gain may be set on any seat; it survives the join below

    def merged(q):
        q.ctl([(1, {"flags": 0}), (3, {"gain": 0.25})])
        q.ctl([(1, {"gain": 1.5}), (3, {"gain": 0.75, "flags": A})])
        q.ctl([(1, {"flags": A | O})])

    def waiting_flags_between(q):
        q.b.change_controls([(0, {"flags": 0, "gain": 0.1}), (4, {"gain": 3.0})])
        q.flags[0], q.gain[0], q.gain[4] = L | O, 0.1, 3.0
        q.b.set_controls(flags=q.flags)                # flags only: the last word on the flags, the gains are the change's
        q.a.set_controls(flags=q.flags, gain=q.gain)

    def waiting_gains_between(q):
        q.b.change_controls([(0, {"gain": 0.2, "flags": A | O}), (4, {"gain": 0.3})])
        q.flags[0], q.gain[0], q.gain[4] = ON, 0.6, 1.0
        q.b.set_controls(gain=q.gain)                  # gains only, whole: seat 4's too
        q.a.set_controls(flags=q.flags, gain=q.gain)

    def waiting_member_between(q):
        q.b.change_controls([(7, {"flags": O})])
        q.b.change(leaves=[7])
        q.b.add_member(7)                              # a NEW endpoint by the waiting call: plumbed, active, output on
        q.members_waiting(q.a, joins=[7])

    script = {3: arrives_muted, 5: rejoins_muted, 8: control_then_leave, 10: leave_then_gain, 12: lambda q: q.members(joins=[5, 6]),
              14: merged, 17: waiting_flags_between, 19: waiting_gains_between, 21: waiting_member_between}
    for t in range(nticks):
        p.tick(state=_same_meters, filling=[script[t]] if t in script else [])
        if t == 5:
            assert p.b.member_count(0) == MM
    # the scene did what it says: seat 2 back and muted, seats 5 and 6 back, seat 6's gain kept across its join
    assert p.flags.tolist() == [ON, ON, L | O, L | A, ON, ON, ON, ON] and p.gain[6] == 2.0 and p.gain[1] == 1.5 and p.gain[3] == 0.75
    assert p.gain[0] == np.float32(0.6) and p.gain[4] == 1.0 and p.b.member_count(1) == MM
    _finish(p, "ordering")


def test_refusals_apply_nothing(ctx):
    """every refusal names the entry point, and the tick that follows -- and the meters after it -- are those of a twin that
    never got the call, the good entries around the bad one included"""
    rows, _ = _noise("g711", 64, 0xC4)
    p = _pair(ctx, "g711", rows)
    p.tick(filling=[lambda q: q.members(leaves=[6])])
    p.tick(filling=[lambda q: q.ctl([(3, {"flags": O, "gain": 0.5})])])
    peer = ms.VolumeBatch.default_params()
    peer.peer = 0
    C = _lib.Control
    good = C(1, ms.MI_CTL_GAIN, 0, 2.0)
    bad = [
        ([good, C(N, ms.MI_CTL_GAIN, 0, 2.0), C(2, ms.MI_CTL_GAIN, 0, 2.0)], _lib.MI_EINVAL, f"stream {N} of {N}"),
        ([good, C(-1, ms.MI_CTL_GAIN, 0, 2.0)], _lib.MI_EINVAL, "stream -1"),
        ([good, C(2, 0, 0, 2.0)], _lib.MI_EINVAL, "what 0x0"),
        ([C(2, 8, 0, 2.0), good], _lib.MI_EINVAL, "what 0x8"),
        ([good, C(2, ms.MI_CTL_FLAGS, L | A, 0.0)], _lib.MI_EINVAL, "MI_MIX_LINKED is membership's"),
        ([good, C(6, ms.MI_CTL_FLAGS, A, 0.0)], _lib.MI_EINVAL, "stream 6, which is no member"),
        ([good, C(2, ms.MI_CTL_FLAGS, 0, 0.0), C(1, ms.MI_CTL_FLAGS, 0, 0.0)], _lib.MI_EINVAL, "stream 1 a second time"),
        ([good, C(2, ms.MI_CTL_VOLUME, 0, 0.0, peer)], _lib.MI_ENOTSUP, "echo-limiter peer (0)"),
    ]
    Lb = ctx.L
    for entries, code, text in bad:
        arr = (C * len(entries))(*entries)
        assert Lb.mi_bridge_change_controls(p.b.h, arr, len(entries)) == code
        msg = Lb.mi_last_error().decode()
        assert "mi_bridge_change_controls" in msg and text in msg, msg
        p.tick(state=_same_meters)
        p.tick(state=_same_meters)
    arr = (C * 1)(good)
    assert Lb.mi_bridge_change_controls(None, arr, 1) == _lib.MI_EINVAL
    assert Lb.mi_bridge_change_controls(p.b.h, arr, -1) == _lib.MI_EINVAL
    assert Lb.mi_bridge_change_controls(p.b.h, None, 1) == _lib.MI_EINVAL and b"mi_bridge_change_controls" in Lb.mi_last_error()
    assert Lb.mi_bridge_change_controls(p.b.h, None, 0) == _lib.MI_OK
    assert Lb.mi_bridge_set_reports(p.b.h, 4) == _lib.MI_EINVAL
    for _ in range(3):
        p.tick(state=_same_meters)
    _finish(p, "refusals")


# ---- reports

def _bursts(oracle, nticks, talk, seed):
    """mu-law rows in which member talk[c](t) of conference c speaks at a loudness of its own and the others idle far below
    -30 dBm0.  talk: {conference: [(first tick, member or None), ...]}"""
    rng = np.random.default_rng(seed)
    sigma = np.full((nticks, N), 40.0)
    for c, plan in talk.items():
        for k, (first, m) in enumerate(plan):
            last = plan[k + 1][0] if k + 1 < len(plan) else nticks
            if m is not None:
                sigma[first:last, c * MM + m] = 4000.0 * 1.3 ** m
    pcm = (rng.normal(0, 1, (nticks, N, 80)) * sigma[:, :, None]).round().clip(-32767, 32767).astype(np.int16)
    return np.stack([oracle.g711_encode(ms.MI_LAW_PCMU, pcm[t]) for t in range(nticks)])


def test_every_ticks_report_is_the_twins_poll(ctx, oracle):
    """140 ticks -- the one-second window restarts -- of bursts that move between members, with mutes, one leave and one
    re-join: every tick's levels, winner and max_db are what the waiting polls answer after the same tick"""
    nticks = 140
    talk = {0: [(0, None), (4, 0), (22, 1), (40, 3), (58, None), (75, 2), (104, 0), (122, 1)],
            1: [(0, 2), (15, None), (30, 0), (50, 3), (70, 1), (95, None), (110, 2)]}
    rows = _bursts(oracle, nticks, talk, 0xC5)
    p = _pair(ctx, "g711", rows)
    p.b.set_reports(speakers=True, levels=True)
    script = {
        30: lambda q: q.ctl([(1, {"flags": O})]),            # the loudest so far is muted: the election falls back
        46: lambda q: q.ctl([(3, {"flags": O}), (1, {"flags": A | O})]),
        52: lambda q: q.members(leaves=[3]),                 # ... and leaves
        64: lambda q: q.members(joins=[3]),                  # a NEW endpoint: fresh meter, last of the joining order
        60: lambda q: q.ctl([(7, {"flags": A})]),            # listen-only off does not change the election
        80: lambda q: q.ctl([(5, {"flags": 0, "gain": 0.5})]),
        90: lambda q: q.ctl([(5, {"flags": A | O})]),
    }
    flags = []
    for t in range(nticks):
        p.tick(poll=True, filling=[script[t]] if t in script else [])
        flags.append(p.flags.copy())
    p.drain()
    p.assert_same_rows("reports")
    winners = np.stack([w for w, _, _ in p.polls])
    changes = [int((winners[1:, c] != winners[:-1, c]).sum()) for c in range(2)]
    assert min(changes) >= 3, changes                       # the scene: the twin's winner changes at least three times
    assert (winners == -1).any() and (winners >= 0).any()
    # the precondition of comparing a linear election with the reference's: no two eligible maxima that are distinct floats
    # with one dBm0 float, anywhere in the scene
    assert ambiguous_maxima(p.maxima, flags, MM) == []
    p.assert_same_reports(what="reports")
    p.close()


def test_of_equal_maxima_the_first_to_join_wins(ctx, oracle):
    """two members fed identical rows have identical meters; the earlier joiner is elected.  After that member has left and
    re-joined the other one wins; and two NEW endpoints seated by one call in the order (1, 0) elect seat 1 on equal maxima"""
    nticks = 70
    rows = _bursts(oracle, nticks, {0: [(0, 0)], 1: [(0, 1)]}, 0xC6)
    rows[:, 1] = rows[:, 0]
    rows[:, 4] = rows[:, 5]
    p = _pair(ctx, "g711", rows)
    p.b.set_reports(speakers=True)
    script = {20: lambda q: q.members(leaves=[0]), 24: lambda q: q.members(joins=[0]), 45: lambda q: q.members(joins=[1, 0])}
    for t in range(nticks):
        p.tick(poll=True, filling=[script[t]] if t in script else [])
    p.drain()
    win = np.stack([r["winner"] for r in p.reports])
    twin = np.stack([w for w, _, _ in p.polls])
    np.testing.assert_array_equal(win, twin)
    mx = np.stack(p.maxima)
    assert (words(mx[5:20, 0]) == words(mx[5:20, 1])).all() and (win[5:20, 0] == 0).all()    # equal: the earlier joiner
    assert (win[20:45, 0] == 1).all()                                                          # seat 0 away, then the later joiner
    assert (words(mx[50:, 0]) == words(mx[50:, 1])).all() and (win[50:, 0] == 1).all()       # equal again: seat 1 joined first
    assert (win[5:, 1] == 4).all()                                                             # conference 1: seats 4 and 5 equal throughout
    for r, (_, db, _) in zip(p.reports, p.polls):
        np.testing.assert_array_equal(words(r["max_db"]), words(db))
        assert "levels" not in r
    p.close()


def test_reports_off_and_switched_on_mid_run(ctx):
    rows, _ = _noise("g711", 16, 0xC7)
    p = _pair(ctx, "g711", rows)
    with pytest.raises(ms.MiError) as e:
        p.b.collected_report()                      # nothing collected yet
    assert e.value.code == _lib.MI_EINVAL and "mi_bridge_collected_report" in str(e.value)
    for t in range(6):
        p.tick(poll=True)
    assert p.reports == [None] * 3                  # off: MI_EINVAL
    p.b.set_reports(speakers=True, levels=True)     # ticks 3..5 are in flight without one; tick 6 is the first
    for t in range(6, 12):
        p.tick(poll=True)
    p.b.set_reports()                               # off again from tick 12 on
    for t in range(12, 16):
        p.tick(poll=True)
    p.drain()
    assert [r is not None for r in p.reports] == [6 <= t < 12 for t in range(16)]
    assert [p.reports[t]["seq"] for t in range(6, 12)] == list(range(6, 12))
    for t in range(6, 12):
        win, db, lev = p.polls[t]
        np.testing.assert_array_equal(p.reports[t]["winner"], win)
        np.testing.assert_array_equal(words(p.reports[t]["levels"]), words(lev))
    p.assert_same_rows("reports on and off")
    p.close()


def test_moderated_bridge_example_runs(tmp_path):
    """the plain-C server loop with small sizes: it checks itself against a twin bridge driven by the waiting calls and prints ok"""
    pkg, exe = os.path.join(ROOT, "mediastreamer2_amd"), tmp_path / "moderated_bridge"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "moderated_bridge.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe), "2", "4", "120"], capture_output=True, text=True, timeout=120)
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines[-1] == "ok", (run.stdout, run.stderr)
