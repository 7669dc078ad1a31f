"""mi_session_change_controls, mi_session_set_reports and mi_session_collected_report (include/msmi355x_session_controls.h): a
running session is steered -- mute, listen-only, input gain -- and observed -- levels, the elected speaker -- without ever
waiting for the device.

The yardstick is the waiting path of the same build on the same device (tests/controls_pair.py): the SUBJECT keeps three ticks
in flight across every call, the TWIN is fed the same blocks, driven by mi_session_set_controls / _remove_member / _add_member
one tick at a time and polled after every tick.  Output rows, the meters' read-outs and every report are compared bit for bit.
2 conferences x 3 legs: at 8 kHz (the 64-sample group canceller), at 16 -> 48 kHz, and the latter with use_graphs, where the
control and report launches sit in front of and behind the slot's graph.

mi_session has no read-out of the one-second maxima (mi_bridge_get_volume_max is the bridge's), so the precondition of
tests/test_gpu_bridge_controls.py's report scene -- no two eligible maxima that are distinct floats with one dBm0 float -- cannot
be asserted here; the comparison of every tick's winner with the twin's is what would show such a case."""
import numpy as np
import pytest

import mediastreamer2_amd as ms
from conftest import synth_pcm
from controls_pair import A, L, O, ON, Pair, words
from mediastreamer2_amd import _lib

pytestmark = pytest.mark.gpu

N, MM = 6, 3
SHAPES = {
    "8k": dict(in_rate=8000, rate=8000, use_graphs=False),
    "16k-48k": dict(in_rate=16000, rate=48000, use_graphs=False),
    "16k-48k-graphs": dict(in_rate=16000, rate=48000, use_graphs=True),
}


def _signals(cfg, nticks, seed, loud=None):
    """mic [N][in_len * nticks], ref [N][len * nticks].  loud [nticks][N]: the microphone's level per tick, or None: 2500"""
    in_len, ln = cfg["in_rate"] // 100, cfg["rate"] // 100
    mic = np.random.default_rng(seed).normal(0, 1, (N, in_len * nticks))
    level = np.full((nticks, N), 2500.0) if loud is None else loud
    mic = (mic * np.repeat(level.T, in_len, axis=1)).round().clip(-32767, 32767).astype(np.int16)
    ref = np.stack([synth_pcm(seed + 500 + s, ln * nticks, rate=cfg["rate"], sigma=300.0) for s in range(N)])
    return mic, ref


def _pair(ctx, shape, sig):
    cfg = SHAPES[shape]
    mic, ref = sig
    in_len, ln = cfg["in_rate"] // 100, cfg["rate"] // 100
    b, a = (ms.Session(ctx, N, members=MM, tail_ms=32, agc=True, **cfg) for _ in range(2))

    def fill(se, t):
        h_mic, h_ref = se.acquire()
        h_mic[:] = mic[:, t * in_len:(t + 1) * in_len]
        h_ref[:] = ref[:, t * ln:(t + 1) * ln]

    return Pair(b, a, fill)


def _same_answers(b, a, t):
    np.testing.assert_array_equal(words(b.levels()), words(a.levels()), err_msg=f"get_levels after tick {t}")
    (wb, db), (wa, da) = b.active_speakers(0), a.active_speakers(0)
    np.testing.assert_array_equal(wb, wa, err_msg=f"active_speakers after tick {t}")
    np.testing.assert_array_equal(words(db), words(da), err_msg=f"active_speakers' level after tick {t}")
    assert [b.member_count(c) for c in range(N // MM)] == [a.member_count(c) for c in range(N // MM)]


def _finish(p, what):
    p.drain()
    p.assert_same_rows(what)
    _same_answers(p.b, p.a, "last")
    p.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_churn_of_mute_listen_only_and_gain(ctx, shape):
    """40 ticks; mute, un-mute, listen-only and gain on a seeded seat in most of them, between acquire and submit or with three
    ticks in flight and none collected; in_flight stays 3 across every call (Pair.tick asserts it)"""
    nticks = 40
    p = _pair(ctx, shape, _signals(SHAPES[shape], nticks, 0xD0))
    rng = np.random.default_rng(0xD1)
    for t in range(nticks):
        acts = []
        if t % 4 != 3:
            s1, s2 = (int(v) for v in rng.choice(N, 2, replace=False))
            ch = [(s1, {"flags": int(rng.choice([0, A, O, A | O]))}), (s2, {"gain": float(rng.choice([0.25, 0.5, 1.0, 1.5, 2.0]))})]
            if t % 5 == 0:
                ch[1][1]["flags"] = A | O
            acts = [lambda q, ch=ch: q.ctl(ch)]
        when = "full" if t >= 3 and t % 3 == 0 else "filling"
        p.tick(state=_same_answers if t % 4 == 0 else None, **{when: acts})
    assert p.got_a[-1].any() and (p.flags != ON).any() and (p.gain != 1).any()
    _finish(p, shape)


@pytest.mark.parametrize("shape", ["8k", "16k-48k-graphs"])
def test_ordering_inside_a_tick(ctx, shape):
    """a join that arrives muted; a LEAVE and a control on one seat before the same submit, either way round; several calls
    merged per seat and field; a waiting setter between a change and its submit"""
    nticks = 28
    p = _pair(ctx, shape, _signals(SHAPES[shape], nticks, 0xD2))

    def rejoins_muted(q):
        q.members(joins=[2])
        q.ctl([(2, {"flags": O})])

    def control_then_leave(q):
        q.ctl([(5, {"flags": A, "gain": 0.5})])
        q.members(leaves=[5])

    def leave_then_gain(q):
        q.members(leaves=[4])
        q.ctl([(4, {"gain": 2.0})])  # gain may be set on any seat; it survives the join below

    def merged(q):
        q.ctl([(1, {"flags": 0}), (3, {"gain": 0.25})])
        q.ctl([(1, {"gain": 1.5}), (3, {"gain": 0.75, "flags": A})])
        q.ctl([(1, {"flags": A | O})])

    def waiting_flags_between(q):
        q.b.change_controls([(0, {"flags": 0, "gain": 0.1}), (3, {"gain": 3.0})])
        q.flags[0], q.gain[0], q.gain[3] = L | O, 0.1, 3.0
        q.b.set_controls(flags=q.flags)                # flags only: the last word on the flags, the gains are the change's
        q.a.set_controls(flags=q.flags, gain=q.gain)

    def waiting_gains_between(q):
        q.b.change_controls([(0, {"gain": 0.2, "flags": A | O}), (3, {"gain": 0.3})])
        q.flags[0], q.gain[0], q.gain[3] = ON, 0.6, 1.0
        q.b.set_controls(gain=q.gain)                  # gains only, whole: seat 3's too
        q.a.set_controls(flags=q.flags, gain=q.gain)

    def waiting_member_between(q):
        q.b.change_controls([(1, {"flags": O})])
        q.b.change_members([(1, ms.MI_SESSION_LEAVE)])
        q.b.add_member(1)                              # a NEW endpoint by the waiting call: plumbed, active, output on
        q.members_waiting(q.a, joins=[1])
        q.flags[1] = ON

    script = {3: lambda q: q.members(leaves=[2]), 5: rejoins_muted, 8: control_then_leave, 10: leave_then_gain,
              12: lambda q: q.members(joins=[5, 4]), 14: merged, 17: waiting_flags_between, 19: waiting_gains_between, 21: waiting_member_between}
    for t in range(nticks):
        p.tick(state=_same_answers if t in script else None, filling=[script[t]] if t in script else [])
    assert p.flags.tolist() == [ON, ON, L | O, L | A, ON, ON] and p.gain[4] == 2.0 and p.gain[0] == np.float32(0.6) and p.gain[3] == 1.0
    _finish(p, shape)


def test_refusals_apply_nothing(ctx):
    """every refusal names the entry point, and the ticks that follow -- and the meters after them -- are those of a twin that
    never got the call, the good entries around the bad one included"""
    shape = "8k"
    p = _pair(ctx, shape, _signals(SHAPES[shape], 48, 0xD3))
    p.tick(filling=[lambda q: q.members(leaves=[4])])
    p.tick(filling=[lambda q: q.ctl([(3, {"flags": O, "gain": 0.5})])])
    C = _lib.SessionControl
    good = C(1, ms.MI_CTL_GAIN, 0, 2.0)
    bad = [
        ([good, C(N, ms.MI_CTL_GAIN, 0, 2.0), C(2, ms.MI_CTL_GAIN, 0, 2.0)], f"stream {N} of {N}"),
        ([good, C(-1, ms.MI_CTL_GAIN, 0, 2.0)], "stream -1"),
        ([good, C(2, 0, 0, 2.0)], "what 0x0"),
        ([C(2, ms.MI_CTL_VOLUME, 0, 2.0), good], "what 0x4"),  # the session has no MI_CTL_VOLUME
        ([good, C(2, ms.MI_CTL_FLAGS, L | A, 0.0)], "MI_MIX_LINKED is membership's"),
        ([good, C(4, ms.MI_CTL_FLAGS, A, 0.0)], "stream 4, which is no member"),
        ([good, C(2, ms.MI_CTL_FLAGS, 0, 0.0), C(1, ms.MI_CTL_FLAGS, 0, 0.0)], "stream 1 a second time"),
    ]
    Ls = ctx.L
    for entries, text in bad:
        arr = (C * len(entries))(*entries)
        assert Ls.mi_session_change_controls(p.b.h, arr, len(entries)) == _lib.MI_EINVAL
        msg = Ls.mi_last_error().decode()
        assert "mi_session_change_controls" in msg and text in msg, msg
        p.tick(state=_same_answers)
        p.tick()
    arr = (C * 1)(good)
    assert Ls.mi_session_change_controls(None, arr, 1) == _lib.MI_EINVAL
    assert Ls.mi_session_change_controls(p.b.h, arr, -1) == _lib.MI_EINVAL
    assert Ls.mi_session_change_controls(p.b.h, None, 1) == _lib.MI_EINVAL and b"mi_session_change_controls" in Ls.mi_last_error()
    assert Ls.mi_session_change_controls(p.b.h, None, 0) == _lib.MI_OK
    assert Ls.mi_session_set_reports(p.b.h, 4) == _lib.MI_EINVAL
    for _ in range(3):
        p.tick(state=_same_answers)
    _finish(p, "refusals")


# ---- reports

def _bursts(nticks, talk):
    """loud [nticks][N]: member talk[c](t) of conference c speaks at a loudness of its own, the others idle far below -30 dBm0"""
    loud = np.full((nticks, N), 30.0)
    for c, plan in talk.items():
        for k, (first, m) in enumerate(plan):
            last = plan[k + 1][0] if k + 1 < len(plan) else nticks
            if m is not None:
                loud[first:last, c * MM + m] = 4000.0 * 1.4 ** m
    return loud


@pytest.mark.parametrize("shape", ["8k", "16k-48k-graphs"])
def test_every_ticks_report_is_the_twins_poll(ctx, shape):
    """136 ticks -- the one-second window restarts -- of bursts that move between members, with mutes, one leave and one
    re-join: every tick's levels, winner and max_db are what the waiting polls answer after the same tick"""
    nticks = 136
    talk = {0: [(0, None), (4, 0), (22, 1), (40, 2), (58, None), (75, 1), (104, 0), (120, 2)],
            1: [(0, 1), (15, None), (30, 0), (50, 2), (70, 1), (95, None), (110, 0)]}
    p = _pair(ctx, shape, _signals(SHAPES[shape], nticks, 0xD5, _bursts(nticks, talk)))
    p.b.set_reports(speakers=True, levels=True)
    script = {
        30: lambda q: q.ctl([(1, {"flags": O})]),            # the loudest so far is muted: the election falls back
        46: lambda q: q.ctl([(2, {"flags": O}), (1, {"flags": A | O})]),
        52: lambda q: q.members(leaves=[2]),                 # ... and leaves
        64: lambda q: q.members(joins=[2]),                  # a NEW endpoint: fresh meter, last of the joining order
        60: lambda q: q.ctl([(5, {"flags": A})]),            # listen-only off does not change the election
        80: lambda q: q.ctl([(4, {"flags": 0, "gain": 0.5})]),
        90: lambda q: q.ctl([(4, {"flags": A | O})]),
    }
    for t in range(nticks):
        p.tick(poll=True, filling=[script[t]] if t in script else [])
    p.drain()
    p.assert_same_rows(shape)
    winners = np.stack([w for w, _, _ in p.polls])
    changes = [int((winners[1:, c] != winners[:-1, c]).sum()) for c in range(2)]
    assert min(changes) >= 3, changes                       # the scene: the twin's winner changes at least three times
    assert (winners >= 0).any()
    p.assert_same_reports(what=shape)
    p.close()


def test_of_equal_maxima_the_first_to_join_wins(ctx):
    """two legs fed identical blocks have identical meters; the earlier joiner is elected.  After that leg has left and
    re-joined the other one wins; and two NEW endpoints seated by one call in the order (1, 0) elect seat 1 on equal maxima"""
    shape, nticks = "8k", 70
    mic, ref = _signals(SHAPES[shape], nticks, 0xD6, _bursts(nticks, {0: [(0, 0)], 1: [(0, 1)]}))
    mic[1], ref[1] = mic[0], ref[0]
    mic[3], ref[3] = mic[4], ref[4]
    p = _pair(ctx, shape, (mic, ref))
    p.b.set_reports(speakers=True)
    script = {20: lambda q: q.members(leaves=[0]), 24: lambda q: q.members(joins=[0]), 45: lambda q: q.members(joins=[1, 0])}
    for t in range(nticks):
        p.tick(poll=True, filling=[script[t]] if t in script else [])
    p.drain()
    win = np.stack([r["winner"] for r in p.reports])
    np.testing.assert_array_equal(win, np.stack([w for w, _, _ in p.polls]))
    lev = np.stack([l for _, _, l in p.polls])
    assert (words(lev[:20, 0]) == words(lev[:20, 1])).all() and (win[8:20, 0] == 0).all()     # equal: the earlier joiner
    assert (win[20:45, 0] == 1).all()                                                          # seat 0 away, then the later joiner
    assert (words(lev[45:, 0]) == words(lev[45:, 1])).all() and (win[53:, 0] == 1).all()      # equal again: seat 1 joined first
    assert (win[8:, 1] == 3).all()                                                             # conference 1: seats 3 and 4 equal throughout
    for r, (_, db, _) in zip(p.reports, p.polls):
        np.testing.assert_array_equal(words(r["max_db"]), words(db))
        assert "levels" not in r
    p.close()


def test_reports_off_and_switched_on_mid_run(ctx):
    shape = "16k-48k-graphs"
    p = _pair(ctx, shape, _signals(SHAPES[shape], 16, 0xD7))
    with pytest.raises(ms.MiError) as e:
        p.b.collected_report()                      # nothing collected yet
    assert e.value.code == _lib.MI_EINVAL and "mi_session_collected_report" in str(e.value)
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
