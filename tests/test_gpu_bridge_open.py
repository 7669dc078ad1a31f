"""GPU parity of bridge seats that change hands without a drain (mi_bridge_create_open, mi_bridge_change_members,
include/msmi355x_bridge.h): members join, leave and change kind while three ticks are in flight, the changes applied on the
device in stream order ahead of the tick they travel with (bridge_roster_kernel, csrc/bridge_roster.hip; plc_seats_kernel,
csrc/plc.hip).

The yardstick is tests/bridge_open_parts.py's OpenParts (through open_pair) -- tests/bridge_parts.py's Parts chain on the C ABI with batches for
every admitted rate from the start, a seat's new kind a relabelling plus restart(s) -- and every comparison with it is
BIT-EXACT over all legs, samples and ticks: output bytes, mi_volume_state bytes, meter maxima.  Two conferences of three
seats.  Between the two rooms of test (c) each of the six leg forms -- at the mix, whole below, whole above, 3/2 or 2/3,
ratio 4, a : b -- is once the kind a seat leaves and once the kind it takes."""
import os
import subprocess

import numpy as np
import pytest

import mediastreamer2_amd as ms
from bridge_open_parts import OpenConcealedParts, open_pair, same_labels
from bridge_parts import Parts, assert_same_meters, leg_rows, loss_patterns, mk, one_tick  # noqa: F401 (mk: a fixture)
from mediastreamer2_amd import _lib

pytestmark = pytest.mark.gpu

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
K8U, K8A, K16, K48, K32, K24, K12 = ((8000, PCMU, PCMU), (8000, PCMA, PCM16), (16000, PCM16, PCM16), (48000, PCM16, PCM16),
                                     (32000, PCM16, PCM16), (24000, PCM16, PCM16), (12000, PCM16, PCM16))
MM = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# conference rate, the six seats at creation, the admitted kinds, and {tick: the calls made before that tick is filled}, a
# call being (joins, leaves).  16 kHz: 8 kHz is whole below, 16 at the mix, 32 and 48 whole above, 24 at 3/2, 12 at 3 : 4.
# 8 kHz: 8 at the mix, 32 at ratio 4, 12 at 3/2.
ROOMS = {
    "16k": (16000, [K8U, K16, K48, K24, K12, K8A], [K32], {
        0: [([(0, K12)], [])],                          # a replacement on tick 0: whole below -> a : b
        1: [([(4, K24)], [])],                          # one change per tick on three consecutive submits, none collected yet:
        2: [([(1, K48)], [])],                          # a : b -> 3/2, at the mix -> whole above
        6: [([], [3])],                                 # 3/2 leaves ...
        7: [([(3, K8U)], [])],                          # ... and a tick later another kind, whole below, takes the seat
        12: [([(2, K16), (5, K32)], [1])],              # three changes in one call, two of them in conference 0: whole above -> at the mix
        15: [([(1, K8A), (4, K48)], []), ([(1, K16)], [4])],  # two calls before one submit on the same seats: the last wins
        20: [([(4, K8U)], [])],
    }),
    "8k": (8000, [K32, K8U, K12, K8U, K32, K12], [K12], {  # (a kind that is there: nadmit > 0 is what opens the bridge)
        0: [([(0, K8U)], [])],                          # ratio 4 -> at the mix
        1: [([(1, K32)], [])],                          # at the mix -> ratio 4
        2: [([(2, K32)], [])],                          # 3/2 -> ratio 4
        6: [([], [4])],
        7: [([(4, K12)], [])],                          # ratio 4 left, 3/2 takes the seat
        12: [([(3, K12), (0, K32)], [5])],
        15: [([(5, K8U)], []), ([(5, K32)], [])],
        20: [([(1, K8U)], [])],
    }),
}


def _apply(br, parts, calls):
    for joins, leaves in calls:
        br.change(joins=joins, leaves=leaves)
        for s in leaves:
            parts.leave_seat(s)
        for s, kind in joins:
            parts.join_seat(s, kind)


def _present(parts, rng, lossy=0.2):
    """a seeded fifth of the legs absent, and nobody sends on a pin that is not plumbed"""
    return ((rng.random(parts.n) >= lossy) & ((parts.flags & L) != 0)).astype(np.uint8)


def _pipelined(br, ticks):
    """submit every (x, present) produced by `ticks` with up to three in flight -> the collected rows, in order"""
    got = []
    for x, present in ticks:
        if br.in_flight() == 3:
            got.append(br.collect().copy())
        h_in, h_present = br.acquire()
        h_in[:] = x
        h_present[:] = present
        br.submit()
    while br.in_flight():
        got.append(br.collect().copy())
    return got


def test_nothing_admitted_is_the_ratios_bridge(ctx, mk):
    """(a) nadmit == 0: the same tick_bytes, and 12 ticks and the meters bit for bit ratios='"""
    conf, legs = 16000, [K8U, K12, K48, K24, K16, K8A]
    old, new = mk(ms.Bridge, 6, members=MM, rate=conf, ratios=legs), mk(ms.Bridge, 6, members=MM, rate=conf, open=legs)
    none = mk(ms.Bridge, 6, members=MM, rate=conf, open=legs, admit=[])
    assert new.tick_bytes() == old.tick_bytes() == none.tick_bytes()
    rng = np.random.default_rng(0x0A)
    for t in range(12):
        x = rng.integers(0, 256, (6, old.tick_bytes()[0]), dtype=np.uint8)
        present = (rng.random(6) >= 0.2).astype(np.uint8)
        want = one_tick(old, x, present)
        np.testing.assert_array_equal(one_tick(new, x, present), want, err_msg=f"tick {t}")
        np.testing.assert_array_equal(one_tick(none, x, present), want, err_msg=f"tick {t}")
    assert bytes(new.volume_state()) == bytes(old.volume_state()) == bytes(none.volume_state())
    uniform = mk(ms.Bridge, 6, members=MM, rate=8000, open=[K8U] * 6)  # mi_bridge_create_rated's bridge, as ratios= gives it
    assert uniform.tick_bytes() == (80, 80)


def test_nothing_changed_is_the_closed_bridge(ctx, mk):
    """(b) an open bridge on which nothing changes against the closed bridge of the same legs: every leg's slice, the meters
    and the election over 12 ticks, although the kernel family and the pitch differ"""
    conf, legs, admit = 16000, [K8U, K16, K8U, K16, K8A, K8U], [K48, K12]
    closed, br = mk(ms.Bridge, 6, members=MM, rate=conf, ratios=legs), mk(ms.Bridge, 6, members=MM, rate=conf, open=legs, admit=admit)
    parts = Parts(ctx, mk, MM, conf, legs)
    assert closed.tick_bytes() == (320, 320) and br.tick_bytes() == (960, 960)
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    closed.set_volume_params([p] * 6)
    br.set_volume_params([p] * 6)
    parts.set_params([p] * 6)
    rng = np.random.default_rng(0x0B)
    for t in range(12):
        x = parts.rows(rng)
        wide = rng.integers(0, 256, (6, 960), dtype=np.uint8)  # the tails are random on both
        wide[:, :320] = x
        present = (rng.random(6) >= 0.2).astype(np.uint8)
        got, want = one_tick(br, wide, present), one_tick(closed, x, present)
        parts.tick(x, present)
        for s in range(6):
            np.testing.assert_array_equal(br.leg_out(got, s), closed.leg_out(want, s), err_msg=f"tick {t} leg {s}")
    parts.check_state(br)
    parts.check_state(closed)
    for a, b in zip(br.active_speakers(), closed.active_speakers()):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("room", list(ROOMS))
def test_seats_changing_kind(ctx, mk, room):
    """(c) 30 ticks, three in flight throughout, against the yardstick: every tick's rows over the whole pitch, at the end the
    meters and their maxima.  AGC and DC removal on; pin 1 with an input gain, which a join leaves as it is; a fifth of the
    legs absent per tick"""
    conf, legs, admit, script = ROOMS[room]
    n, nticks = len(legs), 30
    br = mk(ms.Bridge, n, members=MM, rate=conf, open=legs, admit=admit)
    parts = open_pair(br, ctx, mk, MM, conf, legs, admit)
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    br.set_volume_params([p] * n)
    parts.set_params([p] * n)
    parts.gain[1] = 1.6
    br.set_controls(flags=parts.flags, gain=parts.gain)
    parts.set_controls()
    rng = np.random.default_rng(0x0C + conf)
    want = []

    def ticks():
        for t in range(nticks):
            _apply(br, parts, script.get(t, []))
            same_labels(br, parts)  # the host answers for the new roster as soon as the call returns
            x, present = parts.rows(rng), _present(parts, rng)
            want.append(parts.tick(x, present))
            yield x, present

    got = _pipelined(br, ticks())
    assert len(got) == nticks
    for t in range(nticks):
        np.testing.assert_array_equal(got[t], want[t], err_msg=f"tick {t}")
    parts.check_state(br)


def test_a_seat_that_left(ctx, mk):
    """(d) seats 0 and 1 of conference 0 talk, seat 2 is silent.  Seat 1 leaves on tick 4, three ticks in flight, and KEEPS
    sending a loud signal flagged present.  Before, its row is audio in every staging slot; from tick 4 on it reads zero over
    the whole pitch in each of the next five collected ticks, and seats 0 and 2 hear only each other: seat 0 silence, seat 2
    seat 0's samples at unity gain"""
    conf, legs, gone, nticks = 16000, [K16] * 6, 4, 9
    br = mk(ms.Bridge, 6, members=MM, rate=conf, open=legs, admit=[K48])
    pitch = br.tick_bytes()[0]
    rng = np.random.default_rng(0x0D)
    sent = []

    def ticks():
        for t in range(nticks):
            if t == gone:
                br.change(leaves=[1])
                assert br.member_count(0) == 2 and br.member_count(1) == 3
            x = np.zeros((6, pitch), np.uint8)
            for s in (0, 1, 4):  # the others send digital silence
                x[s, :320] = rng.normal(0.0, 5000.0, 160).astype(np.int16).view(np.uint8)
            sent.append(x)
            yield x, np.ones(6, np.uint8)

    got = _pipelined(br, ticks())
    assert pitch == 960 and len(got) == nticks
    for t in range(nticks):
        if t < gone:
            assert got[t][1, :320].any() and got[t][0, :320].any(), t  # they hear each other, in slots 0, 1, 2 and 0 again
            assert not np.array_equal(got[t][2, :320], sent[t][0, :320]), t
        else:
            assert not got[t][1].any(), t               # zero over the whole pitch, every slot
            assert not got[t][0].any(), t               # seat 0 hears seat 2's silence, not seat 1
            np.testing.assert_array_equal(got[t][2, :320], sent[t][0, :320], err_msg=f"tick {t}")  # seat 2 hears seat 0 alone
        assert got[t][[3, 5]].any() and not got[t][4].any(), t
    assert br.active_speakers()[0][0] != 1


def test_plc_seats_changing_kind(ctx, mk, oracle):
    """(e) cfg.plc, 45 ticks of bridge_parts' loss patterns over kinds in three rate classes, a fourth admitted: seat 3 (a
    25-tick outage from tick 12) replaced on tick 20, in the middle of it -- the new endpoint's concealer starts from nothing
    --; seat 2 replaced on tick 16 into 48 kHz, a class that had no member at creation; seat 5 leaves on tick 30.  Three ticks in
    flight throughout: the concealer's apply launch is ordered against them.  Against the decoders, a PlcBatch per admitted
    rate and the plc-less open bridge"""
    conf, nticks = 16000, 45
    legs, admit = [K8U, K16, K12, K8A, K16, K8U], [K48]
    n = len(legs)
    br = mk(ms.Bridge, n, members=MM, rate=conf, open=legs, admit=admit, plc=True)
    parts = OpenConcealedParts(ctx, mk, MM, conf, legs, admit)
    assert br.tick_bytes()[0] == 960
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    br.set_volume_params([p] * n)
    parts.inner.set_volume_params([p] * n)
    script = {16: ([(2, K48)], []), 20: ([(3, K12)], []), 30: ([], [5])}
    labels = [list(legs)]
    for t in range(1, nticks):
        now = list(labels[-1])
        for s, kind in script.get(t, ([], []))[0]:
            now[s] = kind
        labels.append(now)
    rows = {}  # a leg's signal per kind it ever has, cut per tick
    for kinds in {tuple(l) for l in labels}:
        rows[kinds] = leg_rows(oracle, list(kinds), nticks)
    present = loss_patterns(n, nticks)
    gone, want, here_at = set(), [], []

    def ticks():
        for t in range(nticks):
            joins, leaves = script.get(t, ([], []))
            if joins or leaves:
                br.change(joins=joins, leaves=leaves)  # (with three of the bridge's ticks in flight)
                for s in leaves:
                    parts.leave_seat(s)
                    gone.add(s)
                for s, kind in joins:
                    parts.join_seat(s, kind)
            x = np.zeros((n, 960), np.uint8)
            src = rows[tuple(labels[t])][t]
            x[:, :src.shape[1]] = src
            here = present[t].copy()
            here[list(gone)] = 0
            want.append(parts.tick(x, here))
            yield x, here

    got = _pipelined(br, ticks())
    for t in range(nticks):
        for s, (rate, _, oc) in enumerate(labels[t]):  # the leg's slice as its kind was on that tick
            own = rate // 100 * (1 if oc else 2)
            np.testing.assert_array_equal(got[t][s, :own], want[t][s, :own], err_msg=f"tick {t} leg {s}")
    assert_same_meters(br, parts.inner)


@pytest.mark.parametrize("form", ["create", "rated", "plc"])
def test_older_constructors(ctx, mk, form):
    """(f) twin bridges from an older constructor, one driven by remove_member / add_member, the other by change() with the
    seat's own kind: rows, meters, member_count and the election.  Seat 0 leaves on tick 3; on tick 5 seat 2 is replaced and
    THEN seat 0 taken again: from there the two are new endpoints that send the same bytes, equally loud to the bit, seat 1
    is silent, and the election must name 2, the earlier joiner, where pin order would name 0"""
    n = 6
    kw = {"create": dict(rate=8000), "rated": dict(rate=16000, leg_rates=[8000, 16000, 8000] * 2), "plc": dict(rate=8000, plc=True)}[form]
    a, b = mk(ms.Bridge, n, members=MM, **kw), mk(ms.Bridge, n, members=MM, **kw)
    own = lambda s: (a.leg_rate(s), *a.leg_codec(s))
    rng = np.random.default_rng(0x0F)
    shape = (n, a.in_len)  # code words at the widest leg's tick
    for t in range(14):
        if t == 3:
            a.remove_member(0), b.change(leaves=[0])
        if t == 5:
            a.remove_member(2), a.add_member(2), a.add_member(0)
            b.change(joins=[(2, own(2)), (0, own(0))])
        if t == 7:  # a replacement is a leave and a join
            a.remove_member(4), a.add_member(4), b.change(joins=[(4, own(4))])
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        x[2], x[1] = x[0], 0xFF  # equally loud; mu-law silence
        present = np.ones(n, np.uint8)
        present[0] = not 3 <= t < 5
        np.testing.assert_array_equal(one_tick(b, x, present), one_tick(a, x, present), err_msg=f"tick {t}")
        assert [a.member_count(c) for c in range(2)] == [b.member_count(c) for c in range(2)]
    assert bytes(a.volume_state()) == bytes(b.volume_state())
    np.testing.assert_array_equal(a.volume_max().view(np.uint32), b.volume_max().view(np.uint32))
    wa, wb = a.active_speakers(), b.active_speakers()
    np.testing.assert_array_equal(wa[0], wb[0])
    np.testing.assert_array_equal(wa[1].view(np.uint32), wb[1].view(np.uint32))
    assert wa[0][0] == 2
    with pytest.raises(ms.MiError) as e:  # a closed bridge admits the seat's own kind only
        b.change(joins=[(1, (48000, PCM16, PCM16))])
    assert e.value.code == _lib.MI_ENOTSUP and "seat 1" in str(e.value) and "48000" in str(e.value)


def test_refusals_apply_nothing(ctx, mk):
    """(g) one call holding one bad entry between two good ones applies nothing -- the host's answers and the next ticks still
    equal the yardstick's, which saw no change --; a kind not admitted is MI_ENOTSUP with seat and rate in the message, a LEAVE
    of a non-member MI_EINVAL"""
    conf, legs, admit = 16000, [K8U, K16, K48, K24, K12, K8A], [K32]
    br = mk(ms.Bridge, 6, members=MM, rate=conf, open=legs, admit=admit)
    parts = open_pair(br, ctx, mk, MM, conf, legs, admit)
    rng = np.random.default_rng(0x10)

    def refused(code, values, **kw):
        with pytest.raises(ms.MiError) as e:
            br.change(**kw)
        assert e.value.code == code, str(e.value)
        for v in values:
            assert str(v) in str(e.value), str(e.value)

    for t in range(6):
        if t == 1:
            refused(_lib.MI_ENOTSUP, ["entry 1", "seat 3", "44100 Hz", "7 kinds"], joins=[(0, K48), (3, (44100, PCM16, PCM16)), (5, K16)])
            refused(_lib.MI_ENOTSUP, ["entry 0", "seat 2", "8000 Hz"], joins=[(2, (8000, PCMU, PCMA))], leaves=[1])
        if t == 2:
            br.change(leaves=[4])
            parts.leave_seat(4)
            refused(_lib.MI_EINVAL, ["entry 1", "stream 4 is no member"], joins=[(0, K48)], leaves=[4])
            refused(_lib.MI_EINVAL, ["stream 6"], leaves=[6])
            refused(_lib.MI_EINVAL, ["stream 2 a second time"], joins=[(2, K16)], leaves=[2])
        same_labels(br, parts)
        x, present = parts.rows(rng), _present(parts, rng)
        np.testing.assert_array_equal(one_tick(br, x, present), parts.tick(x, present), err_msg=f"tick {t}")
    parts.check_state(br)


def test_a_waiting_call_has_the_last_word(ctx, mk):
    """a waiting call between a change and the submit that carries it decides the pin's flags, and device and roster agree
    afterwards.  Against a twin driven by the waiting calls alone: LEAVE then add_member (the twin: remove + add), JOIN then
    remove_member (the twin: nothing, the seat stays free), JOIN then set_controls that mutes the seat (the twin: add_member
    and the same set_controls).  Rows and member counts every tick, the meters at the end"""
    legs = [K16] * 6
    a, b = (mk(ms.Bridge, 6, members=MM, rate=16000, open=legs, admit=[K48]) for _ in range(2))
    rng = np.random.default_rng(0x11)
    flags = np.full(6, L | A | O, np.uint8)
    flags[2] = L | O
    for t in range(10):
        if t == 2:
            a.remove_member(1), a.add_member(1)
            b.change(leaves=[1]), b.add_member(1)
        if t == 3:
            a.remove_member(2), b.change(leaves=[2])
        if t == 5:
            b.change(joins=[(2, K16)]), b.remove_member(2)
        if t == 7:
            a.add_member(2), a.set_controls(flags=flags)
            b.change(joins=[(2, K16)]), b.set_controls(flags=flags)
        x = np.zeros((6, 960), np.uint8)
        x[:, :320] = rng.normal(0.0, 5000.0, (6, 160)).astype(np.int16).view(np.uint8)
        present = np.ones(6, np.uint8)
        present[2] = not 3 <= t < 7
        np.testing.assert_array_equal(one_tick(b, x, present), one_tick(a, x, present), err_msg=f"tick {t}")
        assert [a.member_count(c) for c in range(2)] == [b.member_count(c) for c in range(2)], t
    assert bytes(a.volume_state()) == bytes(b.volume_state())
    np.testing.assert_array_equal(a.volume_max().view(np.uint32), b.volume_max().view(np.uint32))


def test_churning_bridge_example_runs(tmp_path):
    """120 ticks of a 16 kHz room of mu-law trunks whose seats change hands every four ticks, three ticks in flight, through the
    plain-C example; it checks its own pitch and return codes and prints the roster and the active speaker"""
    pkg, exe = os.path.join(ROOT, "mediastreamer2_amd"), tmp_path / "churning_bridge"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "churning_bridge.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines[-1] == "ok", (run.stdout, run.stderr)
    assert len(lines) == 7 and all("room 3" in l and "speaker" in l for l in lines[:-1]), run.stdout
    print(run.stdout)
