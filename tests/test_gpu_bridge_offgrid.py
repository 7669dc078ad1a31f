"""GPU parity of bridges with legs at 44 100 Hz (mi_bridge_create_offgrid, include/msmi355x_bridge.h): L16 / 44 100 members, a
441-sample tick -- 55 groups of eight and one sample -- and resamplers of 48 to 264 taps on per-phase tables of 28 to 92 KB
read from memory, inside the bridge's one launch per tick (bridge_offgrid_kernel, csrc/bridge_offgrid.hip), next to legs of
every older form.

The yardstick is tests/bridge_parts.py's Parts on the C ABI -- mi_g711_decode once per law -> [mi_plc_process] ->
mi_volume_process (a batch per leg rate) -> mi_resampler_process_masked (leg -> conference) -> mi_mixer_process ->
mi_resampler_process_masked (conference -> leg) -> mi_g711_encode once per law --, tests/bridge_open_parts.py's for seats that
change hands, and every comparison with it is BIT-EXACT over all legs, samples and ticks: output rows over the whole pitch
(the tails past a leg's 882 or 441 bytes stay as they were), mi_volume_state bytes (the meters' float state word for word),
meter maxima.  The bridge has no read-out of a resampler's history or of the concealer's state: they are held to the parts
through every later tick's output, which is a function of them -- the rows of a leg that was absent, or whose pin had no
output, match on the following ticks only if both histories stayed as the parts' did, and the 45 ticks of the concealment
test replay the concealer's whole state machine.  The parts themselves (mi_resampler at the new pairs) are held to the
oracle's resampler by the criterion of tests/test_gpu_resample.py."""
import os
import subprocess

import numpy as np
import pytest

import mediastreamer2_amd as ms
from bridge_open_parts import OpenConcealedParts, open_pair, same_labels, union
from bridge_parts import NTICKS, ConcealedParts, _Legs, assert_same_meters, assert_same_rows, leg_rows, loss_patterns, mk, one_tick, up16  # noqa: F401 (mk: a fixture)
from bridge_parts import pair as _pair
from mediastreamer2_amd import _lib
from test_gpu_resample import RMS_TOL, _run_both  # the criterion applied to (44100, 48000, 441), as it stands there

pytestmark = pytest.mark.gpu

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16, ULAW = (PCM16, PCM16), (PCMU, PCMU)
CD = 44100
KCD, K8U, K16 = (CD, *P16), (8000, *ULAW), (16000, *P16)
MIXES = (8000, 12000, 16000, 24000, 32000, 48000)


def _agc(br, parts, n):
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    br.set_volume_params([p] * n)
    parts.set_params([p] * n)


@pytest.mark.parametrize("rate", [8000, 12000, 16000, 24000, 32000])
@pytest.mark.parametrize("down", [True, False], ids=["from-44100", "to-44100"])
def test_the_parts_at_the_new_pairs(ctx, oracle, rate, down):
    """mi_resampler 44 100 -> r and r -> 44 100 against the oracle's resampler, 4 streams, 12 ticks of one whole 10 ms block: at
    most 1 LSB and RMS_TOL of full scale, the criterion of tests/test_gpu_resample.py for (44100, 48000, 441), unchanged"""
    a, b = (CD, rate) if down else (rate, CD)
    worst, rms = _run_both(ctx, oracle, a, b, nstreams=4, in_len=a // 100, nticks=12)
    print(f"mi_resampler {a} -> {b} vs the oracle: max |diff| {worst} LSB, rms {rms:.3e} of full scale")
    assert worst <= 1, f"max |gpu-oracle| = {worst} LSB"
    assert rms <= RMS_TOL, f"rms = {rms}"


def test_one_conference_with_every_form(ctx, mk):
    """2 conferences x 6 members in a 16 kHz mix: whole below (8 kHz mu-law), 44.1 kHz PCM, at the mix, 44.1 kHz mu-law in and
    A-law out (a G.711 leg's tail group is one code byte), whole above (48 kHz: the rows are 480 samples) and a : b (12 kHz).  12
    ticks reuse every staging slot and carry the histories, every byte of every row's tail random on the way in.  AGC and DC
    removal on (the tail word's padding must stay zero under the DC offset); pin 1, a 44.1 kHz one, without MI_MIX_OUTPUT for the
    first half -- its out-history stays and its row is held per slot -- and with it for the second; pin 3 muted with an input
    gain, pin 9 with a gain; a seeded fifth of the legs absent per tick, whose histories and meters must have stayed put for
    the later ticks to match"""
    mm, conf, nticks = 6, 16000, 12
    legs = [K8U, KCD, K16, (CD, PCMU, PCMA), (48000, *P16), (12000, *P16)] * 2
    n = len(legs)
    br = mk(ms.Bridge, n, members=mm, rate=conf, offgrid=legs)
    parts = _pair(br, ctx, mk, mm, conf, legs)
    assert br.tick_bytes() == (960, 960) and br.leg_bytes(1) == (882, 882) and br.leg_bytes(3) == (441, 441)
    _agc(br, parts, n)
    parts.flags[1] = L | A
    parts.flags[3] = L | O
    parts.gain[3] = 1.6
    parts.gain[9] = 0.7
    br.set_controls(flags=parts.flags, gain=parts.gain)
    parts.set_controls()
    rng = np.random.default_rng(0x0FF6)
    for t in range(nticks):
        if t == nticks // 2:
            parts.flags[1], parts.flags[mm + 1] = L | A | O, L | A
            br.set_controls(flags=parts.flags)
            parts.set_controls()
        x = parts.rows(rng)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        if t in (3, 4, 5):
            present[1] = 0  # the 44.1 kHz leg of conference 0, three ticks running
        got, want = one_tick(br, x, present), parts.tick(x, present)
        np.testing.assert_array_equal(got, want, err_msg=f"tick {t}")
    parts.check_state(br)


@pytest.mark.parametrize("conf", MIXES)
def test_every_mix(ctx, mk, conf):
    """2 conferences x 3 members: a 44.1 kHz PCM leg, a leg at the mix's rate and an 8 kHz mu-law leg (in the 8 kHz mix a 16 kHz
    PCM leg), 8 ticks.  8 kHz is the 264-tap filter and the 263-sample history; 16 and 32 kHz are the 441-phase tables (441 : 160
    and 441 : 320); 12 and 24 kHz have 147; at 48 kHz the leg is BELOW the mix and the 56-tap filter is the out_resampler's"""
    mm, nticks = 3, 8
    third = K16 if conf == 8000 else K8U
    legs = [KCD, (conf, *P16), third] * 2
    n = len(legs)
    br = mk(ms.Bridge, n, members=mm, rate=conf, offgrid=legs)
    parts = _pair(br, ctx, mk, mm, conf, legs)
    _agc(br, parts, n)
    rng = np.random.default_rng(0xCD00 + conf // 100)
    for t in range(nticks):
        x = parts.rows(rng)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        got, want = one_tick(br, x, present), parts.tick(x, present)
        np.testing.assert_array_equal(got, want, err_msg=f"tick {t}")
    parts.check_state(br)


class CdConcealedParts(ConcealedParts):
    """ConcealedParts whose plc-less inner bridge is an offgrid= one: its rows are 882 bytes of PCM in a pitch of 896, so the
    concealed PCM is laid into rows of that pitch (ConcealedParts itself expects a pitch of exactly 2 * width)"""

    def __init__(self, ctx, mk, mm, conf, legs):
        _Legs.__init__(self, ctx, legs, lambda widest: widest)
        self.plc = {int(r): mk(ms.PlcBatch, self.n, int(r), max_block=self.width) for r in sorted(set(self.rates))}
        self.inner = mk(ms.Bridge, self.n, members=mm, rate=conf, offgrid=[(r, PCM16, oc) for r, oc in zip(self.rates, self.oc)])
        assert self.inner.tick_bytes()[0] == up16(2 * self.width)
        self.t.cuda.synchronize()

    def tick(self, x, present):
        pcm = np.ascontiguousarray(self.conceal(x, present)).view(np.uint8)
        rows = np.zeros((self.n, self.inner.tick_bytes()[0]), np.uint8)
        rows[:, :pcm.shape[1]] = pcm
        return one_tick(self.inner, rows)


class CdOpenConcealedParts(OpenConcealedParts):
    """OpenConcealedParts likewise: a PlcBatch per admitted rate and a plc-less OPEN offgrid= bridge behind them, the concealed
    PCM laid into rows of its pitch"""
    tick = CdConcealedParts.tick

    def __init__(self, ctx, mk, mm, conf, legs, admit):
        kinds = union(legs, admit)
        widest = max(k[0] for k in kinds) // 100
        _Legs.__init__(self, ctx, legs, lambda _: widest)
        self.plc = {r: mk(ms.PlcBatch, self.n, r, max_block=self.width) for r in sorted(set(k[0] for k in kinds))}
        behind = lambda k: (k[0], PCM16, k[2])  # behind the concealer a leg's input is PCM
        self.inner = mk(ms.Bridge, self.n, members=mm, rate=conf, offgrid=[behind(k) for k in legs], admit=[behind(k) for k in kinds])
        assert self.inner.tick_bytes()[0] == up16(2 * self.width)
        self.t.cuda.synchronize()


def test_concealment(ctx, mk, oracle):
    """cfg.plc = 1, one conference of a 44.1 kHz PCM leg, an 8 kHz mu-law leg and a 16 kHz PCM leg in a 16 kHz mix, NTICKS ticks
    of bridge_parts' loss patterns: the 25-tick outage (fade, silence, the cross-fade back) on the 44.1 kHz leg, single losses
    and 15 % random loss on the others.  Bit for bit the decoders -> mi_plc_process per rate (441-sample blocks in the 44.1 kHz
    batch) -> the plc-less offgrid= bridge, the relation of tests/test_gpu_bridge_concealed.py"""
    mm, conf = 3, 16000
    legs = [KCD, K8U, K16]
    n = len(legs)
    br = mk(ms.Bridge, n, members=mm, rate=conf, offgrid=legs, plc=True)
    parts = CdConcealedParts(ctx, mk, mm, conf, legs)
    assert br.tick_bytes() == (896, 896) == parts.inner.tick_bytes()
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    br.set_volume_params([p] * n)
    parts.inner.set_volume_params([p] * n)
    x = leg_rows(oracle, legs, NTICKS)
    present = loss_patterns(6, NTICKS)[:, [3, 1, 5]]
    assert (present[12:37, 0] == 0).all() and present[:12, 0].all() and present[37:, 0].all()
    for t in range(NTICKS):
        assert_same_rows(br, one_tick(br, x[t], present[t]), parts.tick(x[t], present[t]), t)
    assert_same_meters(br, parts.inner)


def test_open_seats(ctx, mk):
    """2 conferences x 4 members, the initial legs 8 kHz mu-law, 44.1 kHz PCM and 16 kHz PCM admitted; 16 ticks with three in
    flight from tick 3 on.  Seat 1 goes 8 kHz -> 44.1 kHz (tick 3) -> 16 kHz (tick 6) -> 44.1 kHz (tick 10): both histories zeroed at
    the new lengths, a fresh meter, and back; seat 6 leaves on tick 4 and rejoins at 44.1 kHz on tick 8.  Every tick's rows over
    the whole pitch against the yardstick -- the ticks submitted before a change, collected after it, among them --, the labels
    at once, the meters at the end"""
    mm, conf, nticks = 4, 16000, 16
    legs, admit = [K8U] * 8, [KCD, K16]
    script = {3: ([(1, KCD)], []), 4: ([], [6]), 6: ([(1, K16)], []), 8: ([(6, KCD)], []), 10: ([(1, KCD)], [])}
    n = len(legs)
    br = mk(ms.Bridge, n, members=mm, rate=conf, offgrid=legs, admit=admit)
    parts = open_pair(br, ctx, mk, mm, conf, legs, admit)
    assert br.tick_bytes() == (896, 896)
    _agc(br, parts, n)
    rng = np.random.default_rng(0x0E0E)
    want, got = [], []
    for t in range(nticks):
        if t in script:
            joins, leaves = script[t]
            assert br.in_flight() == 3  # the change is made with three ticks submitted and not collected
            br.change(joins=joins, leaves=leaves)
            for s in leaves:
                parts.leave_seat(s)
            for s, kind in joins:
                parts.join_seat(s, kind)
            same_labels(br, parts)
        x = parts.rows(rng)
        present = ((rng.random(n) >= 0.2) & ((parts.flags & L) != 0)).astype(np.uint8)
        want.append(parts.tick(x, present))
        if br.in_flight() == 3:
            got.append(br.collect().copy())
        h_in, h_present = br.acquire()
        h_in[:] = x
        h_present[:] = present
        br.submit()
    while br.in_flight():
        got.append(br.collect().copy())
    assert len(got) == nticks
    for t in range(nticks):
        np.testing.assert_array_equal(got[t], want[t], err_msg=f"tick {t}")
    assert br.leg_rate(1) == CD and br.leg_rate(6) == CD and br.leg_bytes(1) == (882, 882)
    parts.check_state(br)


def test_open_seats_with_concealment(ctx, mk):
    """cfg.plc = 1 on an open bridge, one conference of four 8 kHz mu-law seats, 44.1 kHz PCM and 16 kHz PCM admitted: seat 1
    goes 8 kHz -> 44.1 kHz (tick 3: a fresh concealer in the 44.1 kHz class) -> 16 kHz (tick 8) -> 44.1 kHz (tick 11) and is
    lost on ticks 5, 6 and 12, seat 2 on ticks 4 and 9; 14 ticks bit for bit the decoders -> mi_plc_process per admitted rate ->
    the plc-less open offgrid= bridge"""
    mm, conf, nticks = 4, 16000, 14
    legs, admit = [K8U] * 4, [KCD, K16]
    script = {3: KCD, 8: K16, 11: KCD}
    br = mk(ms.Bridge, mm, members=mm, rate=conf, offgrid=legs, admit=admit, plc=True)
    parts = CdOpenConcealedParts(ctx, mk, mm, conf, legs, admit)
    assert br.tick_bytes() == (896, 896) == parts.inner.tick_bytes()
    rng = np.random.default_rng(0x9C9C)
    for t in range(nticks):
        if t in script:
            br.change(joins=[(1, script[t])])
            parts.join_seat(1, script[t])
            assert br.leg_rate(1) == script[t][0]
        x = rng.integers(0, 256, (mm, 896), dtype=np.uint8)
        for s in np.nonzero(parts.ic == PCM16)[0]:
            x[s, :parts.in_bytes[s]] = rng.normal(0.0, 4000.0, parts.leg_len[s]).astype(np.int16).view(np.uint8)
        present = np.ones(mm, np.uint8)
        present[1] = t not in (5, 6, 12)
        present[2] = t not in (4, 9)
        assert_same_rows(br, one_tick(br, x, present), parts.tick(x, present), t)
    assert_same_meters(br, parts.inner)


def test_no_such_leg_is_the_open_bridge(ctx, mk):
    """offgrid= with legs and admitted kinds on the grid only is open=: the same tick bytes, 6 ticks and the meter state bit for
    bit"""
    n, mm, conf = 8, 4, 16000
    legs, admit = [K8U, (24000, *P16), K16, (12000, *P16)] * 2, [(48000, *P16)]
    old, new = mk(ms.Bridge, n, members=mm, rate=conf, open=legs, admit=admit), mk(ms.Bridge, n, members=mm, rate=conf, offgrid=legs, admit=admit)
    assert new.tick_bytes() == old.tick_bytes() == (960, 960)
    assert [new.leg_bytes(s) for s in range(n)] == [old.leg_bytes(s) for s in range(n)]
    p = ms.VolumeBatch.default_params()
    p.agc_enabled = 1
    old.set_volume_params([p] * n)
    new.set_volume_params([p] * n)
    rng = np.random.default_rng(0x5A3F)
    for t in range(6):
        x = rng.integers(0, 256, (n, old.tick_bytes()[0]), dtype=np.uint8)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        if t == 3:
            for b in (old, new):
                b.change(joins=[(2, (48000, *P16))])
        np.testing.assert_array_equal(one_tick(new, x, present), one_tick(old, x, present), err_msg=f"tick {t}")
    assert bytes(new.volume_state()) == bytes(old.volume_state())
    np.testing.assert_array_equal(new.volume_max().view(np.uint32), old.volume_max().view(np.uint32))


def test_refusals(ctx, mk):
    """through the library, before anything is allocated: the texts name the leg or admitted kind, both rates and the reason;
    the eight older constructors keep refusing 44.1 kHz in their own words; a bridge that does not admit a 44.1 kHz kind
    refuses a JOIN of one; the context stays usable"""
    def refused(values, *a, **kw):
        with pytest.raises(ms.MiError) as e:
            mk(ms.Bridge, *a, **kw)
        assert e.value.code == _lib.MI_ENOTSUP, str(e.value)
        for v in values:
            assert str(v) in str(e.value), str(e.value)

    new = "mi_bridge_create_offgrid"
    ok8, ok16 = [K8U] * 6, [K16] * 6
    refused([new, "leg 5 at 22050 Hz in a 16000 Hz", "220.50 samples"], 6, members=3, rate=16000, offgrid=ok16[:5] + [(22050, *P16)])
    refused([new, "leg 2 at 11025 Hz in a 8000 Hz", "110.25 samples"], 6, members=3, rate=8000, offgrid=ok8[:2] + [(11025, *P16)] + ok8[3:])
    refused([new, "admitted kind 1 at 22050 Hz in a 16000 Hz"], 6, members=3, rate=16000, offgrid=ok16, admit=[KCD, (22050, *P16)])
    refused([new, "leg 0 at 44200 Hz in a 16000 Hz", "no multiple of 800"], 6, members=3, rate=16000, offgrid=[(44200, *P16)] + ok16[:5])
    refused(["rate 44100", "no multiple of 800"], 6, members=3, rate=CD, offgrid=[KCD] * 6)
    refused([new, "leg 5 at 44100 Hz in a 4000 Hz", "441 : 40", "536 taps"], 6, members=3, rate=4000, offgrid=[(4000, *P16)] * 5 + [KCD])
    refused([new, "leg 5 at 40000 Hz in a 8000 Hz", "ratio 5"], 6, members=3, rate=8000, offgrid=ok8[:5] + [(40000, *P16)], admit=[KCD])
    refused([new, "leg 5 at 64000 Hz in a 8000 Hz", "ratio 8"], 6, members=3, rate=8000, offgrid=ok8[:5] + [(64000, *P16)])
    refused([new, "admitted kind 0 at 28000 Hz in a 8000 Hz", "7 : 2"], 6, members=3, rate=8000, offgrid=ok8, admit=[(28000, *P16)])
    refused([new, "leg 2 at 14400 Hz in a 12800 Hz", "9 : 8"], 6, members=3, rate=12800, offgrid=[(12800, *P16)] * 2 + [(14400, *P16)] + [(12800, *P16)] * 3)
    refused(["LDS", "46 members x 480 samples"], 46, members=46, rate=16000, offgrid=([KCD, (48000, *P16)] * 23))
    full = mk(ms.Bridge, 45, members=45, rate=16000, offgrid=([KCD, (48000, *P16)] * 23)[:45])  # the header's cap
    assert one_tick(full, np.zeros((45, 960), np.uint8)).shape == (45, 960)
    fifty = mk(ms.Bridge, 50, members=50, rate=48000, offgrid=[KCD] * 50)  # 58 896 bytes: the mixer's own limit
    assert one_tick(fifty, np.zeros((50, 896), np.uint8)).shape == (50, 896)
    legs = ok8[:5] + [KCD]
    for kw in ("endpoints", "concealed", "rational"):  # the older constructors keep their refusals
        refused(["leg 5 at 44100", "5.513"], 6, members=3, rate=8000, **{kw: legs})
    refused(["mi_bridge_create_ratios", "leg 5 at 44100 Hz in a 8000 Hz", "441 : 80"], 6, members=3, rate=8000, ratios=legs)
    refused(["mi_bridge_create_ratios", "leg 5 at 44100 Hz in a 8000 Hz", "441 : 80"], 6, members=3, rate=8000, open=legs)
    refused(["mi_bridge_create_ratios", "admitted kind 0 at 44100 Hz"], 6, members=3, rate=8000, open=ok8, admit=[KCD])
    refused(["leg 5 at 44100 Hz", "above"], 6, members=3, rate=8000, in_codec=PCM16, out_codec=PCM16, leg_rates=[8000] * 5 + [CD])
    refused(["44100"], 6, members=3, rate=8000, legs=legs)
    # a bridge that does not admit a 44.1 kHz kind keeps refusing a JOIN of one, whichever constructor built it
    for br in (mk(ms.Bridge, 6, members=3, rate=16000, offgrid=ok16, admit=[K8U]), mk(ms.Bridge, 6, members=3, rate=16000, open=ok16, admit=[K8U])):
        with pytest.raises(ms.MiError) as e:
            br.change(joins=[(2, KCD)])
        assert e.value.code == _lib.MI_ENOTSUP and "44100 Hz" in str(e.value), str(e.value)
        assert one_tick(br, np.zeros((6, 320), np.uint8)).shape == (6, 320)  # and stays usable


def test_cd_rate_room_example_runs(tmp_path):
    """300 ticks of a 16 kHz room of mu-law and A-law trunks, 16 kHz PCM members and L16 / 44 100 members whose bytes the host
    swaps, through the plain-C example; it checks its own row sizes and return codes"""
    pkg, exe = os.path.join(ROOT, "mediastreamer2_amd"), tmp_path / "cd_rate_room"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cd_rate_room.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", (run.stdout, run.stderr)
