"""GPU parity of bridges whose legs each bring their own codec (mi_bridge_create_legs, include/msmi355x_bridge.h): A-law,
mu-law and 16-bit PCM legs, at their own rates, in one conference and one launch per tick.

The yardstick is the parts on the C ABI -- mi_g711_decode once per law over that law's rows (PCM rows copied) ->
mi_volume_process (a batch per leg rate) -> mi_resampler_process_masked -> mi_mixer_process -> mi_resampler_process_masked
-> mi_g711_encode once per law -- and every comparison is BIT-EXACT: output bytes, mi_volume_state bytes, meter maxima."""
import numpy as np
import pytest

import mediastreamer2_amd as ms
from bridge_parts import mk  # noqa: F401 (a fixture)
from bridge_parts import one_tick as _one_tick
from bridge_parts import pair as _pair
from mediastreamer2_amd import _lib

pytestmark = pytest.mark.gpu

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
def _run_with_controls(br, parts, nticks, seed):
    """AGC and DC removal on, an inactive pin, an input gain != 1, a pin with its output off (moved to another pin half
    way), a seeded fifth of the legs absent per tick"""
    n = parts.n
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
    rng = np.random.default_rng(seed)
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


def _same_rate_legs(n, rate=8000):
    return [(rate, (PCMU, PCMA, PCM16)[s % 3], (PCMA, PCM16, PCMU)[s % 3]) for s in range(n)]


@pytest.mark.parametrize("nconf", [1, 9])
@pytest.mark.parametrize("mm", [3, 9, 35])
def test_same_rate_mixed_codecs(ctx, mk, mm, nconf):
    """8 kHz, the three in-codecs and three out-codecs in turn: 9 members give one wavefront all three kinds, 35 give phase
    (A) a second, partial round of 32 members; 12 ticks reuse each staging slot four times"""
    legs = _same_rate_legs(mm * nconf)
    br = mk(ms.Bridge, mm * nconf, members=mm, rate=8000, legs=legs)
    _run_with_controls(br, _pair(br, ctx, mk, mm, 8000, legs), 12, 0x1E650 + mm)


WIDE48 = [(8000, PCMU, PCMU), (8000, PCMA, PCMA), (16000, PCM16, PCM16), (48000, PCM16, PCM16), (16000, PCM16, PCMA),
          (8000, PCMU, PCMA), (8000, PCMA, PCM16), (48000, PCM16, PCM16), (16000, PCM16, PCM16)]
WIDE16 = [(8000, PCMU, PCMU), (8000, PCMA, PCMA), (16000, PCM16, PCM16), (8000, PCMA, PCMU), (16000, PCM16, PCMA),
          (16000, PCM16, PCM16), (8000, PCMU, PCM16), (8000, PCMU, PCMU), (16000, PCMA, PCM16)]


@pytest.mark.parametrize("nconf", [1, 9])
@pytest.mark.parametrize("conf,table", [(48000, WIDE48), (16000, WIDE16)], ids=["48k", "16k"])
def test_mixed_rates_and_codecs(ctx, mk, conf, table, nconf):
    """8 kHz mu-law, 8 kHz A-law, 16 kHz PCM and 48 kHz PCM legs side by side in a 48 kHz conference of 9, one 16 kHz leg PCM
    in and A-law out; and the deployment this is built for: 8 kHz G.711 legs and 16 kHz PCM legs in a 16 kHz mix (ratio 2)"""
    legs = table * nconf
    br = mk(ms.Bridge, 9 * nconf, members=9, rate=conf, legs=np.array(legs, np.int32))
    _run_with_controls(br, _pair(br, ctx, mk, 9, conf, legs), 12, 0x1E651)


@pytest.mark.parametrize("conf,legs", [(8000, _same_rate_legs(6)), (16000, WIDE16[:6])], ids=["same-rate", "rated"])
def test_row_tails_and_unwritten_rows(ctx, mk, conf, legs):
    """What a tick leaves alone.  collect() hands out the DOWNLOAD of the slot's device rows, so a pattern written into the
    host views would be replaced whole by the next download whatever the kernel did; the pattern that can be held against
    the kernel is what the device rows hold.  The tails past leg_bytes hold the zeros of creation and no launch may touch
    them, while the legs' own bytes are audio (not zeros); a pin whose output is turned off keeps, slot by slot, the
    bytes of the last tick that wrote its row; a removed member's row reads zeros over the whole pitch."""
    n, mm = 6, 3
    br = mk(ms.Bridge, n, members=mm, rate=conf, legs=legs)
    parts = _pair(br, ctx, mk, mm, conf, legs)
    assert (parts.out_bytes < parts.out_pitch).any()  # there are tails to keep
    rng = np.random.default_rng(0x7A11)
    seen = []
    for t in range(10):
        if t == 3:
            parts.flags[[1, 4]] = L | A
        if t == 7:
            br.remove_member(2)
            parts.flags[2] = 0
            parts.held[:, 2] = 0
        if t in (3, 7):
            br.set_controls(flags=parts.flags)
            parts.set_controls()
        x = parts.rows(rng)
        got = _one_tick(br, x)
        np.testing.assert_array_equal(got, parts.tick(x), err_msg=f"tick {t}")
        seen.append(got)
        for s in range(n):
            assert not got[s, parts.out_bytes[s]:].any(), (t, s)
    for s in range(n):
        assert all(seen[t][s, :parts.out_bytes[s]].any() for t in range(3)), s  # the pattern is not zeros
    for t in range(3, 7):  # output off: the slot's row as its last writer left it, over the whole pitch
        for s in (1, 4):
            np.testing.assert_array_equal(seen[t][s], seen[t % 3][s], err_msg=f"tick {t} leg {s}")
    for t in range(7, 10):
        assert seen[t - 3][2].any() and not seen[t][2].any(), t
        np.testing.assert_array_equal(seen[t][1], seen[t % 3][1])
    assert br.in_flight() == 0


@pytest.mark.parametrize("conf,rates,pair", [(8000, [8000] * 6, (PCM16, PCMA)), (16000, [8000, 16000, 8000, 8000, 16000, 16000], (PCMA, PCMU))],
                         ids=["same-rate", "rated"])
def test_uniform_legs_are_the_old_bridge(ctx, mk, conf, rates, pair):
    """legs= with one codec pair everywhere is mi_bridge_create_rated's bridge: the same tick_bytes, 12 ticks byte for byte"""
    n, mm = 6, 3
    old = mk(ms.Bridge, n, members=mm, rate=conf, in_codec=pair[0], out_codec=pair[1], leg_rates=rates)
    new = mk(ms.Bridge, n, members=mm, rate=conf, legs=[(r, pair[0], pair[1]) for r in rates])
    assert new.tick_bytes() == old.tick_bytes()
    assert [new.leg_codec(s) for s in range(n)] == [pair] * n == [old.leg_codec(s) for s in range(n)]
    assert [new.leg_bytes(s) for s in range(n)] == [old.leg_bytes(s) for s in range(n)]
    p = ms.VolumeBatch.default_params()
    p.agc_enabled = 1
    old.set_volume_params([p] * n)
    new.set_volume_params([p] * n)
    rng = np.random.default_rng(0x01D)
    for t in range(12):
        shape = (n, old.len)
        x = rng.integers(0, 256, shape, dtype=np.uint8) if pair[0] else rng.normal(0, 5000, shape).astype(np.int16)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        want = _one_tick(old, x, present)
        got = _one_tick(new, x.view(np.uint8).reshape(n, -1), present)
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, want.view(np.uint8).reshape(n, -1), err_msg=f"tick {t}")
    assert bytes(new.volume_state()) == bytes(old.volume_state())
    np.testing.assert_array_equal(new.volume_max().view(np.uint32), old.volume_max().view(np.uint32))


def test_leg_views(ctx, mk):
    """leg_in / leg_out: a leg's own slice of a staging row, typed by its codec"""
    legs = WIDE16[:6]
    br = mk(ms.Bridge, 6, members=3, rate=16000, legs=legs)
    h_in, h_present = br.acquire()
    assert h_in.dtype == np.uint8 and h_in.shape == (6, 320) and h_present.shape == (6,)
    for s, (rate, ic, oc) in enumerate(legs):
        v = br.leg_in(h_in, s)
        assert v.dtype == (np.uint8 if ic else np.int16) and v.shape == (rate // 100,)
        v[:] = 0xD5 if ic == PCMA else 0xFF if ic == PCMU else 0
        assert np.shares_memory(v, h_in)
    br.submit()
    out = br.collect()
    assert out.dtype == np.uint8 and out.shape == (6, 320)
    for s, (rate, ic, oc) in enumerate(legs):
        v = br.leg_out(out, s)
        assert v.dtype == (np.uint8 if oc else np.int16) and v.shape == (rate // 100,)
    with pytest.raises(ms.MiError):
        br.leg_codec(6)
    with pytest.raises(ms.MiError):
        br.leg_bytes(-1)


def test_membership(ctx, mk):
    """reset_streams and add_member after a remove_member, on a G.711 leg and on a PCM leg of a mixed rated bridge: from
    that tick on the leg is a fresh parts chain (fresh meter, zero resampler histories), the others carry on"""
    mm, conf = 3, 16000
    legs = WIDE16[:6]  # legs 0, 1, 3 G.711 at 8 kHz (3 in conference 1), 2, 4, 5 PCM in at 16 kHz
    n = len(legs)
    br = mk(ms.Bridge, n, members=mm, rate=conf, legs=legs)
    parts = _pair(br, ctx, mk, mm, conf, legs)
    rng = np.random.default_rng(0x3E3B)
    gone = {0: (4, 7), 5: (5, 8)}  # leg: (removed at, added back at)
    for t in range(11):
        present = np.ones(n, np.uint8)
        if t == 2:
            for s in (1, 2):
                br.reset_streams(s, 1)
                parts.restart(s)
        for s, (off, on) in gone.items():
            if t == off:
                br.remove_member(s)
                parts.flags[s] = 0
                parts.set_controls()
                parts.held[:, s] = 0
                assert br.member_count(s // mm) == mm - 1
            if off <= t < on:
                present[s] = 0  # nobody sends on a pin that is not plumbed
            if t == on:
                br.add_member(s)
                parts.flags[s] = L | A | O
                parts.set_controls()
                parts.restart(s)
        x = parts.rows(rng)
        np.testing.assert_array_equal(_one_tick(br, x, present), parts.tick(x, present), err_msg=f"tick {t}")
    parts.check_state(br)


def test_refusals(ctx, mk):
    def refused(value, *a, **kw):
        with pytest.raises(ms.MiError) as e:
            mk(ms.Bridge, *a, **kw)
        assert e.value.code == _lib.MI_ENOTSUP and str(value) in str(e.value), str(e.value)

    ok = [(8000, PCMU, PCMU)] * 6
    refused("leg 5 names codec 7", 6, members=3, rate=8000, legs=ok[:5] + [(8000, PCMU, 7)])
    refused("leg 3 names codec -1", 6, members=3, rate=8000, legs=ok[:3] + [(8000, -1, PCMU)] + ok[4:])
    refused("leg 4", 6, members=3, rate=8000, legs=ok[:4] + [(8000, PCMA, PCMU)] + ok[5:], plc=True)   # plc wants one pair
    refused("leg 5 at 16000", 6, members=3, rate=8000, legs=ok[:5] + [(16000, PCM16, PCM16)])           # above the conference
    refused("leg 5 at 8000 Hz in a 32000 Hz conference is ratio 4", 6, members=3, rate=32000,
            legs=[(32000, PCM16, PCM16)] * 5 + [(8000, PCMU, PCMU)])
    br = mk(ms.Bridge, 6, members=3, rate=8000, legs=_same_rate_legs(6))                                 # the context is usable afterwards
    assert _one_tick(br, np.zeros((6, 160), np.uint8)).shape == (6, 160)


def test_plc_with_uniform_legs_is_the_plc_bridge(ctx, mk):
    """plc=1 with one codec pair through legs= works and equals the existing plc bridge, lost ticks concealed"""
    mm, n, conf, nticks = 3, 6, 16000, 8
    old = mk(ms.Bridge, n, members=mm, rate=conf, in_codec=PCMU, out_codec=PCMA, leg_rates=[8000] * n, plc=True)
    new = mk(ms.Bridge, n, members=mm, rate=conf, legs=[(8000, PCMU, PCMA)] * n, plc=True)
    assert new.tick_bytes() == old.tick_bytes() == (80, 80)
    lost = {1: {2}, 4: {4, 5, 6}}
    rng = np.random.default_rng(21)
    for t in range(nticks):
        x = rng.integers(0, 256, (n, 80), dtype=np.uint8)
        present = np.array([0 if t in lost.get(s, ()) else 1 for s in range(n)], np.uint8)
        np.testing.assert_array_equal(_one_tick(new, x, present), _one_tick(old, x, present), err_msg=f"tick {t}")
    assert bytes(new.volume_state()) == bytes(old.volume_state())


def test_gateway_bridge_example_runs(tmp_path):
    """300 ticks of 384 legs -- mu-law and A-law trunks and 16 kHz PCM members in 16 kHz conferences -- through the plain-C
    example; it checks its own row sizes and return codes"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg, exe = os.path.join(root, "mediastreamer2_amd"), tmp_path / "gateway_bridge"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "gateway_bridge.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", (run.stdout, run.stderr)
