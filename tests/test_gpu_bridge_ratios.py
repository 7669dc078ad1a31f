"""GPU parity of bridges with legs at 4 and 1/4 of the mix's rate and at a : b of it (mi_bridge_create_ratios,
include/msmi355x_bridge.h): a 12 kHz member of a 16 kHz room, 32 kHz members of 8, 12 and 24 kHz rooms -- the resampler's
ratio-4 tile kernels and its generic-order arithmetic inside the bridge's one launch per tick (bridge_ratios_kernel,
csrc/bridge_ratios.hip), next to legs at 1, 2, 3, 6 and 3/2 below and above.

The yardstick is tests/bridge_parts.py's Parts on the C ABI -- mi_g711_decode once per law -> mi_volume_process (a batch per
leg rate) -> mi_resampler_process_masked (leg -> conference) -> mi_mixer_process -> mi_resampler_process_masked (conference
-> leg) -> mi_g711_encode once per law -- and every comparison with it is BIT-EXACT over all legs, samples and ticks: output
bytes, mi_volume_state bytes, meter maxima.  The ratio-4 shapes lie where mi_resampler runs its tile kernel (launch_split,
csrc/resample.hip: nq <= 192, ticks of at most 576 samples on the wider side; the widest here is 480); for a : b
mi_resampler has one form, resample_generic_kernel, at every shape.  Against the oracle chain the meters are bit-exact and
the audio is held to the float resampler path's bar (tests/test_gpu_resample.py): 1e-4 RMS of full scale and at most 1 LSB."""
import os
import subprocess
from math import gcd

import numpy as np
import pytest

import mediastreamer2_amd as ms
from bridge_parts import FLOAT_STATE, INT_STATE, ConcealedParts, Parts, assert_same_meters, assert_same_rows, leg_rows, loss_patterns, mk, one_tick  # noqa: F401 (mk: a fixture)
from bridge_parts import bits as _bits
from bridge_parts import pair as _pair
from conftest import synth_pcm
from mediastreamer2_amd import _lib

pytestmark = pytest.mark.gpu

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16, ULAW = (PCM16, PCM16), (PCMU, PCMU)

# conference rate, and the five members of a conference in pin order (members = 3 takes the first three)
CASES = {
    "a-12k-in-16k": (16000, [(12000, *P16), (8000, *ULAW), (16000, *P16), (32000, *P16), (12000, *P16)]),
    "b-16k-32k-in-12k": (12000, [(16000, *P16), (32000, *P16), (12000, *P16), (8000, *ULAW), (32000, *P16)]),
    "c-32k-in-8k": (8000, [(32000, *P16), (8000, *ULAW), (32000, PCMU, PCM16), (8000, *P16), (32000, *P16)]),
    "d-12k-in-48k": (48000, [(12000, *P16), (32000, *P16), (48000, *P16), (8000, PCMA, PCMA), (12000, *P16)]),
    "e-24k-40k-8k-in-32k": (32000, [(24000, *P16), (40000, *P16), (8000, *ULAW), (32000, *P16), (24000, *P16)]),
    "f-3200-in-2400": (2400, [(3200, *P16), (2400, *P16), (3200, *P16), (2400, *P16), (3200, *P16)]),
    "f-2400-in-3200": (3200, [(2400, *P16), (3200, *P16), (2400, *P16), (3200, *P16), (2400, *P16)]),
}


def _legs(case, mm, nconf=2):
    conf, five = CASES[case]
    return conf, [five[s % mm] for s in range(mm * nconf)]


@pytest.mark.parametrize("mm", [3, 5])
@pytest.mark.parametrize("case", list(CASES))
def test_equal_to_the_parts(ctx, mk, case, mm):
    """(a) 3/4 below the mix beside ratio 2 both ways, a leg tick of 120 samples, 15 groups; (b) 4/3 and 8/3 above, the
    127-sample history, rows wider than the mix, 2/3 beside them; (c) ratio 4 above, a G.711 leg above the mix; (d) ratio 4
    below at 480 samples beside 3/2 and 6; (e) 3/4, 5/4 and 4 in one conference; (f) ticks of 24 and 32 samples, shorter than
    either history (47 / 63): the new history is partly the old one.  Two conferences; 3 members leave a wave idle, 5 give wave
    0 a second member on the scratch its first has just read out.  12 ticks reuse every staging slot and carry the
    histories; AGC and DC removal on; pin 1 muted with an input gain != 1, pin 3 with a gain; pin 0 without MI_MIX_OUTPUT for
    the first half and the same pin of the second conference for the second half, a seeded fifth of the legs absent per tick:
    the histories of absent and output-less pins must have stayed as they were for the later ticks to match."""
    n, nticks = 2 * mm, 12
    conf, legs = _legs(case, mm)
    br = mk(ms.Bridge, n, members=mm, rate=conf, ratios=legs)
    parts = _pair(br, ctx, mk, mm, conf, legs)
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    br.set_volume_params([p] * n)
    parts.set_params([p] * n)
    parts.flags[0] = L | A
    parts.flags[1] = L | O
    parts.gain[1] = 1.6
    parts.gain[3] = 0.7
    br.set_controls(flags=parts.flags, gain=parts.gain)
    parts.set_controls()
    rng = np.random.default_rng(0x4A71 + mm)
    for t in range(nticks):
        if t == nticks // 2:
            parts.flags[0], parts.flags[mm] = L | A | O, L | A
            br.set_controls(flags=parts.flags)
            parts.set_controls()
        x = parts.rows(rng)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        got, want = one_tick(br, x, present), parts.tick(x, present)
        np.testing.assert_array_equal(got, want, err_msg=f"tick {t}")
    parts.check_state(br)


@pytest.mark.parametrize("conf,kinds,gone,again", [(16000, (12000, 32000), 0, 4), (12000, (32000, 16000), 0, 4), (8000, (32000, 12000), 4, 0)],
                         ids=["remove-3/4-reset-2", "remove-8/3-reset-4/3", "remove-3/2-reset-4"])
def test_membership_and_reset(ctx, mk, conf, kinds, gone, again):
    """rooms of two kinds of members and one at the mix's rate: one removed at tick 2 and added back at tick 5, reset_streams on
    one of the other kind at tick 4: the parts with both resamplers and the meter restarted at those ticks; the removed row
    reads zeros over the whole pitch"""
    mm = 3
    one, other = kinds
    legs = [(one, *P16), (other, *P16), (conf, *P16), (one, *P16), (other, *P16), (other, *P16)]
    n = len(legs)
    br = mk(ms.Bridge, n, members=mm, rate=conf, ratios=legs)
    parts = _pair(br, ctx, mk, mm, conf, legs)
    rng = np.random.default_rng(0x3E3C + gone + conf)
    off, on = 2, 5
    for t in range(9):
        present = np.ones(n, np.uint8)
        if t == 4:
            br.reset_streams(again, 1)
            parts.restart(again)
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
        got = one_tick(br, x, present)
        np.testing.assert_array_equal(got, parts.tick(x, present), err_msg=f"tick {t}")
        assert got.shape[1] == br.tick_bytes()[1] and got[gone].any() == (not off <= t < on), t
    parts.check_state(br)


def test_three_ticks_in_flight(ctx, mk):
    """the 12 kHz room of (b) submitted three deep returns the rows of the same ticks submitted one at a time"""
    mm, nticks = 4, 7
    conf, legs = _legs("b-16k-32k-in-12k", mm)
    n = len(legs)
    deep, single = mk(ms.Bridge, n, members=mm, rate=conf, ratios=legs), mk(ms.Bridge, n, members=mm, rate=conf, ratios=legs)
    rng = np.random.default_rng(11)
    xs = [rng.integers(0, 256, (n, deep.tick_bytes()[0]), dtype=np.uint8) for _ in range(nticks)]
    want = [one_tick(single, x) for x in xs]
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


def test_geometry(ctx, mk):
    """the pitch is the widest leg's tick in bytes; a leg's own bytes are audio and the tails past them stay zeros; a room
    whose widest leg is an 8/3 one; ratios=None is the plain bridge"""
    legs = [(8000, *ULAW), (12000, *P16), (32000, *P16)] * 2
    br = mk(ms.Bridge, 6, members=3, rate=16000, ratios=np.array(legs, np.int32))
    assert br.tick_bytes() == (640, 640)
    assert [br.leg_bytes(s) for s in range(3)] == [(80, 80), (240, 240), (640, 640)]
    assert [br.leg_rate(s) for s in range(6)] == [l[0] for l in legs]
    assert [br.leg_codec(s) for s in range(6)] == [l[1:] for l in legs]
    with pytest.raises(ms.MiError):
        br.leg_rate(6)
    rng = np.random.default_rng(0x6E0)
    for t in range(3):
        got = one_tick(br, rng.integers(0, 256, (6, 640), dtype=np.uint8))
        for s in range(6):
            own = br.leg_bytes(s)[1]
            assert got[s, :own].any() and not got[s, own:].any(), (t, s)
            assert br.leg_out(got, s).shape == (legs[s][0] // 100,)
    above = mk(ms.Bridge, 3, members=3, rate=12000, ratios=[(32000, PCMU, PCM16), (12000, *ULAW), (8000, PCMA, PCMA)])
    assert above.tick_bytes() == (320, 640) and above.leg_bytes(0) == (320, 640) and above.leg_rate(0) == 32000
    kw = dict(members=3, rate=8000, in_codec=PCMA, out_codec=PCMU)
    plain, none = mk(ms.Bridge, 6, **kw), mk(ms.Bridge, 6, ratios=None, **kw)
    assert none.tick_bytes() == plain.tick_bytes() == (80, 80)
    for t in range(3):
        x = rng.integers(0, 256, (6, 80), dtype=np.uint8)
        np.testing.assert_array_equal(one_tick(none, x), one_tick(plain, x), err_msg=f"tick {t}")
    assert bytes(none.volume_state()) == bytes(plain.volume_state())
    with pytest.raises(AssertionError):
        ms.Bridge(ctx, 6, members=3, rate=16000, ratios=legs, rational=legs)


@pytest.mark.parametrize("plc", [False, True], ids=["", "plc"])
def test_no_such_leg_is_the_rational_bridge(ctx, mk, plc):
    """ratios= with no leg at 4, 1/4 or a : b is rational=: the same tick_bytes, 6 ticks and the meter state bit for bit"""
    n, mm, conf = 8, 4, 16000
    legs = [(8000, *ULAW), (24000, *P16), (16000, *P16), (48000, *P16)] * 2
    old, new = mk(ms.Bridge, n, members=mm, rate=conf, rational=legs, plc=plc), mk(ms.Bridge, n, members=mm, rate=conf, ratios=legs, plc=plc)
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
        np.testing.assert_array_equal(one_tick(new, x, present), one_tick(old, x, present), err_msg=f"tick {t}")
    assert bytes(new.volume_state()) == bytes(old.volume_state())
    np.testing.assert_array_equal(new.volume_max().view(np.uint32), old.volume_max().view(np.uint32))


def test_plc_equal_to_the_parts(ctx, mk, oracle):
    """a 16 kHz room of 16 kHz mu-law, 12 kHz PCM and 16 kHz PCM legs with scattered losses: bit for bit mi_g711_decode per law
    -> mi_plc_process per rate -> the plc-less ratios= bridge, the relation of tests/test_gpu_bridge_concealed.py"""
    mm, conf, nticks = 3, 16000, 45
    legs = [(16000, *ULAW), (12000, *P16), (16000, *P16)] * 2
    n = len(legs)
    br = mk(ms.Bridge, n, members=mm, rate=conf, ratios=legs, plc=True)
    parts = ConcealedParts(ctx, mk, mm, conf, legs, form="ratios")
    assert br.tick_bytes() == (320, 320) == parts.inner.tick_bytes()
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    br.set_volume_params([p] * n)
    parts.inner.set_volume_params([p] * n)
    x, present = leg_rows(oracle, legs, nticks), loss_patterns(n, nticks)
    for t in range(nticks):
        assert_same_rows(br, one_tick(br, x[t], present[t]), parts.tick(x[t], present[t]), t)
    assert_same_meters(br, parts.inner)


def _older(a, b):
    """a : b in lowest terms is a ratio the six older constructors serve"""
    hi, lo = max(a, b), min(a, b)
    return (lo == 1 and hi in (1, 2, 3, 6)) or (hi, lo) == (3, 2)


def test_rule_against_the_resampler(ctx, mk):
    """legs at 1600 a Hz in a room at 1600 b Hz, a, b in 1 .. 9: creation succeeds exactly where the older constructors serve the
    pair, or it is ratio 4, or mi_resampler_info calls both resamplers' tables direct with at most 128 taps -- the plan's
    restatement of design_filter's rule held to design_filter itself --, and the context stays usable after every refusal"""
    served = []
    for a in range(1, 10):
        for b in range(1, 10):
            g = gcd(a, b)
            ra, rb = a // g, b // g
            want = _older(ra, rb) or (min(ra, rb) == 1 and max(ra, rb) == 4)
            if not want and min(ra, rb) != 1:
                info = [mk(ms.ResamplerBatch, 1, i, o).info() for i, o in ((1600 * a, 1600 * b), (1600 * b, 1600 * a))]
                want = all(v["direct"] and v["filt_len"] <= 128 for v in info)
            legs = [(1600 * a, *P16)] * 2
            if want:
                br = mk(ms.Bridge, 2, members=2, rate=1600 * b, ratios=legs)
                assert one_tick(br, np.zeros((2, br.tick_bytes()[0]), np.uint8)).shape == (2, br.tick_bytes()[1])
                served.append((ra, rb))
            else:
                with pytest.raises(ms.MiError) as e:
                    mk(ms.Bridge, 2, members=2, rate=1600 * b, ratios=legs)
                assert e.value.code == _lib.MI_ENOTSUP and f"leg 0 at {1600 * a}" in str(e.value), str(e.value)
    new = sorted(set(r for r in served if not _older(*r)))
    print("served beyond the older constructors:", new)
    for r in [(4, 1), (1, 4), (4, 3), (3, 4), (5, 4), (5, 3), (5, 2), (6, 5), (7, 3), (8, 3), (3, 8)]:
        assert r in new, r
    for r in [(5, 1), (7, 1), (8, 1), (9, 1), (7, 2), (9, 8), (9, 4)]:
        assert r not in new, r


def test_refusals(ctx, mk):
    """through the library, before anything is allocated: the texts name leg, rates and ratio; what the concealer cannot serve
    is still its refusal; the six older constructors keep theirs; the context stays usable"""
    def refused(values, *a, **kw):
        with pytest.raises(ms.MiError) as e:
            mk(ms.Bridge, *a, **kw)
        assert e.value.code == _lib.MI_ENOTSUP, str(e.value)
        for v in values:
            assert str(v) in str(e.value), str(e.value)

    ok8, ok16, ok24 = [(8000, *ULAW)] * 6, [(16000, *P16)] * 6, [(24000, *P16)] * 6
    refused(["mi_bridge_create_ratios", "leg 5 at 44100 Hz in a 8000 Hz", "441 : 80"], 6, members=3, rate=8000, ratios=ok8[:5] + [(44100, *P16)])
    refused(["leg 5 at 40000 Hz in a 8000 Hz", "ratio 5"], 6, members=3, rate=8000, ratios=ok8[:5] + [(40000, *P16)])
    refused(["leg 5 at 28000 Hz in a 8000 Hz", "7 : 2"], 6, members=3, rate=8000, ratios=ok8[:5] + [(28000, *P16)])
    refused(["leg 4's rate 1000"], 6, members=3, rate=800, ratios=[(800, *P16)] * 4 + [(1000, *P16)] * 2)
    refused(["leg 5 names codec 3"], 6, members=3, rate=16000, ratios=ok16[:5] + [(12000, PCMU, 3)])
    refused(["leg 5", 64000], 6, members=3, rate=24000, ratios=ok24[:5] + [(64000, *P16)], plc=True)  # the concealer's: above 48 kHz
    br = mk(ms.Bridge, 6, members=3, rate=24000, ratios=ok24[:5] + [(64000, *P16)])  # 8 : 3, legal without the concealer
    assert one_tick(br, np.zeros((6, 1280), np.uint8)).shape == (6, 1280)
    refused(["LDS", "46 members x 480 samples"], 46, members=46, rate=16000, ratios=([(12000, *P16), (48000, *P16)] * 23))
    full = mk(ms.Bridge, 45, members=45, rate=16000, ratios=([(12000, *P16), (48000, *P16)] * 23)[:45])  # the header's cap
    assert one_tick(full, np.zeros((45, 960), np.uint8)).shape == (45, 960)
    for kw in ("endpoints", "concealed", "rational"):  # the older constructors keep their refusals
        refused(["leg 5 at 32000", "ratio 4"], 6, members=3, rate=8000, **{kw: ok8[:5] + [(32000, *P16)]})
        refused(["leg 2 at 12000", "1.333"], 6, members=3, rate=16000, **{kw: ok16[:2] + [(12000, *P16)] + ok16[3:]})
    br = mk(ms.Bridge, 6, members=3, rate=16000, ratios=ok16[:2] + [(12000, *P16)] + ok16[3:])  # the context is usable afterwards
    assert one_tick(br, np.zeros((6, 320), np.uint8)).shape == (6, 320)


@pytest.mark.parametrize("leg,conf", [(12000, 16000), (32000, 12000), (32000, 8000)])
def test_against_the_oracle_chain(ctx, mk, oracle, leg, conf):
    """per leg g711_decode -> Volume.chunk -> Resampler(leg, conf) -> mixer_tick -> Resampler(conf, leg); three members,
    mu-law in, PCM16 out, 12 ticks: the meters bit-exact, the audio within 1e-4 RMS of full scale and 1 LSB (the figures are
    printed).  resample_generic_kernel had not been held to the oracle at these ratios, so the unchanged parts run against it
    at the same shapes: where THEY exceed the bar the bridge's figures must equal theirs instead (profiles/bridge_ratios.md
    records both)."""
    n, ll, ns, nticks = 3, leg // 100, conf // 100, 12
    legs = [(leg, PCMU, PCM16)] * n
    br = mk(ms.Bridge, n, members=n, rate=conf, ratios=legs)
    parts = Parts(ctx, mk, n, conf, legs)
    vol = [oracle.Volume(leg) for _ in range(n)]
    mx = [oracle.Extremum(1000) for _ in range(n)]
    res_in = [oracle.Resampler(leg, conf) for _ in range(n)]
    res_out = [oracle.Resampler(conf, leg) for _ in range(n)]
    sig = np.stack([synth_pcm(40 + s, ll * nticks, sigma=3000.0, rate=leg) for s in range(n)])
    fig = {"bridge": [0.0, 0, 0], "parts": [0.0, 0, 0]}  # sum of squares, samples, worst
    for t in range(nticks):
        x = np.zeros((n, br.tick_bytes()[0]), np.uint8)
        x[:, :ll] = oracle.g711_encode(ms.MI_LAW_PCMU, sig[:, t * ll:(t + 1) * ll])
        rows = {"bridge": one_tick(br, x), "parts": parts.tick(x)}
        pcm = oracle.g711_decode(ms.MI_LAW_PCMU, x[:, :ll])
        mixed = np.zeros((n, ns), np.int16)
        for s in range(n):
            lev = vol[s].chunk(pcm[s])
            mx[s].record_max(10 * t, vol[s].v.energy)
            mixed[s] = res_in[s].process(lev)[:ns]
        mix, _ = oracle.mixer_tick(mixed)
        want = np.stack([res_out[s].process(mix[s])[:ll] for s in range(n)])
        for who, r in rows.items():
            d = np.ascontiguousarray(r[:, :2 * ll]).view(np.int16).astype(np.float64) - want
            f = fig[who]
            f[0], f[1], f[2] = f[0] + float((d * d).sum()), f[1] + d.size, max(f[2], int(np.abs(d).max()))
    rms = {who: np.sqrt(f[0] / f[1]) / 32768.0 for who, f in fig.items()}
    worst = {who: f[2] for who, f in fig.items()}
    for who in fig:
        print(f"{who} {leg} in {conf} vs oracle chain: rms {rms[who]:.3e} of full scale, max |diff| {worst[who]}")
    if rms["parts"] <= 1e-4 and worst["parts"] <= 1:
        assert rms["bridge"] <= 1e-4 and worst["bridge"] <= 1, f"rms {rms['bridge']:.3e} of full scale, max |diff| {worst['bridge']} LSB"
    else:  # a finding about resample_generic_kernel, which the bridge only repeats
        assert (rms["bridge"], worst["bridge"]) == (rms["parts"], worst["parts"]), (rms, worst)
    st, bmx = br.volume_state(), br.volume_max()
    for s in range(n):
        for name in FLOAT_STATE:
            assert _bits(getattr(st[s], name)) == _bits(getattr(vol[s].v, name)), (s, name)
        for name in INT_STATE:
            assert getattr(st[s], name) == getattr(vol[s].v, name), (s, name)
        assert _bits(bmx[s]) == _bits(mx[s].current), (s, "max")


def test_mixed_rate_room_example_runs(tmp_path):
    """300 ticks of a 16 kHz room of mu-law trunks, 12 and 32 kHz PCM members through the plain-C example; it checks its own row
    sizes and return codes"""
    pkg, exe = os.path.join(ROOT, "mediastreamer2_amd"), tmp_path / "mixed_rate_room"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mixed_rate_room.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", (run.stdout, run.stderr)
