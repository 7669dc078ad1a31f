"""GPU parity of bridges with legs at 3/2 and 2/3 of the mix's rate (mi_bridge_create_rational, include/msmi355x_bridge.h):
a 32 kHz member of a 48 kHz room, a 24 kHz member of a 16 kHz one, 12 kHz in 8 kHz -- the resampler's 3/2 and 2/3 tile-FIR
arithmetic inside the bridge's one launch per tick (bridge_rational_kernel), next to legs at 1, 2, 3 and 6 below and above.

The yardstick is tests/bridge_parts.py's Parts on the C ABI -- mi_g711_decode once per law ->
mi_volume_process (a batch per leg rate) -> mi_resampler_process_masked (leg -> conference) -> mi_mixer_process ->
mi_resampler_process_masked (conference -> leg) -> mi_g711_encode once per law -- and every comparison with it is BIT-EXACT
over all legs, samples and ticks: output bytes, mi_volume_state bytes, meter maxima.  Every shape here lies where
mi_resampler runs its tile kernel for 3/2 and 2/3 (launch_split, csrc/resample.hip: input ticks of at most 696 samples and
at most 30 KB of LDS; the widest input here is 480 samples) -- past that it takes its generic kernel, whose sums run in
another order.  Against the oracle chain the meters are bit-exact and the audio is held to the float resampler path's
tolerance (tests/test_gpu_resample.py): 1e-4 RMS of full scale and at most 1 LSB."""
import os
import subprocess

import numpy as np
import pytest

import mediastreamer2_amd as ms
from bridge_parts import FLOAT_STATE, INT_STATE, ConcealedParts, assert_same_meters, assert_same_rows, leg_rows, loss_patterns, mk, one_tick  # noqa: F401 (mk: a fixture)
from bridge_parts import bits as _bits
from bridge_parts import one_tick as _one_tick
from bridge_parts import pair as _pair
from conftest import synth_pcm
from kernel_remarks import bridge_budget, bridge_lds
from mediastreamer2_amd import _lib

pytestmark = pytest.mark.gpu

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = (PCM16, PCM16)

# conference rate, and the five members of a conference in pin order (members = 3 takes the first three)
CASES = {
    "a-24k-in-16k": (16000, [(24000, *P16), (8000, PCMU, PCMU), (16000, *P16), (48000, *P16), (24000, *P16)]),
    "b-32k-in-48k": (48000, [(32000, *P16), (8000, PCMA, PCMA), (24000, *P16), (48000, *P16), (32000, *P16)]),
    "c-12k-ulaw-in-8k": (8000, [(12000, PCMU, PCMU), (8000, PCMU, PCMU), (12000, PCMU, PCM16), (8000, *P16), (12000, PCMU, PCMU)]),
    "d-16k-36k-in-24k": (24000, [(16000, *P16), (36000, *P16), (24000, *P16), (36000, *P16), (16000, *P16)]),
}


def _legs(case, mm, nconf=2):
    conf, five = CASES[case]
    return conf, [five[s % mm] for s in range(mm * nconf)]


@pytest.mark.parametrize("mm", [3, 5])
@pytest.mark.parametrize("case", list(CASES))
def test_equal_to_the_parts(ctx, mk, case, mm):
    """(a) a 24 kHz member of a 16 kHz room of mu-law trunks and 16 kHz members, a 48 kHz one beside it at members = 5;
    (b) 32 kHz in 48 kHz beside ratios 6, 2 and 1; (c) the smallest tick, a 12 kHz mu-law leg in 8 kHz: 120 samples, 15
    groups, 5 tiles, most lanes masked off, a G.711 leg above the mix; (d) both new ratios in one 24 kHz conference.  Two
    conferences; 3 members leave a wave idle, 5 give wave 0 a second member -- a leg at 3/2 or 2/3 again -- on the scratch its
    first has just read out.  12 ticks reuse every staging slot and carry the histories; AGC and DC removal on; pin 1 muted
    with an input gain != 1, pin 3 with a gain; pin 0 (a 3/2 or 2/3 leg) without MI_MIX_OUTPUT for the first half and the
    same pin of the second conference for the second half, a seeded fifth of the legs absent per tick: the histories of
    absent and output-less pins must have stayed as they were for the later ticks to match.  All these shapes lie where
    mi_resampler runs its tile kernel for 3/2 and 2/3 (launch_split: input ticks <= 696 samples, LDS <= 30 KB)."""
    n, nticks = 2 * mm, 12
    conf, legs = _legs(case, mm)
    br = mk(ms.Bridge, n, members=mm, rate=conf, rational=legs)
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
    rng = np.random.default_rng(0x3212 + mm)
    for t in range(nticks):
        if t == nticks // 2:
            parts.flags[0], parts.flags[mm] = L | A | O, L | A
            br.set_controls(flags=parts.flags)
            parts.set_controls()
        x = parts.rows(rng)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        got, want = _one_tick(br, x, present), parts.tick(x, present)
        np.testing.assert_array_equal(got, want, err_msg=f"tick {t}")
    parts.check_state(br)


@pytest.mark.parametrize("gone,again", [(0, 4), (4, 0)], ids=["remove-2/3-reset-3/2", "remove-3/2-reset-2/3"])
def test_membership_and_reset(ctx, mk, gone, again):
    """a 24 kHz room of 16 kHz (2/3) and 36 kHz (3/2) members: one removed at tick 2 and added back at tick 5, reset_streams
    on one of the other kind at tick 4: the parts with both resamplers and the meter restarted at those ticks; the removed
    row reads zeros over the whole pitch"""
    mm, conf = 3, 24000
    legs = [(16000, *P16), (36000, *P16), (24000, *P16), (16000, *P16), (36000, *P16), (36000, *P16)]
    n = len(legs)
    br = mk(ms.Bridge, n, members=mm, rate=conf, rational=legs)
    parts = _pair(br, ctx, mk, mm, conf, legs)
    rng = np.random.default_rng(0x3E3C + gone)
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
        got = _one_tick(br, x, present)
        np.testing.assert_array_equal(got, parts.tick(x, present), err_msg=f"tick {t}")
        assert got.shape[1] == 720 and got[gone].any() == (not off <= t < on), t
    parts.check_state(br)


def test_three_ticks_in_flight(ctx, mk):
    """the 48 kHz room of (b) submitted three deep returns the rows of the same ticks submitted one at a time"""
    mm, nticks = 4, 7
    conf, legs = _legs("b-32k-in-48k", mm)
    n = len(legs)
    deep, single = mk(ms.Bridge, n, members=mm, rate=conf, rational=legs), mk(ms.Bridge, n, members=mm, rate=conf, rational=legs)
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


@pytest.mark.parametrize("leg,conf", [(32000, 48000), (24000, 16000), (12000, 8000)])
def test_against_the_oracle_chain(ctx, mk, oracle, leg, conf):
    """per leg g711_decode -> Volume.chunk -> Resampler(leg, conf) -> mixer_tick -> Resampler(conf, leg); three members,
    mu-law in, PCM16 out, 12 ticks: the meters bit-exact, the audio within 1e-4 RMS of full scale and 1 LSB (the figures are
    printed)"""
    n, ll, ns, nticks = 3, leg // 100, conf // 100, 12
    br = mk(ms.Bridge, n, members=n, rate=conf, rational=[(leg, PCMU, PCM16)] * n)
    vol = [oracle.Volume(leg) for _ in range(n)]
    mx = [oracle.Extremum(1000) for _ in range(n)]
    res_in = [oracle.Resampler(leg, conf) for _ in range(n)]
    res_out = [oracle.Resampler(conf, leg) for _ in range(n)]
    sig = np.stack([synth_pcm(40 + s, ll * nticks, sigma=3000.0, rate=leg) for s in range(n)])
    err2, cnt, worst = 0.0, 0, 0
    for t in range(nticks):
        x = np.zeros((n, br.tick_bytes()[0]), np.uint8)
        x[:, :ll] = oracle.g711_encode(ms.MI_LAW_PCMU, sig[:, t * ll:(t + 1) * ll])
        got = np.ascontiguousarray(_one_tick(br, x)[:, :2 * ll]).view(np.int16)
        pcm = oracle.g711_decode(ms.MI_LAW_PCMU, x[:, :ll])
        mixed = np.zeros((n, ns), np.int16)
        for s in range(n):
            lev = vol[s].chunk(pcm[s])
            mx[s].record_max(10 * t, vol[s].v.energy)
            mixed[s] = res_in[s].process(lev)[:ns]
        mix, _ = oracle.mixer_tick(mixed)
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
    """the pitch is the widest leg's tick in bytes; a leg's own bytes are audio and the tails past them stay zeros; a room
    whose widest leg is a 3/2 one; rational=None is the plain bridge"""
    legs = [(8000, PCMU, PCMU), (32000, PCM16, PCM16), (48000, PCM16, PCM16)] * 2
    br = mk(ms.Bridge, 6, members=3, rate=48000, rational=np.array(legs, np.int32))
    assert br.tick_bytes() == (960, 960)
    assert [br.leg_bytes(s) for s in range(3)] == [(80, 80), (640, 640), (960, 960)]
    assert [br.leg_rate(s) for s in range(6)] == [l[0] for l in legs]
    assert [br.leg_codec(s) for s in range(6)] == [l[1:] for l in legs]
    with pytest.raises(ms.MiError):
        br.leg_rate(6)
    rng = np.random.default_rng(0x6E0)
    for t in range(3):
        got = _one_tick(br, rng.integers(0, 256, (6, 960), dtype=np.uint8))
        for s in range(6):
            own = br.leg_bytes(s)[1]
            assert got[s, :own].any() and not got[s, own:].any(), (t, s)
            assert br.leg_out(got, s).shape == (legs[s][0] // 100,)
    above = mk(ms.Bridge, 3, members=3, rate=16000, rational=[(24000, PCMU, PCM16), (16000, PCMU, PCMU), (8000, PCMA, PCMA)])
    assert above.tick_bytes() == (240, 480) and above.leg_bytes(0) == (240, 480) and above.leg_rate(0) == 24000
    kw = dict(members=3, rate=8000, in_codec=PCMA, out_codec=PCMU)
    plain, none = mk(ms.Bridge, 6, **kw), mk(ms.Bridge, 6, rational=None, **kw)
    assert none.tick_bytes() == plain.tick_bytes() == (80, 80)
    for t in range(3):
        x = rng.integers(0, 256, (6, 80), dtype=np.uint8)
        np.testing.assert_array_equal(_one_tick(none, x), _one_tick(plain, x), err_msg=f"tick {t}")
    assert bytes(none.volume_state()) == bytes(plain.volume_state())
    with pytest.raises(AssertionError):
        ms.Bridge(ctx, 6, members=3, rate=48000, rational=legs, endpoints=legs)


@pytest.mark.parametrize("plc", [False, True], ids=["", "plc"])
def test_no_such_leg_is_the_concealed_bridge(ctx, mk, plc):
    """rational= with no leg at 3/2 or 2/3 is concealed=: the same tick_bytes, 6 ticks and the meter state bit for bit"""
    n, mm, conf = 8, 4, 16000
    legs = [(8000, PCMU, PCMU), (8000, PCMA, PCMA), (16000, PCM16, PCM16), (48000, PCM16, PCM16)] * 2
    old, new = mk(ms.Bridge, n, members=mm, rate=conf, concealed=legs, plc=plc), mk(ms.Bridge, n, members=mm, rate=conf, rational=legs, plc=plc)
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


def _lds_cap(conf, rates):
    """the member cap of a conference whose legs' rates are `rates`, from creation's formula (plan_bridge, csrc/bridge_plan.hpp):
    rows of the widest tick at an odd number of 8-byte words, the int32 sum row, four wavefronts' resampler scratch -- the
    largest form any leg needs -- and the kernel's own RATED_STATIC_LDS, within 64 KB"""
    static = bridge_budget()[0]
    return max(mm for mm in range(1, 129) if bridge_lds(conf, rates, mm) + static <= 64 * 1024)


def test_refusals(ctx, mk):
    def refused(values, *a, **kw):
        with pytest.raises(ms.MiError) as e:
            mk(ms.Bridge, *a, **kw)
        assert e.value.code == _lib.MI_ENOTSUP, str(e.value)
        for v in values:
            assert str(v) in str(e.value), str(e.value)

    ok8, ok16, ok48 = [(8000, PCMU, PCMU)] * 6, [(16000, PCM16, PCM16)] * 6, [(48000, PCM16, PCM16)] * 6
    refused(["leg 5 at 44100"], 6, members=3, rate=8000, rational=ok8[:5] + [(44100, PCM16, PCM16)])
    refused(["leg 4 at 32000", "1.333"], 6, members=3, rate=24000, rational=[(24000, PCM16, PCM16)] * 4 + [(32000, PCM16, PCM16)] * 2)
    refused(["leg 5 at 32000", "ratio 4"], 6, members=3, rate=8000, rational=ok8[:5] + [(32000, PCM16, PCM16)])
    refused(["leg 4's rate 1200"], 6, members=3, rate=800, rational=[(800, PCM16, PCM16)] * 4 + [(1200, PCM16, PCM16)] * 2)
    refused(["leg 4's rate 4400"], 6, members=3, rate=8800, rational=[(8800, PCM16, PCM16)] * 4 + [(4400, PCM16, PCM16)] * 2)
    refused(["leg 5 names codec 3"], 6, members=3, rate=8000, rational=ok8[:5] + [(12000, PCMU, 3)])
    refused(["leg 5", 72000], 6, members=3, rate=48000, rational=ok48[:5] + [(72000, PCM16, PCM16)], plc=True)
    br = mk(ms.Bridge, 6, members=3, rate=48000, rational=ok48[:5] + [(72000, PCM16, PCM16)])  # legal without the concealer
    assert _one_tick(br, np.zeros((6, 1440), np.uint8)).shape == (6, 1440)
    # 32 kHz legs in a 48 kHz conference: created at the cap the header names, refused one past it
    cap = _lds_cap(48000, [32000, 48000])
    assert cap == 43 and _lds_cap(16000, [24000, 48000]) == 45  # the figures of msmi355x_bridge.h
    room = lambda mm: [(32000, PCM16, PCM16), (48000, PCM16, PCM16)] * mm
    full = mk(ms.Bridge, cap, members=cap, rate=48000, rational=room(cap)[:cap])
    assert _one_tick(full, np.zeros((cap, 960), np.uint8)).shape == (cap, 960)
    refused(["LDS", f"{cap + 1} members x 480 samples"], cap + 1, members=cap + 1, rate=48000, rational=room(cap + 1)[:cap + 1])
    for kw in ("endpoints", "concealed"):  # the older constructors keep their refusal
        refused(["leg 2 at 24000", "1.5"], 6, members=3, rate=16000, **{kw: ok16[:2] + [(24000, PCM16, PCM16)] + ok16[3:]})
    br = mk(ms.Bridge, 6, members=3, rate=16000, rational=ok16[:2] + [(24000, PCM16, PCM16)] + ok16[3:])  # the context is usable afterwards
    assert _one_tick(br, np.zeros((6, 480), np.uint8)).shape == (6, 480)


def test_plc_equal_to_the_parts(ctx, mk, oracle):
    """a 16 kHz room of 16 kHz mu-law, 24 kHz PCM and 16 kHz PCM legs with scattered losses: bit for bit mi_g711_decode per law
    -> mi_plc_process per rate -> the plc-less rational= bridge, the relation of tests/test_gpu_bridge_concealed.py"""
    mm, conf, nticks = 3, 16000, 45
    legs = [(16000, PCMU, PCMU), (24000, PCM16, PCM16), (16000, PCM16, PCM16)] * 2
    n = len(legs)
    br = mk(ms.Bridge, n, members=mm, rate=conf, rational=legs, plc=True)
    parts = ConcealedParts(ctx, mk, mm, conf, legs, form="rational")
    assert br.tick_bytes() == (480, 480) == parts.inner.tick_bytes()
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    br.set_volume_params([p] * n)
    parts.inner.set_volume_params([p] * n)
    x, present = leg_rows(oracle, legs, nticks), loss_patterns(n, nticks)
    for t in range(nticks):
        assert_same_rows(br, one_tick(br, x[t], present[t]), parts.tick(x[t], present[t]), t)
    assert_same_meters(br, parts.inner)


def test_superwideband_room_example_runs(tmp_path):
    """300 ticks of a 48 kHz room of mu-law trunks, 16, 32 and 48 kHz PCM members through the plain-C example; it checks its
    own row sizes and return codes"""
    pkg, exe = os.path.join(ROOT, "mediastreamer2_amd"), tmp_path / "superwideband_room"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "superwideband_room.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", (run.stdout, run.stderr)
