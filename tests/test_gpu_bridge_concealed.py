"""GPU parity of loss concealment on bridges whose legs differ in rate and codec (mi_bridge_create_concealed,
include/msmi355x_bridge.h): a concealer per leg behind the leg's own decoder -- plc_legs_received_kernel and
plc_legs_conceal_kernel, csrc/plc.hip -- in front of the bridge's unchanged tick kernel.

Every comparison is BIT-EXACT over all legs, samples and ticks.  The yardsticks:
  * the parts on the C ABI: mi_g711_decode once per law -> one mi_plc_process per distinct rate over all rows (mode 0 for
    the legs of other rates) -> a plc-less endpoints= bridge with the same rates and out codecs, fed the concealed PCM
    with every leg present;
  * the oracle: g711_decode -> Plc(rate) per leg, a listener's row being the saturated sum of the other members'."""
import numpy as np
import pytest

import mediastreamer2_amd as ms
from bridge_parts import LAW, NTICKS, assert_same_meters, assert_same_rows, leg_rows, loss_patterns, mk, one_tick  # noqa: F401 (mk: a fixture)
from bridge_parts import ConcealedParts as Parts
from bridge_parts import up16 as _up16
from mediastreamer2_amd import _lib

pytestmark = pytest.mark.gpu

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
MM = 3

GATEWAY16 = [(8000, PCMU, PCMU), (8000, PCMA, PCMU), (16000, PCM16, PCM16), (48000, PCM16, PCM16), (8000, PCMA, PCMA), (16000, PCMU, PCM16)]
CODECS8 = [(8000, PCMU, PCMU), (8000, PCMA, PCM16), (8000, PCM16, PCMA), (8000, PCMA, PCMA), (8000, PCM16, PCM16), (8000, PCMU, PCMA)]
RATES16 = [(8000, PCMU, PCMA), (16000, PCMU, PCMA)] * 3


def tiled(legs, n):
    return [legs[s % len(legs)] for s in range(n)]


@pytest.mark.parametrize("conf,turn", [(16000, GATEWAY16), (8000, CODECS8), (16000, RATES16)], ids=["gateway-16k", "codecs-8k", "rates-16k"])
def test_equal_to_the_parts(ctx, mk, oracle, conf, turn):
    """the gateway shape -- legs below, at and above a 16 kHz mix, both laws and PCM (bridge_updown_kernel behind the
    concealer) --, three codecs at one rate (bridge_legs_kernel<false>) and one codec pair at two rates (the rated route);
    every loss pattern on some leg of every rate class; AGC and DC removal on, so the gains ride on what the concealer made"""
    n = 2 * MM
    legs = tiled(turn, n)
    br = mk(ms.Bridge, n, members=MM, rate=conf, concealed=legs, plc=True)
    parts = Parts(ctx, mk, MM, conf, legs)
    assert br.tick_bytes() == (_up16(parts.in_bytes.max()), parts.inner.tick_bytes()[1])
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    br.set_volume_params([p] * n)
    parts.inner.set_volume_params([p] * n)
    x, present = leg_rows(oracle, legs), loss_patterns(n)
    for t in range(NTICKS):
        assert_same_rows(br, one_tick(br, x[t], present[t]), parts.tick(x[t], present[t]), t)
    assert_same_meters(br, parts.inner)


def _oracle_listeners(oracle, legs, x, present, members):
    """per tick the rows the members of one conference hear: g711_decode -> Plc per leg, then the saturated sum of the
    other members' (unity gains, one rate: MSVolume and the mixer add nothing else)"""
    rate = legs[members[0]][0]
    ll = rate // 100
    plc = {s: oracle.Plc(rate) for s in members}
    out = []
    for t in range(len(x)):
        heard = {}
        for s in members:
            ic = legs[s][1]
            blk = np.ascontiguousarray(x[t, s, :2 * ll]).view(np.int16) if ic == PCM16 else oracle.g711_decode(LAW[ic], x[t, s, :ll])
            heard[s] = (plc[s].received(blk) if present[t, s] else plc[s].conceal(ll)).astype(np.int64)
        total = sum(heard.values())
        out.append({s: np.clip(total - heard[s], -32768, 32767).astype(np.int16) for s in members})
    return out


@pytest.mark.parametrize("talker", [0, 1, 2])
def test_against_the_oracle_at_8k(ctx, mk, oracle, talker):
    """an 8 kHz mix of a mu-law, an A-law and a PCM leg, PCM out, unity gain; one leg of each conference talks with losses
    -- singles, a burst, an outage --, the other two send digital silence and are always there: what a listener hears is
    the talker's concealed PCM (plus the A-law leg's silence, which decodes to 8) sample for sample"""
    legs = [(8000, PCMU, PCM16), (8000, PCMA, PCM16), (8000, PCM16, PCM16)] * 2
    n, talkers = len(legs), (talker, MM + talker)
    br = mk(ms.Bridge, n, members=MM, rate=8000, concealed=legs, plc=True)
    x = leg_rows(oracle, legs, seed=3 + talker, talk=talkers)
    present = np.ones((NTICKS, n), np.uint8)
    present[[5, 9], talkers[0]] = 0
    present[14:26, talkers[0]] = 0
    present[0:2, talkers[1]] = 0
    present[8:33, talkers[1]] = 0
    present[40, talkers[1]] = 0
    want = [_oracle_listeners(oracle, legs, x, present, range(c * MM, (c + 1) * MM)) for c in range(2)]
    for t in range(NTICKS):
        got = one_tick(br, x[t], present[t])
        for s in range(n):
            np.testing.assert_array_equal(br.leg_out(got, s), want[s // MM][t][s], err_msg=f"tick {t} leg {s}")


def test_against_the_oracle_at_16k(ctx, mk, oracle):
    """a 16 kHz mix: conference 0 all 16 kHz PCM, every member talking and losing packets its own way; conference 1 of 8 kHz
    mu-law legs only makes the bridge a mixed one.  Conference 0 against Plc(16000), exact"""
    legs = [(16000, PCM16, PCM16)] * MM + [(8000, PCMU, PCMU)] * MM
    n = len(legs)
    br = mk(ms.Bridge, n, members=MM, rate=16000, concealed=legs, plc=True)
    x = leg_rows(oracle, legs, seed=11)
    present = loss_patterns(n, seed=3)[:, [2, 3, 5, 0, 1, 4]]
    want = _oracle_listeners(oracle, legs, x, present, range(MM))
    for t in range(NTICKS):
        got = one_tick(br, x[t], present[t])
        for s in range(MM):
            np.testing.assert_array_equal(br.leg_out(got, s), want[t][s], err_msg=f"tick {t} leg {s}")


@pytest.mark.parametrize("conf,leg,old", [(8000, (8000, PCMU, PCMA), "legs"), (8000, (16000, PCMU, PCMA), "endpoints"),
                                          (16000, (16000, PCM16, PCM16), "legs")], ids=["8k-g711", "16k-above-8k", "16k-pcm"])
def test_uniform_legs_are_the_old_plc_bridge(ctx, mk, oracle, conf, leg, old):
    n = 2 * MM
    legs = [leg] * n
    new, was = mk(ms.Bridge, n, members=MM, rate=conf, concealed=legs, plc=True), mk(ms.Bridge, n, members=MM, rate=conf, plc=True, **{old: legs})
    assert new.tick_bytes() == was.tick_bytes()
    x, present = leg_rows(oracle, legs, seed=5), loss_patterns(n)
    assert x.shape[2] == new.tick_bytes()[0]
    for t in range(NTICKS):
        np.testing.assert_array_equal(one_tick(new, x[t], present[t]), one_tick(was, x[t], present[t]), err_msg=f"tick {t}")
    assert_same_meters(new, was)


def test_without_plc_is_the_endpoints_bridge(ctx, mk, oracle):
    n = 2 * MM
    legs = tiled(GATEWAY16, n)
    new, was = mk(ms.Bridge, n, members=MM, rate=16000, concealed=legs, plc=False), mk(ms.Bridge, n, members=MM, rate=16000, endpoints=legs)
    assert new.tick_bytes() == was.tick_bytes()
    x, present = leg_rows(oracle, legs, nticks=8, seed=6), loss_patterns(n)
    for t in range(8):
        np.testing.assert_array_equal(one_tick(new, x[t], present[t + 8]), one_tick(was, x[t], present[t + 8]), err_msg=f"tick {t}")
    assert_same_meters(new, was)


def test_a_replaced_leg(ctx, mk, oracle):
    """reset_streams on leg 2 (16 kHz PCM) in the middle of its burst and remove_member / add_member around leg 3's (48 kHz,
    in its outage): the parts with PlcBatch.reset on that stream and the same calls on the plc-less bridge; every other
    leg's rows and meters are those of the parts too, so nothing else was disturbed"""
    n, conf = 2 * MM, 16000
    legs = tiled(GATEWAY16, n)
    br = mk(ms.Bridge, n, members=MM, rate=conf, concealed=legs, plc=True)
    parts = Parts(ctx, mk, MM, conf, legs)
    x, present = leg_rows(oracle, legs, seed=8), loss_patterns(n)
    for t in range(NTICKS):
        if t == 18:
            for b in (br, parts.inner):
                b.reset_streams(2, 1)
            parts.restart(2)
        if t == 20:
            for b in (br, parts.inner):
                b.remove_member(3)
            assert br.member_count(1) == MM - 1
        if t == 24:
            for b in (br, parts.inner):
                b.add_member(3)
            parts.restart(3)
        got = one_tick(br, x[t], present[t])
        assert_same_rows(br, got, parts.tick(x[t], present[t]), t)
        assert got[3].any() == (not 20 <= t < 24), t
    assert_same_meters(br, parts.inner)


def test_three_ticks_in_flight(ctx, mk, oracle):
    """the mixed bridge with losses submitted three deep returns the rows of the same ticks submitted one at a time"""
    n, nticks = 2 * MM, 20
    legs = tiled(GATEWAY16, n)
    deep, single = (mk(ms.Bridge, n, members=MM, rate=16000, concealed=legs, plc=True) for _ in range(2))
    x, present = leg_rows(oracle, legs, nticks=nticks, seed=9), loss_patterns(n, seed=1)[8:]
    want = [one_tick(single, x[t], present[t]) for t in range(nticks)]
    got = []
    for t in range(nticks):
        if deep.in_flight() == 3:
            got.append(deep.collect().copy())
        h_in, h_present = deep.acquire()
        h_in[:] = x[t]
        h_present[:] = present[t]
        deep.submit()
    assert deep.in_flight() == 3
    while deep.in_flight():
        got.append(deep.collect().copy())
    for t in range(nticks):
        np.testing.assert_array_equal(got[t], want[t], err_msg=f"tick {t}")
    assert_same_meters(deep, single)


def test_refusals(ctx, mk):
    def refused(values, *a, **kw):
        with pytest.raises(ms.MiError) as e:
            mk(ms.Bridge, *a, **kw)
        assert e.value.code == _lib.MI_ENOTSUP, str(e.value)
        for v in values:
            assert str(v) in str(e.value), str(e.value)

    room = [(16000, PCMU, PCMU)] * 3 + [(96000, PCM16, PCM16)] + [(16000, PCM16, PCM16)] * 2
    refused(["leg 3", 96000], 6, members=MM, rate=16000, concealed=room, plc=True)
    br = mk(ms.Bridge, 6, members=MM, rate=16000, concealed=room, plc=False)  # legal without plc, and the context is usable
    assert one_tick(br, np.zeros((6, br.tick_bytes()[0]), np.uint8), np.ones(6, np.uint8)).shape == (6, 1920)
    refused(["leg 4 names codec 3"], 6, members=MM, rate=16000, concealed=room[:3] + [(16000, PCMU, PCMU), (16000, 3, PCMU), room[5]], plc=True)
    refused(["leg 0", 46400, "prime factor above 17"], 6, members=MM, rate=46400, concealed=[(46400, PCM16, PCM16)] * 6, plc=True)
    with pytest.raises(ms.MiError) as e:  # the older constructors keep their refusals, word for word
        mk(ms.Bridge, 6, members=MM, rate=16000, endpoints=tiled(GATEWAY16[:3], 6), plc=True)
    assert e.value.code == _lib.MI_ENOTSUP and "the concealer batch sits behind one decoder" in str(e.value)
    with pytest.raises(ms.MiError) as e:
        mk(ms.Bridge, 6, members=MM, rate=16000, leg_rates=[8000, 16000] * 3, plc=True)
    assert e.value.code == _lib.MI_ENOTSUP and "the concealer batch has one rate" in str(e.value)


def test_lossy_gateway_example_runs(tmp_path):
    """300 ticks of 384 legs -- mu-law and A-law trunks losing every 20th packet, 16 kHz PCM members -- through the plain-C
    example; it checks its own row sizes and return codes"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg, exe = os.path.join(root, "mediastreamer2_amd"), tmp_path / "lossy_gateway"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "lossy_gateway.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", (run.stdout, run.stderr)
