"""GPU parity of bridges whose legs run at their own rate (mi_bridge_create_rated, include/msmi355x_bridge.h): the in_resampler
and out_resampler of plumb_to_conf (audioconference.c:209-257) inside the bridge's one launch per tick.

Against the parts on the C ABI -- mi_g711_decode -> mi_volume_process (a batch per leg rate) -> mi_resampler_process_masked ->
mi_mixer_process -> mi_resampler_process_masked -> mi_g711_encode -- every comparison is BIT-EXACT: the fused kernel runs the
parts' arithmetic in the parts' order.  Against the oracle chain the meter is bit-exact (MSVolume sits in front of the
resampler) and the audio is held to the float resampler path's tolerance, 1e-4 RMS of full scale (tests/test_gpu_resample.py):
the oracle multiplies and adds separately where the kernels fuse."""
import ctypes as C

import numpy as np
import pytest

import mediastreamer2_amd as ms
from bridge_parts import FLOAT_STATE, INT_STATE, mk  # noqa: F401 (mk: a fixture)
from bridge_parts import SampleParts as Parts
from bridge_parts import bits as _bits
from bridge_parts import one_tick as _one_tick
from conftest import synth_pcm
from mediastreamer2_amd import _lib

pytestmark = pytest.mark.gpu

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
def _law(codec):
    return ms.MI_LAW_PCMA if codec == PCMA else ms.MI_LAW_PCMU


def _rates(n, case):
    leg, conf = case
    if leg == "mixed":
        return np.array([(8000, 16000, 48000)[s % 3] for s in range(n)], np.int32), conf
    return np.full(n, leg, np.int32), conf


def _codes(rng, n, pitch):
    return rng.integers(0, 256, (n, pitch), dtype=np.uint8)


@pytest.mark.parametrize("nconf", [1, 9])
@pytest.mark.parametrize("mm", [3, 9])
@pytest.mark.parametrize("case", [(8000, 16000), (16000, 48000), (8000, 48000), ("mixed", 48000)], ids=str)
def test_equal_to_the_parts(ctx, mk, case, mm, nconf):
    """ratios 2, 3 and 6 (the 287-sample out-history takes a wave more than one staging pass) and 8 / 16 / 48 kHz legs side by
    side in one 48 kHz conference; 9 members give a wave a second member; A-law in, mu-law out, AGC and DC removal on, an
    inactive pin, an input gain != 1, a pin with its output off (moved to another pin half way: both out-resamplers must
    have kept their state while off), a seeded fifth of the legs absent per tick"""
    n = mm * nconf
    rates, conf = _rates(n, case)
    br = mk(ms.Bridge, n, members=mm, rate=conf, in_codec=PCMA, out_codec=PCMU, leg_rates=rates)
    parts = Parts(ctx, mk, n, mm, conf, rates, PCMA, PCMU)
    assert br.tick_bytes() == (parts.pitch, parts.pitch)
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
    rng = np.random.default_rng(0xB21D6E)
    for t in range(6):
        if t == 3:
            parts.flags[2], parts.flags[0] = L | A | O, L | A
            br.set_controls(flags=parts.flags)
            parts.set_controls()
        x = _codes(rng, n, parts.pitch)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        got, want = _one_tick(br, x, present), parts.tick(x, present)
        np.testing.assert_array_equal(got, want, err_msg=f"tick {t}")
    parts.check_state(br)


class OracleChain:
    """per leg: g711_decode -> Volume.chunk -> Resampler(leg, conf) -> mixer_tick -> Resampler(conf, leg)"""

    def __init__(self, oracle, n, leg, conf, in_codec):
        self.o, self.n, self.leg, self.conf, self.in_codec = oracle, n, leg, conf, in_codec
        self.vol = [oracle.Volume(leg) for _ in range(n)]
        self.max = [oracle.Extremum(1000) for _ in range(n)]
        self.up = [oracle.Resampler(leg, conf) for _ in range(n)]
        self.down = [oracle.Resampler(conf, leg) for _ in range(n)]
        self.clock = 0

    def tick(self, x):
        pcm = self.o.g711_decode(_law(self.in_codec), x) if self.in_codec else x
        wide = np.zeros((self.n, self.conf // 100), np.int16)
        for s in range(self.n):
            lev = self.vol[s].chunk(pcm[s])
            self.max[s].record_max(self.clock, self.vol[s].v.energy)
            wide[s] = self.up[s].process(lev)[:self.conf // 100]
        self.clock += 10
        mix, _ = self.o.mixer_tick(wide)
        return np.stack([self.down[s].process(mix[s])[:self.leg // 100] for s in range(self.n)])

    def check_meters(self, br):
        st, mx = br.volume_state(), br.volume_max()
        for s in range(self.n):
            for name in FLOAT_STATE:
                assert _bits(getattr(st[s], name)) == _bits(getattr(self.vol[s].v, name)), (s, name)
            for name in INT_STATE:
                assert getattr(st[s], name) == getattr(self.vol[s].v, name), (s, name)
            assert _bits(mx[s]) == _bits(self.max[s].current), (s, "max")


@pytest.mark.parametrize("case", [(8000, 16000), (16000, 48000)], ids=str)
def test_against_the_oracle_chain(ctx, mk, oracle, case):
    """three members, mu-law in, PCM16 out, unity gain, 12 ticks: the meters bit-exact, the audio within 1e-4 RMS of full
    scale (max |diff| reported, not bounded); a second bridge with A-law out gives g711_encode of the first one's PCM"""
    leg, conf = case
    n, ll, nticks = 3, leg // 100, 12
    br = mk(ms.Bridge, n, members=n, rate=conf, in_codec=PCMU, out_codec=PCM16, leg_rates=[leg] * n)
    br_a = mk(ms.Bridge, n, members=n, rate=conf, in_codec=PCMU, out_codec=PCMA, leg_rates=[leg] * n)
    orc = OracleChain(oracle, n, leg, conf, PCMU)
    sig = np.stack([synth_pcm(40 + s, ll * nticks, sigma=3000.0, rate=leg) for s in range(n)])
    err2, cnt, worst = 0.0, 0, 0
    for t in range(nticks):
        x = oracle.g711_encode(ms.MI_LAW_PCMU, sig[:, t * ll:(t + 1) * ll])
        got, want = _one_tick(br, x), orc.tick(x)
        np.testing.assert_array_equal(_one_tick(br_a, x), oracle.g711_encode(ms.MI_LAW_PCMA, got), err_msg=f"tick {t}")
        d = got.astype(np.float64) - want
        err2, cnt, worst = err2 + float((d * d).sum()), cnt + d.size, max(worst, int(np.abs(d).max()))
    rms = np.sqrt(err2 / cnt) / 32768.0
    print(f"bridge {leg} in {conf} vs oracle chain: rms {rms:.3e} of full scale, max |diff| {worst}")
    assert rms <= 1e-4, f"rms {rms:.3e} of full scale, max |diff| {worst} LSB"
    orc.check_meters(br)


def test_default_path_identical(ctx, mk):
    """leg_rates=None and leg_rates all equal to the conference's rate are mi_bridge_create: outputs and state byte for byte"""
    mm, n, rate, ns = 3, 6, 8000, 80
    kw = dict(members=mm, rate=rate, in_codec=PCMA, out_codec=PCMU)
    plain = mk(ms.Bridge, n, **kw)  # mi_bridge_create
    none, same = mk(ms.Bridge, n, leg_rates=None, **kw), mk(ms.Bridge, n, leg_rates=[rate] * n, **kw)
    p = ms.VolumeBatch.default_params()
    p.agc_enabled = 1
    for b in (plain, none, same):
        b.set_volume_params([p] * n)
        assert b.tick_bytes() == (ns, ns) and b.leg_rate(n - 1) == rate
    rng = np.random.default_rng(5)
    for t in range(3):
        x = _codes(rng, n, ns)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        want = _one_tick(plain, x, present)
        for b in (none, same):
            np.testing.assert_array_equal(_one_tick(b, x, present), want, err_msg=f"tick {t}")
    for b in (none, same):
        assert bytes(b.volume_state()) == bytes(plain.volume_state())
        np.testing.assert_array_equal(b.volume_max().view(np.uint32), plain.volume_max().view(np.uint32))


def test_membership(ctx, mk):
    """reset_streams and add_member on a rated leg: from that tick on the leg is a fresh parts chain (zero histories), the
    others carry on; remove_member then add_member does not replay what the old endpoint left in the resamplers"""
    mm, n, conf = 3, 6, 16000
    rates = np.full(n, 8000, np.int32)
    br = mk(ms.Bridge, n, members=mm, rate=conf, in_codec=PCM16, out_codec=PCM16, leg_rates=rates)
    parts = Parts(ctx, mk, n, mm, conf, rates, PCM16, PCM16)
    sig = np.stack([synth_pcm(70 + s, 80 * 10, sigma=5000.0, rate=8000) for s in range(n)])
    for t in range(10):
        present = np.ones(n, np.uint8)
        if t == 2:
            br.reset_streams(1, 1)
            parts.restart(1)
        if t == 4:
            br.remove_member(4)
            parts.flags[4] = 0
            parts.set_controls()
            parts.held[:, 4] = 0
            assert br.member_count(1) == mm - 1
        if 4 <= t < 7:
            present[4] = 0  # nobody sends on a pin that is not plumbed
        if t == 7:
            br.add_member(4)
            parts.flags[4] = L | A | O
            parts.set_controls()
            parts.restart(4)
        x = sig[:, t * 80:(t + 1) * 80]
        np.testing.assert_array_equal(_one_tick(br, x, present), parts.tick(x, present), err_msg=f"tick {t}")
    parts.check_state(br)


def test_three_ticks_in_flight(ctx, mk):
    """a rated bridge submitted three deep returns the rows of one tick at a time"""
    mm, n, conf, nticks = 3, 6, 16000, 7
    kw = dict(members=mm, rate=conf, in_codec=PCMU, out_codec=PCMU, leg_rates=[8000] * n)
    deep, single = mk(ms.Bridge, n, **kw), mk(ms.Bridge, n, **kw)
    rng = np.random.default_rng(11)
    xs = [_codes(rng, n, 80) for _ in range(nticks)]
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


def test_refusals(ctx, mk):
    def refused(value, *a, **kw):
        with pytest.raises(ms.MiError) as e:
            mk(ms.Bridge, *a, **kw)
        assert e.value.code == _lib.MI_ENOTSUP and str(value) in str(e.value), str(e.value)

    refused(16000, 6, members=3, rate=8000, leg_rates=[8000] * 5 + [16000])                 # a leg above the conference
    refused("ratio 4", 6, members=3, rate=32000, leg_rates=[32000] * 5 + [8000])
    refused(1.5, 6, members=3, rate=24000, leg_rates=[24000] * 5 + [16000])                 # no whole ratio
    refused(16000, 6, members=3, rate=48000, leg_rates=[8000] * 5 + [16000], plc=True)      # the concealer batch has one rate
    refused("LDS", 50, members=50, rate=48000, leg_rates=[8000] * 50)
    br = mk(ms.Bridge, 6, members=3, rate=16000, leg_rates=[8000] * 6)                      # the context is usable afterwards
    assert _one_tick(br, np.full((6, 80), 0xFF, np.uint8)).shape == (6, 80)


def test_plc_at_the_legs_rate(ctx, mk):
    """plc with one common leg rate below the conference's: mi_plc_process at the leg's rate in front of the parts"""
    mm, n, conf, nticks = 3, 6, 16000, 8
    rates = np.full(n, 8000, np.int32)
    br = mk(ms.Bridge, n, members=mm, rate=conf, in_codec=PCMU, out_codec=PCMA, leg_rates=rates, plc=True)
    parts = Parts(ctx, mk, n, mm, conf, rates, PCMU, PCMA, plc=True)
    lost = {1: {2}, 4: {4, 5, 6}}
    rng = np.random.default_rng(21)
    for t in range(nticks):
        x = _codes(rng, n, 80)
        present = np.array([0 if t in lost.get(s, ()) else 1 for s in range(n)], np.uint8)
        np.testing.assert_array_equal(_one_tick(br, x, present), parts.tick(x, present), err_msg=f"tick {t}")
    parts.check_state(br)


def test_geometry(ctx, mk):
    """the row pitch is the widest leg's tick; a narrower leg's row is written for its own samples only"""
    rates = [8000, 16000, 48000, 8000, 8000, 16000]
    br = mk(ms.Bridge, 6, members=3, rate=48000, in_codec=PCM16, out_codec=PCM16, leg_rates=rates)
    assert br.tick_bytes() == (960, 960)
    assert [br.leg_rate(s) for s in range(6)] == rates
    with pytest.raises(ms.MiError):
        br.leg_rate(6)
    narrow = mk(ms.Bridge, 6, members=3, rate=48000, in_codec=PCMU, out_codec=PCMU, leg_rates=[8000] * 6)
    assert narrow.tick_bytes() == (80, 80)  # 8 kHz G.711 legs in a 48 kHz conference still move 80-byte rows
    sig = np.stack([synth_pcm(90 + s, 480 * 3, sigma=6000.0, rate=48000) for s in range(6)])
    for t in range(3):
        out = _one_tick(br, sig[:, t * 480:(t + 1) * 480])
    for s, r in enumerate(rates):
        assert out[s, :r // 100].any(), s
        assert not out[s, r // 100:].any(), s
