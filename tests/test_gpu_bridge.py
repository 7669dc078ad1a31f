"""GPU parity of mi_bridge (include/msmi355x_bridge.h): one launch per conference tick against the oracle's functions
chained per leg -- g711_decode -> Volume.chunk -> mixer_tick -> g711_encode --, an absent leg skipping the volume and
feeding the mixer nothing.  Every comparison is BIT-EXACT: each stage is bit-exact against the oracle on its own, and
fusing them changes no arithmetic.  Float state is compared as uint32 words."""
import ctypes as C

import numpy as np
import pytest

import mediastreamer2_amd as ms
from conftest import synth_pcm
from mediastreamer2_amd import _lib

pytestmark = pytest.mark.gpu

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
FLOAT_STATE = ("energy", "level_pk", "instant_energy", "lt_speaker_en", "gain", "target_gain", "ng_gain")
INT_STATE = ("dc_offset", "sustain_dur", "ng_noise_dur", "fast_upramp")


def _bits(f):
    return np.float32(f).view(np.uint32)


def _law(codec):
    return ms.MI_LAW_PCMA if codec == PCMA else ms.MI_LAW_PCMU


def _signal(n, ns, nticks, rate, sigma=3000.0, first_id=0):
    """[n, nticks * ns] int16: the benchmark's synthetic audio (noise + a -20 dBFS tone), one generator per leg"""
    return np.stack([synth_pcm(first_id + s, ns * nticks, sigma=sigma, rate=rate) for s in range(n)])


class OracleBridge:
    """the yardstick: per leg a decoder, an MSVolume (with the one-second maximum MSVolume keeps beside it) and a mixer pin"""

    def __init__(self, oracle, n, mm, rate, in_codec, out_codec):
        self.o, self.n, self.mm, self.rate, self.ns = oracle, n, mm, rate, rate // 100
        self.in_codec, self.out_codec = in_codec, out_codec
        self.flags = np.full(n, L | A | O, np.uint8)
        self.gain = np.ones(n, np.float32)
        self.vol = [self._new_volume() for _ in range(n)]
        self.max = [oracle.Extremum(1000) for _ in range(n)]
        self.clock = np.zeros(n, np.int64)  # a meter's own chunks are its clock, 10 ms each
        self.rows = np.zeros((n, self.ns), np.uint8 if out_codec else np.int16)  # rows of pins whose output is off stay

    def _new_volume(self):
        return self.o.Volume(self.rate)

    def configure(self, s, **kw):
        for k, v in kw.items():
            setattr(self.vol[s].v, k, v)

    def restart(self, s, **kw):
        self.vol[s], self.max[s], self.clock[s] = self._new_volume(), self.o.Extremum(1000), 0
        self.configure(s, **kw)

    def decode(self, x):
        return self.o.g711_decode(_law(self.in_codec), x) if self.in_codec else np.array(x, np.int16)

    def tick(self, x, present=None, pcm=None):
        """x [n, ns] as it arrives (pcm: already decoded / concealed rows instead) -> what leaves [n, ns]"""
        present = np.ones(self.n, np.uint8) if present is None else np.asarray(present, np.uint8)
        pcm = self.decode(x) if pcm is None else pcm
        lev = np.zeros((self.n, self.ns), np.int16)
        for s in range(self.n):
            if present[s]:
                lev[s] = self.vol[s].chunk(pcm[s])
                self.max[s].record_max(int(self.clock[s]), self.vol[s].v.energy)
                self.clock[s] += 10
        for c in range(self.n // self.mm):
            k = slice(c * self.mm, (c + 1) * self.mm)
            f = self.flags[k]
            mix, _ = self.o.mixer_tick(lev[k], has_data=present[k] & ((f & L) != 0), gain=self.gain[k], active=(f & A) != 0,
                                       out_enabled=(f & O) != 0)
            out = self.o.g711_encode(_law(self.out_codec), mix) if self.out_codec else mix
            on = (f & O) != 0
            self.rows[k][on] = out[on]
        return self.rows.copy()

    def check_state(self, br, tag):
        st = br.volume_state()
        mx = br.volume_max()
        for s in range(self.n):
            for name in FLOAT_STATE:
                assert _bits(getattr(st[s], name)) == _bits(getattr(self.vol[s].v, name)), (tag, s, name)
            for name in INT_STATE:
                assert getattr(st[s], name) == getattr(self.vol[s].v, name), (tag, s, name)
            assert _bits(mx[s]) == _bits(self.max[s].current), (tag, s, "max", mx[s], self.max[s].current)


@pytest.fixture
def mk(ctx):
    """Bridge(ctx, ...) that is closed with the test, passed or failed, while the context is still there"""
    made = []

    def make(*a, **kw):
        made.append(ms.Bridge(ctx, *a, **kw))
        return made[-1]
    yield make
    for b in made:
        b.close()


def _arrive(orc, pcm):
    """the rows as the legs send them: code words of the bridge's input codec, or the PCM itself"""
    return orc.o.g711_encode(_law(orc.in_codec), pcm) if orc.in_codec else pcm


def _one_tick(br, x, present=None):
    h_in, h_present = br.acquire()
    assert h_present.all()
    h_in[:] = x
    if present is not None:
        h_present[:] = present
    br.submit()
    return br.collect().copy()


@pytest.mark.parametrize("rate", [8000, 48000])
@pytest.mark.parametrize("nconf", [1, 9])
@pytest.mark.parametrize("mm", [3, 8, 33, 50])
def test_members_conferences_rates(ctx, mk, oracle, mm, nconf, rate):
    """3 .. 50 members (33 and 50 take a second round of the eight-lanes-per-member loads), 1 and 9 conferences (more than
    the XCDs), 80- and 480-sample ticks; mu-law in, A-law out"""
    n, ns, nticks = mm * nconf, rate // 100, 3
    br = mk(n, members=mm, rate=rate, in_codec=PCMU, out_codec=PCMA)
    assert br.tick_bytes() == (ns, ns)
    orc = OracleBridge(oracle, n, mm, rate, PCMU, PCMA)
    sig = _signal(n, ns, nticks, rate)
    for t in range(nticks):
        x = _arrive(orc, sig[:, t * ns:(t + 1) * ns])
        np.testing.assert_array_equal(_one_tick(br, x), orc.tick(x), err_msg=f"tick {t}")
    orc.check_state(br, "end")
    br.close()


@pytest.mark.parametrize("out_codec", [PCM16, PCMA, PCMU])
@pytest.mark.parametrize("in_codec", [PCM16, PCMA, PCMU])
def test_codec_pairs(ctx, mk, oracle, in_codec, out_codec):
    mm, n, rate, ns, nticks = 3, 6, 8000, 80, 20
    br = mk(n, members=mm, rate=rate, in_codec=in_codec, out_codec=out_codec)
    assert br.tick_bytes() == (ns * (1 if in_codec else 2), ns * (1 if out_codec else 2))
    orc = OracleBridge(oracle, n, mm, rate, in_codec, out_codec)
    sig = _signal(n, ns, nticks, rate, sigma=6000.0, first_id=10)
    for t in range(nticks):
        x = _arrive(orc, sig[:, t * ns:(t + 1) * ns])
        np.testing.assert_array_equal(_one_tick(br, x), orc.tick(x), err_msg=f"tick {t}")
    orc.check_state(br, "end")
    br.close()


def test_mixer_edges(ctx, mk, oracle):
    """full-scale PCM with -32768 on every member (the mix saturates at +-32767), an inactive pin, a pin whose output is off
    (its row is left as it was: zeros from the start), an input gain != 1; then a member leaves and a new one takes the
    slot: its meter starts over, the others keep theirs"""
    mm, n, rate, ns = 8, 16, 8000, 80
    br = mk(n, members=mm, rate=rate, in_codec=PCM16, out_codec=PCM16)
    orc = OracleBridge(oracle, n, mm, rate, PCM16, PCM16)
    orc.flags[1] = L | O      # muted
    orc.flags[2] = L | A      # no return
    orc.flags[mm + 3] = L | O
    orc.gain[4], orc.gain[mm + 5] = 0.5, 1.75
    br.set_controls(flags=orc.flags, gain=orc.gain)
    rng = np.random.default_rng(7)
    sig = _signal(n, ns, 12, rate, sigma=5000.0, first_id=30)
    for t in range(12):
        x = sig[:, t * ns:(t + 1) * ns].copy()
        if t in (1, 2):       # rails: every member at full scale, the sign per member and sample
            x = np.where(rng.integers(0, 2, (n, ns)) == 1, 32767, -32768).astype(np.int16)
            x[:mm, :8] = -32768
            x[mm:, :8] = 32767
        present = np.ones(n, np.uint8)
        if t == 5:
            br.remove_member(6)
            orc.flags[6] = 0
            orc.rows[6] = 0
            assert br.member_count(0) == mm - 1 and br.member_count(1) == mm
        if 5 <= t < 8:
            present[6] = 0    # nobody sends on a pin that is not plumbed
        if t == 8:
            br.add_member(6)
            orc.flags[6] = L | A | O
            orc.restart(6)
            assert br.member_count(0) == mm
        got, want = _one_tick(br, x, present), orc.tick(x, present)
        np.testing.assert_array_equal(got, want, err_msg=f"tick {t}")
        if t in (1, 2):
            assert (np.abs(want.astype(np.int32)) == 32767).any() and want.min() >= -32767
        if t in (7, 8, 11):
            orc.check_state(br, t)
    assert not got[2].any()
    br.close()


def test_absent_legs(ctx, mk, oracle):
    """a seeded fifth of the legs absent per tick: no chunk for their MSVolume (state unchanged that tick), silence on the pin"""
    mm, n, rate, ns, nticks = 8, 24, 8000, 80, 15
    br = mk(n, members=mm, rate=rate, in_codec=PCMA, out_codec=PCMU)
    orc = OracleBridge(oracle, n, mm, rate, PCMA, PCMU)
    p = ms.VolumeBatch.default_params()
    p.agc_enabled = 1
    br.set_volume_params([p] * n)
    for s in range(n):
        orc.configure(s, agc_enabled=1)
    rng = np.random.default_rng(0xAB5E)
    sig = _signal(n, ns, nticks, rate, sigma=4000.0, first_id=60)
    for t in range(nticks):
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        before = bytes(br.volume_state())
        x = _arrive(orc, sig[:, t * ns:(t + 1) * ns])
        x[present == 0] = 0x2A  # whatever the staging holds for an absent leg is ignored
        np.testing.assert_array_equal(_one_tick(br, x, present), orc.tick(x, present), err_msg=f"tick {t}")
        after = bytes(br.volume_state())
        sz = C.sizeof(ms.VolumeState)
        for s in range(n):
            same = before[s * sz:(s + 1) * sz] == after[s * sz:(s + 1) * sz]
            assert same == (present[s] == 0), (t, s, present[s])
        orc.check_state(br, t)
    br.close()


def test_volume_agc_gate_dc_gain(ctx, mk, oracle):
    """AGC, noise gate, DC removal and a static gain of 0.5, 130 ticks of the benchmark's synthetic signal with loud and
    quiet stretches (the AGC gain and the gate move, the one-second windows start over); state and MS_VOLUME_GET_MAX
    bit-equal at tick 60 and at the end"""
    mm, n, rate, ns, nticks = 5, 10, 8000, 80, 130
    cfgs = [dict(agc_enabled=1), dict(noise_gate_enabled=1), dict(remove_dc=1), dict(static_gain=0.5),
            dict(agc_enabled=1, noise_gate_enabled=1, remove_dc=1, static_gain=0.5)]
    br = mk(n, members=mm, rate=rate, in_codec=PCMU, out_codec=PCMU)
    orc = OracleBridge(oracle, n, mm, rate, PCMU, PCMU)
    params = []
    for s in range(n):
        cfg = cfgs[s % len(cfgs)]
        p = ms.VolumeBatch.default_params()
        for k, v in cfg.items():
            setattr(p, k, v)
        params.append(p)
        orc.configure(s, **cfg)
    br.set_volume_params(params)
    sig = _signal(n, ns, nticks, rate, sigma=3000.0).astype(np.int32)
    env = np.where((np.arange(ns * nticks) // (ns * 30)) % 3 == 0, 1.0, 0.02)   # 300 ms loud, 600 ms nearly silent (the gate's hold is 400 ms)
    sig = (sig * env + 700).clip(-32767, 32767).astype(np.int16)                # and a DC offset for the DC removers
    gains, gates = set(), set()
    for t in range(nticks):
        x = _arrive(orc, sig[:, t * ns:(t + 1) * ns])
        np.testing.assert_array_equal(_one_tick(br, x), orc.tick(x), err_msg=f"tick {t}")
        gains.add(_bits(orc.vol[0].v.gain).item())
        gates.add(_bits(orc.vol[1].v.ng_gain).item())
        if t == 60:
            orc.check_state(br, t)
    assert len(gains) > 10 and len(gates) > 10, "the AGC gain and the gate must actually move"
    orc.check_state(br, "end")
    br.close()


def test_equal_to_the_parts(ctx, mk):
    """the same input through mi_g711_decode -> mi_volume_process -> mi_mixer_process -> mi_g711_encode on the C ABI"""
    import torch
    mm, n, rate, ns, nticks = 33, 99, 8000, 80, 6
    br = mk(n, members=mm, rate=rate, in_codec=PCMA, out_codec=PCMU)
    vol = ms.VolumeBatch(ctx, n, rate)
    mix = ms.MixerBatch(ctx, n // mm, mm, ns)
    p = ms.VolumeBatch.default_params()
    p.agc_enabled, p.remove_dc = 1, 1
    br.set_volume_params([p] * n)
    vol.set_params([p] * n)
    flags = np.full(n, L | A | O, np.uint8)
    flags[7] = L | O
    gain = np.ones(n, np.float32)
    gain[40] = 0.7
    br.set_controls(flags=flags, gain=gain)
    mix.set_controls(flags=flags, gain=gain)
    rng = np.random.default_rng(3)
    pcm = torch.zeros((n, ns), dtype=torch.int16, device="cuda")
    out = torch.zeros((n // mm, mm, ns), dtype=torch.int16, device="cuda")
    codes_out = torch.zeros((n, ns), dtype=torch.uint8, device="cuda")
    for t in range(nticks):
        x = rng.integers(0, 256, (n, ns), dtype=np.uint8)
        present = (rng.random(n) >= 0.2).astype(np.uint8)
        got = _one_tick(br, x, present)
        codes = torch.from_numpy(x).cuda()
        has = torch.from_numpy(present).cuda()
        lens = torch.from_numpy(present.astype(np.int32) * ns).cuda()
        torch.cuda.synchronize()
        ms.g711_decode(ctx, ms.MI_LAW_PCMA, codes, pcm)
        vol.process(pcm, per_stream=lens)
        mix.process(pcm.view(n // mm, mm, ns), has, 1, out)
        ms.g711_encode(ctx, ms.MI_LAW_PCMU, out.view(n, ns), codes_out)
        ctx.sync()
        np.testing.assert_array_equal(got, codes_out.cpu().numpy(), err_msg=f"tick {t}")
    assert bytes(br.volume_state()) == b"".join(bytes(s) for s in vol.get_state())
    np.testing.assert_array_equal(br.volume_max().view(np.uint32), vol.get_max().view(np.uint32))
    for o in (br, vol, mix):
        o.close()


@pytest.mark.parametrize("in_codec", [PCM16, PCMU])
def test_plc(ctx, mk, in_codec):
    """plc = 1: losses of 1 and 3 consecutive ticks on two legs; the output equals mi_plc_process followed by the bridge's
    chain without plc on the concealed rows (a concealed leg counts as present)"""
    import torch
    mm, n, rate, ns, nticks = 4, 8, 8000, 80, 14
    br = mk(n, members=mm, rate=rate, in_codec=in_codec, out_codec=PCMA, plc=True)
    plain = mk(n, members=mm, rate=rate, in_codec=PCM16, out_codec=PCMA)
    plc = ms.PlcBatch(ctx, n, rate, max_block=ns)
    lost = {2: {3}, 5: {6, 7, 8}}
    sig = _signal(n, ns, nticks, rate, sigma=4000.0, first_id=80)
    lens = torch.full((n,), ns, dtype=torch.int32, device="cuda")
    for t in range(nticks):
        x = sig[:, t * ns:(t + 1) * ns]
        present = np.array([0 if t in lost.get(s, ()) else 1 for s in range(n)], np.uint8)
        if in_codec:
            codes = torch.from_numpy(np.random.default_rng(t).integers(0, 256, (n, ns), dtype=np.uint8)).cuda()
            rows = torch.zeros((n, ns), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            ms.g711_decode(ctx, ms.MI_LAW_PCMU, codes, rows)
            arrive = codes.cpu().numpy()
        else:
            rows = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            arrive = x
        modes = torch.from_numpy(np.where(present, ms.MI_PLC_RECEIVED, ms.MI_PLC_CONCEAL).astype(np.uint8)).cuda()
        torch.cuda.synchronize()
        plc.process(rows, lens, modes)
        ctx.sync()
        want = _one_tick(plain, rows.cpu().numpy())
        np.testing.assert_array_equal(_one_tick(br, arrive, present), want, err_msg=f"tick {t}")
    assert bytes(br.volume_state()) == bytes(plain.volume_state())
    for o in (br, plain, plc):
        o.close()


def test_pipeline_three_in_flight(ctx, mk, oracle):
    """three ticks in flight, collected in order; reset_streams and set_controls act on the ticks submitted afterwards"""
    mm, n, rate, ns, nticks = 8, 16, 8000, 80, 12
    br = mk(n, members=mm, rate=rate, in_codec=PCMU, out_codec=PCMU)
    orc = OracleBridge(oracle, n, mm, rate, PCMU, PCMU)
    p = ms.VolumeBatch.default_params()
    p.agc_enabled = 1
    br.set_volume_params([p] * n)
    for s in range(n):
        orc.configure(s, agc_enabled=1)
    sig = _signal(n, ns, nticks, rate, sigma=5000.0, first_id=100)
    want, got = [], []
    for t in range(nticks):
        if t == 6:                       # (both wait for the three ticks in flight)
            br.reset_streams(3, 2)
            orc.restart(3, agc_enabled=1)
            orc.restart(4, agc_enabled=1)
        if t == 9:
            orc.flags[5] = L | O
            orc.gain[9] = 0.25
            br.set_controls(flags=orc.flags, gain=orc.gain)
        if br.in_flight() == 3:
            got.append(br.collect().copy())
        x = _arrive(orc, sig[:, t * ns:(t + 1) * ns])
        h_in, _ = br.acquire()
        h_in[:] = x
        br.submit()
        want.append(orc.tick(x))
    assert br.in_flight() == 3
    with pytest.raises(ms.MiError):
        br.acquire()
    while br.in_flight():
        got.append(br.collect().copy())
    assert len(got) == nticks
    for t in range(nticks):
        np.testing.assert_array_equal(got[t], want[t], err_msg=f"tick {t}")
    orc.check_state(br, "end")
    br.close()


def test_active_speakers(ctx, mk):
    """the winner is the session's rule on the same levels (mi_session's and mi_bridge's elections run one function): the
    unmuted, plumbed member with the largest one-second maximum above -30 dBm0; of two equally loud, who joined first"""
    mm, n, rate, ns = 4, 12, 8000, 80
    br = mk(n, members=mm, rate=rate, in_codec=PCM16, out_codec=PCM16)
    sig = _signal(n, ns, 30, rate, sigma=20.0, first_id=120) // 1024          # everybody near silence (-38 dBm0)
    loud = synth_pcm(200, ns * 30, sigma=6000.0, rate=rate)
    louder = synth_pcm(201, ns * 30, sigma=12000.0, rate=rate)
    sig[1], sig[2] = loud, louder                   # conference 0: pin 2 wins, until it is muted
    sig[mm + 1], sig[mm + 3] = loud, loud           # conference 1: a tie between pins 1 and 3
    flags = np.full(n, L | A | O, np.uint8)         # conference 2: nobody above -30 dB
    br.remove_member(mm + 1)                         # pin 1 of conference 1 leaves and joins again: now the LATER joiner
    br.add_member(mm + 1)
    for t in range(30):
        _one_tick(br, sig[:, t * ns:(t + 1) * ns])
    mx = br.volume_max()
    assert _bits(mx[mm + 1]) == _bits(mx[mm + 3])
    win, db = br.active_speakers()
    assert list(win) == [2, mm + 3, -1], (win, db)
    assert abs(db[0] - 10 * np.log10(mx[2])) < 1e-4 and db[0] > -30 and db[2] == -120.0
    np.testing.assert_array_equal(br.levels().view(np.uint32),
                                  np.array([s.energy for s in br.volume_state()], np.float32).view(np.uint32))
    flags[2] = L | O
    br.set_controls(flags=flags)
    win, _ = br.active_speakers()
    assert list(win) == [1, mm + 3, -1]
    br.close()


def test_refusals(ctx, mk):
    with pytest.raises(ms.MiError) as e:
        mk(6, members=3, rate=11025)
    assert e.value.code == _lib.MI_ENOTSUP and "11025" in str(e.value)
    br = mk(6, members=3)
    p = ms.VolumeBatch.default_params()
    p.peer = 1
    with pytest.raises(ms.MiError) as e:
        br.set_volume_params([p], first=2)
    assert e.value.code == _lib.MI_ENOTSUP and "peer" in str(e.value)
    with pytest.raises(ms.MiError) as e:
        mk(7, members=3)
    assert e.value.code == _lib.MI_EINVAL
    br.close()


def test_g711_bridge_example_runs(tmp_path):
    """300 ticks of a 2048-leg mu-law bridge through the plain-C example; it checks the speaker it elects"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg, exe = os.path.join(root, "mediastreamer2_amd"), tmp_path / "g711_bridge"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "g711_bridge.c"), "-L", pkg,
                        "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", (run.stdout, run.stderr)
