"""The yardstick of the bridge's GPU tests (tests/test_gpu_bridge_*.py): the chain of C-ABI batches called one by one that a
bridge's one launch per tick must equal BIT FOR BIT -- mi_g711_decode once per law -> [mi_plc_process] -> mi_volume_process (a
batch per leg rate) -> mi_resampler_process_masked (leg -> conference) -> mi_mixer_process -> mi_resampler_process_masked
(conference -> leg) -> mi_g711_encode once per law -- written once, and the helpers those tests share.  A helper module like
tests/conference_glue.py; `mk` is a fixture the test modules import."""
import numpy as np
import pytest

import mediastreamer2_amd as ms

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
LAW = {PCMA: ms.MI_LAW_PCMA, PCMU: ms.MI_LAW_PCMU}
FLOAT_STATE = ("energy", "level_pk", "instant_energy", "lt_speaker_en", "gain", "target_gain", "ng_gain")
INT_STATE = ("dc_offset", "sustain_dur", "ng_noise_dur", "fast_upramp")
NTICKS = 45  # of the loss patterns: long enough for a 25-tick outage and the cross-fade back


@pytest.fixture
def mk(ctx):
    """factory(cls, ...) whose objects are closed with the test, passed or failed, while the context is still there"""
    made = []

    def make(cls, *a, **kw):
        made.append(cls(ctx, *a, **kw))
        return made[-1]
    yield make
    for b in reversed(made):
        b.close()


def up16(v):
    return (int(v) + 15) & ~15


def bits(f):
    return np.float32(f).view(np.uint32)


def one_tick(br, x, present=None):
    h_in, h_present = br.acquire()
    assert h_present.all()
    h_in[:] = x
    if present is not None:
        h_present[:] = present
    br.submit()
    return br.collect().copy()


class _Legs:
    """what both chains start with: the legs' rates and codecs, byte rows laid out as the bridge's, and the decoders"""

    def __init__(self, ctx, legs, width):
        import torch
        self.t = torch
        legs = np.asarray(legs, np.int32)
        self.ctx, self.n = ctx, len(legs)
        self.rates, self.ic, self.oc = legs[:, 0].copy(), legs[:, 1].copy(), legs[:, 2].copy()
        self.leg_len = self.rates // 100
        self.in_bytes = self.leg_len * np.where(self.ic, 1, 2)
        self.out_bytes = self.leg_len * np.where(self.oc, 1, 2)
        self.width = width(int(self.leg_len.max()))  # samples per row of the buffers at the legs' rates
        self.pcm = torch.zeros((self.n, self.width), dtype=torch.int16, device="cuda")
        self.lens = self._dev(self.leg_len.astype(np.int32))
        self.law_in = {c: self._dev(np.where(self.ic == c, self.leg_len, 0).astype(np.int32)) for c in LAW if (self.ic == c).any()}

    def _dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).cuda()

    def decode(self, x):
        """byte rows -> self.pcm: the PCM legs' samples copied, then one mi_g711_decode per law over that law's rows"""
        pcm = np.zeros((self.n, self.width), np.int16)
        for s in np.nonzero(self.ic == PCM16)[0]:
            pcm[s, :self.leg_len[s]] = x[s, :self.in_bytes[s]].view(np.int16)
        arrive = self._dev(x)
        self.ctx.sync()
        self.pcm.copy_(self._dev(pcm))
        self.t.cuda.synchronize()
        for c, lens in self.law_in.items():
            ms.g711_decode(self.ctx, LAW[c], arrive, self.pcm, length=int(self.leg_len.max()), lens=lens)


class Parts(_Legs):
    """the stages called one by one over byte rows laid out as the bridge's: every batch over all n streams with a run mask
    / a length of 0 for the streams that are not its own.  A leg's in_resampler runs leg rate -> conference rate and its
    out_resampler conference rate -> leg rate, whichever of the two is the larger.  A resampler that is no whole up-sampler
    wants mi_resampler_out_capacity = out_len + 1 samples per output row: the rows at the legs' rates are eight samples wider
    than the widest tick, and such an in_resampler writes roomy rows from which the rows that ran are moved onto the mixer's.
    plc: one rate, one pair -- MSGenericPLC behind the decoder, after which every leg counts as present."""
    ALIGN = 16  # bytes: what the pitches of the byte rows are rounded up to

    def __init__(self, ctx, mk, mm, conf, legs, plc=False):
        self.mm, self.conf, self.ns = mm, conf, conf // 100
        super().__init__(ctx, legs, lambda widest: max(self.ns, widest) + 8)
        n, torch = self.n, self.t
        self.in_pitch, self.out_pitch = (-(-int(b.max()) // self.ALIGN) * self.ALIGN for b in (self.in_bytes, self.out_bytes))
        self.distinct = sorted(set(int(r) for r in self.rates))
        self.vol = {r: mk(ms.VolumeBatch, n, r) for r in self.distinct}
        self.res_in = {r: mk(ms.ResamplerBatch, n, r, conf) for r in self.distinct if r != conf}
        self.res_out = {r: mk(ms.ResamplerBatch, n, conf, r) for r in self.distinct if r != conf}
        self.mix = mk(ms.MixerBatch, n // mm, mm, self.ns)
        self.plc = mk(ms.PlcBatch, n, self.distinct[0], max_block=self.width - 8) if plc else None
        self.flags = np.full(n, L | A | O, np.uint8)
        self.gain = np.ones(n, np.float32)
        # a row that is not written keeps what ITS staging slot held; the bridge rotates three slots, one per tick
        self.held = np.zeros((3, n, self.out_pitch), np.uint8)
        self.ticks = 0
        z = lambda cols, dt=torch.int16: torch.zeros((n, cols), dtype=dt, device="cuda")
        self.back = z(self.width)                       # at the legs' rates, like self.pcm
        self.wide, self.mixed = z(self.ns), z(self.ns)  # at the conference's
        self.narrow = z(self.ns + 8)                    # the roomy rows
        self.codes_out = z(self.out_pitch, torch.uint8)
        self.law_out = {c: self._dev(np.where(self.oc == c, self.leg_len, 0).astype(np.int32)) for c in LAW if (self.oc == c).any()}
        torch.cuda.synchronize()

    def rows(self, rng):
        """a tick of input rows: every byte random (the tails must be ignored), PCM legs a moderate noise"""
        x = rng.integers(0, 256, (self.n, self.in_pitch), dtype=np.uint8)
        for s in np.nonzero(self.ic == PCM16)[0]:
            x[s, :self.in_bytes[s]] = rng.normal(0.0, 5000.0, self.leg_len[s]).astype(np.int16).view(np.uint8)
        return x

    def set_params(self, params):
        for v in self.vol.values():
            v.set_params(params)

    def set_controls(self):
        self.mix.set_controls(flags=self.flags, gain=self.gain)

    def restart(self, s):
        """a NEW endpoint on stream s: fresh MSVolume, both resamplers fresh"""
        r = int(self.rates[s])
        st = ms.VolumeState()
        st.gain = st.target_gain = st.ng_gain = 1.0
        self.vol[r].set_state([st], first=s)
        self.vol[r].reset_max(s, 1)
        if r in self.res_in:
            self.res_in[r].reset(s, 1)
            self.res_out[r].reset(s, 1)

    def arrive(self, x):
        """a tick as the test hands it over -> byte rows [n, in_pitch]"""
        return x

    def leave(self, held):
        """the byte rows a slot holds -> a tick as the bridge's collect() returns it"""
        return held.copy()

    def tick(self, x, present=None):
        t, n, ns, W, Lb = self.t, self.n, self.ns, self.width, self.ctx.L
        present = np.ones(n, np.uint8) if present is None else np.asarray(present, np.uint8)
        linked, output = (self.flags & L) != 0, (self.flags & O) != 0
        roomy = lambda r: r > self.conf or self.conf % r != 0  # the in_resampler is no whole up-sampler
        self.wide.zero_()
        self.codes_out.zero_()
        self.decode(self.arrive(x))
        if self.plc is not None:
            modes = self._dev(np.where(present, ms.MI_PLC_RECEIVED, ms.MI_PLC_CONCEAL).astype(np.uint8))
            t.cuda.synchronize()
            self.plc.process(self.pcm, self.lens, modes)
            present = np.ones(n, np.uint8)  # a concealed leg counts as present: the masks below hold for every leg
        masks = {r: (self._dev((present != 0) & (self.rates == r) & linked), self._dev(output & (self.rates == r)),
                     self._dev(np.where((present != 0) & (self.rates == r), self.leg_len, 0).astype(np.int32))) for r in self.distinct}
        has = self._dev(present)
        same = self._dev(self.rates == self.conf)
        t.cuda.synchronize()
        for r in self.distinct:
            self.vol[r].process(self.pcm, nsamples=int(r) // 100, per_stream=masks[r][2])
        for r, rs in self.res_in.items():
            if roomy(r):  # one ratio at a time through the roomy rows; the rows that ran, onto the mixer's contiguous rows
                ms.check(Lb.mi_resampler_process_masked(rs.h, ms._ptr(self.pcm), r // 100, W, ms._ptr(self.narrow), ns + 8, None, ms._ptr(masks[r][0])))
                self.ctx.sync()
                ran = masks[r][0]
                self.wide[ran] = self.narrow[ran][:, :ns]
                t.cuda.synchronize()
            else:
                ms.check(Lb.mi_resampler_process_masked(rs.h, ms._ptr(self.pcm), r // 100, W, ms._ptr(self.wide), ns, None, ms._ptr(masks[r][0])))
        self.ctx.sync()
        self.wide[same] = self.pcm[same][:, :ns]
        t.cuda.synchronize()
        self.mix.process(self.wide.view(n // self.mm, self.mm, ns), has, 1, self.mixed.view(n // self.mm, self.mm, ns))
        for r, rs in self.res_out.items():
            ms.check(Lb.mi_resampler_process_masked(rs.h, ms._ptr(self.mixed), ns, ns, ms._ptr(self.back), W, None, ms._ptr(masks[r][1])))
        self.ctx.sync()
        self.back[:, :ns][same] = self.mixed[same]
        t.cuda.synchronize()
        for c, lens in self.law_out.items():
            ms.g711_encode(self.ctx, LAW[c], self.back, self.codes_out, length=int(self.leg_len.max()), lens=lens)
        self.ctx.sync()
        codes, back = self.codes_out.cpu().numpy(), self.back.cpu().numpy()
        held = self.held[self.ticks % 3]
        self.ticks += 1
        for s in np.nonzero(output)[0]:
            ll = self.leg_len[s]
            held[s, :self.out_bytes[s]] = codes[s, :ll] if self.oc[s] else back[s, :ll].view(np.uint8)
        return self.leave(held)

    def state_bytes(self):
        st = {r: self.vol[r].get_state() for r in self.distinct}
        return b"".join(bytes(st[int(self.rates[s])][s]) for s in range(self.n))

    def maxima(self):
        mx = {r: self.vol[r].get_max() for r in self.distinct}
        return np.array([mx[int(self.rates[s])][s] for s in range(self.n)], np.float32)

    def check_state(self, br):
        assert bytes(br.volume_state()) == self.state_bytes()
        np.testing.assert_array_equal(br.volume_max().view(np.uint32), self.maxima().view(np.uint32))


class SampleParts(Parts):
    """the same chain for mi_bridge_create_rated's bridge, which moves rows of SAMPLES of one codec pair, code words or
    PCM, at the widest leg's tick: only how a row enters and how the result is handed back differ"""
    ALIGN = 1

    def __init__(self, ctx, mk, n, mm, conf, rates, in_codec, out_codec, plc=False):
        assert len(rates) == n
        super().__init__(ctx, mk, mm, conf, [(r, in_codec, out_codec) for r in rates], plc=plc)
        self.pitch = int(self.leg_len.max())

    def arrive(self, x):
        return np.ascontiguousarray(x).view(np.uint8).reshape(self.n, self.in_pitch)

    def leave(self, held):
        return held.view(np.uint8 if self.oc[0] else np.int16).copy()


def pair(br, ctx, mk, mm, conf, legs, **kw):
    """the parts of a bridge with those legs, their geometry checked against the bridge's"""
    parts = Parts(ctx, mk, mm, conf, legs, **kw)
    assert br.tick_bytes() == (parts.in_pitch, parts.out_pitch)
    for s in range(parts.n):
        assert br.leg_codec(s) == (parts.ic[s], parts.oc[s]) and br.leg_bytes(s) == (parts.in_bytes[s], parts.out_bytes[s])
        assert br.leg_rate(s) == parts.rates[s]
    return parts


# ---- loss concealment for legs of any rate and codec (tests/test_gpu_bridge_concealed.py)

class ConcealedParts(_Legs):
    """another chain: the decoders, a PlcBatch per distinct rate over all n rows (mode 0 for the legs of other rates), and a
    plc-less bridge (`inner`, made with the keyword `form`) that takes the concealed PCM with every leg present"""

    def __init__(self, ctx, mk, mm, conf, legs, form="endpoints"):
        super().__init__(ctx, legs, lambda widest: widest)
        self.plc = {int(r): mk(ms.PlcBatch, self.n, int(r), max_block=self.width) for r in sorted(set(self.rates))}
        self.inner = mk(ms.Bridge, self.n, members=mm, rate=conf, **{form: [(r, PCM16, oc) for r, oc in zip(self.rates, self.oc)]})
        assert self.inner.tick_bytes()[0] == 2 * self.width
        self.t.cuda.synchronize()

    def restart(self, s):
        """a new endpoint's concealer on stream s"""
        self.plc[int(self.rates[s])].reset(s, 1)

    def conceal(self, x, present):
        """the decoders and the concealers: [n, width] int16, a leg's tick at the head of its row"""
        R, C_ = ms.MI_PLC_RECEIVED, ms.MI_PLC_CONCEAL
        modes = {r: self._dev(np.where(self.rates == r, np.where(present, R, C_), 0).astype(np.uint8)) for r in self.plc}
        self.decode(x)
        for r, plc in self.plc.items():
            plc.process(self.pcm, self.lens, modes[r])
        self.ctx.sync()
        return self.pcm.cpu().numpy()

    def tick(self, x, present):
        return one_tick(self.inner, self.conceal(x, present).view(np.uint8))


def loss_patterns(n, nticks=NTICKS, seed=7):
    """present [nticks, n]: per leg none / single losses / a 12-tick burst (past about 90 ms the generated signal is extended
    from itself: the second fftbf) / a 25-tick outage (fade, silence, the cross-fade back) / loss on ticks 0-1 / 15 % random"""
    rng = np.random.default_rng(seed)
    present = np.ones((nticks, n), np.uint8)
    for s in range(n):
        kind = s % 6
        if kind == 1:
            present[[10, 25, 40], s] = 0
        elif kind == 2:
            present[14:26, s] = 0
        elif kind == 3:
            present[12:37, s] = 0
        elif kind == 4:
            present[0:2, s] = 0
        elif kind == 5:
            present[:, s] = rng.random(nticks) >= 0.15
    return present


def leg_rows(oracle, legs, nticks=NTICKS, seed=0, talk=None):
    """[nticks, n, pitch] uint8: every leg's voiced signal through its own encoder at the head of its byte row, the tails
    random (they must be ignored).  talk: the legs that speak; the others send digital silence"""
    from test_gpu_plc import voiced  # the concealer tests' signal
    n = len(legs)
    pitch = up16(max(r // 100 * (1 if ic else 2) for r, ic, _ in legs))
    rng = np.random.default_rng(0xC0 + seed)
    x = rng.integers(0, 256, (nticks, n, pitch), dtype=np.uint8)
    for s, (rate, ic, _) in enumerate(legs):
        ll = rate // 100
        sig = voiced(seed + s, ll * nticks, rate) if talk is None or s in talk else np.zeros(ll * nticks, np.int16)
        sig = sig.reshape(nticks, ll)
        if ic == PCM16:
            x[:, s, :2 * ll] = sig.view(np.uint8)
        else:
            x[:, s, :ll] = oracle.g711_encode(LAW[ic], sig)
    return x


def assert_same_rows(br, got, want, t):
    for s in range(br.n):
        np.testing.assert_array_equal(br.leg_out(got, s), br.leg_out(want, s), err_msg=f"tick {t} leg {s}")


def assert_same_meters(br, inner):
    assert bytes(br.volume_state()) == bytes(inner.volume_state())
    np.testing.assert_array_equal(br.levels().view(np.uint32), inner.levels().view(np.uint32))
    for a, b in zip(br.active_speakers(), inner.active_speakers()):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
