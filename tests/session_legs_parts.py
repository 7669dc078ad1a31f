"""The yardstick of tests/test_gpu_session_legs.py: what mi_session_create_legs' session computes, from parts called one by
one.  A twin mi_session_create session runs at in_rate == rate with 16-bit PCM in and out -- the same tail_ms, agc, stagger,
ref_loopback, ref_delay_ms and members, plc off -- wrapped in per-kind class batches of the existing C ABI: in front
mi_g711_decode per law -> (mi_plc_process at the class's rate) -> mi_resampler_process, behind mi_resampler_process ->
mi_g711_encode.  A seat's class resamplers and concealer are reset at the tick its JOIN or reset takes effect.  Every leg's
first leg_bytes of every tick's output must equal this BIT FOR BIT: the same arithmetic on the same device.  A helper module
like tests/bridge_parts.py, whose `mk` fixture the test module imports from there."""
import numpy as np

import mediastreamer2_amd as ms
from conftest import synth_pcm

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
LAW = {PCMA: ms.MI_LAW_PCMA, PCMU: ms.MI_LAW_PCMU}
JOIN, LEAVE = ms.MI_SESSION_JOIN, ms.MI_SESSION_LEAVE


def up16(v):
    return (int(v) + 15) & ~15


class Shape:
    """the legs' geometry as the header states it: byte rows at the widest leg's tick in bytes, rounded up to 16"""

    def __init__(self, legs, rate):
        self.legs = np.asarray(legs, np.int32)
        self.n, self.rate, self.len = len(self.legs), rate, rate // 100
        self.rates, self.ic, self.oc = self.legs[:, 0], self.legs[:, 1], self.legs[:, 2]
        self.leg_len = self.rates // 100
        self.mic_bytes = self.leg_len * np.where(self.ic, 1, 2)
        self.out_bytes = self.leg_len * np.where(self.oc, 1, 2)
        self.mic_pitch, self.out_pitch = up16(self.mic_bytes.max()), up16(self.out_bytes.max())
        self.kinds = sorted({tuple(int(v) for v in k) for k in self.legs})
        self.members = {k: np.nonzero((self.legs == np.array(k)).all(axis=1))[0] for k in self.kinds}


def signals(oracle, shape, nticks, seed=0, echo=True):
    """speech-like noise with a tone per leg and, with `echo`, the far end's echo 5 ms late at 0.4: (mic [n] rows of bytes over
    nticks at each leg's rate and codec, ref [n, nticks * len] at `rate`)"""
    ref = np.stack([synth_pcm(seed + 500 + s, shape.len * nticks, rate=shape.rate, sigma=3000.0) for s in range(shape.n)])
    mic = []
    for s in range(shape.n):
        r, ll = shape.rate // int(shape.rates[s]), int(shape.leg_len[s])
        x = synth_pcm(seed + 40 + s, ll * nticks, rate=int(shape.rates[s]), sigma=2500.0, tone_hz=400.0 + 60 * s).astype(np.int32)
        if echo:
            far = ref[s, ::r].astype(np.int32)
            x[ll // 2:] += (far[:len(x) - ll // 2] * 2) // 5
        x = np.clip(x, -32767, 32767).astype(np.int16)
        mic.append(oracle.g711_encode(LAW[int(shape.ic[s])], x[None])[0] if shape.ic[s] else x.view(np.uint8))
    return mic, ref


def fill(se, shape, sig, t, rng, lost=None):
    """one tick into a legs session's staging: each leg's own bytes, the rest of every mic row random (never read).  Returns
    copies of what was staged, for the yardstick"""
    mic, ref = sig
    h_mic, h_ref = se.acquire()
    assert h_mic.shape == (shape.n, shape.mic_pitch) and h_mic.dtype == np.uint8
    h_mic[:] = rng.integers(0, 256, h_mic.shape, dtype=np.uint8)
    for s in range(shape.n):
        b = int(shape.mic_bytes[s])
        h_mic[s, :b] = mic[s][t * b:(t + 1) * b]
    if h_ref is not None:
        h_ref[:] = ref[:, t * shape.len:(t + 1) * shape.len]
    if lost is not None:
        se.events()[lost] = ms.MI_PLC_CONCEAL
    return h_mic.copy(), None if h_ref is None else h_ref.copy()


class Yardstick:
    """the twin and the class batches.  tick() takes what fill() stages and returns the byte rows [n, out_pitch] a legs session
    must produce (a leg's first out_bytes; the rest zero).  The twin runs one tick at a time"""

    def __init__(self, ctx, mk, shape, members, plc=False, **cfg):
        import torch
        self.t, self.ctx, self.shape, self.plc_on = torch, ctx, shape, plc
        self.twin = mk(ms.Session, shape.n, members=members, in_rate=shape.rate, rate=shape.rate, tail_ms=32, plc=False, **cfg)
        self.cls = {}
        for kind, idx in shape.members.items():
            rate, k = kind[0], len(idx)
            c = dict(idx=idx, rank={int(s): i for i, s in enumerate(idx)})
            c["plc"] = mk(ms.PlcBatch, k, rate, max_block=rate // 100) if plc else None
            c["up"] = mk(ms.ResamplerBatch, k, rate, shape.rate) if rate != shape.rate else None
            c["down"] = mk(ms.ResamplerBatch, k, shape.rate, rate) if rate != shape.rate else None
            c["lens"] = torch.full((k,), rate // 100, dtype=torch.int32, device="cuda")
            self.cls[kind] = c
        torch.cuda.synchronize()

    def _dev(self, a):
        d = self.t.from_numpy(np.ascontiguousarray(a)).cuda()
        self.t.cuda.synchronize()
        return d

    def _host(self, d):
        self.ctx.sync()
        return d.cpu().numpy()

    def fresh(self, seat):
        """a NEW endpoint on the seat: its class resamplers' and concealer's state of that stream start over"""
        c = self.cls[tuple(int(v) for v in self.shape.legs[seat])]
        for part in ("up", "down", "plc"):
            if c[part] is not None:
                c[part].reset(c["rank"][int(seat)], 1)

    # membership, as the legs session is told it
    def change_members(self, changes):
        self.twin.change_members(changes)
        for seat, op in changes:
            if op == JOIN:
                self.fresh(seat)

    def remove_member(self, seat):
        self.twin.remove_member(seat)

    def add_member(self, seat):
        self.twin.add_member(seat)
        self.fresh(seat)

    def reset_streams(self, first, count):
        self.twin.reset_streams(first, count)
        for s in range(first, first + count):
            self.fresh(s)

    def front(self, x, lost):
        """byte rows -> the microphone tick at `rate` [n, len], class by class"""
        sh, torch = self.shape, self.t
        mic = np.zeros((sh.n, sh.len), np.int16)
        for kind, c in self.cls.items():
            (rate, ic, _), idx = kind, c["idx"]
            ll = rate // 100
            rows = np.ascontiguousarray(x[idx, :ll * (1 if ic else 2)])
            if ic:
                pcm = torch.zeros((len(idx), ll), dtype=torch.int16, device="cuda")
                torch.cuda.synchronize()
                codes = self._dev(rows)
                ms.g711_decode(self.ctx, LAW[ic], codes, pcm)
                self.ctx.sync()  # (before torch may hand `codes`' memory to the next tensor)
            else:
                pcm = self._dev(rows.view(np.int16))
            if c["plc"] is not None:
                modes = np.where(lost[idx], ms.MI_PLC_CONCEAL, ms.MI_PLC_RECEIVED).astype(np.uint8)
                events = self._dev(modes)
                c["plc"].process(pcm, c["lens"], events)
                self.ctx.sync()
            if c["up"] is not None:
                leg_rate, pcm = pcm, c["up"].process(pcm)[0]
                self.ctx.sync()  # (`leg_rate` is read until here)
            mic[idx] = self._host(pcm)[:, :sh.len]
        return mic

    def back(self, mix):
        """the twin's mixes [n, len] -> byte rows [n, out_pitch], class by class"""
        sh, torch = self.shape, self.t
        out = np.zeros((sh.n, sh.out_pitch), np.uint8)
        for kind, c in self.cls.items():
            (rate, _, oc), idx = kind, c["idx"]
            ll = rate // 100
            pcm = self._dev(mix[idx])
            if c["down"] is not None:
                down = c["down"].process(pcm)[0]
                self.ctx.sync()  # (the slice below is torch's, on its own stream)
                pcm = down[:, :ll].contiguous()
                torch.cuda.synchronize()
            if oc:
                codes = torch.zeros((len(idx), ll), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ms.g711_encode(self.ctx, LAW[oc], pcm, codes)
                out[idx, :ll] = self._host(codes)
            else:
                out[idx, :2 * ll] = self._host(pcm).view(np.uint8)
        return out

    def tick(self, x, ref=None, lost=None):
        lost = np.zeros(self.shape.n, bool) if lost is None else lost
        mic = self.front(x, lost)
        h_mic, h_ref = self.twin.acquire()
        h_mic[:] = mic
        if h_ref is not None:
            h_ref[:] = ref
        self.twin.submit()
        return self.back(self.twin.collect().copy())
