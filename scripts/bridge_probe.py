#!/usr/bin/env python3
"""A conference tick on mi_bridge (one fused launch) against the same work as four C ABI launches --
mi_g711_decode -> mi_volume_process -> mi_mixer_process -> mi_g711_encode --, A/B in one process on one GPU.

    python scripts/bridge_probe.py [--reps 15] [--ticks 200] [--trace]

Two same-rate sizes: 1024 conferences x 32 members at 8 kHz mu-law, and 128 x 32 at 48 kHz PCM (no codec: two launches).
Two sizes with legs at their own rate (bridge_rated_kernel; --same-rate-only leaves them out): 1024 x 32 legs of 8 kHz
mu-law in a 16 kHz conference, and the same legs in a 48 kHz conference; there the parts are six launches -- decode,
volume, up-sample, mix, down-sample, encode.
Three figures per size, each the median of `reps` windows of `ticks` ticks, A and B alternating:
  parts_dev   HIP events on the context's stream around the launches on device-resident buffers (no transfers);
  parts_e2e   host clock around staging -> H2D -> launches -> D2H on the context's stream, synchronised per window;
  fused_e2e   host clock around mi_bridge acquire / submit / collect, three ticks in flight, drained per window.
The kernel's own time comes from a separate run: `rocprofv3 --kernel-trace --stats -d <dir> -- python
scripts/bridge_probe.py --trace` (short windows, no timing printed); bridge_tick_kernel against the sum of the
parts' kernels.  Algorithmic bytes: what arrives plus what leaves, 160 B per 8 kHz G.711 leg-tick."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mediastreamer2_amd as ms  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, spec


def synth(n, ns, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(ns) / rate
    x = rng.normal(0.0, 3000.0, (n, ns)) + 3276.7 * np.sin(2 * np.pi * 1000.0 * t)
    return np.clip(np.round(x), -32767, 32767).astype(np.int16)


def mulaw(pcm):
    """G.711 mu-law of int16 (the probe's input only; the codec under test is the library's)"""
    v = pcm.astype(np.int32) >> 2
    sign = v < 0
    mag = np.minimum(np.abs(v), 8159) + 33
    seg = np.maximum(np.floor(np.log2(mag)).astype(np.int32) - 5, 0)
    code = np.where(seg >= 8, 0x7F, (seg << 4) | ((mag >> (seg + 1)) & 15))
    return (code ^ np.where(sign, 0x7F, 0xFF)).astype(np.uint8)


class Parts:
    """the four launches on device-resident buffers, plus pinned staging for the end-to-end form"""

    def __init__(self, ctx, nconf, mm, rate, codec, x, leg=None):
        self.ctx, self.n, self.mm, self.ns, self.codec = ctx, nconf * mm, mm, rate // 100, codec
        n, ns = self.n, self.ns
        self.leg = leg = leg or rate
        self.ls = ls = leg // 100  # the legs' tick; ns is the conference's
        self.vol = ms.VolumeBatch(ctx, n, leg)
        self.mix = ms.MixerBatch(ctx, nconf, mm, ns)
        self.d_in = torch.from_numpy(x).cuda()
        self.pcm = torch.zeros((n, ls), dtype=torch.int16, device="cuda")
        self.out = torch.zeros((nconf, mm, ns), dtype=torch.int16, device="cuda")
        self.codes = torch.zeros((n, ls), dtype=torch.uint8, device="cuda")
        self.has = torch.ones(n, dtype=torch.uint8, device="cuda")
        if leg != rate:  # in_resampler and out_resampler of every pin (audioconference.c:209-257)
            self.up, self.down = ms.ResamplerBatch(ctx, n, leg, rate), ms.ResamplerBatch(ctx, n, rate, leg)
            self.wide = torch.zeros((n, ns), dtype=torch.int16, device="cuda")
            self.back = torch.zeros((n, ls), dtype=torch.int16, device="cuda")
        self.in_bytes, self.out_bytes = x.nbytes, n * ls * (1 if codec else 2)
        self.h_in = ctx.L.mi_host_alloc(ctx.h, self.in_bytes)
        self.h_out = ctx.L.mi_host_alloc(ctx.h, self.out_bytes)
        C.memmove(self.h_in, x.ctypes.data, self.in_bytes)
        self.x = x
        torch.cuda.synchronize()

    def launches(self):
        if self.codec:
            ms.g711_decode(self.ctx, ms.MI_LAW_PCMU, self.d_in, self.pcm)
            rows = self.pcm
        else:
            rows = self.d_in  # (levelled in place: the probe times, it does not compare)
        self.vol.process(rows)
        if self.leg != self.ns * 100:
            L = self.ctx.L
            ms.check(L.mi_resampler_process(self.up.h, rows.data_ptr(), self.ls, self.ls, self.wide.data_ptr(), self.ns, None))
            self.mix.process(self.wide.view(-1, self.mm, self.ns), self.has, 1, self.out)
            ms.check(L.mi_resampler_process(self.down.h, self.out.data_ptr(), self.ns, self.ns, self.back.data_ptr(), self.ls, None))
            left = self.back
        else:
            self.mix.process(rows.view(-1, self.mm, self.ns), self.has, 1, self.out)
            left = self.out.view(self.n, self.ns)
        if self.codec:
            ms.g711_encode(self.ctx, ms.MI_LAW_PCMU, left, self.codes)

    def dev_window(self, ticks):
        self.ctx.timer_start()
        for _ in range(ticks):
            self.launches()
        return self.ctx.timer_stop() * 1e3 / ticks  # us per tick

    def e2e_window(self, ticks):
        L, c = self.ctx.L, self.ctx.h
        leaving = self.codes if self.codec else (self.back if self.leg != self.ns * 100 else self.out)
        t0 = time.perf_counter()
        for _ in range(ticks):
            C.memmove(self.h_in, self.x.ctypes.data, self.in_bytes)  # the host fills the staging, as it does the bridge's
            ms.check(L.mi_copy_h2d_pinned(c, self.d_in.data_ptr(), self.h_in, self.in_bytes))
            self.launches()
            ms.check(L.mi_copy_d2h_pinned(c, self.h_out, leaving.data_ptr(), self.out_bytes))
        self.ctx.sync()
        return (time.perf_counter() - t0) * 1e6 / ticks

    def close(self):
        self.ctx.sync()
        self.ctx.L.mi_host_free(self.ctx.h, self.h_in)
        self.ctx.L.mi_host_free(self.ctx.h, self.h_out)
        self.vol.close()
        self.mix.close()
        if self.leg != self.ns * 100:
            self.up.close(), self.down.close()


def fused_window(br, x, ticks):
    t0 = time.perf_counter()
    for _ in range(ticks):
        if br.in_flight() == 3:
            br.collect()
        h_in, _ = br.acquire()
        h_in[:] = x
        br.submit()
    while br.in_flight():
        br.collect()
    return (time.perf_counter() - t0) * 1e6 / ticks


def measure(ctx, nconf, mm, rate, codec, reps, ticks, trace, leg=None):
    leg = leg or rate
    n, ns = nconf * mm, leg // 100
    pcm = synth(n, ns, leg, 0x5EED)
    x = mulaw(pcm) if codec else pcm
    kind = ms.MI_SESSION_PCMU if codec else ms.MI_SESSION_PCM16
    rated = dict(leg_rates=[leg] * n) if leg != rate else {}
    br = ms.Bridge(ctx, n, members=mm, rate=rate, in_codec=kind, out_codec=kind, **rated)
    parts = Parts(ctx, nconf, mm, rate, codec, x, leg)
    for _ in range(2):  # warm every shape the windows use
        parts.dev_window(10), parts.e2e_window(10), fused_window(br, x, 10)
    if trace:
        br.close(), parts.close()
        return None
    dev, e2e, fused = [], [], []
    for _ in range(reps):
        dev.append(parts.dev_window(ticks))
        fused.append(fused_window(br, x, ticks))
        e2e.append(parts.e2e_window(ticks))
    br.close(), parts.close()
    alg = n * ns * (2 if codec else 4)  # bytes in + bytes out
    med = {k: statistics.median(v) for k, v in (("parts_dev_us", dev), ("parts_e2e_us", e2e), ("fused_e2e_us", fused))}
    return dict(conferences=nconf, members=mm, rate=rate, leg_rate=leg, codec="pcmu" if codec else "pcm16", algorithmic_bytes=alg,
                launches_parts=(4 if codec else 2) + (2 if leg != rate else 0), **{k: round(v, 2) for k, v in med.items()},
                spread={"parts_dev_us": [round(min(dev), 2), round(max(dev), 2)], "parts_e2e_us": [round(min(e2e), 2), round(max(e2e), 2)],
                        "fused_e2e_us": [round(min(fused), 2), round(max(fused), 2)]},
                fused_over_parts_e2e=round(med["fused_e2e_us"] / med["parts_e2e_us"], 3),
                hbm_time_at_peak_us=round(alg / HBM_PEAK * 1e6, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--trace", action="store_true", help="short untimed windows, for a kernel trace of this command")
    ap.add_argument("--same-rate-only", action="store_true", help="only the two shapes whose legs run at the conference's rate")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bridge_probe: no GPU; nothing is measured without one")
    ctx = ms.Context(0)
    shapes = [(1024, 32, 8000, True, None), (128, 32, 48000, False, None)]
    if not a.same_rate_only:  # 32 members of a 48 kHz conference with ratio-6 scratch are 58 KB of LDS: one workgroup per CU
        shapes += [(1024, 32, 16000, True, 8000), (1024, 32, 48000, True, 8000)]
    for nconf, mm, rate, codec, leg in shapes:
        r = measure(ctx, nconf, mm, rate, codec, a.reps, a.ticks, a.trace, leg)
        if r:
            print(json.dumps(r), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
