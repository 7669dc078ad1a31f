#!/usr/bin/env python3
"""A conference tick whose legs bring their own codec (mi_bridge_create_legs, bridge_legs_kernel) against (a) the only other
way to serve such a conference, the parts one by one on the C ABI, and (b) the uniform mu-law bridge (bridge_tick_kernel<2, 2>),
all three alternating in one process on one GPU.

    python scripts/bridge_legs_probe.py [--reps 15] [--ticks 200] [--trace]

profiles/bridge_tick.md's shape: 1024 conferences x 32 members at 8 kHz; the codecs in thirds: leg s is mu-law, A-law or
16-bit PCM, in and out, by s % 3.  The parts are six launches: mi_g711_decode per law over that law's rows (the PCM legs'
rows already lie decoded in the buffer: the chain is spared a copy), mi_volume_process, mi_mixer_process, mi_g711_encode
per law.  Figures per tick, each the median of `reps` windows of `ticks` ticks:
  parts_dev   HIP events on the context's stream around the six launches on device-resident buffers (no transfers);
  parts_e2e   host clock around staging -> H2D -> launches -> D2H on the context's stream, synchronised per window;
  mixed_e2e   host clock around acquire / submit / collect of the mixed bridge, three ticks in flight, drained per window;
  uniform_e2e the same of the uniform mu-law bridge.
The kernels' own times come from a separate run: `rocprofv3 --kernel-trace --stats -d <dir> -- python
scripts/bridge_legs_probe.py --trace` (short windows, no timing printed): bridge_legs_kernel against the sum of the parts'
kernels and against bridge_tick_kernel.  Bytes per tick over PCIe and HBM: a PCM leg moves 320 B where a G.711 leg moves 160."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import mediastreamer2_amd as ms  # noqa: E402
from bridge_probe import fused_window, mulaw, synth  # noqa: E402

NCONF, MM, RATE, NS = 1024, 32, 8000, 80
KINDS = (ms.MI_SESSION_PCMU, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCM16)


class Chain:
    """decode x 2, volume, mixer, encode x 2 on device-resident buffers, plus pinned staging for the end-to-end form"""

    def __init__(self, ctx, kind, rows):
        self.ctx, n = ctx, NCONF * MM
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.vol, self.mix = ms.VolumeBatch(ctx, n, RATE), ms.MixerBatch(ctx, NCONF, MM, NS)
        self.d_in = dev(rows)
        self.pcm = torch.zeros((n, NS), dtype=torch.int16, device="cuda")
        self.pcm[dev(kind == ms.MI_SESSION_PCM16)] = dev(rows[kind == ms.MI_SESSION_PCM16, :2 * NS].copy().view(np.int16))
        self.out = torch.zeros((NCONF, MM, NS), dtype=torch.int16, device="cuda")
        self.codes = torch.zeros((n, NS), dtype=torch.uint8, device="cuda")
        self.has = torch.ones(n, dtype=torch.uint8, device="cuda")
        self.lens = {law: dev(np.where(kind == k, NS, 0).astype(np.int32))
                     for law, k in ((ms.MI_LAW_PCMU, ms.MI_SESSION_PCMU), (ms.MI_LAW_PCMA, ms.MI_SESSION_PCMA))}
        self.rows, self.nbytes = rows, rows.nbytes
        self.h_in = ctx.L.mi_host_alloc(ctx.h, self.nbytes)
        self.h_out = ctx.L.mi_host_alloc(ctx.h, self.nbytes)
        torch.cuda.synchronize()

    def launches(self):
        for law, lens in self.lens.items():
            ms.g711_decode(self.ctx, law, self.d_in, self.pcm, length=NS, lens=lens)
        self.vol.process(self.pcm)
        self.mix.process(self.pcm.view(NCONF, MM, NS), self.has, 1, self.out)
        for law, lens in self.lens.items():
            ms.g711_encode(self.ctx, law, self.out.view(-1, NS), self.codes, length=NS, lens=lens)

    def dev_window(self, ticks):
        self.ctx.timer_start()
        for _ in range(ticks):
            self.launches()
        return self.ctx.timer_stop() * 1e3 / ticks  # us per tick

    def e2e_window(self, ticks):  # the same bytes each way as the mixed bridge moves (its rows, both directions)
        L, c = self.ctx.L, self.ctx.h
        t0 = time.perf_counter()
        for _ in range(ticks):
            C.memmove(self.h_in, self.rows.ctypes.data, self.nbytes)
            ms.check(L.mi_copy_h2d_pinned(c, self.d_in.data_ptr(), self.h_in, self.nbytes))
            self.launches()
            ms.check(L.mi_copy_d2h_pinned(c, self.h_out, self.d_in.data_ptr(), self.nbytes))
        self.ctx.sync()
        return (time.perf_counter() - t0) * 1e6 / ticks

    def close(self):
        self.ctx.sync()
        self.ctx.L.mi_host_free(self.ctx.h, self.h_in)
        self.ctx.L.mi_host_free(self.ctx.h, self.h_out)
        self.vol.close(), self.mix.close()


def alaw_of_mulaw_rows(ctx, codes):
    """the A-law legs' input: the library's own encoder over the mu-law legs' signal (the probe's input only)"""
    pcm = torch.zeros(codes.shape, dtype=torch.int16, device="cuda")
    out = torch.zeros(codes.shape, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms.g711_decode(ctx, ms.MI_LAW_PCMU, torch.from_numpy(codes).cuda(), pcm)
    ms.g711_encode(ctx, ms.MI_LAW_PCMA, pcm, out)
    ctx.sync()
    return out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--trace", action="store_true", help="short untimed windows, for a kernel trace of this command")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bridge_legs_probe: no GPU; nothing is measured without one")
    ctx = ms.Context(0)
    n = NCONF * MM
    pcm = synth(n, NS, RATE, 0x5EED)
    mu = mulaw(pcm)
    kind = np.array([KINDS[s % 3] for s in range(n)], np.int32)
    mixed = ms.Bridge(ctx, n, members=MM, rate=RATE, legs=[(RATE, k, k) for k in kind])
    uniform = ms.Bridge(ctx, n, members=MM, rate=RATE, in_codec=ms.MI_SESSION_PCMU, out_codec=ms.MI_SESSION_PCMU)
    pitch = mixed.tick_bytes()[0]
    rows = np.zeros((n, pitch), np.uint8)
    rows[:, :NS] = mu
    rows[kind == ms.MI_SESSION_PCMA, :NS] = alaw_of_mulaw_rows(ctx, mu[kind == ms.MI_SESSION_PCMA])
    rows[kind == ms.MI_SESSION_PCM16, :2 * NS] = pcm[kind == ms.MI_SESSION_PCM16].view(np.uint8)
    chain = Chain(ctx, kind, rows)
    for _ in range(2):  # warm every shape the windows use
        chain.dev_window(10), chain.e2e_window(10), fused_window(mixed, rows, 10), fused_window(uniform, mu, 10)
    if not a.trace:
        t = {k: [] for k in ("parts_dev_us", "parts_e2e_us", "mixed_e2e_us", "uniform_e2e_us")}
        for _ in range(a.reps):
            t["parts_dev_us"].append(chain.dev_window(a.ticks))
            t["mixed_e2e_us"].append(fused_window(mixed, rows, a.ticks))
            t["uniform_e2e_us"].append(fused_window(uniform, mu, a.ticks))
            t["parts_e2e_us"].append(chain.e2e_window(a.ticks))
        med = {k: statistics.median(v) for k, v in t.items()}
        print(json.dumps(dict(conferences=NCONF, members=MM, rate=RATE, codecs="pcmu / pcma / pcm16 in thirds", reps=a.reps, ticks=a.ticks,
                              row_pitch_bytes=pitch, bytes_each_way_mixed=int(mixed.n * pitch), bytes_each_way_uniform=int(n * NS),
                              launches_parts=6, **{k: round(v, 2) for k, v in med.items()},
                              spread={k: [round(min(v), 2), round(max(v), 2)] for k, v in t.items()},
                              mixed_over_parts_e2e=round(med["mixed_e2e_us"] / med["parts_e2e_us"], 3),
                              mixed_over_uniform_e2e=round(med["mixed_e2e_us"] / med["uniform_e2e_us"], 3))), flush=True)
    mixed.close(), uniform.close(), chain.close()
    ctx.close()


if __name__ == "__main__":
    main()
