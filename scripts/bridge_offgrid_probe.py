#!/usr/bin/env python3
"""A conference tick with members at 44 100 Hz (mi_bridge_create_offgrid, bridge_offgrid_kernel) against (a) the only other way
to serve such a conference, the parts one by one on the C ABI, and (b) as a sanity figure the same conferences with the
44.1 kHz third moved to 12 kHz, on the grid, where bridge_ratios_kernel runs (ratios=); all three alternating in one process
on one GPU.

    python scripts/bridge_offgrid_probe.py [--reps 15] [--ticks 100]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/bridge_offgrid_probe.py --trace
    python scripts/bridge_offgrid_probe.py --summarise <dir>

The shape: 1024 conferences x 32 legs in a 16 kHz mix, leg s an 8 kHz mu-law trunk, a 44.1 kHz PCM member or a 16 kHz PCM
member by s % 3.  The parts are ten launches: mi_g711_decode over the trunks, mi_volume_process per leg rate (three),
mi_resampler_process_masked 8 -> 16 and 44.1 -> 16 kHz, mi_mixer_process, mi_resampler_process_masked 16 -> 8 and 16 -> 44.1 kHz,
mi_g711_encode over the trunks.  The chain is spared the copies tests/bridge_parts.py makes: the 44.1 -> 16 kHz resampler's rows
(which need room for one sample more than the mixer's contiguous rows have) are not moved onto the mixer's, nor are the 16 kHz
members' -- it reads stand-in rows of the same size.
Figures per tick, each the median of `reps` windows of `ticks` ticks:
  parts_dev     HIP events on the context's stream around the ten launches on device-resident buffers (no transfers);
  offgrid_e2e   host clock around acquire / submit / collect of the bridge, three ticks in flight, drained per window;
  ratios_e2e    the same of the neighbour bridge.
A bridge's kernel cannot be bracketed by HIP events apart from its tick's transfers through the C ABI (the launch waits for
the upload on another stream), so the kernels' own times come from the kernel trace of the same command (--trace: short
untimed windows), medians over its dispatches (--summarise)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

NCONF, MM, CONF, NS = 1024, 32, 16000, 160
RATES = (8000, 44100, 16000)
NEIGHBOUR = (8000, 12000, 16000)
W = 456  # samples per row at the legs' rates: the widest tick and a resampler's one sample of room, rounded to eight


def summarise(d):
    """medians per kernel over the dispatches of a rocprofv3 kernel trace (csv)"""
    dur = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            dur.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if not dur:
        sys.exit(f"bridge_offgrid_probe: no kernel trace under {d}")
    rows = sorted(((k, len(v), statistics.median(v), min(v), max(v)) for k, v in dur.items()), key=lambda r: -r[1] * r[2])
    for k, n, med, lo, hi in rows:
        print(f"{med:10.2f} us median  [{lo:9.2f} .. {hi:9.2f}]  x {n:5d}  sum {med * n:10.1f}  {k[:140]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--trace", action="store_true", help="short untimed windows, for a kernel trace of this command")
    ap.add_argument("--summarise", metavar="DIR", help="medians per kernel of the kernel trace under DIR; nothing runs")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)

    import torch

    import mediastreamer2_amd as ms
    from bridge_probe import fused_window, mulaw, synth

    if not torch.cuda.is_available():
        sys.exit("bridge_offgrid_probe: no GPU; nothing is measured without one")
    PCM16, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMU
    ctx = ms.Context(0)
    n = NCONF * MM
    rate = np.array([RATES[s % 3] for s in range(n)], np.int32)
    leg_len = rate // 100
    triple = lambda s, rates: (int(rates[s % 3]), PCMU if s % 3 == 0 else PCM16, PCMU if s % 3 == 0 else PCM16)
    offgrid = ms.Bridge(ctx, n, members=MM, rate=CONF, offgrid=[triple(s, RATES) for s in range(n)])
    ratios = ms.Bridge(ctx, n, members=MM, rate=CONF, ratios=[triple(s, NEIGHBOUR) for s in range(n)])
    pitch, pitch_ratios = offgrid.tick_bytes()[0], ratios.tick_bytes()[0]
    rows, rows_ratios = np.zeros((n, pitch), np.uint8), np.zeros((n, pitch_ratios), np.uint8)
    for k, (r, rn) in enumerate(zip(RATES, NEIGHBOUR)):
        sel = np.arange(n) % 3 == k
        for dst, rr in ((rows, r), (rows_ratios, rn)):
            pcm = synth(int(sel.sum()), rr // 100, rr, 0x5EED + rr)
            dst[sel, :(rr // 100) * (1 if k == 0 else 2)] = mulaw(pcm) if k == 0 else pcm.view(np.uint8)

    # ---- the parts on device-resident buffers
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    z = lambda cols, dt=torch.int16: torch.zeros((n, cols), dtype=dt, device="cuda")
    d_in, pcm, back, wide, mixed, codes, roomy = dev(rows), z(W), z(W), z(NS), z(NS), z(80, torch.uint8), z(NS + 8)
    for r in (44100, 16000):
        pcm[dev(rate == r), :r // 100] = dev(rows[rate == r, :r // 50].copy().view(np.int16))
    vol = {r: ms.VolumeBatch(ctx, n, r) for r in RATES}
    res_in = {r: ms.ResamplerBatch(ctx, n, r, CONF) for r in RATES if r != CONF}
    res_out = {r: ms.ResamplerBatch(ctx, n, CONF, r) for r in RATES if r != CONF}
    mix = ms.MixerBatch(ctx, NCONF, MM, NS)
    lens = {r: dev(np.where(rate == r, leg_len, 0).astype(np.int32)) for r in RATES}
    mask = {r: dev((rate == r).astype(np.uint8)) for r in RATES}
    has = torch.ones(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def launches():
        ms.g711_decode(ctx, ms.MI_LAW_PCMU, d_in, pcm, length=80, lens=lens[8000])
        for r in RATES:
            vol[r].process(pcm, nsamples=r // 100, per_stream=lens[r])
        for r, rs in res_in.items():
            dst, stride = (roomy, NS + 8) if r > CONF or CONF % r else (wide, NS)
            ms.check(ctx.L.mi_resampler_process_masked(rs.h, ms._ptr(pcm), r // 100, W, ms._ptr(dst), stride, None, ms._ptr(mask[r])))
        mix.process(wide.view(NCONF, MM, NS), has, 1, mixed.view(NCONF, MM, NS))
        for r, rs in res_out.items():
            ms.check(ctx.L.mi_resampler_process_masked(rs.h, ms._ptr(mixed), NS, NS, ms._ptr(back), W, None, ms._ptr(mask[r])))
        ms.g711_encode(ctx, ms.MI_LAW_PCMU, back, codes, length=80, lens=lens[8000])

    def parts_window(ticks):
        ctx.timer_start()
        for _ in range(ticks):
            launches()
        return ctx.timer_stop() * 1e3 / ticks  # us per tick

    for _ in range(2):  # warm every shape the windows use
        parts_window(5), fused_window(offgrid, rows, 5), fused_window(ratios, rows_ratios, 5)
    if not a.trace:
        t = {k: [] for k in ("parts_dev_us", "offgrid_e2e_us", "ratios_e2e_us")}
        for _ in range(a.reps):
            t["parts_dev_us"].append(parts_window(a.ticks))
            t["offgrid_e2e_us"].append(fused_window(offgrid, rows, a.ticks))
            t["ratios_e2e_us"].append(fused_window(ratios, rows_ratios, a.ticks))
        med = {k: statistics.median(v) for k, v in t.items()}
        print(json.dumps(dict(conferences=NCONF, members=MM, rate=CONF, legs="8k pcmu / 44.1k pcm16 / 16k pcm16 in thirds",
                              neighbour="8k pcmu / 12k pcm16 / 16k pcm16 in thirds", reps=a.reps, ticks=a.ticks, row_pitch_bytes=pitch,
                              bytes_each_way=int(n * pitch), launches_parts=10, **{k: round(v, 2) for k, v in med.items()},
                              spread={k: [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})), flush=True)
    offgrid.close(), ratios.close(), mix.close()
    for b in list(vol.values()) + list(res_in.values()) + list(res_out.values()):
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
