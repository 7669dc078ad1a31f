#!/usr/bin/env python3
"""A tick of a session whose legs differ in rate and codec (mi_session_create_legs: session_ingress_kernel, the canceller,
volume + mix, session_egress_kernel) against the only way the same thing could be computed before it: a twin session at the
canceller's rate with PCM in and out, and around it the class batches of the C ABI launched one by one from the same thread
(tests/session_legs_parts.py is that yardstick, checked bit for bit); and, as the figure that must not move, the uniform
16 kHz -> 48 kHz session.  All three alternate in one process on one GPU.

    python scripts/session_legs_probe.py [--blocks 5] [--ticks 50]            # one JSON line
    python scripts/session_legs_probe.py --uniform [--tree PARENT_CHECKOUT]   # the uniform session alone, of another build
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/session_legs_probe.py --trace
    python scripts/session_legs_probe.py --summarise <dir>

The shape: 1024 conferences x 32 legs at 48 kHz, the legs a quarter each of 8 kHz mu-law, 8 kHz A-law, 16 kHz PCM and 48 kHz
PCM, tail_ms 128, AGC, stagger, the far end looped back on the device (no reference upload), no graphs, three ticks in flight.
The yardstick's ten launches per tick: mi_g711_decode per law (2), mi_resampler_process 8 -> 48 and 16 -> 48 kHz (2), the
twin's canceller and volume + mix (2), mi_resampler_process 48 -> 8 and 48 -> 16 kHz (2), mi_g711_encode per law (2); the new
session's four: ingress, canceller, volume + mix, egress.  The class batches run on device-resident stand-in rows of the right
sizes on the context's stream and are spared the copies between them and the twin's staging that the test's yardstick makes
through the host, so the yardstick's figure is a lower bound of what a server on the old interface would pay.
A figure is the median over the ticks of `blocks` blocks of `ticks` ticks after a warm-up block, the three forms taking turns
block by block; a tick is one pass of the loop -- collect the oldest when three are in flight, acquire, submit -- whose
steady-state period is the tick's; the first five passes of a block (the ring filling) are dropped.  The staging is filled
once per slot, not per tick: a memcpy of 31 MB by the host would be most of what is timed.  The kernels' own times come from
the kernel trace of the same command (--trace: short untimed blocks), medians over its dispatches (--summarise).
Measured on one MI355X lease (profiles/session_legs.md has the tables; the host's load average was 41 falling to 34 on 256
CPUs, other work beside it): tick period, median [p10 .. p90] over 225 ticks -- the new session 2463.7 us [2432.6 .. 2506.4],
the yardstick 3205.9 us [3169.9 .. 3256.1], ratio 0.77: not slower than what it replaces; the uniform session 2411.7 and
2439.9 us on this commit against 2521.1 and 2416.5 us on the parent, alternating: inside the run-to-run spread.  Kernel
trace: session_egress_kernel 74.0 us; session_ingress_kernel 44.1 us at its fastest but 608.0 us at the median, which the tick
period does not contain (it exceeds the canceller's 2380.9 us by 82.8 us in all) -- what the trace counts there is open."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCONF, MM, RATE = 1024, 32, 48000
FILL = 5  # passes at the head of a block that do not wait for a collect
LAUNCHES = dict(legs=4, yardstick=10)


def summarise(d):
    """medians per kernel over the dispatches of a rocprofv3 kernel trace (csv)"""
    dur = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            dur.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if not dur:
        sys.exit(f"session_legs_probe: no kernel trace under {d}")
    rows = sorted(((k, len(v), statistics.median(v), min(v), max(v)) for k, v in dur.items()), key=lambda r: -r[1] * r[2])
    for k, n, med, lo, hi in rows:
        print(f"{med:10.2f} us median  [{lo:9.2f} .. {hi:9.2f}]  x {n:5d}  sum {med * n:10.1f}  {k[:140]}")


def step(se):
    if se.in_flight() == 3:
        se.collect()
    se.acquire()
    se.submit()


def drain(se):
    while se.in_flight():
        se.collect()


def block(tick, se, ticks):
    """per-pass host time in us of `ticks` passes, the ring drained behind them"""
    out = []
    for _ in range(ticks):
        t0 = time.perf_counter()
        tick()
        out.append((time.perf_counter() - t0) * 1e6)
    drain(se)
    return out[FILL:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--uniform", action="store_true", help="the uniform 16 -> 48 kHz session alone")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose mediastreamer2_amd is measured (default: this one)")
    ap.add_argument("--trace", action="store_true", help="short untimed blocks, for a kernel trace of this command")
    ap.add_argument("--summarise", metavar="DIR", help="medians per kernel of the kernel trace under DIR; nothing runs")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    assert a.trace or (a.blocks * (a.ticks - FILL) >= 200 and a.ticks >= 50), "a figure is a median of at least 200 ticks after 50"
    sys.path.insert(0, os.path.abspath(a.tree))

    import torch

    import mediastreamer2_amd as ms

    if not torch.cuda.is_available():
        sys.exit("session_legs_probe: no GPU; nothing is measured without one")
    PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
    ctx = ms.Context(0)
    n, q = NCONF * MM, NCONF * MM // 4
    common = dict(members=MM, rate=RATE, tail_ms=128, agc=True, stagger=True, use_graphs=False, ref_loopback=True)
    rng = np.random.default_rng(0x5EED)
    noise = lambda rows, cols: np.clip(rng.normal(0.0, 3000.0, (rows, cols)), -32767, 32767).astype(np.int16)

    def stage(se, rows):
        """every slot's staging filled once"""
        for _ in range(3):
            h_mic, _ = se.acquire()
            h_mic[:] = rows
            se.submit()
        drain(se)

    forms = {}
    uniform = ms.Session(ctx, n, in_rate=16000, **common)
    stage(uniform, noise(n, 160))
    forms["uniform"] = (lambda: step(uniform), uniform)
    made = [uniform]
    if not a.uniform:
        kinds = ((8000, PCMU, PCMU), (8000, PCMA, PCMA), (16000, PCM16, PCM16), (48000, PCM16, PCM16))
        legs = ms.Session(ctx, n, legs=[kinds[s % 4] for s in range(n)], **common)
        mic_pitch, _, out_pitch = legs.tick_bytes()
        rows = np.zeros((n, mic_pitch), np.uint8)
        for s4, (r, ic, _) in enumerate(kinds):
            b = r // 100 * (1 if ic else 2)
            rows[s4::4, :b] = rng.integers(0x90, 0xf0, (q, b), dtype=np.uint8) if ic else noise(q, r // 100).view(np.uint8)
        stage(legs, rows)
        twin = ms.Session(ctx, n, in_rate=RATE, **common)
        stage(twin, noise(n, 480))
        # the class batches on device-resident stand-in rows
        z = lambda r, c, dt=torch.int16: torch.zeros((r, c), dtype=dt, device="cuda")
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        codes_in = {law: dev(rng.integers(0x90, 0xf0, (q, 80), dtype=np.uint8)) for law in (ms.MI_LAW_PCMU, ms.MI_LAW_PCMA)}
        pcm8, pcm16, up8_out, up16_out = z(2 * q, 80), dev(noise(q, 160)), z(2 * q, 480), z(q, 480)
        mix8, mix16 = dev(noise(2 * q, 480)), dev(noise(q, 480))
        up8, up16 = ms.ResamplerBatch(ctx, 2 * q, 8000, RATE), ms.ResamplerBatch(ctx, q, 16000, RATE)
        down8, down16 = ms.ResamplerBatch(ctx, 2 * q, RATE, 8000), ms.ResamplerBatch(ctx, q, RATE, 16000)
        down8_out, down16_out = z(2 * q, (down8.out_capacity(480) + 7) & ~7), z(q, (down16.out_capacity(480) + 7) & ~7)
        codes_out = {law: z(q, 80, torch.uint8) for law in codes_in}
        torch.cuda.synchronize()
        made += [legs, twin, up8, up16, down8, down16]

        def yardstick():
            for i, law in enumerate(codes_in):
                ms.g711_decode(ctx, law, codes_in[law], pcm8[i * q:(i + 1) * q])
            up8.process(pcm8, out=up8_out)
            up16.process(pcm16, out=up16_out)
            step(twin)
            down8.process(mix8, out=down8_out)
            down16.process(mix16, out=down16_out)
            for i, law in enumerate(codes_out):
                ms.g711_encode(ctx, law, down8_out[i * q:(i + 1) * q], codes_out[law], length=80)

        forms["legs"] = (lambda: step(legs), legs)
        forms["yardstick"] = (yardstick, twin)

    t = {k: [] for k in forms}
    for k, (tick, se) in forms.items():  # the warm-up block
        block(tick, se, 10 if a.trace else max(50, a.ticks))
    ctx.sync()
    for _ in range(1 if a.trace else a.blocks):
        for k, (tick, se) in forms.items():
            t[k] += block(tick, se, 10 if a.trace else a.ticks)
            ctx.sync()
    if not a.trace:
        pct = lambda v, p: float(np.percentile(v, p))
        out = dict(conferences=NCONF, members=MM, rate=RATE, tree=os.path.abspath(a.tree), blocks=a.blocks, ticks_per_block=a.ticks,
                   loadavg=[round(x, 2) for x in os.getloadavg()], cpus=os.cpu_count())
        if not a.uniform:
            out.update(legs="8k pcmu / 8k pcma / 16k pcm16 / 48k pcm16 in quarters", row_pitch_bytes=[mic_pitch, out_pitch], launches=LAUNCHES)
        for k, v in t.items():
            out[k + "_tick_us"] = dict(median=round(statistics.median(v), 1), p10=round(pct(v, 10), 1), p90=round(pct(v, 90), 1), ticks=len(v))
        print(json.dumps(out), flush=True)
    for b in made:
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
