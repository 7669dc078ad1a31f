#!/usr/bin/env python3
"""What membership changes cost on a bridge at a size a user runs: 1024 conferences x 32 seats of 8 kHz mu-law trunks, the open
bridge admitting 16 kHz and 48 kHz PCM members as well (mi_bridge_create_open), three ticks in flight.

    python scripts/bridge_open_probe.py [--reps 200]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/bridge_open_probe.py --trace [--ticks 200]
    python scripts/bridge_open_probe.py --summarise <dir> [--ticks 200]

Runs on a tree without mi_bridge_change_members too (the figures that need it are left out), so that two builds can alternate
in one session.  Figures, one JSON line:
  pair_us        host time of a leave + join of one seat through mi_bridge_remove_member + mi_bridge_add_member, the waiting
                 pair, with three ticks in flight: median and [min, max] of `reps`;
  change_us      the same through ONE mi_bridge_change_members call holding a JOIN on the taken seat (a replacement is leave +
                 join); two_calls_us: a LEAVE call and then a JOIN call; change_submit_us: the call and the submit that carries
                 it; submit_us: a submit that carries nothing, for comparison;
  tick_ms[k]     HIP events on the context's stream around the submit of a tick that carries k changes (k = 0, 1, 16, 256,
                 nstreams replacements by a 16 kHz PCM member), the pipe drained before: the wait for the tick's upload, the
                 apply launch and the tick's kernel; median of 15.
--trace: `ticks` ticks without a change on the closed bridge (ratios=) and then on the open one, for a kernel trace of this
command; --summarise: dispatches per tick and the median duration per kernel of that trace."""
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

NCONF, MM, CONF = 1024, 32, 8000


def summarise(d, ticks):
    dur = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            dur.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if not dur:
        sys.exit(f"bridge_open_probe: no kernel trace under {d}")
    for k, v in sorted(dur.items(), key=lambda kv: -len(kv[1]) * statistics.median(kv[1])):
        print(f"{statistics.median(v):10.2f} us median  [{min(v):9.2f} .. {max(v):9.2f}]  x {len(v):5d} = {len(v) / ticks:6.2f} per tick  {k[:120]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--trace", action="store_true", help="ticks without changes on the closed and the open bridge, for a kernel trace")
    ap.add_argument("--summarise", metavar="DIR", help="per kernel of the kernel trace under DIR; nothing runs")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.ticks)

    import torch

    import mediastreamer2_amd as ms
    from bridge_probe import mulaw, synth

    if not torch.cuda.is_available():
        sys.exit("bridge_open_probe: no GPU; nothing is measured without one")
    PCM16, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMU
    TRUNK, WIDE, SUPER = (8000, PCMU, PCMU), (16000, PCM16, PCM16), (48000, PCM16, PCM16)
    has_open = hasattr(ms.Bridge, "change")
    ctx = ms.Context(0)
    n = NCONF * MM
    closed = ms.Bridge(ctx, n, members=MM, rate=CONF, ratios=[TRUNK] * n)
    bridges = {"closed": closed}
    if has_open:
        bridges["open"] = ms.Bridge(ctx, n, members=MM, rate=CONF, open=[TRUNK] * n, admit=[WIDE, SUPER])
    words = mulaw(synth(n, 80, 8000, 0x5EED))

    def fill(br, h_in):
        h_in.view(np.uint8).reshape(n, -1)[:, :80] = words

    def pump(br, ticks, before_submit=None):
        """`ticks` ticks with three in flight; before_submit(t) runs between acquire and submit"""
        for t in range(ticks):
            if br.in_flight() == 3:
                br.collect()
            fill(br, br.acquire()[0])
            if before_submit:
                before_submit(t)
            br.submit()

    def drain(br):
        while br.in_flight():
            br.collect()

    for br in bridges.values():
        pump(br, 10), drain(br)
    if a.trace:
        for br in bridges.values():
            pump(br, a.ticks), drain(br)
        for br in bridges.values():
            br.close()
        return ctx.close()

    def changes(streams, kind):
        ch = np.zeros((len(streams), 5), np.int32)
        ch[:, 0], ch[:, 1], ch[:, 2:] = streams, ms.MI_BRIDGE_JOIN, kind
        return ch

    out = dict(conferences=NCONF, members=MM, rate=CONF, reps=a.reps, change_members=has_open)
    stat = lambda v: dict(median=round(statistics.median(v) * 1e6, 1), spread=[round(min(v) * 1e6, 1), round(max(v) * 1e6, 1)])
    rng = np.random.default_rng(7)
    seats = rng.integers(0, n, a.reps)

    # ---- 1. the host cost of a leave + join of one seat, three ticks in flight
    def timed(br, op):
        t = []

        def one(i):
            t0 = time.perf_counter()
            op(br, int(seats[i]))
            t.append(time.perf_counter() - t0)
        pump(br, a.reps, one)
        drain(br)
        return t

    for name, br in bridges.items():
        out[f"pair_us_{name}"] = stat(timed(br, lambda b, s: (b.remove_member(s), b.add_member(s))))
    if has_open:
        L, br = ctx.L, bridges["open"]
        for name, b in bridges.items():
            out[f"change_us_{name}"] = stat(timed(b, lambda b, s: b.change(joins=[(s, TRUNK)])))
        out["two_calls_us_open"] = stat(timed(br, lambda b, s: (b.change(leaves=[s]), b.change(joins=[(s, WIDE)]))))
        both, bare = [], []
        for i in range(a.reps):
            if br.in_flight() == 3:
                br.collect()
            fill(br, br.acquire()[0])
            t0 = time.perf_counter()
            if i % 2 == 0:
                br.change(joins=[(int(seats[i]), TRUNK)])
            br.submit()
            (both if i % 2 == 0 else bare).append(time.perf_counter() - t0)
        drain(br)
        out["change_submit_us_open"], out["submit_us_open"] = stat(both), stat(bare)

        # ---- 2. the tick with k changes in it, by device events on the context's stream
        out["tick_ms"] = {}
        for k in (0, 1, 16, 256, n):
            ms_ = []
            for rep in range(15):
                drain(br)
                fill(br, br.acquire()[0])
                if k:
                    ch = changes(rng.permutation(n)[:k], WIDE if rep % 2 == 0 else TRUNK)
                    ms.check(L.mi_bridge_change_members(br.h, ch.ctypes.data, len(ch)))
                ctx.timer_start()
                br.submit()
                ms_.append(ctx.timer_stop())
            out["tick_ms"][str(k)] = dict(median=round(statistics.median(ms_), 4), spread=[round(min(ms_), 4), round(max(ms_), 4)])
        drain(br)
    print(json.dumps(out), flush=True)
    for br in bridges.values():
        br.close()
    ctx.close()


if __name__ == "__main__":
    main()
