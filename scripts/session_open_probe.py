#!/usr/bin/env python3
"""What membership changes cost on a session at a size a user runs: 1024 conferences x 32 legs, 16 kHz microphones into a
48 kHz chain, a 128 ms tail, AGC, the product's stagger, three ticks in flight.

    python scripts/session_open_probe.py [--reps 200] [--tree DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/session_open_probe.py --trace [--ticks 100]
    python scripts/session_open_probe.py --summarise <dir> [--ticks 100]

--tree: the checkout whose mediastreamer2_amd is loaded (default: this one).  Runs on a tree without
mi_session_change_members too (the figures that need it are left out), so that two builds can alternate in one job.  Figures,
one JSON line:
  pair_us           host time of replacing one seat through mi_session_remove_member + mi_session_add_member, the waiting pair,
                    with three ticks in flight: median and [min, max] of `reps`;
  change_us         the same through ONE mi_session_change_members call holding a JOIN on the taken seat (a replacement is
                    leave + join); two_calls_us: a LEAVE call and then a JOIN call; change_submit_us: the call and the submit
                    that carries it; submit_us: a submit that carries nothing, for comparison; pair_submit_us: the waiting pair
                    and the submit behind it;
  tick_ms[k]        HIP events on the context's stream around the submit of a tick that carries k replacements (k = 0, 1, 16,
                    256, nstreams), the pipe drained before: the wait for the tick's upload, the apply launch and the tick's
                    kernels; median of 11.
--trace: `ticks` ticks without a change, for a kernel trace of this command; --summarise: dispatches per tick and the median
duration per kernel of that trace."""
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
NCONF, MM = 1024, 32


def summarise(d, ticks):
    dur = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            dur.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if not dur:
        sys.exit(f"session_open_probe: no kernel trace under {d}")
    for k, v in sorted(dur.items(), key=lambda kv: -len(kv[1]) * statistics.median(kv[1])):
        print(f"{statistics.median(v):10.2f} us median  [{min(v):9.2f} .. {max(v):9.2f}]  x {len(v):5d} = {len(v) / ticks:6.2f} per tick  {k[:120]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose mediastreamer2_amd is loaded")
    ap.add_argument("--trace", action="store_true", help="ticks without changes, for a kernel trace")
    ap.add_argument("--summarise", metavar="DIR", help="per kernel of the kernel trace under DIR; nothing runs")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.ticks)
    sys.path.insert(0, os.path.abspath(a.tree))

    import torch

    import mediastreamer2_amd as ms

    if not torch.cuda.is_available():
        sys.exit("session_open_probe: no GPU; nothing is measured without one")
    has_open = hasattr(ms.Session, "change_members")
    ctx = ms.Context(0)
    n = NCONF * MM
    se = ms.Session(ctx, n, members=MM, in_rate=16000, rate=48000, tail_ms=128, agc=True, use_graphs=False, stagger=True)
    rng = np.random.default_rng(0x5EED)
    mic = rng.normal(0, 2500, (n, 160)).round().clip(-32767, 32767).astype(np.int16)
    ref = rng.normal(0, 3000, (n, 480)).round().clip(-32767, 32767).astype(np.int16)

    def fill():
        h_mic, h_ref = se.acquire()
        h_mic[:] = mic
        h_ref[:] = ref

    def pump(ticks, before_submit=None):
        """`ticks` ticks with three in flight; before_submit(t) runs between acquire and submit"""
        for t in range(ticks):
            if se.in_flight() == 3:
                se.collect()
            fill()
            if before_submit:
                before_submit(t)
            se.submit()

    def drain():
        while se.in_flight():
            se.collect()

    pump(12), drain()
    if a.trace:
        pump(a.ticks), drain()
        se.close()
        return ctx.close()

    out = dict(tree=os.path.relpath(os.path.abspath(a.tree), ROOT), conferences=NCONF, members=MM, rate=48000, tail_ms=128, reps=a.reps,
               change_members=has_open)
    stat = lambda v: dict(median=round(statistics.median(v) * 1e6, 1), spread=[round(min(v) * 1e6, 1), round(max(v) * 1e6, 1)])
    seats = rng.integers(0, n, a.reps)

    # ---- 1. the host cost of replacing one seat, three ticks in flight
    def timed(op, with_submit=False):
        t = []
        for i in range(a.reps):
            if se.in_flight() == 3:
                se.collect()
            fill()
            t0 = time.perf_counter()
            op(int(seats[i]))
            if with_submit:
                se.submit()
            t.append(time.perf_counter() - t0)
            if not with_submit:
                se.submit()
        drain()
        return t

    pair = lambda s: (se.remove_member(s), se.add_member(s))
    out["pair_us"] = stat(timed(pair))
    out["pair_submit_us"] = stat(timed(pair, True))
    out["submit_us"] = stat(timed(lambda s: None, True))
    if has_open:
        JOIN, LEAVE = ms.MI_SESSION_JOIN, ms.MI_SESSION_LEAVE
        out["change_us"] = stat(timed(lambda s: se.change_members([(s, JOIN)])))
        out["two_calls_us"] = stat(timed(lambda s: (se.change_members([(s, LEAVE)]), se.change_members([(s, JOIN)]))))
        out["change_submit_us"] = stat(timed(lambda s: se.change_members([(s, JOIN)]), True))

        # ---- 2. the tick with k replacements in it, by device events on the context's stream
        out["tick_ms"] = {}
        for k in (0, 1, 16, 256, n):
            ms_ = []
            for rep in range(11):
                drain()
                fill()
                if k:
                    ch = np.zeros((k, 2), np.int32)
                    ch[:, 0], ch[:, 1] = rng.permutation(n)[:k], JOIN
                    ms.check(ctx.L.mi_session_change_members(se.h, ch.ctypes.data, k))
                ctx.timer_start()
                se.submit()
                ms_.append(ctx.timer_stop())
            out["tick_ms"][str(k)] = dict(median=round(statistics.median(ms_), 4), spread=[round(min(ms_), 4), round(max(ms_), 4)])
        drain()
    print(json.dumps(out), flush=True)
    se.close()
    ctx.close()


if __name__ == "__main__":
    main()
