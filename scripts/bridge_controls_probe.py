#!/usr/bin/env python3
"""What steering and observing a running bridge costs at a size a user runs: 1024 conferences x 32 legs of 8 kHz mu-law
(mi_bridge_create), three ticks in flight.  Writes profiles/bridge_controls.md (or --out).

    python scripts/bridge_controls_probe.py [--reps 200] [--ticks 600] [--out profiles/bridge_controls.md] [--tree DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/bridge_controls_probe.py --trace [--ticks 200]
    python scripts/bridge_controls_probe.py --summarise <dir> [--ticks 200]      (kernel names and counts of that trace)

Figures (the baselines are the waiting calls in the same process):
  1. host time per call, three ticks in flight, the C entry points called with arrays built beforehand: mi_bridge_set_controls
     (whole [nstreams] arrays, waits) against mi_bridge_change_controls of 1, 32 and 1024 seats (flags + gain each);
  2. host time per poll: mi_bridge_active_speakers + mi_bridge_get_levels (wait, copy every meter) against
     mi_bridge_collected_report (pointers into the block that came down with the tick);
  3. the tick's device time by HIP events on the context's stream around the submit, pipe drained before: reports off, speakers,
     speakers + levels;
  4. ticks per second sustained with a poll after every tick, both ways.
--trace: `ticks` ticks without a control change and with reports off, for a kernel trace of this command.
--tree: the checkout whose mediastreamer2_amd is loaded (default: this one), so that two builds can alternate in one job."""
import argparse
import csv
import ctypes as C
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

NCONF, MM = 1024, 32


def summarise(d, ticks):
    count = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            count[row["Kernel_Name"]] = count.get(row["Kernel_Name"], 0) + 1
    if not count:
        sys.exit(f"bridge_controls_probe: no kernel trace under {d}")
    for k, v in sorted(count.items(), key=lambda kv: -kv[1]):
        print(f"{v:6d} = {v / ticks:6.2f} per tick  {k[:120]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bridge_controls.md"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose mediastreamer2_amd is loaded")
    ap.add_argument("--trace", action="store_true", help="ticks without control changes, reports off, for a kernel trace")
    ap.add_argument("--summarise", metavar="DIR", help="kernel names and counts of the kernel trace under DIR; nothing runs")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.ticks)
    sys.path.insert(0, os.path.abspath(a.tree))

    import torch

    import mediastreamer2_amd as ms
    from bridge_probe import mulaw, synth
    from mediastreamer2_amd import _lib

    if not torch.cuda.is_available():
        sys.exit("bridge_controls_probe: no GPU; nothing is measured without one")
    ctx = ms.Context(0)
    L, n = ctx.L, NCONF * MM
    br = ms.Bridge(ctx, n, members=MM)
    words = mulaw(synth(n, 80, 8000, 0x5EED))

    def pump(ticks, before_submit=None, after_submit=None, on_collect=None):
        for t in range(ticks):
            if br.in_flight() == 3:
                br.collect()
                if on_collect:
                    on_collect()
            br.acquire()[0][:] = words
            if before_submit:
                before_submit(t)
            br.submit()
            if after_submit:
                after_submit()

    def drain():
        while br.in_flight():
            br.collect()

    pump(10), drain()
    if a.trace:
        pump(a.ticks), drain()
        br.close()
        return ctx.close()

    stat = lambda v, scale=1e6: (statistics.median(v) * scale, min(v) * scale, max(v) * scale)
    rng = np.random.default_rng(7)
    ON = ms.MI_MIX_LINKED | ms.MI_MIX_ACTIVE | ms.MI_MIX_OUTPUT
    flags, gain = np.full(n, ON, np.uint8), np.ones(n, np.float32)
    lines = []

    # ---- 1. host time per control call, three ticks in flight
    def timed(call):
        t = []

        def one(i):
            t0 = time.perf_counter()
            call(i)
            t.append(time.perf_counter() - t0)
        pump(a.reps, one)
        drain()
        return stat(t)

    def waiting(i):
        flags[int(rng.integers(n))] ^= ms.MI_MIX_ACTIVE
        ms.check(L.mi_bridge_set_controls(br.h, flags.ctypes.data, gain.ctypes.data))

    rows = [("`mi_bridge_set_controls` (flags + gains, whole arrays)", timed(waiting))]
    for k in (1, 32, 1024):
        arrs = []
        for _ in range(8):
            arr = (_lib.Control * k)()
            for c, s in zip(arr, rng.permutation(n)[:k]):
                c.stream, c.what, c.flags, c.gain = int(s), ms.MI_CTL_FLAGS | ms.MI_CTL_GAIN, int(rng.choice([2, 4, 6])), 1.0
            arrs.append(arr)
        rows.append((f"`mi_bridge_change_controls`, {k} seat{'s' if k > 1 else ''} in one call",
                     timed(lambda i, arrs=arrs, k=k: ms.check(L.mi_bridge_change_controls(br.h, arrs[i % 8], k)))))
    lines += ["## 1. Host time per control call, three ticks in flight (µs; median of %d, [min .. max])" % a.reps, "",
              "| call | median | spread |", "|---|---|---|"]
    lines += [f"| {name} | {m:.1f} | {lo:.1f} .. {hi:.1f} |" for name, (m, lo, hi) in rows]
    ms.check(L.mi_bridge_set_controls(br.h, np.full(n, ON, np.uint8).ctypes.data, gain.ctypes.data))

    # ---- 2. host time per poll
    win, db, lev = np.zeros(NCONF, np.int32), np.zeros(NCONF, np.float32), np.zeros(n, np.float32)
    rep = _lib.Report()
    t_wait, t_rep = [], []

    def poll_waiting():
        t0 = time.perf_counter()
        ms.check(L.mi_bridge_active_speakers(br.h, 0, win.ctypes.data, db.ctypes.data))
        ms.check(L.mi_bridge_get_levels(br.h, lev.ctypes.data))
        t_wait.append(time.perf_counter() - t0)

    def poll_report():
        t0 = time.perf_counter()
        ms.check(L.mi_bridge_collected_report(br.h, C.byref(rep)))
        t_rep.append(time.perf_counter() - t0)

    t0 = time.perf_counter()
    pump(a.ticks, after_submit=poll_waiting)
    drain()
    rate_wait = a.ticks / (time.perf_counter() - t0)
    br.set_reports(speakers=True, levels=True)
    pump(6), drain()
    t0 = time.perf_counter()
    pump(a.ticks + 3, on_collect=poll_report)
    rate_rep = a.ticks / (time.perf_counter() - t0)
    drain()
    t0 = time.perf_counter()
    br.set_reports()
    pump(a.ticks + 3)
    rate_none = a.ticks / (time.perf_counter() - t0)
    drain()
    lines += ["", "## 2. Host time per poll of every level and every conference's speaker (µs; median of %d, [min .. max])" % a.ticks, "",
              "| poll | median | spread |", "|---|---|---|"]
    for name, v in (("`mi_bridge_active_speakers` + `mi_bridge_get_levels` after every submit", t_wait),
                    ("`mi_bridge_collected_report` after every collect", t_rep)):
        m, lo, hi = stat(v)
        lines.append(f"| {name} | {m:.1f} | {lo:.1f} .. {hi:.1f} |")

    # ---- 3. the tick's device time
    lines += ["", "## 3. The tick on the device (HIP events on the context's stream around the submit, pipe drained before; ms, median of 25)", "",
              "| reports | median | spread |", "|---|---|---|"]
    for name, kw in (("off", {}), ("speakers", dict(speakers=True)), ("speakers + levels", dict(speakers=True, levels=True)), ("off again", {})):
        br.set_reports(**kw)
        pump(6), drain()
        v = []
        for _ in range(25):
            drain()
            br.acquire()[0][:] = words
            ctx.timer_start()
            br.submit()
            v.append(ctx.timer_stop())
        drain()
        lines.append(f"| {name} | {statistics.median(v):.4f} | {min(v):.4f} .. {max(v):.4f} |")
    br.set_reports()

    # ---- 4. sustained rate
    lines += ["", "## 4. Ticks per second sustained over %d ticks, three in flight, a poll for every tick" % a.ticks, "",
              "| poll | ticks / s |", "|---|---|",
              f"| `mi_bridge_active_speakers` + `mi_bridge_get_levels` after every submit | {rate_wait:.0f} |",
              f"| reports on, `mi_bridge_collected_report` after every collect | {rate_rep:.0f} |",
              f"| no poll, reports off | {rate_none:.0f} |"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    br.close()
    ctx.close()


if __name__ == "__main__":
    main()
