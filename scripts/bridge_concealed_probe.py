#!/usr/bin/env python3
"""A lossy tick of a gateway's conferences with a concealer per leg (mi_bridge_create_concealed: plc_list_kernel,
plc_legs_received_kernel, plc_legs_conceal_kernel, then the bridge's own kernel) against (a) the parts that would serve it
otherwise -- mi_g711_decode per law, one mi_plc_process per leg rate, the plc-less bridge fed the concealed PCM -- and (b)
today's uniform plc bridge (8 kHz mu-law legs: g711_decode_kernel, the three plc kernels, bridge_tick_kernel) at the same
leg count.

    python scripts/bridge_concealed_probe.py [--reps 9] [--ticks 100]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/bridge_concealed_probe.py --trace <subject>
    python scripts/bridge_concealed_probe.py --summarise <dir>

The shape: 1024 conferences x 32 legs in a 16 kHz mix, leg s by s % 6 an 8 kHz mu-law trunk, an 8 kHz A-law trunk with
mu-law out, a 16 kHz PCM member, a 48 kHz PCM member, an 8 kHz A-law trunk, a 16 kHz mu-law leg with PCM out; every tick
a seeded 5 % of the legs lose their packet.  <subject> is concealed, parts or uniform: one subject per trace, because the
parts and the uniform bridge launch kernels of the same names (plc_received_kernel, g711_decode_kernel) and the parts'
plc-less bridge runs the concealed bridge's own bridge_updown_kernel.  --summarise prints medians per kernel over a
trace's dispatches.  Without --trace: host-clock figures per tick, medians of `reps` windows of `ticks` ticks, three
ticks in flight, and HIP events around the parts' eleven launches in front of their bridge."""
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

NCONF, MM, CONF = 1024, 32, 16000
LOSS, NPATTERNS = 0.05, 8


def summarise(d):
    """medians per kernel over the dispatches of a rocprofv3 kernel trace (csv)"""
    dur = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            dur.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if not dur:
        sys.exit(f"bridge_concealed_probe: no kernel trace under {d}")
    rows = sorted(((k, len(v), statistics.median(v), min(v), max(v)) for k, v in dur.items()), key=lambda r: -r[1] * r[2])
    for k, n, med, lo, hi in rows:
        print(f"{med:10.2f} us median  [{lo:9.2f} .. {hi:9.2f}]  x {n:5d}  {k[:140]}")


def window(br, x, present, ticks):
    t0 = time.perf_counter()
    for t in range(ticks):
        if br.in_flight() == 3:
            br.collect()
        h_in, h_present = br.acquire()
        h_in[:] = x
        if present is not None:
            h_present[:] = present[t % len(present)]
        br.submit()
    while br.in_flight():
        br.collect()
    return (time.perf_counter() - t0) * 1e6 / ticks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--trace", choices=("concealed", "parts", "uniform"), help="short untimed windows of one subject, for a kernel trace")
    ap.add_argument("--summarise", metavar="DIR", help="medians per kernel of the kernel trace under DIR; nothing runs")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    import torch

    import mediastreamer2_amd as ms
    from bridge_probe import mulaw, synth
    if not torch.cuda.is_available():
        sys.exit("bridge_concealed_probe: no GPU; nothing is measured without one")
    U, A_, P = ms.MI_SESSION_PCMU, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCM16
    turn = [(8000, U, U), (8000, A_, U), (16000, P, P), (48000, P, P), (8000, A_, A_), (16000, U, P)]
    ctx = ms.Context(0)
    n = NCONF * MM
    legs = np.array([turn[s % 6] for s in range(n)], np.int32)
    rates, ic = legs[:, 0], legs[:, 1]
    ll = rates // 100
    width = int(ll.max())
    rng = np.random.default_rng(0x10557)
    present = (rng.random((NPATTERNS, n)) >= LOSS).astype(np.uint8)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    want = a.trace or "all"

    # the legs' rows: noise + tone at each leg's rate, in its own codec (the A-law rows through the library's own encoder)
    rows = np.zeros((n, 2 * width), np.uint8)
    for r in sorted(set(rates)):
        sel = rates == r
        pcm = synth(int(sel.sum()), r // 100, int(r), 0x5EED + int(r))
        for c in (U, A_, P):
            m = ic[sel] == c
            if not m.any():
                continue
            idx = np.nonzero(sel)[0][m]
            if c == P:
                rows[idx, :2 * (r // 100)] = pcm[m].view(np.uint8)
            elif c == U:
                rows[idx, :r // 100] = mulaw(pcm[m])
            else:
                d_pcm, d_out = dev(pcm[m]), torch.zeros((int(m.sum()), r // 100), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ms.g711_encode(ctx, ms.MI_LAW_PCMA, d_pcm, d_out)
                ctx.sync()
                rows[idx, :r // 100] = d_out.cpu().numpy()

    subjects = {}
    if want in ("all", "concealed"):
        br = ms.Bridge(ctx, n, members=MM, rate=CONF, concealed=legs, plc=True)
        x = rows[:, :br.tick_bytes()[0]]
        subjects["concealed"] = (br, lambda ticks, br=br, x=x: window(br, x, present, ticks))
    if want in ("all", "uniform"):
        ub = ms.Bridge(ctx, n, members=MM, rate=8000, in_codec=U, out_codec=U, plc=True)
        ux = mulaw(synth(n, 80, 8000, 0x5EED))
        subjects["uniform"] = (ub, lambda ticks, ub=ub, ux=ux: window(ub, ux, present, ticks))
    front = None
    if want in ("all", "parts"):
        inner = ms.Bridge(ctx, n, members=MM, rate=CONF, endpoints=[(r, P, oc) for r, _, oc in legs])
        plcs = {int(r): ms.PlcBatch(ctx, n, int(r), max_block=width) for r in sorted(set(rates))}
        d_rows, d_pcm = dev(rows), torch.zeros((n, width), dtype=torch.int16, device="cuda")
        d_pcm[dev(ic == P)] = dev(rows[ic == P].view(np.int16))
        law_lens = {law: dev(np.where(ic == c, ll, 0).astype(np.int32)) for law, c in ((ms.MI_LAW_PCMU, U), (ms.MI_LAW_PCMA, A_))}
        lens = dev(ll.astype(np.int32))
        modes = {r: [dev(np.where(rates == r, np.where(p, ms.MI_PLC_RECEIVED, ms.MI_PLC_CONCEAL), 0).astype(np.uint8)) for p in present]
                 for r in plcs}
        inner_x = np.zeros((n, inner.tick_bytes()[0]), np.uint8)
        torch.cuda.synchronize()

        def front(t):  # the eleven launches in front of the plc-less bridge (a PCM leg's row lies decoded in the buffer)
            for law, lz in law_lens.items():
                ms.g711_decode(ctx, law, d_rows, d_pcm, length=width, lens=lz)
            for r, plc in plcs.items():
                plc.process(d_pcm, lens, modes[r][t % NPATTERNS])

        def parts_window(ticks):  # the launches, and the plc-less bridge's tick beside them (no hand-over of the PCM: timing only)
            for t in range(ticks):
                front(t)
            ctx.sync()
            return window(inner, inner_x, None, ticks)
        subjects["parts"] = (inner, parts_window)

    for _, run in subjects.values():  # warm every shape
        run(5)
    if a.trace:
        subjects[a.trace][1](30)
    else:
        t = {f"{k}_e2e_us": [] for k in subjects if k != "parts"}
        t["plcless_bridge_e2e_us"], t["parts_front_dev_us"] = [], []
        for _ in range(a.reps):
            for k, (_, run) in subjects.items():
                if k != "parts":
                    t[f"{k}_e2e_us"].append(run(a.ticks))
            t["plcless_bridge_e2e_us"].append(window(subjects["parts"][0], inner_x, None, a.ticks))
            ctx.timer_start()
            for i in range(a.ticks):
                front(i)
            t["parts_front_dev_us"].append(ctx.timer_stop() * 1e3 / a.ticks)
        print(json.dumps(dict(conferences=NCONF, members=MM, mix_rate=CONF, loss=LOSS, reps=a.reps, ticks=a.ticks,
                              **{k: round(statistics.median(v), 2) for k, v in t.items()},
                              spread={k: [round(min(v), 2), round(max(v), 2)] for k, v in t.items()})), flush=True)
    for br, _ in subjects.values():
        br.close()
    if front is not None:
        for p in plcs.values():
            p.close()
    ctx.close()


if __name__ == "__main__":
    main()
