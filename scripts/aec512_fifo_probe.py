"""Dev tool: the canceller's FIFO entry at 512-sample frames (aec_tick_kernel<512, TICK_FIFO>): 48 kHz legs fed 480-sample ticks,
post-filter on, the legs staggered as the plugin staggers them.  Prints one JSON line: us per launch (host clock around the
launch and a sync of the context's stream: an upper bound), algorithmic bytes per launch and the fraction of 8 TB/s.  Run it
under `rocprofv3 --kernel-trace --stats -f csv -- python ...` for the kernel's own time.   python scripts/aec512_fifo_probe.py [legs] [tail_ms] [ticks]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import mediastreamer2_amd as ms

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
tail_ms = int(sys.argv[2]) if len(sys.argv) > 2 else 250
nticks = int(sys.argv[3]) if len(sys.argv) > 3 else 64
rate, F, ns, warm = 48000, 512, 480, 16
flen = tail_ms * rate // 1000
M, N = (flen + F - 1) // F, 2 * F
ctx = ms.Context(0)
aec = ms.AecBatch(ctx, n, rate, frame_size=F, filter_length=flen)
fm, fr, fo = (ms.FifoBatch(ctx, n, 4 * F) for _ in range(3))
aec.stagger_fifos(fm, fr, ns)
rng = np.random.default_rng(5)
period = 16  # ticks of distinct input, cycled
mic = torch.from_numpy(rng.normal(0, 2500, (period, n, ns)).round().clip(-32767, 32767).astype(np.int16)).cuda()
ref = torch.from_numpy(rng.normal(0, 3000, (period, n, ns)).round().clip(-32767, 32767).astype(np.int16)).cuda()
out = torch.zeros((n, ns), dtype=torch.int16, device="cuda")
cnt = torch.zeros(n, dtype=torch.uint8, device="cuda")
frames, times = 0, []
for t in range(warm + nticks):
    torch.cuda.synchronize()
    ctx.sync()
    t0 = time.perf_counter()
    aec.process_fifos(fm, mic[t % period], fr, ref[t % period], fo, tick_len=ns, max_frames=2, count_out=cnt)
    ctx.sync()
    t1 = time.perf_counter()
    fo.pop(ns, out, zero_fill=True)
    ctx.sync()
    if t >= warm:
        times.append((t1 - t0) * 1e6)
        frames += int(cnt.sum().item())
# SURVEY 8(d)'s algorithmic bytes of a frame (the probe of the other sizes, scripts/aec_rate_probe.py, counts the same): microphone,
# far end and output samples + W read and written, foreground read, the X history and the newest block
per_frame = 3 * F * 2 + (3 * M * N + (M + 1) * N + N) * 4
us = float(np.median(times))
bytes_launch = frames / nticks * per_frame
print(json.dumps({"F": F, "rate": rate, "legs": n, "tail_ms": tail_ms, "M": M, "frames_per_leg_per_tick": round(frames / nticks / n, 4),
                  "us_per_launch_median": round(us, 1), "us_per_launch_min": round(min(times), 1),
                  "algorithmic_bytes_per_launch": int(bytes_launch), "algorithmic_TBps": round(bytes_launch / us / 1e6, 3),
                  "fraction_of_8TBps": round(bytes_launch / us / 1e6 / 8.0, 3),
                  "overflows": fm.overflows() + fr.overflows() + fo.overflows()}), flush=True)
