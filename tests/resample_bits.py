"""The batch resampler's output bits, case by case: what tests/golden/make_resample_bits.py records once and
tests/test_gpu_resample_bits.py recomputes.  The input is made with integer arithmetic alone, so it is the same
numbers on every machine and under every numpy."""
import hashlib

import numpy as np

TICKS = 3  # consecutive ticks per case: the history carries

# (in_rate, out_rate, in_len, nstreams, masked)
CASES = [(a, b, n, 8, False) for a, b, n in (
    # the triples of test_gpu_resample.py::test_resampler_matches_oracle
    (16000, 48000, 160), (8000, 48000, 80), (8000, 16000, 80), (48000, 16000, 480), (44100, 48000, 441),
    (16000, 8000, 160), (48000, 44100, 480), (48000, 8000, 480), (32000, 8000, 320), (48000, 24000, 480),
    (32000, 48000, 320), (48000, 32000, 480), (16000, 24000, 160), (12000, 8000, 120),
    (16000, 48000, 320),  # the up-sampler's form with several trips of lanes and two staging quads (3 x 40 lanes > 64)
    (48000, 24000, 640),  # the split kernel with more than one trip of lanes (2 x 40 > 64), 184 staging quads: still fast
)] + [
    # a wave walks more than one stream, every fifth masked out: the prefetch across streams, the masked-stream branch
    (16000, 48000, 160, 4100, True),
    (48000, 16000, 480, 4100, True),
]


def case_key(case):
    a, b, n, streams, masked = case
    return f"{a}_{b}_{n}_{streams}" + ("_masked" if masked else "")


def pcm(nstreams, n):
    """[nstreams][n] int16: full-scale noise, the top 16 bits of one 32-bit linear congruential generator per stream
    (Numerical Recipes' constants), and on stream 1 a slow +-32767 square, which drives the FIR's overshoot into
    WORD2INT's clamp"""
    state = (np.arange(nstreams, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
    x = np.empty((nstreams, n), np.int16)
    for k in range(n):
        state = (state * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)
        x[:, k] = (state >> np.uint64(16)).astype(np.uint16).view(np.int16)
    if nstreams > 1:
        x[1] = np.where((np.arange(n) // 37) % 2 == 0, 32767, -32767)
    return x


def run_mask(nstreams):
    m = np.ones(nstreams, np.uint8)
    m[4::5] = 0
    return m


def case_hashes(ms, torch, ctx, case):
    """one SHA-256 per tick over the whole zero-initialised output buffer (so a store past a row's end shows too) and out_len"""
    in_rate, out_rate, in_len, nstreams, masked = case
    rs = ms.ResamplerBatch(ctx, nstreams, in_rate, out_rate)
    x = torch.from_numpy(pcm(nstreams, in_len * TICKS)).cuda()
    run = torch.from_numpy(run_mask(nstreams)).cuda() if masked else None
    ostride = (rs.out_capacity(in_len) + 7) & ~7
    hashes = []
    for t in range(TICKS):
        xt = x[:, t * in_len:(t + 1) * in_len].contiguous()
        out = torch.zeros((nstreams, ostride), dtype=torch.int16, device="cuda")
        olen = torch.full((nstreams,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ms.check(ctx.L.mi_resampler_process_masked(rs.h, xt.data_ptr(), in_len, xt.stride(0), out.data_ptr(), out.stride(0), olen.data_ptr(),
                                                   run.data_ptr() if masked else None))
        ctx.sync()
        h = hashlib.sha256()
        h.update(np.ascontiguousarray(out.cpu().numpy()).tobytes())
        h.update(np.ascontiguousarray(olen.cpu().numpy()).tobytes())
        hashes.append(h.hexdigest())
    rs.close()
    return hashes
