"""GPU parity: mi_scaler_* vs the oracle's integer restatement (libyuv C-path
bilinear in 16.16 + in-tree Q13 BT.601).  All integer: BIT-EXACT."""
import numpy as np
import pytest

import mediastreamer2_amd as ms

pytestmark = pytest.mark.gpu


def synth_i420(seed, w, h):
    """gradient + noise luma, low-frequency chroma ramps."""
    rng = np.random.default_rng(0x5EED + seed)
    h2 = h + (h & 1)
    yy, xx = np.mgrid[0:h2, 0:w]
    y = (16 + 200 * (xx + yy) / (w + h2) + rng.normal(0, 12, (h2, w))).clip(0, 255).astype(np.uint8)
    cy, cx = np.mgrid[0:h2 // 2, 0:w // 2]
    u = (128 + 100 * np.sin(2 * np.pi * cx / max(w // 2, 1) + seed)).clip(0, 255).astype(np.uint8)
    v = (128 + 100 * np.cos(2 * np.pi * cy / max(h2 // 2, 1) + seed)).clip(0, 255).astype(np.uint8)
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


SIZES = [
    (1920, 1080, 1280, 720),   # BASELINE config 5
    (640, 480, 320, 240),      # exact 2x
    (352, 288, 176, 144),
    (1280, 720, 640, 360),
    (320, 240, 426, 320),      # up-scale
    (176, 144, 352, 288),
    (642, 362, 318, 182),      # sizes that are not multiples of 16/4
    (64, 64, 64, 64),          # identity
    (3840, 2160, 1920, 1080),  # 4K source: the widest rows the strip kernel stages
    (3840, 2160, 1280, 720),   # 3x down: source span per 256-pixel strip beyond the fast path -> generic kernel
    (16, 16, 2, 2),            # smallest output
    (1280, 720, 1920, 1080),   # 1.5x up
]


@pytest.mark.parametrize("sw,sh,dw,dh", SIZES)
def test_scale_to_rgb24_bit_exact(ctx, oracle, sw, sh, dw, dh):
    sc = ms.ScalerBatch(ctx, sw, sh, dw, dh, ms.MI_PIX_RGB24)
    assert sc.src_bytes == oracle.i420_size(sw, sh)
    nf = 3 if sw >= 1280 else 5
    src = np.stack([synth_i420(i, sw, sh) for i in range(nf)])
    if nf > 2:
        src[1][:] = 0
        src[2][:] = 255   # extremes: clamp paths of the colour stage
    got = sc.process(src)
    for i in range(nf):
        ref = oracle.i420_scale_to_rgb24(src[i], sw, sh, dw, dh)
        np.testing.assert_array_equal(got[i].reshape(dh, dw, 3), ref, err_msg=f"frame {i}")
    sc.close()


@pytest.mark.parametrize("sw,sh,dw,dh", SIZES)
def test_scale_to_i420_bit_exact(ctx, oracle, sw, sh, dw, dh):
    """MSSizeConv's actual output format (sizeconv.c:133-181)."""
    sc = ms.ScalerBatch(ctx, sw, sh, dw, dh, ms.MI_PIX_I420)
    assert sc.dst_bytes == oracle.i420_size(dw, dh)
    src = np.stack([synth_i420(10 + i, sw, sh) for i in range(2)])
    got = sc.process(src)
    for i in range(2):
        np.testing.assert_array_equal(got[i], oracle.i420_scale(src[i], sw, sh, dw, dh), err_msg=f"frame {i}")
    sc.close()


def test_colour_stage_known_answers(ctx, oracle):
    """BT.601 limited range anchors: (16,128,128)->black, (235,128,128)->white, primaries."""
    sw = sh = 16
    sc = ms.ScalerBatch(ctx, sw, sh, sw, sh, ms.MI_PIX_RGB24)
    cases = {(16, 128, 128): (0, 0, 0), (235, 128, 128): (255, 255, 255), (81, 90, 240): (255, 0, 0),
             (145, 54, 34): (0, 255, 0), (41, 240, 110): (0, 0, 255)}
    for (y, u, v), rgb in cases.items():
        f = np.concatenate([np.full(sw * sh, y, np.uint8), np.full(sw * sh // 4, u, np.uint8),
                            np.full(sw * sh // 4, v, np.uint8)])[None]
        got = sc.process(f)[0].reshape(sh, sw, 3)
        assert np.abs(got.astype(int) - np.array(rgb)).max() <= 1, ((y, u, v), got[0, 0])
        np.testing.assert_array_equal(got, oracle.i420_scale_to_rgb24(f[0], sw, sh, sw, sh))
    sc.close()


def test_full_size_batch_device_resident(ctx, oracle):
    """A 16-frame 1080p batch on the device path; frames with equal content give equal bytes,
    constant frames stay constant (scaling a flat picture is the identity on values)."""
    torch = pytest.importorskip("torch")
    sw, sh, dw, dh = 1920, 1080, 1280, 720
    sc = ms.ScalerBatch(ctx, sw, sh, dw, dh, ms.MI_PIX_RGB24)
    frames = [synth_i420(i % 4, sw, sh) for i in range(16)]
    frames[5] = np.concatenate([np.full(sw * sh, 120, np.uint8), np.full(sw * sh // 4, 90, np.uint8),
                                np.full(sw * sh // 4, 200, np.uint8)])
    d = torch.from_numpy(np.stack(frames)).cuda()
    o = sc.process(d)
    ctx.sync()
    torch.cuda.synchronize()
    out = o.cpu().numpy()
    for i in (4, 8, 12):
        np.testing.assert_array_equal(out[i], out[0])
    px = out[5].reshape(dh, dw, 3)
    assert (px == px[0, 0]).all()
    np.testing.assert_array_equal(out[1].reshape(dh, dw, 3), oracle.i420_scale_to_rgb24(frames[1], sw, sh, dw, dh))
    sc.close()


def test_the_pipelined_scaler_equals_the_synchronous_one(ctx):
    """mi_scaler_pipe (host frames in, host frames out; upload | kernel | download on three streams, several batches in
    flight -- the host path of BASELINE config 5) delivers exactly what mi_scaler_process_host does, batch after batch, with
    partial batches, and refuses a batch beyond its depth until the oldest has been collected."""
    rng = np.random.default_rng(5)
    w, h, dw, dh = 640, 360, 320, 180
    sc = ms.ScalerBatch(ctx, w, h, dw, dh, ms.MI_PIX_RGB24)
    pipe = ms.ScalerPipe(sc, 6, depth=3)
    frames = rng.integers(0, 256, (40, sc.src_bytes), dtype=np.uint8)
    want = sc.process(frames)
    got, sent, sizes = [], 0, [6, 6, 3, 6, 1, 6, 6, 6]
    pending = []
    for n in sizes:
        if pipe.in_flight() == 3:
            with pytest.raises(ms.MiError):
                pipe.acquire()
            got.append(pipe.collect()[:, :sc.dst_bytes].copy())
            pending.pop(0)
        buf = pipe.acquire()
        buf[:n, :sc.src_bytes] = frames[sent:sent + n]
        pipe.submit(n)
        pending.append(n)
        sent += n
    while pipe.in_flight():
        got.append(pipe.collect()[:, :sc.dst_bytes].copy())
    got = np.concatenate(got)
    assert sent == 40 and got.shape[0] == 40
    np.testing.assert_array_equal(got, want)
    pipe.close()
    sc.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_the_scaler_pipe_reuses_its_slots(ctx, depth):
    """mi_scaler_pipe at depth 1 (every submit reuses the one slot) and 2: five batches of up to two 16x16 -> 8x8 frames,
    the last of one frame, come out bit-equal to mi_scaler_process_host with the right frame count per batch; submit
    without acquire, collect with nothing in flight and an acquire beyond the depth raise MiError and leave in_flight()
    where it was."""
    rng = np.random.default_rng(17)
    sc = ms.ScalerBatch(ctx, 16, 16, 8, 8, ms.MI_PIX_RGB24)
    pipe = ms.ScalerPipe(sc, 2, depth=depth)
    sizes = [2, 2, 2, 2, 1]
    frames = rng.integers(0, 256, (sum(sizes), sc.src_bytes), dtype=np.uint8)
    want = sc.process(frames)

    def refused(call):
        held = pipe.in_flight()
        with pytest.raises(ms.MiError):
            call()
        assert pipe.in_flight() == held

    refused(lambda: pipe.submit(1))
    refused(pipe.collect)
    got, sent = [], 0
    for n in sizes:
        if pipe.in_flight() == depth:
            refused(pipe.acquire)
            refused(lambda: pipe.submit(1))
            got.append(pipe.collect()[:, :sc.dst_bytes].copy())
        buf = pipe.acquire()
        buf[:n, :sc.src_bytes] = frames[sent:sent + n]
        pipe.submit(n)
        sent += n
    while pipe.in_flight():
        got.append(pipe.collect()[:, :sc.dst_bytes].copy())
    refused(pipe.collect)
    assert [g.shape[0] for g in got] == sizes
    np.testing.assert_array_equal(np.concatenate(got), want)
    pipe.close()
    sc.close()
