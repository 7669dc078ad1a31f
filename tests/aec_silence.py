"""Digital silence for the echo canceller's tests (helper module, not a test): the echo scene every canceller test uses,
the same scene with exact zeros on one or both pins for a span (a muted microphone, a held call, an empty conference),
and the bookkeeping that shows what those zeros do to the canceller's float32 state.

About a quarter of a second after both pins go quiet the whole error spectrum E of the library's canceller is
subnormal (the notch and pre-emphasis memories decay geometrically), and Davg1/2 and Dvar1/2 among the scalars
follow: the x86 float build the oracle restates keeps those words, so the kernels must too.  `PREMISE` holds the
conditions a scene has to meet for a bit-for-bit comparison through it to compare anything; the CPU test pins them on
the oracle alone and the GPU tests re-assert them on their own oracle runs."""
import numpy as np

TINY = np.finfo(np.float32).tiny  # the smallest normal float32

# (rate, F, tail_ms): the geometries the premise is pinned for
GEOMETRIES = [(8000, 64, 128), (16000, 128, 128), (48000, 256, 128), (48000, 512, 128),
              (16000, 128, 512),   # M = 64 blocks
              (96000, 512, 128)]
ONSETS = (6, 10)          # active frames before the zeros
SILENT_S = 1.5
BACK_FRAMES = 6
PREMISE = {"min_subnormal_frames": 100}   # (measured minimum: 121, at 48 kHz / 512)


def make_echo_scene(seed, rate, nsamp, near_sigma=300.0, far_sigma=3000.0):
    """mic = 0.5*ref through a fixed 64-tap decaying IR, 20 ms delay, + near-end noise."""
    rng = np.random.default_rng(0x5EED + seed)
    far = rng.normal(0, far_sigma, nsamp)
    far = np.convolve(far, [0.5, 0.3, 0.2])[:nsamp] + 3276.7 * np.sin(2 * np.pi * 1000 * np.arange(nsamp) / rate)
    ir = np.random.default_rng(1234).normal(0, 1, 64) * np.exp(-np.arange(64) / 12.0)
    ir /= np.sqrt((ir ** 2).sum())
    d = int(0.020 * rate)
    echo = 0.5 * np.convolve(np.concatenate([np.zeros(d), far]), ir)[:nsamp]
    mic = echo + rng.normal(0, near_sigma, nsamp)
    to16 = lambda v: np.clip(np.round(v), -32767, 32767).astype(np.int16)
    return to16(mic), to16(far)


def silent_frames(rate, F, silent_s):
    return int(round(silent_s * rate / F))


def silence_scene(seed, rate, F, active_frames, silent_s, back_frames, mode):
    """make_echo_scene(seed, ...) over active_frames + silent_s seconds + back_frames frames of F samples, with the pins
    `mode` names ("both", "mic", "far"; "none" leaves the scene as it is) set to exact 0 over the silent span.
    -> (mic, far, (first silent frame, first frame back))"""
    nsil = silent_frames(rate, F, silent_s)
    total = active_frames + nsil + back_frames
    mic, far = make_echo_scene(seed, rate, F * total)
    span = slice(active_frames * F, (active_frames + nsil) * F)
    if mode not in ("both", "mic", "far", "none"):
        raise ValueError(mode)
    if mode in ("both", "mic"):
        mic[span] = 0
    if mode in ("both", "far"):
        far[span] = 0
    return mic, far, (active_frames, active_frames + nsil)


def count_words(a):
    """(subnormal words, non-finite words) of a float32 state array"""
    a = np.asarray(a, np.float32)
    fin = np.isfinite(a)
    mag = np.abs(np.where(fin, a, 0))
    return int(((mag != 0) & (mag < TINY)).sum()), int((~fin).sum())


def state_list(F, M):
    """the state arrays test_mdf_bit_exact_before_adaptation compares, with their lengths"""
    N = 2 * F
    return (("W", M * N), ("foreground", M * N), ("X", (M + 1) * N), ("E", N), ("power", F + 1), ("power_1", F + 1),
            ("Eh", F + 1), ("Yh", F + 1), ("last_y", N), ("scalars", 16))


def blocks(rate, F, tail_ms):
    return (tail_ms * rate // 1000 + F - 1) // F


def oracle_run(oracle, rate, F, tail_ms, mic, far, postfilter=False, snapshots=()):
    """The oracle's canceller (+ post-filter) over a whole scene, frame by frame.
    -> {"out": int16 [frames * F], "sub": subnormal words in the whole state after each frame, "sub_E": ... in E,
        "nonfinite": non-finite state words after each frame, "adapted": scalars[8] after each frame,
        "snap": {frame: {array name: float32 copy}} for the frames in `snapshots`, "ec": the canceller}"""
    flen = tail_ms * rate // 1000
    M = blocks(rate, F, tail_ms)
    ec = oracle.Echo(F, flen, rate)
    pp = oracle.Preproc(F, rate, ec) if postfilter else None
    nfr = len(mic) // F
    out = np.zeros(nfr * F, np.int16)
    sub, sub_E, bad, adapted = (np.zeros(nfr, np.int64) for _ in range(4))
    snap = {}
    want = set(int(f) for f in snapshots)
    for f in range(nfr):
        sl = slice(f * F, (f + 1) * F)
        o = ec.cancel(mic[sl], far[sl])
        out[sl] = pp.run(o) if pp is not None else o
        st = {what: ec.get(what, n) for what, n in state_list(F, M)}
        for what, a in st.items():
            s_, b_ = count_words(a)
            sub[f] += s_
            bad[f] += b_
            if what == "E":
                sub_E[f] = s_
        adapted[f] = int(st["scalars"][8])
        if f in want:
            snap[f] = st
    return {"out": out, "sub": sub, "sub_E": sub_E, "nonfinite": bad, "adapted": adapted, "snap": snap, "ec": ec, "pp": pp}


def assert_premise(run, F, label=""):
    """The conditions that keep a bit-for-bit test through the zeros from comparing nothing (the caps of the table in
    DESIGN 3, "AEC through digital silence"): never adapted, at least 100 frames with a subnormal state word, a frame with
    more than F subnormal words in E, every state word finite."""
    assert not run["adapted"].any(), f"{label}: the oracle adapted at frame {int(np.argmax(run['adapted']))}: bit-exactness ends there"
    n = int((run["sub"] > 0).sum())
    assert n >= PREMISE["min_subnormal_frames"], f"{label}: only {n} frames hold a subnormal word"
    assert run["sub_E"].max() > F, f"{label}: E never holds more than {int(run['sub_E'].max())} subnormal words (F = {F})"
    assert not run["nonfinite"].any(), f"{label}: non-finite state at frame {int(np.argmax(run['nonfinite'] > 0))}"


def checkpoints(run, span, nframes):
    """the frames whose full state a test compares: the first frame of zeros, the oracle's first subnormal frame, the
    frame where its E holds the most subnormal words, the last silent frame, the last frame"""
    first_sub = int(np.argmax(run["sub"] > 0))
    return {"first_silent": span[0], "first_subnormal": first_sub, "most_subnormal_E": int(np.argmax(run["sub_E"])),
            "last_silent": span[1] - 1, "last": nframes - 1}
