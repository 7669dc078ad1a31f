"""CPU-side checks of mi_session_create_legs (include/msmi355x_session.h): the plan alone (csrc/session_plan.hpp through
tests/host/session_legs_plan_check.cpp, built here with AddressSanitizer + UBSan and run as a child process) -- every refusal
and its message, the pitches, the ratio bytes, the history lengths and strides, the LDS, "all one kind" as the uniform plan --;
the refusals through the library itself, which plans before it asks for a device; the new entry points declared in the header
and their symbols listed and exported; the header as plain C99; examples/mixed_rate_session.c built with -Werror and loud without a device; the Python
constructor; and, compile-only, the two new kernels' resources from the build's own remarks."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import kernel_remarks
import mediastreamer2_amd as ms
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "session_legs_plan_check.cpp")
NEW = ("mi_session_create_legs", "mi_session_leg_rate", "mi_session_leg_codec", "mi_session_leg_bytes")
PCM16, PCMA, PCMU = 0, 1, 2
# the GPU tests' first shape: 2 conferences x 5 members in a 48 kHz session
FIRST = ["8000:2:2", "8000:1:0", "16000:0:0", "24000:0:2", "48000:1:0", "48000:0:0", "8000:2:2", "16000:0:0", "24000:0:2", "8000:1:0"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("session_legs") / "session_legs_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(path)


def _plan(exe, rate, members, plc, legs):
    """-> (rc, the refusal's text) or (0, {field: value}) with the per-leg lists as lists of int"""
    r = subprocess.run([exe, str(rate), str(members), str(plc), *legs], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]  # a sanitizer's report ends the program and is its stderr
    rc, _, rest = r.stdout.strip().partition(" ")
    if int(rc) != 0:
        return int(rc), rest
    out = {}
    for kv in rest.split():
        k, v = kv.split("=")
        out[k] = [int(x) for x in v.split(",")] if "," in v else v
    return 0, out


# ---- the plan alone

@pytest.mark.parametrize("rate, plc, legs, words", [
    (48000, 0, ["8000:2:2", "96000:0:0"], ["leg 1", "96000 Hz", "48000 Hz", "above"]),
    (16000, 0, ["16000:0:0", "48000:0:0"], ["leg 1", "48000 Hz", "16000 Hz", "above"]),
    (48000, 0, ["8000:2:2", "16000:0:0", "12000:0:0"], ["leg 2", "12000 Hz", "48000 Hz", "ratio 4", "1, 2, 3, 6"]),
    (48000, 0, ["32000:0:0", "8000:2:2"], ["leg 0", "32000 Hz", "48000 Hz", "no whole ratio", "1.500"]),
    (48000, 0, ["8000:2:2", "18000:0:0"], ["leg 1", "18000 Hz", "48000 Hz", "no whole ratio"]),
    (48000, 0, ["8000:2:2", "44100:0:0"], ["leg 1", "44100 Hz", "48000 Hz", "no whole ratio"]),
    (16000, 0, ["8000:2:2", "4000:0:0"], ["leg 1", "4000 Hz", "16000 Hz", "ratio 4"]),
    (48000, 0, ["8000:3:2", "16000:0:0"], ["leg 0", "8000 Hz", "48000 Hz", "codec 3"]),
    (48000, 0, ["8000:2:2", "16000:0:-1"], ["leg 1", "16000 Hz", "48000 Hz", "codec -1"]),
    (192000, 0, ["32000:0:0", "192000:0:0"], ["192000 Hz", "ratio 6", "LDS"]),
])
def test_refusals_name_the_leg_both_rates_and_the_reason(exe, rate, plc, legs, words):
    rc, text = _plan(exe, rate, len(legs), plc, legs)
    assert rc == _lib.MI_ENOTSUP and "mi_session_create_legs" in text, text
    for w in words:
        assert w in text, (w, text)


def test_the_first_shape(exe):
    rc, p = _plan(exe, 48000, 5, 0, FIRST)
    assert rc == 0 and p["uniform"] == "0"
    assert p["tick_bytes"] == [960, 960]  # the widest PCM leg's tick: 480 samples of 16 bits, mic and out alike
    assert p["ratio"] == [6, 6, 3, 2, 1, 1, 6, 3, 2, 6]
    assert p["codec"] == [PCMU | PCMU << 2, PCMA, PCM16, PCMU << 2, PCMA, PCM16, PCMU | PCMU << 2, PCM16, PCMU << 2, PCMA]
    assert p["mic_bytes"] == [80, 80, 320, 480, 480, 960, 80, 320, 480, 80]
    assert p["out_bytes"] == [80, 160, 320, 240, 960, 960, 80, 320, 240, 160]
    # what a leg's resamplers keep: 47 samples in front of the canceller, ratio x 48 - 1 behind the mix (none at ratio 1)
    assert set(p["up_hist"]) == {47}
    assert p["down_hist"] == [287, 287, 143, 95, 0, 0, 287, 143, 95, 287]
    assert p["hist_stride"] == [48, 288]  # whole groups of eight: the pad slot, the widest ratio
    assert p["pcm_pitch"] == "480" and p["max_ratio"] == "6"
    ingress, egress = p["lds"]
    assert 0 < ingress <= 64 * 1024 and 0 < egress <= 64 * 1024
    row, scratch, down = p["wave"]  # a wavefront's share: the ingress' row and flat window, the egress' phase arrays and sums
    assert row == 960 and ingress == 4 * (row + scratch) and egress == 4 * down
    # at ratio 6 from 48 kHz the six phase arrays are under 4 KB per wavefront; with the 480 partial sums 5376 bytes
    assert down == 5376 and down - 480 * 4 < 4096


def test_pitches_follow_the_widest_leg_in_bytes(exe):
    assert _plan(exe, 48000, 2, 0, ["8000:2:2", "8000:1:1"])[1]["tick_bytes"] == [80, 80]  # every leg 8 kHz G.711
    assert _plan(exe, 48000, 2, 0, ["8000:2:0", "8000:1:1"])[1]["tick_bytes"] == [80, 160]
    assert _plan(exe, 48000, 2, 0, ["24000:2:2", "8000:0:0"])[1]["tick_bytes"] == [240, 240]
    assert _plan(exe, 48000, 3, 0, ["8000:2:2", "16000:1:2", "8000:0:2"])[1]["tick_bytes"] == [160, 160]
    rc, p = _plan(exe, 16000, 3, 1, ["8000:2:2", "8000:1:1", "16000:0:0"])  # the second shape, plc on
    assert rc == 0 and p["tick_bytes"] == [320, 320] and p["ratio"] == [2, 2, 1] and p["down_hist"] == [95, 95, 0]
    assert p["hist_stride"] == [48, 96] and p["pcm_pitch"] == "160"
    rc, p = _plan(exe, 48000, 2, 0, ["48000:1:0", "48000:0:0"])  # codecs alone differ: no resampler, no scratch
    assert rc == 0 and p["ratio"] == [1, 1] and p["lds"] == [4 * 960, 0]


def test_all_one_kind_is_the_uniform_plan(exe):
    rc, p = _plan(exe, 48000, 4, 0, ["16000:2:2"] * 8)
    assert rc == 0 and p == dict(uniform="1", in_rate="16000", out_rate="16000", mic_codec="2", out_codec="2", rate="48000")
    rc, p = _plan(exe, 48000, 2, 1, ["48000:0:0"] * 2)
    assert rc == 0 and p["uniform"] == "1" and p["in_rate"] == p["out_rate"] == "48000"
    assert _plan(exe, 48000, 2, 0, ["16000:2:2", "16000:2:1"])[1]["uniform"] == "0"


# ---- the library without a device

def _cfg(L, n, members, rate, plc=0):
    cfg = ms.SessionConfig()
    L.mi_session_default_config(C.byref(cfg))
    cfg.nstreams, cfg.members_per_conference, cfg.rate, cfg.tail_ms, cfg.plc = n, members, rate, 32, plc
    return cfg


def test_new_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "msmi355x_session.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    L = _lib.load()
    # the documented names are inline functions of the header over the library's symbols, which carry a prefix of their own:
    # every exported mi_session_* symbol belongs to one of the lists the older entry points were frozen with
    for name, symbol in zip(NEW, _lib.SESSION_LEG_EXPORTS):
        assert re.search(rf"\bstatic\s+inline\s+int\s+{name}\s*\([^)]*\)\s*\{{[^}}]*\b{symbol}\s*\(", code), f"{name} is not defined over {symbol}"
        assert re.search(rf"\bint\s+{symbol}\s*\([^)]*\)\s*;", code), f"{symbol} is not declared in msmi355x_session.h"
        assert symbol not in _lib.EXPORTS and symbol not in _lib.SESSION_EXPORTS and not symbol.startswith("mi_session_")
        assert re.search(rf"\sT {symbol}$", out, flags=re.M), f"{symbol} is not defined in the built library"
        assert not re.search(rf"\s{name}$", out, flags=re.M)
        assert getattr(L, symbol).argtypes
        assert name not in open(os.path.join(ROOT, "include", "msmi355x.h")).read()
    assert len(_lib.SESSION_LEG_EXPORTS) == len(NEW) == 4
    assert re.search(r"typedef\s+struct\s+mi_session_leg\s*\{\s*int32_t\s+rate\s*,\s*mic_codec\s*,\s*out_codec\s*;\s*\}\s*mi_session_leg\s*;", code)
    assert "mi_bridge has those" not in hdr and "a seat changing kind at a join" in hdr.lower()
    assert L.mi_abi_version() == 3


def test_the_library_refuses_before_it_asks_for_a_device():
    """the plan runs first: a refusal needs no context, and the concealer's own rule (plc.hip) is reached through it"""
    L = _lib.load()
    h = C.c_void_p()
    for rate, plc, legs, words in [(48000, 0, [(8000, 2, 2), (44100, 0, 0)], ["leg 1", "44100", "48000"]),
                                   (48000, 0, [(8000, 2, 2), (96000, 0, 0)], ["leg 1", "96000", "48000", "above"]),
                                   (24000, 1, [(24000, 0, 0), (4000, 0, 0)], ["leg 1", "4000", "24000", "concealer"])]:
        lg = np.ascontiguousarray(legs, np.int32)
        cfg = _cfg(L, len(legs), len(legs), rate, plc)
        assert L.mi_legs_session_create(None, C.byref(cfg), lg.ctypes.data, C.byref(h)) == _lib.MI_ENOTSUP
        text = L.mi_last_error().decode()
        assert "mi_session_create_legs" in text and all(w in text for w in words), text
    lg = np.ascontiguousarray([(8000, 2, 2), (16000, 0, 0)], np.int32)  # nothing to refuse: the missing context is what is wrong
    assert L.mi_legs_session_create(None, C.byref(_cfg(L, 2, 2, 48000)), lg.ctypes.data, C.byref(h)) == _lib.MI_EINVAL
    assert L.mi_legs_session_create(None, C.byref(_cfg(L, 2, 2, 48000)), None, C.byref(h)) == _lib.MI_EINVAL  # mi_session_create's


def test_null_session_is_einval():
    L = _lib.load()
    a, b = C.c_int32(-7), C.c_int32(-7)
    assert L.mi_legs_session_rate(None, 0) == _lib.MI_EINVAL
    assert L.mi_legs_session_codec(None, 0, C.byref(a), C.byref(b)) == _lib.MI_EINVAL
    assert L.mi_legs_session_bytes(None, 0, C.byref(a), C.byref(b)) == _lib.MI_EINVAL
    assert (a.value, b.value) == (-7, -7)


def _gpu_present():
    import torch
    return torch.cuda.is_available()


def test_the_python_constructor_is_loud_without_a_device():
    assert "legs" in inspect.signature(ms.Session.__init__).parameters
    if _gpu_present():
        pytest.skip("GPU present")
    with pytest.raises(ms.MiError) as e:
        ctx = ms.Context(0)
        ms.Session(ctx, 2, members=2, rate=48000, legs=[(8000, PCMU, PCMU), (16000, PCM16, PCM16)])
    assert e.value.code == _lib.MI_ENODEV


def test_the_header_is_plain_c99(tmp_path):
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_session.h"\n'
                     "int main(void) { mi_session *s = 0; int i = 0, o = 0; mi_session_config c;\n"
                     "  const mi_session_leg legs[2] = {{8000, MI_SESSION_PCMU, MI_SESSION_PCMA}, {16000, MI_SESSION_PCM16, MI_SESSION_PCM16}};\n"
                     "  mi_session_default_config(&c);\n"
                     "  return mi_session_create_legs(0, &c, legs, &s) == MI_OK || mi_session_leg_rate(s, 0) > 0 ||\n"
                     "         mi_session_leg_codec(s, 0, &i, &o) == MI_OK || mi_session_leg_bytes(s, 1, &i, &o) == MI_OK || i + o; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o",
                        str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_example_builds_and_is_loud_without_a_device(tmp_path):
    pkg, exe = os.path.join(ROOT, "mediastreamer2_amd"), tmp_path / "mixed_rate_session"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "mixed_rate_session.c"), "-L", pkg, "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if _gpu_present():  # (tests/test_gpu_session_legs.py runs it there)
        pytest.skip("GPU present")
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "no CPU fallback" in run.stderr and "ok" not in run.stdout.split(), (run.stdout, run.stderr)


# ---- the two kernels, compile-only

def test_the_two_kernels_use_no_scratch_and_no_lds_beyond_the_plan(exe):
    found = dict(kernel_remarks.kernels(kernel_remarks.remarks("session_legs.hip")))
    names = sorted(found)
    assert len(names) == 2 and "session_egress_kernel" in names[0] and "session_ingress_kernel" in names[1], names
    # the plan's dynamic LDS is all there is: a static array would come on top of it and past what it checked against 64 KB
    ingress, egress = _plan(exe, 48000, 5, 0, FIRST)[1]["lds"]
    for name, budget in zip(names, (egress, ingress)):
        u = found[name]
        assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
        assert int(u["LDS Size [bytes/block]"]) == 0 <= budget <= 64 * 1024, (name, u)
        print(name, {k: u[k] for k in ("VGPRs", "SGPRs", "Occupancy [waves/SIMD]") if k in u})
