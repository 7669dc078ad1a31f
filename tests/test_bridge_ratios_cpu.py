"""CPU-side checks of the bridge's legs at 4, 1/4 and a : b of the mix's rate (mi_bridge_create_ratios): the entry point is
declared, listed and exported; the header is still plain C99; examples/mixed_rate_room.c builds against the library alone;
what creation plans and refuses under the new rules (csrc/bridge_plan.hpp run alone: tests/host/bridge_ratios_plan_check.cpp,
built here with AddressSanitizer + UBSan and run as a child process, as tests/test_bridge_plan_cpu.py does); and, compile-only,
the one kernel of csrc/bridge_ratios.hip spills nothing, uses no scratch memory and keeps its static LDS inside what creation
budgets."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kernel_remarks
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "bridge_ratios_plan_check.cpp")
NEW = "mi_bridge_create_ratios"
PCM16, PCMA, PCMU = 0, 1, 2  # MI_SESSION_* (include/msmi355x.h)
MI_EINVAL, MI_ENOTSUP = -1, -4
P16, ULAW, ALAW = (PCM16, PCM16), (PCMU, PCMU), (PCMA, PCMA)


def test_entry_point_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "msmi355x_bridge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(rf"\bint\s+{NEW}\s*\(\s*mi_ctx\s*\*\s*\w+\s*,\s*const\s+mi_bridge_config\s*\*\s*\w+\s*,\s*const\s+mi_bridge_leg\s*\*\s*\w+\s*,"
                     rf"\s*mi_bridge\s*\*\*\s*\w+\s*\)\s*;", code), f"{NEW} is not declared in msmi355x_bridge.h with mi_bridge_create_legs' arguments"
    assert NEW in _lib.BRIDGE_EXPORTS
    assert re.search(rf"\sT {NEW}$", out, flags=re.M), f"{NEW} is not defined in the built library"
    L = _lib.load()
    assert getattr(L, NEW).argtypes == L.mi_bridge_create_legs.argtypes
    assert L.mi_abi_version() == 3


def test_bad_arguments_are_einval_without_a_device():
    L = _lib.load()
    h = C.c_void_p(0x1)
    assert getattr(L, NEW)(None, None, None, C.byref(h)) == _lib.MI_EINVAL
    legs = (C.c_int32 * 3)(12000, 0, 0)
    assert getattr(L, NEW)(None, None, legs, C.byref(h)) == _lib.MI_EINVAL


def test_header_is_still_plain_c99(tmp_path):
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_bridge.h"\n'
                     "int main(void) { mi_bridge *b = 0; int i = 0, o = 0; mi_bridge_config c;\n"
                     "  const mi_bridge_leg legs[2] = {{8000, MI_SESSION_PCMU, MI_SESSION_PCMA}, {12000, MI_SESSION_PCM16, MI_SESSION_PCM16}};\n"
                     "  mi_bridge_default_config(&c);\n"
                     "  c.rate = 16000;\n"
                     "  return mi_bridge_create_ratios(0, &c, legs, &b) == MI_OK || mi_bridge_leg_bytes(b, 1, &i, &o) == MI_OK ||\n"
                     "         mi_bridge_leg_rate(b, 1) == 12000 || i + o; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o",
                        str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_mixed_rate_room_example_builds(tmp_path):
    """examples/mixed_rate_room.c builds as C99 against libmsmi355x.so alone, the way superwideband_room.c does"""
    pkg = os.path.join(ROOT, "mediastreamer2_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "mixed_rate_room.c"), "-L", pkg, "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o",
                        str(tmp_path / "mixed_rate_room")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the plan alone

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("bridge_ratios_plan") / "bridge_ratios_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(path)


def _child(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]  # a sanitizer's report ends the program and is its stderr
    return r.stdout.strip()


@pytest.fixture(scope="module")
def plan(exe):
    def run(rules, conf, members, legs, plc=False):
        """-> (return code, the error text or {name: value} of the plan)"""
        code, _, rest = _child(exe, rules, conf, members, int(plc), *[f"{a}:{b}:{c}" for a, b, c in legs]).partition(" ")
        return int(code), (rest if int(code) else dict(kv.split("=") for kv in rest.split()))
    return run


# tests/test_gpu_bridge_ratios.py's conferences of five: (conference rate, members, tick_bytes, the five ratio bytes).  A byte:
# the whole ratio, | 0x80 above the mix, | 0x40 at 3/2; a : b is 0x20 | (a - 1) | (b - 1) & 3 << 3 | (b - 1) & 4 << 4, | 0x80 above
SHAPES = {
    "a": (16000, [(12000, *P16), (8000, *ULAW), (16000, *P16), (32000, *P16), (12000, *P16)], (640, 640), "3a,02,01,82,3a"),
    "b": (12000, [(16000, *P16), (32000, *P16), (12000, *P16), (8000, *ULAW), (32000, *P16)], (640, 640), "b3,b7,01,41,b7"),
    "c": (8000, [(32000, *P16), (8000, *ULAW), (32000, PCMU, PCM16), (8000, *P16), (32000, *P16)], (640, 640), "84,01,84,01,84"),
    "d": (48000, [(12000, *P16), (32000, *P16), (48000, *P16), (8000, *ALAW), (12000, *P16)], (960, 960), "04,41,01,06,04"),
    "e": (32000, [(24000, *P16), (40000, *P16), (8000, *ULAW), (32000, *P16), (24000, *P16)], (800, 800), "3a,bc,04,01,3a"),
    "f-up": (2400, [(3200, *P16), (2400, *P16), (3200, *P16), (2400, *P16), (3200, *P16)], (64, 64), "b3,01,b3,01,b3"),
    "f-down": (3200, [(2400, *P16), (3200, *P16), (2400, *P16), (3200, *P16), (2400, *P16)], (64, 64), "3a,01,3a,01,3a"),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_family_and_tick_bytes_of_the_gpu_shapes(plan, case):
    conf, legs, tick_bytes, ratio_bytes = SHAPES[case]
    code, p = plan("ratios", conf, 5, legs * 2)
    assert code == 0 and p["family"] == "RATIOS", p
    assert tuple(int(v) for v in p["tick_bytes"].split(",")) == tick_bytes and p["bytes"] == ",".join([ratio_bytes] * 2), p
    assert int(p["lds"]) + kernel_remarks.bridge_budget()[0] <= 64 * 1024
    # samples per member of either history: the longest filter of the conference, as mi_resampler strides it -- (a) ratio 2's
    # 2 * 48 over 4 : 3's 64, (b) 8 : 3's 128, (c) (e) ratio 4's 192, (d) ratio 6's 288, (f) 4 : 3's 64
    stride = {"a": 96, "b": 128, "c": 192, "d": 288, "e": 192, "f-up": 64, "f-down": 64}[case]
    assert p["hist"] == f"{stride},{stride}", p


def test_no_such_leg_plans_the_rational_bridge(plan):
    """without a leg of the new kinds: mi_bridge_create_rational's plan, field for field"""
    for conf, legs in [(16000, [(8000, *ULAW), (24000, *P16), (16000, *P16), (48000, *P16)] * 2), (8000, [(8000, *ULAW)] * 8),
                       (16000, [(8000, *ULAW), (16000, *P16)] * 4)]:
        for plc in (False, True):
            old, new = plan("rational", conf, 4, legs, plc), plan("ratios", conf, 4, legs, plc)
            assert old[0] == 0 and new[0] == 0
            assert new[1].pop("generic") == "0" and old[1].pop("generic") == "0"
            assert new[1] == old[1] and new[1]["family"] != "RATIOS"


ok8, ok24 = [(8000, *ULAW)] * 6, [(24000, *P16)] * 6
at = lambda rate, n, pair=P16: [(rate, *pair)] * n
REFUSALS = [  # (what the text must contain, rules, conference rate, members, legs, plc)
    # off the 800 grid
    (["mi_bridge_create_ratios", "leg 5 at 44100 Hz in a 8000 Hz", "441 : 80"], "ratios", 8000, 3, ok8[:5] + at(44100, 1), False),
    (["leg 4's rate 1000"], "ratios", 800, 3, at(800, 4) + at(1000, 2), False),  # 5 : 4, but no whole groups of eight
    (["leg 4's rate 4400"], "ratios", 8800, 3, at(8800, 4) + at(4400, 2), False),
    (["rate 11025"], "ratios", 11025, 3, at(11025, 6), False),
    # whole ratios 5, 7, 8 and up
    (["leg 5 at 40000 Hz in a 8000 Hz", "ratio 5"], "ratios", 8000, 3, ok8[:5] + at(40000, 1), False),
    (["leg 5 at 8000 Hz in a 56000 Hz", "ratio 7"], "ratios", 56000, 3, at(56000, 5) + at(8000, 1, ULAW), False),
    (["leg 5 at 64000 Hz in a 8000 Hz", "ratio 8"], "ratios", 8000, 3, ok8[:5] + at(64000, 1), False),
    (["leg 5 at 96000 Hz in a 8000 Hz", "ratio 12"], "ratios", 8000, 3, ok8[:5] + at(96000, 1), False),
    # a : b beyond the rule
    (["leg 5 at 28000 Hz in a 8000 Hz", "7 : 2", "168 taps"], "ratios", 8000, 3, ok8[:5] + at(28000, 1), False),
    (["leg 5 at 8000 Hz in a 28000 Hz", "2 : 7", "168"], "ratios", 28000, 3, at(28000, 5) + at(8000, 1, ULAW), False),
    (["leg 2 at 14400 Hz in a 12800 Hz", "9 : 8", "interpolated"], "ratios", 12800, 3, at(12800, 2) + at(14400, 1) + at(12800, 3), False),
    (["leg 0 at 35200 Hz in a 12800 Hz", "11 : 4"], "ratios", 12800, 3, at(35200, 1) + at(12800, 5), False),
    # whatever mi_bridge_create_rational refuses otherwise
    (["leg 5 names codec 3"], "ratios", 16000, 3, at(16000, 5) + [(12000, PCMU, 3)], False),
    (["LDS", "46 members x 480 samples", "a : b"], "ratios", 16000, 46, ([(12000, *P16), (48000, *P16)] * 23), False),
    # the older rules keep their refusals
    (["mi_bridge_create_rational", "leg 5 at 32000", "ratio 4"], "rational", 8000, 3, ok8[:5] + at(32000, 1), False),
    (["mi_bridge_create_rational", "leg 4 at 32000", "1.333"], "rational", 24000, 3, ok24[:4] + at(32000, 2), False),
    (["leg 3 at 12000", "2.667"], "rational", 32000, 3, at(32000, 3) + at(12000, 3), False),
]


@pytest.mark.parametrize("values,rules,conf,members,legs,plc", REFUSALS, ids=[f"{r[1]}-{r[0][-1]}" for r in REFUSALS])
def test_refusals(plan, values, rules, conf, members, legs, plc):
    code, text = plan(rules, conf, members, legs, plc)
    assert code == MI_ENOTSUP, text
    for v in values:
        assert str(v) in text, text


def test_member_caps_of_the_header(plan):
    """include/msmi355x_bridge.h: 12 kHz legs in a 16 kHz room that also holds 48 kHz members, up to 45: the cap is planned, one
    more is refused for its LDS; 32 kHz legs in a 24 kHz conference fit at the mixer's own 50 members with 42 640 bytes, and 51
    are refused as the mixer refuses them"""
    static, limit = kernel_remarks.bridge_budget()[:2]
    room = [(12000, *P16), (48000, *P16)]
    code, p = plan("ratios", 16000, 45, (room * 45)[:45])
    assert code == 0 and p["family"] == "RATIOS" and int(p["lds"]) + static <= limit, p
    code, text = plan("ratios", 16000, 46, (room * 46)[:46])
    assert code == MI_ENOTSUP and "LDS" in text and "46 members x 480 samples" in text, text
    code, p = plan("ratios", 24000, 50, at(32000, 50))
    assert code == 0 and p["family"] == "RATIOS" and int(p["lds"]) == 42640, p
    assert plan("ratios", 24000, 51, at(32000, 51))[0] == MI_EINVAL
    hdr = open(os.path.join(ROOT, "include", "msmi355x_bridge.h")).read()
    assert "up to 45 members" in hdr and "42 640 bytes" in hdr


def test_the_filter_rule_is_the_one_the_issue_derives(exe):
    """filter_rule restates design_filter (csrc/resample.hip): a non-whole a : b has both tables direct with at most 128 taps
    exactly where max(a, b) <= 8 and max / min <= 8/3 (tests/test_gpu_bridge_ratios.py holds the same rule to
    mi_resampler_info); the lengths of the ratios the GPU tests run"""
    from math import gcd
    rule = lambda num, den: tuple(int(v) for v in _child(exe, "rule", num, den).split())
    for a in range(1, 13):
        for b in range(1, 13):
            if gcd(a, b) != 1 or min(a, b) == 1:
                continue
            (fi, di), (fo, do) = rule(a, b), rule(b, a)
            served = bool(di and do and fi <= 128 and fo <= 128)
            assert served == (max(a, b) <= 8 and 3 * max(a, b) <= 8 * min(a, b)), (a, b, fi, di, fo, do)
    assert rule(4, 3) == (64, 1) and rule(3, 4) == (48, 1) and rule(8, 3) == (128, 1) and rule(3, 8) == (48, 1)
    assert rule(5, 4) == (64, 1) and rule(7, 2) == (168, 1) and rule(9, 8) == (56, 1) and rule(8, 9) == (48, 0) and rule(4, 1) == (192, 1)


# ---- the kernel, compile-only

@pytest.fixture(scope="module")
def remarks():
    return kernel_remarks.remarks("bridge_ratios.hip")


def test_one_kernel_that_spills_nothing_and_fits_the_lds_budget(remarks):
    """mi_bridge_create_ratios accepts a shape when its dynamic LDS + RATED_STATIC_LDS <= 64 KB, so the kernel's static LDS must
    stay inside that constant"""
    budget, _, src = kernel_remarks.bridge_budget()
    assert "lds + RATED_STATIC_LDS > BRIDGE_LDS_MAX" in src
    found = kernel_remarks.kernels(remarks)
    assert len(found) == 1, [n for n, _ in found]
    name, u = found[0]
    assert "bridge_ratios_kernel" in name, name
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
    assert int(u["LDS Size [bytes/block]"]) <= budget, u
    print(name, {k: u[k] for k in ("VGPRs", "SGPRs", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]") if k in u})
