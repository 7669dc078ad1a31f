"""CPU-side checks of bridge seats that change hands (mi_bridge_create_open, mi_bridge_change_members): both entry points are
declared, listed and exported; the header is still plain C99; examples/churning_bridge.c builds against the library alone;
the plan for a union of kinds and the validation of a change list (csrc/bridge_plan.hpp run alone:
tests/host/bridge_open_check.cpp, built here with AddressSanitizer + UBSan and run as a child process, as
tests/test_bridge_plan_cpu.py does); and, compile-only, the two kernels that apply a tick's changes on the device
(csrc/bridge_roster.hip, plc_seats_kernel in csrc/plc.hip) spill nothing and use no scratch memory.  The tick kernels' own
resource figures are pinned where they always were: tests/test_bridge_rates_cpu.py, _legs_, _endpoints_, _rational_,
_ratios_ and _concealed_cpu.py, which this change leaves as they are."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kernel_remarks
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "bridge_open_check.cpp")
PCM16, PCMA, PCMU = 0, 1, 2  # MI_SESSION_* (include/msmi355x.h)
JOIN, LEAVE = 1, 2           # MI_BRIDGE_* (include/msmi355x_bridge.h)
MI_EINVAL, MI_ENOTSUP = -1, -4
P16, ULAW, ALAW = (PCM16, PCM16), (PCMU, PCMU), (PCMA, PCMA)


def test_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "msmi355x_bridge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bint\s+mi_bridge_create_open\s*\(\s*mi_ctx\s*\*\s*\w+\s*,\s*const\s+mi_bridge_config\s*\*\s*\w+\s*,\s*const\s+mi_bridge_leg\s*\*"
                     r"\s*\w+\s*,\s*const\s+mi_bridge_leg\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*mi_bridge\s*\*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+mi_bridge_change_members\s*\(\s*mi_bridge\s*\*\s*\w+\s*,\s*const\s+mi_bridge_change\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"#define\s+MI_BRIDGE_JOIN\s+1\b", code) and re.search(r"#define\s+MI_BRIDGE_LEAVE\s+2\b", code)
    L = _lib.load()
    for name in ("mi_bridge_create_open", "mi_bridge_change_members"):
        assert name in _lib.BRIDGE_EXPORTS
        assert re.search(rf"\sT {name}$", out, flags=re.M), f"{name} is not defined in the built library"
        assert getattr(L, name).argtypes
    assert L.mi_abi_version() == 3


def test_bad_arguments_are_einval_without_a_device():
    L = _lib.load()
    h = C.c_void_p(0x1)
    legs = (C.c_int32 * 3)(8000, PCMU, PCMU)
    assert L.mi_bridge_create_open(None, None, None, None, 0, C.byref(h)) == _lib.MI_EINVAL
    assert L.mi_bridge_create_open(None, None, legs, legs, 1, C.byref(h)) == _lib.MI_EINVAL
    assert L.mi_bridge_create_open(None, None, legs, None, 1, None) == _lib.MI_EINVAL
    change = (C.c_int32 * 5)(0, JOIN, 8000, PCMU, PCMU)
    assert L.mi_bridge_change_members(None, change, 1) == _lib.MI_EINVAL
    assert L.mi_bridge_change_members(None, None, 0) == _lib.MI_EINVAL


def test_header_is_still_plain_c99(tmp_path):
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_bridge.h"\n'
                     "int main(void) { mi_bridge *b = 0; mi_bridge_config c;\n"
                     "  const mi_bridge_leg legs[2] = {{8000, MI_SESSION_PCMU, MI_SESSION_PCMU}, {8000, MI_SESSION_PCMU, MI_SESSION_PCMU}};\n"
                     "  const mi_bridge_leg admit[1] = {{48000, MI_SESSION_PCM16, MI_SESSION_PCM16}};\n"
                     "  mi_bridge_change ch[2] = {{0, MI_BRIDGE_JOIN, {48000, MI_SESSION_PCM16, MI_SESSION_PCM16}}, {1, MI_BRIDGE_LEAVE, {0, 0, 0}}};\n"
                     "  mi_bridge_default_config(&c);\n"
                     "  c.nstreams = c.members_per_conference = 2;\n"
                     "  return mi_bridge_create_open(0, &c, legs, admit, 1, &b) == MI_OK || mi_bridge_change_members(b, ch, 2) == MI_OK; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o",
                        str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_churning_bridge_example_builds(tmp_path):
    """examples/churning_bridge.c builds as C99 against libmsmi355x.so alone, the way mixed_rate_room.c does"""
    pkg = os.path.join(ROOT, "mediastreamer2_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "churning_bridge.c"), "-L", pkg, "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o",
                        str(tmp_path / "churning_bridge")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the plan alone

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("bridge_open") / "bridge_open_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(path)


def _child(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]  # a sanitizer's report ends the program and is its stderr
    code, _, rest = r.stdout.strip().partition(" ")
    return int(code), (rest if int(code) else dict(kv.split("=") for kv in rest.split()))


def _t(legs):
    return [f"{a}:{b}:{c}" for a, b, c in legs]


@pytest.fixture(scope="module")
def run(exe):
    class Run:
        @staticmethod
        def open(conf, mm, legs, admit, plc=False):
            return _child(exe, "open", conf, mm, int(plc), *_t(legs), "/", *_t(admit))

        @staticmethod
        def closed(conf, mm, legs, plc=False):
            return _child(exe, "closed", conf, mm, int(plc), *_t(legs))

        @staticmethod
        def change(conf, mm, legs, admit, gone, changes, plc=False):
            """admit None: the closed plan of `legs`.  changes: (stream, op, (rate, in, out))"""
            return _child(exe, "change", conf, mm, int(plc), *_t(legs), "/", *(["closed"] if admit is None else _t(admit)), "/", *gone, "/",
                          *[f"{s}:{op}:{k[0]}:{k[1]}:{k[2]}" for s, op, k in changes])
    return Run


# what a plan decides that is not per seat (the issue's list), as tests/host/bridge_open_check.cpp prints it
SHARED = ("family", "wide", "row_w", "lds", "scratch_off", "scratch_per_wave", "hin_stride", "hout_stride", "in_bytes", "out_bytes", "pitch",
          "used", "above", "r32", "generic", "leg_plc")
K8U, K8A, K16, K48, K32, K24, K12 = ((8000, *ULAW), (8000, PCMA, PCM16), (16000, *P16), (48000, *P16), (32000, *P16), (24000, *P16),
                                     (12000, *P16))
# (conference rate, members, initial legs, admitted kinds)
UNIONS = {
    "whole-below-and-above": (16000, 3, [K8U, K16, K8U] * 2, [K48]),
    "3/2": (16000, 3, [K16] * 6, [K24]),
    "ratio-4": (8000, 3, [K8U] * 6, [K32]),
    "a:b": (16000, 3, [K8U, K16, K16] * 2, [K12]),
    "the-gpu-room": (16000, 3, [K8U, K8A, K16] * 2, [K48, K32, K24, K12]),
    "the-gpu-room-at-8k": (8000, 3, [K8U] * 6, [K32, K12]),
    "uniform-legs-wider-kinds": (8000, 4, [K8U] * 8, [K16, K48]),
    "uniform-legs-another-codec": (8000, 4, [K8U] * 4, [(8000, PCMA, PCMA)]),
    "an-admitted-kind-that-is-there": (16000, 3, [K8U, K16, K48] * 2, [K16, K48]),
}


@pytest.mark.parametrize("plc", [False, True], ids=["", "plc"])
@pytest.mark.parametrize("case", list(UNIONS))
def test_the_plan_of_a_union(run, case, plc):
    """every field that is not per seat equals the plan of the closed bridge that holds the legs followed by whole conferences
    of the admitted kinds; the per-seat vectors are there, and they are the legs'"""
    conf, mm, legs, admit = UNIONS[case]
    code, p = run.open(conf, mm, legs, admit, plc)
    assert code == 0, p
    code, q = run.closed(conf, mm, legs + [k for k in admit for _ in range(mm)], plc)
    assert code == 0, q
    assert {k: p[k] for k in SHARED} == {k: q[k] for k in SHARED}
    assert p["open"] == "1" and int(p["n"]) == len(legs) and int(p["nconf"]) == len(legs) // mm
    assert int(p["kinds"]) == len(set(legs + admit))
    assert p["leg_rate"] == "[" + ",".join(str(l[0]) for l in legs) + "]"
    assert p["leg_codec"] == "[" + ",".join(str(l[1] | l[2] << 2) for l in legs) + "]"
    seats = q["ratio"][1:-1].split(",")[:len(legs)] if q["ratio"] != "[]" else ["1"] * len(legs)  # (no resamplers: every leg at the mix)
    assert p["ratio"] == "[" + ",".join(seats) + "]"


def test_nothing_admitted_is_the_ratios_plan(run):
    """nadmit == 0: plan_legs(RULES_RATIOS, ...) field for field -- every name the program prints, the per-seat vectors' presence
    included"""
    for conf, mm, legs, _ in UNIONS.values():
        for plc in (False, True):
            assert run.open(conf, mm, legs, [], plc) == run.closed(conf, mm, legs, plc)
    assert run.open(8000, 4, [K8U] * 8, [])[1]["leg_rate"] == "[8000,8000,8000,8000,8000,8000,8000,8000]"
    assert run.open(8000, 4, [K8U] * 8, [])[1]["ratio"] == "[]"


def test_refusals_name_the_admitted_kind(run):
    ok = [K8U] * 6
    for values, conf, mm, legs, admit, plc in [
        (["mi_bridge_create_ratios", "admitted kind 1 at 44100 Hz in a 8000 Hz", "441 : 80"], 8000, 3, ok, [K16, (44100, *P16)], False),
        (["admitted kind 0 at 28000 Hz in a 8000 Hz", "7 : 2"], 8000, 3, ok, [(28000, *P16)], False),
        (["admitted kind 2 names codec 7"], 8000, 3, ok, [K16, K48, (8000, PCMU, 7)], False),
        (["leg 5 names codec 7"], 8000, 3, ok[:5] + [(8000, PCMU, 7)], [K16], False),  # (a leg is still a leg)
        # 50 members at 8 kHz fit; admitting 48 kHz PCM makes the rows 480 samples wide: mi_bridge_create_endpoints' cap is 42
        (["LDS", "50 members x 480 samples"], 8000, 50, [K8U] * 50, [K48], False),
        (["admitted kind 1 at 64000 Hz", "the concealer"], 24000, 3, [K24] * 6, [K12, (64000, *P16)], True),
    ]:
        code, text = run.open(conf, mm, legs, admit, plc)
        assert code == MI_ENOTSUP, text
        for v in values:
            assert v in text, text
    assert run.open(8000, 50, [K8U] * 50, [])[0] == 0 and run.open(8000, 42, [K8U] * 42, [K48])[0] == 0
    assert run.open(24000, 3, [K24] * 6, [K12, (64000, *P16)])[0] == 0  # 8 : 3, legal without the concealer


def test_eight_distinct_rates_with_plc(run):
    """a 48 kHz room: 8, 12, 16, 24, 32 and 48 kHz, and 19.2 and 28.8 kHz at 2 : 5 and 3 : 5 -- every one a ratio the plan serves"""
    legs = [K48, K8U, K12] * 2
    admit = [K16, K24, K32, (19200, *P16), (28800, *P16)]
    assert run.open(48000, 3, legs, admit)[0] == 0
    code, text = run.open(48000, 3, legs, admit, plc=True)
    assert code == MI_ENOTSUP and "8 distinct rates" in text and "7 rate classes" in text, text
    assert run.open(48000, 3, legs, admit[:-1], plc=True)[0] == 0


def test_change_lists(run):
    conf, mm, legs, admit = UNIONS["the-gpu-room"]
    ok = lambda changes, gone=(): run.change(conf, mm, legs, admit, gone, changes)
    # ratio_byte's and gen_byte's bytes: 8 kHz in 16 kHz 2; 48 kHz 0x83; 32 kHz 0x82; 24 kHz 3/2 above 0xc1; 12 kHz 3 : 4 0x3a; 16 kHz 1
    code, got = ok([(0, JOIN, K48), (1, JOIN, K32), (2, JOIN, K24), (3, JOIN, K12), (4, JOIN, K16), (5, LEAVE, K8U)])
    assert code == 0 and got["ratio"] == f"[{0x83},{0x82},{0xc1},{0x3a},1,0]", got
    code, got = run.change(8000, 3, [K8U] * 6, [K32, K12], (), [(0, JOIN, K32), (4, JOIN, K12), (5, JOIN, K8U)])
    assert code == 0 and got["ratio"] == f"[{0x84},{0xc1},1]", got
    assert ok([]) == (0, {"ratio": "[]"})
    assert ok([(2, JOIN, K8A)], gone=[2])[0] == 0  # a free seat, and a taken one above
    for code, values, changes, gone in [
        (MI_ENOTSUP, ["entry 1", "seat 4", "44100 Hz", "in 0, out 0", "admits 7 kinds"], [(0, JOIN, K48), (4, JOIN, (44100, *P16))], ()),
        (MI_ENOTSUP, ["entry 0", "seat 1", "8000 Hz", "in 2, out 1"], [(1, JOIN, (8000, PCMU, PCMA))], ()),
        (MI_EINVAL, ["entry 1", "stream 3 is no member"], [(0, JOIN, K48), (3, LEAVE, K8U)], [3]),
        (MI_EINVAL, ["entry 0", "stream 6 of 6"], [(6, LEAVE, K8U), (0, JOIN, K48)], ()),
        (MI_EINVAL, ["entry 1", "stream -1"], [(0, JOIN, K48), (-1, JOIN, K48)], ()),
        (MI_EINVAL, ["entry 0", "op 3"], [(0, 3, K48)], ()),
        (MI_EINVAL, ["entry 0", "op 0"], [(0, 0, K48)], ()),
        (MI_EINVAL, ["entry 2", "stream 1 a second time"], [(1, JOIN, K48), (0, JOIN, K48), (1, LEAVE, K48)], ()),
    ]:
        got, text = ok(changes, gone)
        assert got == code, text
        for v in values:
            assert v in text, text


def test_a_closed_plan_admits_each_seats_own_kind_only(run):
    legs = [K8U, K16, K48] * 2
    for plc in (False, True):
        ch = lambda changes, gone=(): run.change(16000, 3, legs, None, gone, changes, plc)
        assert ch([(0, JOIN, K8U), (1, JOIN, K16), (5, JOIN, K48), (3, LEAVE, K8U)]) == (0, {"ratio": f"[2,1,{0x83},0]"})
        code, text = ch([(0, JOIN, K16)])  # a kind the bridge holds, on another seat
        assert code == MI_ENOTSUP and "entry 0" in text and "seat 0" in text and "16000 Hz" in text and "1 kind is admitted" in text, text
        assert ch([(4, LEAVE, K16)], gone=[4])[0] == MI_EINVAL
    # a uniform bridge, whose plan has no per-seat vectors
    assert run.change(8000, 3, [K8U] * 6, None, (), [(2, JOIN, K8U)]) == (0, {"ratio": "[1]"})
    assert run.change(8000, 3, [K8U] * 6, None, (), [(2, JOIN, K8A)])[0] == MI_ENOTSUP


# ---- the kernels, compile-only

def _clean(found):
    assert len(found) == 1, [n for n, _ in found]
    name, u = found[0]
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
    print(name, {k: u[k] for k in ("VGPRs", "SGPRs", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]") if k in u})


def test_the_roster_kernel_spills_nothing_and_uses_no_scratch():
    found = kernel_remarks.kernels(kernel_remarks.remarks("bridge_roster.hip"))
    assert "bridge_roster_kernel" in found[0][0]
    _clean(found)


def test_the_concealers_seat_kernel_spills_nothing_and_uses_no_scratch():
    _clean(kernel_remarks.usages(kernel_remarks.remarks("plc.hip"), "plc_seats_kernel"))
