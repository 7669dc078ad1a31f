"""CPU-side checks of the bridge's legs at 44 100 Hz (mi_bridge_create_offgrid): the entry point is declared, listed and
exported; the header is still plain C99; examples/cd_rate_room.c builds against the library alone; what creation plans and
refuses under the new rules (csrc/bridge_plan.hpp run alone: tests/host/bridge_offgrid_plan_check.cpp, built here with
AddressSanitizer + UBSan and run as a child process, as tests/test_bridge_ratios_cpu.py does); and, compile-only, the one
kernel of csrc/bridge_offgrid.hip spills nothing, uses no scratch memory and keeps its static LDS inside what creation
budgets."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kernel_remarks
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "bridge_offgrid_plan_check.cpp")
NEW = "mi_bridge_create_offgrid"
PCM16, PCMA, PCMU = 0, 1, 2  # MI_SESSION_* (include/msmi355x.h)
MI_EINVAL, MI_ENOTSUP = -1, -4
P16, ULAW, ALAW = (PCM16, PCM16), (PCMU, PCMU), (PCMA, PCMA)
CD = 44100
MIXES = (8000, 12000, 16000, 24000, 32000, 48000)


def test_entry_point_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "msmi355x_bridge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(rf"\bint\s+{NEW}\s*\(\s*mi_ctx\s*\*\s*\w+\s*,\s*const\s+mi_bridge_config\s*\*\s*\w+\s*,\s*const\s+mi_bridge_leg\s*\*\s*\w+\s*,"
                     rf"\s*const\s+mi_bridge_leg\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*mi_bridge\s*\*\*\s*\w+\s*\)\s*;", code), \
        f"{NEW} is not declared in msmi355x_bridge.h with mi_bridge_create_open's arguments"
    assert NEW in _lib.BRIDGE_EXPORTS
    assert re.search(rf"\sT {NEW}$", out, flags=re.M), f"{NEW} is not defined in the built library"
    L = _lib.load()
    assert getattr(L, NEW).argtypes == L.mi_bridge_create_open.argtypes
    assert L.mi_abi_version() == 3


def test_bad_arguments_are_einval_without_a_device():
    L = _lib.load()
    h = C.c_void_p(0x1)
    legs = (C.c_int32 * 3)(CD, 0, 0)
    assert getattr(L, NEW)(None, None, None, None, 0, C.byref(h)) == _lib.MI_EINVAL
    assert getattr(L, NEW)(None, None, legs, None, 0, C.byref(h)) == _lib.MI_EINVAL
    assert getattr(L, NEW)(None, None, legs, None, 1, C.byref(h)) == _lib.MI_EINVAL  # kinds announced, none given
    assert getattr(L, NEW)(None, None, legs, legs, -1, C.byref(h)) == _lib.MI_EINVAL


def test_header_is_still_plain_c99(tmp_path):
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_bridge.h"\n'
                     "int main(void) { mi_bridge *b = 0; int i = 0, o = 0; mi_bridge_config c;\n"
                     "  const mi_bridge_leg legs[2] = {{8000, MI_SESSION_PCMU, MI_SESSION_PCMA}, {44100, MI_SESSION_PCM16, MI_SESSION_PCM16}};\n"
                     "  mi_bridge_default_config(&c);\n"
                     "  c.rate = 16000;\n"
                     "  return mi_bridge_create_offgrid(0, &c, legs, legs + 1, 1, &b) == MI_OK || mi_bridge_leg_bytes(b, 1, &i, &o) == MI_OK ||\n"
                     "         mi_bridge_leg_rate(b, 1) == 44100 || i + o; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o",
                        str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cd_rate_room_example_builds(tmp_path):
    """examples/cd_rate_room.c builds as C99 against libmsmi355x.so alone, the way superwideband_room.c does"""
    pkg = os.path.join(ROOT, "mediastreamer2_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "cd_rate_room.c"), "-L", pkg, "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o",
                        str(tmp_path / "cd_rate_room")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the plan alone

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("bridge_offgrid_plan") / "bridge_offgrid_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(path)


@pytest.fixture(scope="module")
def plan(exe):
    def run(rules, conf, members, legs, admit=(), plc=False):
        """-> (return code, the error text or {name: value} of the plan)"""
        r = subprocess.run([exe, rules, str(conf), str(members), str(int(plc)), str(len(admit)), *[f"{a}:{b}:{c}" for a, b, c in [*legs, *admit]]],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]  # a sanitizer's report ends the program and is its stderr
        code, _, rest = r.stdout.strip().partition(" ")
        return int(code), (rest if int(code) else dict(kv.split("=") for kv in rest.split()))
    return run


def filter_len(num, den):
    """design_filter's rule at quality 3 for in : out = num : den (csrc/resample.hip), restated for the test"""
    return 48 if num <= den else ((48 * num // den - 1) & ~7) + 8


up16 = lambda v: (v + 15) & ~15
# the issue's table, which filter_rule must give: mix -> (taps leg -> mix, taps mix -> leg)
TAPS = {8000: (264, 48), 12000: (176, 48), 16000: (136, 48), 24000: (88, 48), 32000: (72, 48), 48000: (48, 56)}


@pytest.mark.parametrize("conf", MIXES)
def test_plan_of_a_cd_rate_leg_in_every_mix(plan, conf):
    """2 x 3 members, the GPU test's conference: family, ratio byte, num : den, both filter lengths, history strides, pitches,
    rows and LDS"""
    from math import gcd
    other = (16000, *P16) if conf == 8000 else (8000, *ULAW)
    legs = [(CD, *P16), (conf, *P16), other] * 2
    code, p = plan("offgrid", conf, 3, legs)
    assert code == 0 and p["family"] == "OFFGRID" and p["offgrid"] == "1", p
    ns, g = conf // 100, gcd(441, conf // 100)
    fin, fout = filter_len(441 // g, ns // g), filter_len(ns // g, 441 // g)
    assert (fin, fout) == TAPS[conf]
    assert p["off"] == f"{441 // g}:{ns // g}" and p["taps"] == f"{fin},{fout}", p
    assert p["bytes"].split(",")[0] == ("10" if conf > CD else "90"), p  # UD_OFF, | UD_ABOVE where the leg is above the mix
    # history: filter length - 1 samples of the longest filter of the conference, at mi_resampler's stride (rounded up to 8)
    longest = max(fin, fout, {8000: 96, 12000: 72, 16000: 96, 24000: 144, 32000: 192, 48000: 288}[conf])
    assert p["hist"] == f"{longest},{longest}" and longest >= fin - 1, p
    # host rows: 882 bytes of PCM rounded up to 16, or the mix's own tick where that is wider; the concealer's PCM rows whole groups
    pitch = max(441, ns)
    assert p["tick_bytes"] == f"{up16(2 * pitch)},{up16(2 * pitch)}" and p["pitch"] == str(pitch) and p["pcm_pitch"] == str((pitch + 7) & ~7), p
    # LDS rows hold 448 samples for a 441-sample tick, at an odd number of 8-byte words
    wide = max(448, ns)
    assert p["wide"] == str(wide) and p["row_w"] == str((wide >> 2) | 1) and int(p["sum_off"]) == up16(3 * ((wide >> 2) | 1) * 8), p
    # a wavefront's scratch holds history ++ tick as floats at least, never a table (28 to 92 KB)
    off_scratch = 4 * max((fin - 1 + 441 + 3) & ~3, (fout - 1 + ns + 3) & ~3)
    per_wave = int(p["scratch"].split("x")[1])
    assert off_scratch <= per_wave < 8 * 1024, p
    assert int(p["lds"]) == up16(int(p["sum_off"]) + 4 * ns) + 4 * per_wave
    assert int(p["lds"]) + kernel_remarks.bridge_budget()[0] <= 64 * 1024


def test_only_cd_rate_legs_keep_the_table_out_of_the_scratch(plan):
    """a conference of 44.1 kHz legs alone: a wavefront's scratch is exactly history ++ tick as floats"""
    for conf, (fin, fout) in TAPS.items():
        code, p = plan("offgrid", conf, 2, [(CD, PCMU, PCMA)] * 4)
        assert code == 0 and p["family"] == "OFFGRID", p
        ns = conf // 100
        assert p["scratch"].split("x")[1] == str(up16(4 * max((fin - 1 + 441 + 3) & ~3, (fout - 1 + ns + 3) & ~3))), p
        assert p["tick_bytes"] == "448,448" and p["hist"] == f"{(max(fin, fout) + 6) & ~7},{(max(fin, fout) + 6) & ~7}", p


def test_no_such_leg_is_the_open_plan(plan):
    """without a 44.1 kHz leg or admitted kind: mi_bridge_create_open's plan, field for field"""
    cases = [(16000, 4, [(8000, *ULAW), (24000, *P16), (16000, *P16), (48000, *P16)] * 2, []),
             (16000, 4, [(8000, *ULAW)] * 8, [(12000, *P16), (48000, PCM16, PCMA)]),
             (8000, 4, [(8000, *ULAW)] * 8, []),
             (12000, 3, [(32000, *P16), (12000, *P16), (8000, *ULAW)] * 2, [(16000, *P16)])]
    for conf, mm, legs, admit in cases:
        for plc in (False, True):
            old, new = plan("open", conf, mm, legs, admit, plc), plan("offgrid", conf, mm, legs, admit, plc)
            assert old[0] == 0 and new[0] == 0, (old, new)
            assert new[1] == old[1] and new[1]["family"] != "OFFGRID" and new[1]["offgrid"] == "0"


def test_an_admitted_kind_alone_plans_the_new_family(plan):
    """initial legs on the grid, 44.1 kHz only among the admitted kinds: the union's family, pitch, strides and ratio bytes"""
    code, p = plan("offgrid", 16000, 4, [(8000, *ULAW)] * 8, [(CD, *P16), (16000, *P16)])
    assert code == 0 and p["family"] == "OFFGRID" and p["open"] == "1" and p["kinds"] == "3", p
    assert p["tick_bytes"] == "896,896" and p["hist"] == "136,136" and p["kind_bytes"] == "02,90,01", p
    assert p["bytes"] == ",".join(["02"] * 8) and p["rates"] == ",".join(["8000"] * 8)
    code, p = plan("offgrid", 16000, 4, [(8000, *ULAW)] * 8, [(CD, *P16), (16000, *P16)], plc=True)
    assert code == 0 and p["leg_plc"] == "1" and p["pcm_pitch"] == "448", p


def test_concealment_goes_through_the_per_leg_concealer(plan):
    """cfg.plc with a 44.1 kHz leg: the per-leg concealer whether the legs differ or not, its PCM rows 448 samples"""
    for legs in ([(CD, *P16), (8000, *ULAW), (16000, *P16)], [(CD, *P16)] * 3):
        code, p = plan("offgrid", 16000, 3, legs, plc=True)
        assert code == 0 and p["leg_plc"] == "1" and p["data"] == "1" and p["pcm_pitch"] == "448" and p["family"] == "OFFGRID", p


ok8, ok16 = [(8000, *ULAW)] * 6, [(16000, *P16)] * 6
at = lambda rate, n, pair=P16: [(rate, *pair)] * n
REFUSALS = [  # (what the text must contain, rules, conference rate, members, legs, admitted kinds)
    # 22.05 and 11.025 kHz, and any other rate off the grid
    ([NEW, "leg 5 at 22050 Hz in a 16000 Hz", "220.50 samples"], "offgrid", 16000, 3, ok16[:5] + at(22050, 1), []),
    ([NEW, "leg 2 at 11025 Hz in a 8000 Hz", "110.25 samples"], "offgrid", 8000, 3, ok8[:2] + at(11025, 1) + ok8[3:], []),
    ([NEW, "admitted kind 1 at 22050 Hz in a 16000 Hz", "220.50"], "offgrid", 16000, 3, ok16, at(CD, 1) + at(22050, 1)),
    ([NEW, "leg 4 at 1000 Hz in a 800 Hz", "no multiple of 800"], "offgrid", 800, 3, at(800, 4) + at(1000, 2), []),
    ([NEW, "leg 0 at 44200 Hz in a 16000 Hz", "no multiple of 800"], "offgrid", 16000, 3, at(44200, 1) + ok16[:5], []),
    ([NEW, "leg 1 at 88200 Hz in a 48000 Hz", "no multiple of 800"], "offgrid", 48000, 3, at(48000, 1) + at(88200, 1) + at(48000, 4), []),
    # a mix at 44.1 kHz; a mix against which the tables fail the rule
    (["rate 44100", "no multiple of 800"], "offgrid", CD, 3, at(CD, 6), []),
    ([NEW, "leg 5 at 44100 Hz in a 4000 Hz", "441 : 40", "536 taps"], "offgrid", 4000, 3, at(4000, 5) + at(CD, 1), []),
    # what mi_bridge_create_ratios refuses on the grid stays refused
    ([NEW, "leg 5 at 40000 Hz in a 8000 Hz", "ratio 5"], "offgrid", 8000, 3, ok8[:5] + at(40000, 1), at(CD, 1)),
    ([NEW, "leg 5 at 8000 Hz in a 56000 Hz", "ratio 7"], "offgrid", 56000, 3, at(56000, 5) + at(8000, 1, ULAW), []),
    ([NEW, "leg 5 at 64000 Hz in a 8000 Hz", "ratio 8"], "offgrid", 8000, 3, ok8[:5] + at(64000, 1), []),
    ([NEW, "admitted kind 0 at 28000 Hz in a 8000 Hz", "7 : 2", "168 taps"], "offgrid", 8000, 3, ok8, at(28000, 1)),
    ([NEW, "leg 2 at 14400 Hz in a 12800 Hz", "9 : 8", "interpolated"], "offgrid", 12800, 3, at(12800, 2) + at(14400, 1) + at(12800, 3), []),
    ([NEW, "leg 5 names codec 3"], "offgrid", 16000, 3, at(16000, 5) + [(CD, PCMU, 3)], []),
    # the LDS, with rows as wide as a 441-sample tick or wider
    (["LDS", "46 members x 480 samples", "44100 Hz"], "offgrid", 16000, 46, ([(CD, *P16), (48000, *P16)] * 23), []),
    # the older rules keep refusing 44.1 kHz, in their own words
    (["mi_bridge_create_ratios", "leg 5 at 44100 Hz in a 8000 Hz", "441 : 80"], "open", 8000, 3, ok8[:5] + at(CD, 1), []),
    (["mi_bridge_create_ratios", "admitted kind 0 at 44100 Hz in a 16000 Hz", "441 : 160"], "open", 16000, 3, ok16, at(CD, 1)),
]


@pytest.mark.parametrize("values,rules,conf,members,legs,admit", REFUSALS, ids=[f"{r[1]}-{r[2]}-{r[0][-1]}" for r in REFUSALS])
def test_refusals(plan, values, rules, conf, members, legs, admit):
    code, text = plan(rules, conf, members, legs, admit)
    assert code == MI_ENOTSUP, text
    for v in values:
        assert str(v) in text, text


def test_member_limits_of_the_header(plan):
    """include/msmi355x_bridge.h: 44.1 kHz legs alone fit at the mixer's own 50 members in each of the six mixes, 58 896 bytes
    at 48 kHz, and 51 are refused as the mixer refuses them; in a 16 kHz room that also holds 48 kHz members the rows are 480
    samples and the ratio-3 down-sampler's scratch decides: 45 are planned at the LDS edge, 46 refused for it"""
    static, limit = kernel_remarks.bridge_budget()[:2]
    for conf in MIXES:
        code, p = plan("offgrid", conf, 50, at(CD, 50))
        assert code == 0 and p["family"] == "OFFGRID" and int(p["lds"]) + static <= limit, p
        assert conf != 48000 or int(p["lds"]) == 58896, p
        assert plan("offgrid", conf, 51, at(CD, 51))[0] == MI_EINVAL
    room = [(CD, *P16), (48000, *P16)]
    code, p = plan("offgrid", 16000, 45, (room * 45)[:45])
    assert code == 0 and p["family"] == "OFFGRID" and int(p["lds"]) + static <= limit, p
    assert int(p["lds"]) + static + 8 * ((480 >> 2) | 1) > limit  # the edge: one more row does not fit
    code, text = plan("offgrid", 16000, 46, (room * 46)[:46])
    assert code == MI_ENOTSUP and "LDS" in text and "46 members x 480 samples" in text, text
    code, text = plan("offgrid", 16000, 46, [(16000, *P16)] * 46, [(CD, *P16), (48000, *P16)])  # by the admitted kinds alone
    assert code == MI_ENOTSUP and "LDS" in text, text
    hdr = open(os.path.join(ROOT, "include", "msmi355x_bridge.h")).read()
    assert "58 896 bytes" in hdr and "members: up to 45 members" in hdr


# ---- the kernel, compile-only

@pytest.fixture(scope="module")
def remarks():
    return kernel_remarks.remarks("bridge_offgrid.hip")


def test_one_kernel_that_spills_nothing_and_fits_the_lds_budget(remarks):
    """mi_bridge_create_offgrid accepts a shape when its dynamic LDS + RATED_STATIC_LDS <= 64 KB, so the kernel's static LDS
    must stay inside that constant; no spill and no scratch memory, with or without an occupancy hint"""
    budget, _, src = kernel_remarks.bridge_budget()
    assert "lds + RATED_STATIC_LDS > BRIDGE_LDS_MAX" in src
    found = kernel_remarks.kernels(remarks)
    assert len(found) == 1, [n for n, _ in found]
    name, u = found[0]
    assert "bridge_offgrid_kernel" in name, name
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
    assert int(u["LDS Size [bytes/block]"]) <= budget, u
    print(name, {k: u[k] for k in ("VGPRs", "SGPRs", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]") if k in u})
