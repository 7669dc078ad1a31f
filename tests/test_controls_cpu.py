"""CPU-side checks of the control plane without a drain -- mi_bridge_change_controls / _set_reports / _collected_report
(include/msmi355x_bridge.h) and the session's three (include/msmi355x_session_controls.h): declared, listed and exported, the
older headers and lists untouched; both headers plain C99; NULL objects refused by name; examples/moderated_bridge.c builds
against the library alone; the host's bookkeeping (csrc/control_changes.hpp run alone: tests/host/controls_check.cpp, built here
with AddressSanitizer + UBSan and run as a child process) -- merge per seat and field, JOIN + FLAGS in one tick, LEAVE after a
control, a waiting setter's last word, refusals that leave the state untouched; the election's threshold float; and,
compile-only, the two kernels of csrc/controls.hip spill nothing and use no scratch memory."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

import kernel_remarks
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "controls_check.cpp")
JOIN, LEAVE = 1, 2
L_, A_, O_ = 1, 2, 4              # MI_MIX_LINKED, _ACTIVE, _OUTPUT
ON = L_ | A_ | O_
FLAGS, GAIN, VOLUME, JOINED = 1, 2, 4, 8  # MI_CTL_*; JOINED is the library's own (csrc/control_changes.hpp)
BRIDGE_NEW = ["mi_bridge_change_controls", "mi_bridge_set_reports", "mi_bridge_collected_report"]
SESSION_NEW = ["mi_session_change_controls", "mi_session_set_reports", "mi_session_collected_report"]


def _code(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def _declared(code, prefix):
    return sorted(set(re.findall(rf"\b({prefix}[a-z0-9_]+)\s*\(", code)))


def _exported():
    return subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout


def test_the_bridge_header_its_list_and_the_library_agree():
    code = _code("msmi355x_bridge.h")
    assert _declared(code, "mi_bridge_") == sorted(_lib.BRIDGE_EXPORTS)
    assert set(re.findall(r"\b(mi_bridge_[a-z0-9_]+)\b", _exported())) == set(_lib.BRIDGE_EXPORTS)
    assert set(BRIDGE_NEW) <= set(_lib.BRIDGE_EXPORTS)
    assert re.search(r"\bint\s+mi_bridge_change_controls\s*\(\s*mi_bridge\s*\*\s*\w+\s*,\s*const\s+mi_bridge_control\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+mi_bridge_set_reports\s*\(\s*mi_bridge\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+mi_bridge_collected_report\s*\(\s*mi_bridge\s*\*\s*\w+\s*,\s*mi_bridge_report\s*\*\s*\w+\s*\)\s*;", code)
    for name, value in (("MI_CTL_FLAGS", 1), ("MI_CTL_GAIN", 2), ("MI_CTL_VOLUME", 4), ("MI_REPORT_SPEAKERS", 1), ("MI_REPORT_LEVELS", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}u\b", code), name
    L = _lib.load()
    assert all(getattr(L, n).argtypes for n in BRIDGE_NEW) and L.mi_abi_version() == 3


def test_the_session_header_its_list_and_the_library_agree():
    code = _code("msmi355x_session_controls.h")
    assert _declared(code, "mi_session_") == sorted(_lib.SESSION_CONTROL_EXPORTS) == sorted(SESSION_NEW)
    out = _exported()
    for name in SESSION_NEW:
        assert re.search(rf"\sT {name}$", out, flags=re.M), f"{name} is not defined in the built library"
    # every mi_session_* symbol of the library is declared in exactly one of the three headers' lists
    lists = [_lib.EXPORTS, _lib.SESSION_EXPORTS, _lib.SESSION_CONTROL_EXPORTS]
    listed = [n for l in lists for n in l if n.startswith("mi_session_")]
    assert sorted(listed) == sorted(set(re.findall(r"\b(mi_session_[a-z0-9_]+)\b", out)))
    assert re.search(r'#include\s+"msmi355x\.h"', code) and "msmi355x_bridge.h" not in code and "msmi355x_session.h" not in code
    assert "MI_CTL_VOLUME" not in code  # the session has no public setter for mi_volume_params
    assert re.search(r"typedef\s+struct\s+mi_session_control\s*\{\s*int32_t\s+stream\s*;\s*uint32_t\s+what\s*;\s*uint32_t\s+flags\s*;\s*float\s+gain\s*;"
                     r"\s*\}\s*mi_session_control\s*;", code)
    L = _lib.load()
    assert all(getattr(L, n).argtypes for n in SESSION_NEW) and L.mi_abi_version() == 3


def test_the_older_headers_and_lists_are_unchanged():
    main = open(os.path.join(ROOT, "include", "msmi355x.h")).read()
    for word in ("change_controls", "set_reports", "collected_report", "MI_CTL_", "MI_REPORT_"):
        assert word not in main and word not in open(os.path.join(ROOT, "include", "msmi355x_session.h")).read(), word
    assert _lib.SESSION_EXPORTS == ["mi_session_change_members"]
    assert not (set(BRIDGE_NEW) | set(SESSION_NEW)) & set(_lib.EXPORTS)


def test_both_headers_are_plain_c99(tmp_path):
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_bridge.h"\n#include "msmi355x_session_controls.h"\n#include "msmi355x_session.h"\n'
                     "int main(void) { mi_bridge *b = 0; mi_session *s = 0; mi_bridge_report rb; mi_session_report rs;\n"
                     "  mi_bridge_control cb[1];\n"
                     "  mi_session_control cs[2] = {{0, MI_CTL_FLAGS, MI_MIX_ACTIVE, 0.f}, {1, MI_CTL_GAIN, 0, 2.f}};\n"
                     "  cb[0].stream = 0, cb[0].what = MI_CTL_FLAGS | MI_CTL_GAIN | MI_CTL_VOLUME, cb[0].flags = MI_MIX_OUTPUT, cb[0].gain = 0.5f;\n"
                     "  mi_volume_default_params(&cb[0].params);\n"
                     "  return mi_bridge_change_controls(b, cb, 1) + mi_session_change_controls(s, cs, 2) + mi_bridge_set_reports(b, MI_REPORT_SPEAKERS)\n"
                     "    + mi_session_set_reports(s, MI_REPORT_LEVELS) + mi_bridge_collected_report(b, &rb) + mi_session_collected_report(s, &rs); }\n")
    for first in ("msmi355x_bridge.h", "msmi355x_session_controls.h"):  # each alone, and both in one unit
        alone = tmp_path / f"alone_{first}.c"
        alone.write_text(f'#include "{first}"\nint f(void) {{ return MI_CTL_FLAGS; }}\n')
        for src in (alone, probe):
            r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                                str(src), "-o", str(tmp_path / "hdr.o")], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr


def test_null_objects_are_einval_and_the_entry_is_named():
    L = _lib.load()
    one = _lib.Control(0, FLAGS, A_, 0.0)
    rep = _lib.Report()
    for p in ("bridge", "session"):
        for name, args in ((f"mi_{p}_change_controls", (None, C.byref(one), 1)), (f"mi_{p}_change_controls", (None, None, 0)),
                           (f"mi_{p}_set_reports", (None, 3)), (f"mi_{p}_collected_report", (None, C.byref(rep)))):
            assert getattr(L, name)(*args) == _lib.MI_EINVAL, name
            assert name.encode() in L.mi_last_error(), (name, L.mi_last_error())


def test_moderated_bridge_example_builds(tmp_path):
    """examples/moderated_bridge.c builds as C99 against libmsmi355x.so alone"""
    pkg = os.path.join(ROOT, "mediastreamer2_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "moderated_bridge.c"), "-L", pkg, "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o",
                        str(tmp_path / "moderated_bridge")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the bookkeeping alone

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("controls") / "controls_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(path)


def _run(exe, kind, n, mm, *steps):
    r = subprocess.run([exe, kind, str(n), str(mm), *steps], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]  # a sanitizer's report ends the program and is its stderr
    return [line.split() for line in r.stdout.strip().splitlines()]


def _rows(lines, tag):
    num = lambda v: float(v) if "." in v or "e" in v else int(v)
    return [sorted(tuple(num(v) for v in c.split(":")) for c in l[1:]) for l in lines if l[0] == tag]


def _state(lines):
    return dict(kv.split("=") for kv in lines[-1][1:])


def test_calls_before_one_submit_merge_per_seat_and_per_field(exe):
    out = _run(exe, "bridge", 8, 4, f"c/2:{FLAGS}:{O_}:0", f"c/2:{GAIN}:0:0.5,3:{GAIN}:0:2", f"c/2:{FLAGS}:{A_}:0,3:{VOLUME}:0:0:3", f"c/3:{GAIN | VOLUME}:0:4:5",
               "s", "s")
    assert [l[:2] for l in out if l[0] == "call"] == [["call", "0"]] * 4
    ctl = _rows(out, "ctl")
    # one command per seat, every touched field in it, the last value of each: (stream, what, flags, gain, joined, static_gain -- 0 without MI_CTL_VOLUME)
    assert ctl[0] == [(2, FLAGS | GAIN, L_ | A_, 0.5, 3, 0), (3, GAIN | VOLUME, ON, 4, 4, 5)]
    assert ctl[1] == [] and _rows(out, "seat") == [[], []]
    st = _state(out)
    assert st["flags"] == "77377777" and st["gain"] == "1,1,0.5,4,1,1,1,1," and st["static"] == "1,1,1,5,1,1,1,1," and st["pending"] == ""


def test_membership_first_then_controls(exe):
    # a JOIN and MI_CTL_FLAGS with ACTIVE clear before one submit: the member arrives muted, in both rows
    out = _run(exe, "session", 4, 4, "r/1", f"m/1:{JOIN}", f"c/1:{FLAGS}:{O_}:0", "s")
    assert _rows(out, "seat") == [[(1, JOIN, L_ | O_)]] and _rows(out, "ctl") == [[(1, FLAGS, L_ | O_, 1, 5, 0)]]
    # a LEAVE after a control on the same seat: unplumbed, and the control's command says so too
    out = _run(exe, "session", 4, 4, f"c/2:{FLAGS | GAIN}:{A_}:3", f"m/2:{LEAVE}", "s")
    assert _rows(out, "seat")[0][0][2] == 0 and _rows(out, "ctl") == [[(2, FLAGS | GAIN, 0, 3, 3, 0)]]
    assert _state(out)["flags"] == "7707"
    # ... and MI_CTL_FLAGS needs a member at the time of the call, membership changes not yet submitted included
    out = _run(exe, "session", 4, 4, f"m/2:{LEAVE}", f"c/2:{FLAGS}:{A_}:0", f"c/2:{GAIN}:0:2", f"m/2:{JOIN}", f"c/2:{FLAGS}:{A_}:0")
    calls = [l for l in out if l[0] == "call"]
    assert [int(c[1]) for c in calls] == [0, -1, 0, 0, 0] and "stream 2, which is no member" in " ".join(calls[1])


def test_a_waiting_setter_before_the_submit_has_the_last_word(exe):
    out = _run(exe, "bridge", 4, 4, f"c/1:{FLAGS | GAIN | VOLUME}:0:0.25:2", f"f/1:{ON}", "g/1:3", "v/1:7", f"c/2:{FLAGS}:0:0", "r/2", "a/2", "s")
    assert _rows(out, "ctl") == [[(1, FLAGS | GAIN | VOLUME, ON, 3, 2, 7), (2, FLAGS, ON, 1, 5, 0)]]
    st = _state(out)
    assert st["flags"] == "7777" and st["gain"] == "1,3,1,1," and st["static"] == "1,7,1,1,"


def test_a_joins_place_in_the_order_rides_along_while_reports_are_on(exe):
    assert _rows(_run(exe, "bridge", 4, 4, f"m/1:{JOIN}", "s"), "ctl") == [[]]
    out = _run(exe, "bridge", 4, 4, "R/1", f"m/1:{JOIN},2:{LEAVE}", f"c/3:{GAIN}:0:2", "s", "s")
    assert _rows(out, "ctl") == [[(1, JOINED, ON, 1, 5, 0), (3, GAIN, ON, 2, 4, 0)], []]


def test_every_seat_in_one_tick_fits_the_row(exe):
    n = 64
    out = _run(exe, "bridge", n, 8, "c/" + ",".join(f"{s}:{FLAGS | GAIN | VOLUME}:{A_}:{s}:2" for s in range(n)), "s", "s")
    ctl = _rows(out, "ctl")
    assert ctl[0] == [(s, FLAGS | GAIN | VOLUME, L_ | A_, s, s + 1, 2) for s in range(n)] and ctl[1] == []
    # an entry that names one field only lists its seat once, whichever field it is, however many calls name it
    for what in (FLAGS, GAIN, VOLUME):
        call = "c/" + ",".join(f"{s}:{what}:{A_}:{s}:2" for s in range(n))
        out = _run(exe, "bridge", n, 8, call, call, "s", "s")
        ctl = _rows(out, "ctl")
        assert [c[:2] for c in ctl[0]] == [(s, what) for s in range(n)] and ctl[1] == [], what


def test_refusals_name_the_entry_and_leave_the_state_untouched(exe):
    for kind, fn in (("bridge", "mi_bridge_change_controls"), ("session", "mi_session_change_controls")):
        prior = ["r/6", f"c/3:{FLAGS | GAIN}:{O_}:0.5"]
        before = _run(exe, kind, 8, 4, *prior)
        unknown = 8 if kind == "bridge" else VOLUME
        cases = [
            (f"c/1:{GAIN}:0:2,8:{GAIN}:0:2,2:{GAIN}:0:2", -1, ["entry 1", "stream 8 of 8"]),
            (f"c/1:{GAIN}:0:2,-1:{GAIN}:0:2", -1, ["entry 1", "stream -1"]),
            (f"c/1:{GAIN}:0:2,2:0:0:2", -1, ["entry 1", "what 0x0"]),
            (f"c/2:{unknown}:0:2,1:{GAIN}:0:2", -1, ["entry 0", f"what 0x{unknown:x}"]),
            (f"c/1:{GAIN}:0:2,2:{FLAGS}:{L_ | A_}:0", -1, ["entry 1", "flags 0x3", "MI_MIX_LINKED is membership's"]),
            (f"c/1:{GAIN}:0:2,2:{FLAGS}:8:0", -1, ["entry 1", "flags 0x8"]),
            (f"c/1:{GAIN}:0:2,6:{FLAGS}:{A_}:0", -1, ["entry 1", "stream 6, which is no member"]),
            (f"c/1:{GAIN}:0:2,2:{FLAGS}:0:0,1:{FLAGS}:0:0", -1, ["entry 2", "stream 1 a second time"]),
            ("n/-1", -1, ["-1 changes"]),
            ("n/2", -1, ["null h_changes"]),
        ]
        if kind == "bridge":
            cases.append((f"c/1:{GAIN}:0:2,2:{VOLUME}:0:0:2:0", -4, ["entry 1", "echo-limiter peer (0)"]))
        for bad, code, values in cases:
            out = _run(exe, kind, 8, 4, *prior, bad)
            call = out[-2]
            assert call[0] == "call" and int(call[1]) == code and fn in " ".join(call), call
            for v in values:
                assert v in " ".join(call), call
            assert out[-1] == before[-1], (bad, out[-1])
            # ... and the tick that follows carries what was pending before it, nothing of the refused call
            assert _rows(_run(exe, kind, 8, 4, *prior, bad, "s"), "ctl") == [[(3, FLAGS | GAIN, L_ | O_, 0.5, 4, 0)]]
        assert _run(exe, kind, 8, 4, *prior, "c/")[-2][:2] == ["call", "0"]  # count == 0 is MI_OK
        assert _run(exe, kind, 8, 4, *prior, "c/")[-1] == before[-1]
        # gain (and the bridge's parameters) may be set on a seat nobody holds
        ok = f"c/6:{GAIN | (VOLUME if kind == 'bridge' else 0)}:0:2:3"
        assert _run(exe, kind, 8, 4, *prior, ok)[-2][:2] == ["call", "0"]


# ---- the threshold

def test_the_threshold_is_the_dbm0_comparison_to_the_ulp(exe):
    line = _run(exe, "bridge", 4, 4, "thr")[0]
    assert line[0] == "thr" and line[2] == "ok", line
    bits = int(line[1], 16)
    thr = struct.unpack("<f", struct.pack("<I", bits))[0]
    assert abs(thr - 1e-3) < 1e-6
    # the same with this process's libm, which is the library's
    libm = C.CDLL("libm.so.6")
    libm.log10f.restype, libm.log10f.argtypes = C.c_float, [C.c_float]
    f32 = lambda v: C.c_float(v).value
    above = lambda x: f32(10 * libm.log10f(x)) > -30.0 if x > 0 else False
    for d in range(-64, 65):
        x = struct.unpack("<f", struct.pack("<I", bits + d))[0]
        assert above(x) == (x >= thr), (d, x)
    assert above(0.0) == (0.0 >= thr)


# ---- the kernels, compile-only

def test_the_two_kernels_spill_nothing_and_use_no_scratch():
    found = kernel_remarks.kernels(kernel_remarks.remarks("controls.hip"))
    assert len(found) == 2, [n for n, _ in found]
    assert any("controls_kernel" in n for n, _ in found) and any("report_kernel" in n for n, _ in found)
    for name, u in found:
        assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
        assert int(u["LDS Size [bytes/block]"]) == 0, (name, u)
        print(name, {k: u[k] for k in ("VGPRs", "SGPRs", "Occupancy [waves/SIMD]") if k in u})
