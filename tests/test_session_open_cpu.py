"""CPU-side checks of mi_session_change_members (include/msmi355x_session.h): the entry point is declared, listed and exported,
and msmi355x.h and its export list do not name it; the header is plain C99; examples/churning_session.c builds against the
library alone; the host's bookkeeping that the bridge and the session share (csrc/seat_changes.hpp run alone:
tests/host/session_open_check.cpp, built here with AddressSanitizer + UBSan and run as a child process, as
tests/test_bridge_open_cpu.py does for the plan) -- merge per seat, the SLOTS - 1 clear schedule, refusals that leave the state
untouched; and, compile-only, the kernel that applies a tick's changes on the device (csrc/session_roster.hip) spills nothing
and uses no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kernel_remarks
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "session_open_check.cpp")
JOIN, LEAVE, CLEAR = 1, 2, 4  # MI_SESSION_JOIN / _LEAVE (include/msmi355x_session.h); MI_SEAT_CLEAR (csrc/seat_changes.hpp)
ON = 7                        # MI_MIX_LINKED | MI_MIX_ACTIVE | MI_MIX_OUTPUT
MI_EINVAL = -1


def test_the_entry_point_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "msmi355x_session.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bint\s+mi_session_change_members\s*\(\s*mi_session\s*\*\s*\w+\s*,\s*const\s+mi_session_change\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"#define\s+MI_SESSION_JOIN\s+1\b", code) and re.search(r"#define\s+MI_SESSION_LEAVE\s+2\b", code)
    assert re.search(r"typedef\s+struct\s+mi_session_change\s*\{\s*int32_t\s+stream\s*,\s*op\s*;\s*\}\s*mi_session_change\s*;", code)
    assert re.search(r'#include\s+"msmi355x\.h"', code)
    L = _lib.load()
    assert _lib.SESSION_EXPORTS == ["mi_session_change_members"]
    assert re.search(r"\sT mi_session_change_members$", out, flags=re.M), "mi_session_change_members is not defined in the built library"
    assert L.mi_session_change_members.argtypes
    assert L.mi_abi_version() == 3


def test_the_main_header_and_its_export_list_do_not_name_it():
    assert "mi_session_change" not in open(os.path.join(ROOT, "include", "msmi355x.h")).read()
    assert "mi_session_change_members" not in _lib.EXPORTS and "mi_session_change_members" not in _lib.BRIDGE_EXPORTS


def test_a_null_session_is_einval_without_a_device():
    L = _lib.load()
    change = (C.c_int32 * 2)(0, JOIN)
    assert L.mi_session_change_members(None, change, 1) == _lib.MI_EINVAL
    assert b"mi_session_change_members" in L.mi_last_error()
    assert L.mi_session_change_members(None, None, 0) == _lib.MI_EINVAL


def test_the_header_is_plain_c99(tmp_path):
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_session.h"\n'
                     "int main(void) { mi_session *s = 0;\n"
                     "  mi_session_change ch[2] = {{0, MI_SESSION_JOIN}, {1, MI_SESSION_LEAVE}};\n"
                     "  return mi_session_change_members(s, ch, 2) == MI_OK; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o",
                        str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_churning_session_example_builds(tmp_path):
    """examples/churning_session.c builds as C99 against libmsmi355x.so alone, the way churning_bridge.c does"""
    pkg = os.path.join(ROOT, "mediastreamer2_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "churning_session.c"), "-L", pkg, "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o",
                        str(tmp_path / "churning_session")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the shared bookkeeping alone

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("session_open") / "session_open_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(path)


def _run(exe, n, mm, slots, *steps):
    """-> the program's lines, split: ["row", "3:1:7", ...]"""
    r = subprocess.run([exe, str(n), str(mm), str(slots), *steps], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]  # a sanitizer's report ends the program and is its stderr
    return [line.split() for line in r.stdout.strip().splitlines()]


def _rows(lines):
    return [sorted(tuple(int(v) for v in c.split(":")) for c in l[1:]) for l in lines if l[0] == "row"]


def _state(lines):
    return dict(kv.split("=") for kv in lines[-1][1:])


def test_calls_before_one_submit_merge_per_seat_and_the_last_one_wins(exe):
    out = _run(exe, 8, 4, 3, f"c/2:{LEAVE}", f"c/2:{JOIN}", f"c/5:{JOIN},6:{LEAVE}", f"c/6:{JOIN}", f"c/6:{LEAVE}", "s", "s")
    assert [l[:2] for l in out if l[0] == "call"] == [["call", "0"]] * 5
    rows = _rows(out)
    # one command per seat; a seat that was a member when a change came has its row cleared, a taken seat that is joined included
    assert rows[0] == [(2, JOIN | CLEAR, ON), (5, JOIN | CLEAR, ON), (6, LEAVE | CLEAR, 0)]
    assert rows[1] == [(2, CLEAR, 0), (5, CLEAR, 0), (6, CLEAR, 0)]
    assert _state(out)["members"] == "11111101" and _state(out)["pending"] == ""


def test_the_clear_repeats_until_every_slot_has_had_it(exe):
    for slots in (1, 2, 3, 4):
        out = _run(exe, 4, 4, slots, f"c/1:{LEAVE}", *["s"] * (slots + 1))
        rows = _rows(out)
        assert rows[0] == [(1, LEAVE | CLEAR, 0)]
        assert rows[1:] == [[(1, CLEAR, 0)]] * (slots - 1) + [[]], (slots, rows)
        assert _state(out)["clearing"] == ""
    # a seat plumbed again while a clear is owed: the JOIN carries it, and the schedule runs on from the first leave
    out = _run(exe, 4, 4, 3, f"c/1:{LEAVE}", "s", f"c/1:{JOIN}", "s", "s", "s")
    assert _rows(out) == [[(1, LEAVE | CLEAR, 0)], [(1, JOIN | CLEAR, ON)], [(1, CLEAR, 0)], []]
    # ... and a JOIN of a seat nobody held, with nothing owed, clears nothing
    out = _run(exe, 4, 4, 3, "r/1", f"c/1:{JOIN}", "s", "s")
    assert _rows(out) == [[(1, JOIN, ON)], []]
    # a second leave while clears are owed starts the count again; two seats keep their own counts
    out = _run(exe, 4, 4, 3, f"c/1:{LEAVE}", "s", f"c/2:{LEAVE}", "s", "s", "s", "s")
    assert _rows(out) == [[(1, LEAVE | CLEAR, 0)], [(1, CLEAR, 0), (2, LEAVE | CLEAR, 0)], [(1, CLEAR, 0), (2, CLEAR, 0)], [(2, CLEAR, 0)], []]


def test_every_seat_in_one_tick_fits_the_row(exe):
    n = 64
    out = _run(exe, n, 8, 3, "c/" + ",".join(f"{s}:{LEAVE}" for s in range(n)), "s", "c/" + ",".join(f"{s}:{JOIN}" for s in range(n)), "s", "s", "s")
    rows = _rows(out)
    assert [len(r) for r in rows] == [n, n, n, 0]
    assert rows[1] == [(s, JOIN | CLEAR, ON) for s in range(n)] and rows[2] == [(s, CLEAR, 0) for s in range(n)]


def test_refusals_name_the_entry_and_leave_the_state_untouched(exe):
    fn = "mi_session_change_members"
    before = _run(exe, 8, 4, 3, "r/6", f"c/3:{JOIN}")
    for bad, values in [
        (f"c/1:{JOIN},8:{LEAVE},2:{LEAVE}", ["entry 1", "stream 8 of 8"]),
        (f"c/1:{JOIN},-1:{JOIN}", ["entry 1", "stream -1"]),
        (f"c/1:{JOIN},2:3", ["entry 1", "op 3", "MI_SESSION_JOIN (1) or MI_SESSION_LEAVE (2)"]),
        (f"c/2:0,1:{JOIN}", ["entry 0", "op 0"]),
        (f"c/1:{JOIN},6:{LEAVE},2:{LEAVE}", ["entry 1", "stream 6 is no member"]),
        (f"c/1:{JOIN},2:{LEAVE},1:{LEAVE}", ["entry 2", "stream 1 a second time"]),
        ("n/-1", ["-1 changes"]),
        ("n/2", ["null h_changes"]),
    ]:
        out = _run(exe, 8, 4, 3, "r/6", f"c/3:{JOIN}", bad)
        call = out[-2]
        assert call[0] == "call" and int(call[1]) == MI_EINVAL and fn in " ".join(call), call
        for v in values:
            assert v in " ".join(call), call
        assert out[-1] == before[-1], (bad, out[-1])
        # ... and the tick that follows carries what was pending before it, nothing of the refused call
        assert _rows(_run(exe, 8, 4, 3, "r/6", f"c/3:{JOIN}", bad, "s")) == [[(3, JOIN | CLEAR, ON)]]
    assert _run(exe, 8, 4, 3, "r/6", f"c/3:{JOIN}", "c/")[-2][:2] == ["call", "0"]  # count == 0 is MI_OK
    assert _run(exe, 8, 4, 3, "r/6", f"c/3:{JOIN}", "c/")[-1] == before[-1]


def test_a_waiting_call_before_the_submit_has_the_last_word_on_the_flags(exe):
    out = _run(exe, 4, 4, 3, f"c/1:{JOIN}", "r/1", f"c/2:{LEAVE}", "a/2", "s")
    assert _rows(out) == [[(1, JOIN | CLEAR, 0), (2, LEAVE | CLEAR, ON)]]
    assert _state(out)["members"] == "1011"


def test_a_new_endpoint_is_the_last_of_the_joining_order(exe):
    st = _state(_run(exe, 4, 4, 3, f"c/1:{JOIN}", f"c/0:{LEAVE}", f"c/0:{JOIN}"))
    assert st["joined"] == "6,5,3,4,"  # created in pin order 1..4; seat 1 rejoined as 5, seat 0 as 6


# ---- the kernel, compile-only

def test_the_roster_kernel_spills_nothing_and_uses_no_scratch():
    found = kernel_remarks.kernels(kernel_remarks.remarks("session_roster.hip"))
    assert len(found) == 1 and "session_roster_kernel" in found[0][0], [n for n, _ in found]
    name, u = found[0]
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
    assert int(u["LDS Size [bytes/block]"]) == 0, (name, u)
    print(name, {k: u[k] for k in ("VGPRs", "SGPRs", "Occupancy [waves/SIMD]") if k in u})
