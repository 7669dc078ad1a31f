"""CPU-side checks of the bridge's legs at 3/2 and 2/3 of the mix's rate (mi_bridge_create_rational): the entry point is
declared, listed and exported; the header is still plain C99; examples/superwideband_room.c builds against the library
alone; and, compile-only as tests/test_bridge_endpoints_cpu.py does it, the one kernel that runs such a leg spills nothing,
uses no scratch memory and keeps its static LDS inside what creation budgets."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kernel_remarks
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "mi_bridge_create_rational"
OLD_KERNELS = ("bridge_tick_kernel", "bridge_rated_kernel", "bridge_legs_kernel", "bridge_updown_kernel")


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
    legs = (C.c_int32 * 3)(32000, 0, 0)
    assert getattr(L, NEW)(None, None, legs, C.byref(h)) == _lib.MI_EINVAL


def test_header_is_still_plain_c99(tmp_path):
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_bridge.h"\n'
                     "int main(void) { mi_bridge *b = 0; int i = 0, o = 0; mi_bridge_config c;\n"
                     "  const mi_bridge_leg legs[2] = {{8000, MI_SESSION_PCMU, MI_SESSION_PCMA}, {32000, MI_SESSION_PCM16, MI_SESSION_PCM16}};\n"
                     "  mi_bridge_default_config(&c);\n"
                     "  c.rate = 48000;\n"
                     "  return mi_bridge_create_rational(0, &c, legs, &b) == MI_OK || mi_bridge_leg_bytes(b, 1, &i, &o) == MI_OK ||\n"
                     "         mi_bridge_leg_rate(b, 1) == 32000 || i + o; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o",
                        str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_superwideband_room_example_builds(tmp_path):
    """examples/superwideband_room.c builds as C99 against libmsmi355x.so alone, the way wideband_room.c does"""
    pkg = os.path.join(ROOT, "mediastreamer2_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "superwideband_room.c"), "-L", pkg, "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o",
                        str(tmp_path / "superwideband_room")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def remarks():
    return kernel_remarks.remarks("bridge.hip")


def test_one_new_kernel_that_spills_nothing_and_fits_the_lds_budget(remarks):
    """exactly one kernel beside the four older families, whatever it is called; direction, ratio and codec are per-member
    data.  mi_bridge_create_rational accepts a shape when its dynamic LDS + RATED_STATIC_LDS <= 64 KB, so the kernel's
    static LDS must stay inside that constant"""
    budget = kernel_remarks.bridge_budget()[0]
    new = [(n, u) for n, u in kernel_remarks.kernels(remarks) if not any(old in n for old in OLD_KERNELS)]
    assert len(new) == 1, [n for n, _ in new]
    name, u = new[0]
    assert "rational" in name, name
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
    assert int(u["LDS Size [bytes/block]"]) <= budget, u
