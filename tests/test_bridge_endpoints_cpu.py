"""CPU-side checks of the bridge's endpoints on either side of the mix (mi_bridge_create_endpoints): the entry point is
declared, listed and exported; the header is still plain C99; examples/wideband_room.c builds against the library alone;
and, compile-only as tests/test_bridge_legs_cpu.py does it, the kernel that runs a leg above the mix spills nothing, uses
no scratch memory and keeps its static LDS inside what creation budgets."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kernel_remarks
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "mi_bridge_create_endpoints"
KERNEL = "bridge_updown_kernel"
OLD_KERNELS = ("bridge_tick_kernel", "bridge_rated_kernel", "bridge_legs_kernel")


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


def test_header_is_still_plain_c99(tmp_path):
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_bridge.h"\n'
                     "int main(void) { mi_bridge *b = 0; int i = 0, o = 0; mi_bridge_config c;\n"
                     "  const mi_bridge_leg legs[2] = {{8000, MI_SESSION_PCMU, MI_SESSION_PCMA}, {48000, MI_SESSION_PCM16, MI_SESSION_PCM16}};\n"
                     "  mi_bridge_default_config(&c);\n"
                     "  c.rate = 16000;\n"
                     "  return mi_bridge_create_endpoints(0, &c, legs, &b) == MI_OK || mi_bridge_leg_bytes(b, 1, &i, &o) == MI_OK ||\n"
                     "         mi_bridge_leg_rate(b, 1) == 48000 || i + o; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o",
                        str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_wideband_room_example_builds(tmp_path):
    """examples/wideband_room.c builds as C99 against libmsmi355x.so alone, the way gateway_bridge.c does"""
    pkg = os.path.join(ROOT, "mediastreamer2_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "wideband_room.c"), "-L", pkg, "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o",
                        str(tmp_path / "wideband_room")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def remarks():
    return kernel_remarks.remarks("bridge.hip")


def test_updown_kernel_spills_nothing_and_fits_the_lds_budget(remarks):
    """one kernel, codec and direction per-member data; mi_bridge_create_endpoints accepts a shape when its dynamic LDS +
    RATED_STATIC_LDS <= 64 KB, so the kernel's static LDS must stay inside that constant"""
    budget = kernel_remarks.bridge_budget()[0]
    found = kernel_remarks.usages(remarks, KERNEL)
    assert len(found) == 1, [n for n, _ in found]
    name, u = found[0]
    assert not any(old in name for old in OLD_KERNELS), name  # the older kernels' pins count instantiations by these names
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
    assert int(u["LDS Size [bytes/block]"]) <= budget, u
