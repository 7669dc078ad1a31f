"""CPU-side checks of loss concealment for legs of any rate and codec (mi_bridge_create_concealed): the entry point is
declared, listed and exported; the header is still plain C99; examples/lossy_gateway.c builds against the library alone;
and, compile-only as tests/test_bridge_endpoints_cpu.py does it for bridge.hip, the per-leg concealer's two kernels spill
nothing and use no scratch memory while the three older kernels of plc.hip keep the resources they had."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kernel_remarks
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "mi_bridge_create_concealed"
NEW_KERNELS = ("plc_legs_received_kernel", "plc_legs_conceal_kernel")
# (VGPRs, TotalSGPRs, LDS bytes / block, scratch bytes / lane, SGPRs spilled, VGPRs spilled) of plc.hip as of commit 7d53fc1,
# the parent of the per-leg concealer, from this same compile line.  plc_conceal_kernel's scratch is the generic
# butterfly's private float2[17]
PARENT = {
    "plc_list_kernel": (8, 21, 0, 0, 0, 0),
    "plc_received_kernel": (75, 38, 0, 0, 0, 0),
    "plc_conceal_kernel": (126, 106, 0, 144, 82, 0),
}


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


def test_the_per_leg_concealer_has_no_symbol_of_the_main_header():
    """it is reached through the bridge: the main header's concealer is the five calls it was"""
    assert sorted(n for n in _lib.EXPORTS if n.startswith("mi_plc_")) == ["mi_plc_create", "mi_plc_destroy", "mi_plc_info", "mi_plc_process",
                                                                           "mi_plc_reset"]


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
                     "  c.rate = 16000, c.plc = 1;\n"
                     "  return mi_bridge_create_concealed(0, &c, legs, &b) == MI_OK || mi_bridge_leg_bytes(b, 1, &i, &o) == MI_OK ||\n"
                     "         mi_bridge_leg_rate(b, 1) == 48000 || i + o; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o",
                        str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_lossy_gateway_example_builds(tmp_path):
    """examples/lossy_gateway.c builds as C99 against libmsmi355x.so alone, the way gateway_bridge.c does"""
    pkg = os.path.join(ROOT, "mediastreamer2_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "lossy_gateway.c"), "-L", pkg, "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o",
                        str(tmp_path / "lossy_gateway")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def remarks():
    return kernel_remarks.remarks("plc.hip")


@pytest.mark.parametrize("kernel", NEW_KERNELS)
def test_new_kernels_spill_nothing_and_use_no_scratch(remarks, kernel):
    found = kernel_remarks.usages(remarks, kernel)
    assert len(found) == 1, [n for n, _ in found]
    name, u = found[0]
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)


@pytest.mark.parametrize("kernel", sorted(PARENT))
def test_older_kernels_keep_their_resources(remarks, kernel):
    found = kernel_remarks.usages(remarks, f"{len(kernel)}{kernel}E")  # the mangled name: its length, the name, the end of the nested name
    assert len(found) == 1, [n for n, _ in found]
    name, u = found[0]
    got = tuple(int(u[k]) for k in ("VGPRs", "TotalSGPRs", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill"))
    assert got == PARENT[kernel], (name, u)
