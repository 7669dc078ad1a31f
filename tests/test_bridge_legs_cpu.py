"""CPU-side checks of the bridge's legs with their own codec (mi_bridge_create_legs): the three new entry points are declared,
listed and exported; the header is still plain C99; and, compile-only as tests/test_bridge_rates_cpu.py does it, the
kernels of the mixed case spill nothing and the one with the resamplers keeps its static LDS inside what creation budgets."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kernel_remarks
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi_bridge_create_legs", "mi_bridge_leg_codec", "mi_bridge_leg_bytes")
KERNEL = "bridge_legs_kernel"  # <false>: legs at the conference's rate; <true>: with the two resamplers


def test_new_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "msmi355x_bridge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in msmi355x_bridge.h"
        assert name in _lib.BRIDGE_EXPORTS
        assert re.search(rf"\sT {name}$", out, flags=re.M), f"{name} is not defined in the built library"
    assert re.search(r"typedef\s+struct\s+mi_bridge_leg\s*\{[^}]*\brate\b[^}]*\bin_codec\b[^}]*\bout_codec\b[^}]*\}\s*mi_bridge_leg\s*;", code)
    L = _lib.load()
    assert all(getattr(L, name).argtypes is not None for name in NEW)
    assert L.mi_abi_version() == 3


def test_null_bridge_is_einval():
    L = _lib.load()
    a, b = C.c_int32(-7), C.c_int32(-7)
    assert L.mi_bridge_leg_codec(None, 0, C.byref(a), C.byref(b)) == _lib.MI_EINVAL
    assert L.mi_bridge_leg_bytes(None, 0, C.byref(a), C.byref(b)) == _lib.MI_EINVAL
    assert L.mi_bridge_leg_codec(None, 0, None, None) == _lib.MI_EINVAL
    assert (a.value, b.value) == (-7, -7)


def test_header_is_still_plain_c99(tmp_path):
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_bridge.h"\n'
                     "int main(void) { mi_bridge *b = 0; int i = 0, o = 0; mi_bridge_config c;\n"
                     "  const mi_bridge_leg legs[2] = {{8000, MI_SESSION_PCMU, MI_SESSION_PCMA}, {16000, MI_SESSION_PCM16, MI_SESSION_PCM16}};\n"
                     "  mi_bridge_default_config(&c);\n"
                     "  return mi_bridge_create_legs(0, &c, legs, &b) == MI_OK || mi_bridge_leg_codec(b, 0, &i, &o) == MI_OK ||\n"
                     "         mi_bridge_leg_bytes(b, 1, &i, &o) == MI_OK || i + o; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o",
                        str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_gateway_example_builds(tmp_path):
    """examples/gateway_bridge.c builds as C99 against libmsmi355x.so alone, the way g711_bridge.c does"""
    pkg = os.path.join(ROOT, "mediastreamer2_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "gateway_bridge.c"), "-L", pkg, "-lmsmi355x", f"-Wl,-rpath,{pkg}", "-o",
                        str(tmp_path / "gateway_bridge")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def remarks():
    return kernel_remarks.remarks("bridge.hip")


def test_mixed_kernels_spill_nothing_and_fit_the_lds_budget(remarks):
    """one form without resamplers, one with; mi_bridge_create_legs accepts a rated shape when its dynamic LDS +
    RATED_STATIC_LDS <= 64 KB, so the rated form's static LDS must stay inside that constant"""
    budget = kernel_remarks.bridge_budget()[0]
    legs = dict(kernel_remarks.usages(remarks, KERNEL))
    plain = [n for n in legs if f"{KERNEL}ILb0E" in n]
    rated = [n for n in legs if f"{KERNEL}ILb1E" in n]
    assert len(legs) == 2 and len(plain) == 1 and len(rated) == 1, sorted(legs)
    for name, u in legs.items():
        assert "bridge_tick_kernel" not in name and "bridge_rated_kernel" not in name
        assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
    assert int(legs[rated[0]]["LDS Size [bytes/block]"]) <= budget, legs[rated[0]]
    assert int(legs[plain[0]]["LDS Size [bytes/block]"]) <= budget, legs[plain[0]]
