"""CPU-side checks of the bridge's legs at their own rate (mi_bridge_create_rated): the two new entry points are declared,
listed and exported; the header is still plain C99; and, compile-only as tests/test_kernel_resources_cpu.py does it, the
rated kernel spills nothing and keeps its static LDS inside what mi_bridge_create_rated budgets for it, while the same-rate
kernel is built exactly as before."""
import os
import re
import subprocess

import pytest

import kernel_remarks
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi_bridge_create_rated", "mi_bridge_leg_rate")

# (VGPRs, static LDS bytes) of bridge_tick_kernel<IN, OUT> per input kind, recorded from a build of the commit BEFORE the rated
# kernel was added (same flags): the same-rate path must not pay for the feature
PARENT_TICK = {0: (67, 1216), 1: (72, 1216), 2: (69, 1216)}


def test_new_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "msmi355x_bridge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in msmi355x_bridge.h"
        assert name in _lib.BRIDGE_EXPORTS
        assert re.search(rf"\sT {name}$", out, flags=re.M), f"{name} is not defined in the built library"
    L = _lib.load()
    assert L.mi_bridge_create_rated.argtypes is not None and L.mi_bridge_leg_rate.argtypes is not None
    assert L.mi_bridge_leg_rate(None, 0) == _lib.MI_EINVAL
    assert L.mi_abi_version() == 3


def test_header_is_still_plain_c99(tmp_path):
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_bridge.h"\n'
                     "int main(void) { mi_bridge *b = 0; const int32_t r[2] = {8000, 8000}; mi_bridge_config c; mi_bridge_default_config(&c);\n"
                     "  return mi_bridge_create_rated(0, &c, r, &b) == MI_OK || mi_bridge_leg_rate(b, 0) >= 0; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(probe), "-o",
                        str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def remarks():
    return kernel_remarks.remarks("bridge.hip")


def test_rated_kernel_spills_nothing_and_fits_its_lds_budget(remarks):
    """mi_bridge_create_rated accepts a shape when its dynamic LDS + RATED_STATIC_LDS <= 64 KB: every instantiation's static
    LDS must stay inside that constant, so the largest accepted shape is inside 64 KB"""
    budget, limit, src = kernel_remarks.bridge_budget()
    assert limit == 65536 and "lds + RATED_STATIC_LDS > BRIDGE_LDS_MAX" in src
    rated = kernel_remarks.usages(remarks, "bridge_rated_kernel")
    assert len(rated) == 9, [n for n, _ in rated]
    for name, u in rated:
        assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
        assert int(u["LDS Size [bytes/block]"]) <= budget, (name, u)


def test_same_rate_kernel_is_built_as_before(remarks):
    tick = kernel_remarks.usages(remarks, "bridge_tick_kernel")
    assert len(tick) == 9, [n for n, _ in tick]
    for name, u in tick:
        kind = int(re.search(r"bridge_tick_kernelILi(\d)ELi\dE", name).group(1))
        assert (int(u["VGPRs"]), int(u["LDS Size [bytes/block]"])) == PARENT_TICK[kind], (name, u)
        assert int(u["VGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
