"""The compiler's kernel-resource-usage remarks of a HIP unit, compile-only (hipcc cross-compiles without a GPU): one compile
per unit and pytest process, shared by every test module that asks about that unit's kernels."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mediastreamer2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]


def compile_unit(unit, obj):
    """compile csrc/<unit> device-only into obj -> the remarks (the compiler's stderr)"""
    r = subprocess.run([HIPCC, *FLAGS, "-c", os.path.join(CSRC, unit), "-o", str(obj)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


@functools.lru_cache(maxsize=None)
def remarks(unit):
    with tempfile.TemporaryDirectory(prefix="kernel_remarks_") as d:
        return compile_unit(unit, os.path.join(d, "dev.o"))


def usages(remarks, kernel_substr):
    """[(function name, {field: value})] of every remark block whose function name contains kernel_substr"""
    out = []
    for b in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = b.split()[0]
        if kernel_substr in name:
            out.append((name, {m.group(1).strip(): m.group(2).strip() for m in re.finditer(r"remark:\s+([A-Za-z /\[\]]+):\s+(\S+)", b)}))
    return out


def kernels(remarks):
    """(name, resource usage) of every __global__ function of the unit"""
    return usages(remarks, "kernel")


def bridge_budget():
    """(RATED_STATIC_LDS, BRIDGE_LDS_MAX, the source that holds them and the comparison that uses them)"""
    src = open(os.path.join(CSRC, "bridge_plan.hpp")).read()
    limit = re.search(r"BRIDGE_LDS_MAX\s*=\s*(\d+)\s*\*\s*(\d+)", src)
    return int(re.search(r"RATED_STATIC_LDS\s*=\s*(\d+)", src).group(1)), int(limit.group(1)) * int(limit.group(2)), src


def bridge_lds(conf, rates, mm):
    """the dynamic LDS of a conference of mm members whose legs' rates are `rates`, as the header's member caps
    are worked out: rows of the widest tick where a leg is above the mix at an odd number of 8-byte words, the int32 sum row, and
    with resamplers four wavefronts' scratch -- the largest form any leg needs"""
    up16 = lambda v: (v + 15) & ~15
    ns, wide = conf // 100, max(conf, max(rates)) // 100
    rated_plen = lambda num, in_len: ((num * 48 - 1 + in_len + num - 1) // num + 8 + 8 + 3) & ~3
    rational = lambda m, in_len: 2 * m * (((((24 * m - 1 + in_len + m - 1) // m) + 8 + 8 + 3) & ~3) | 4) * 4
    scratch = 0
    for r in set(rates):
        if 2 * r == 3 * conf:
            need = max(rational(3, ns // 2 * 3), rational(2, ns))
        elif 3 * r == 2 * conf:
            need = max(rational(2, ns // 3 * 2), rational(3, ns))
        elif r < conf:
            k = conf // r
            need = max(((47 + ns // k + 8 + 1 + 3) & ~3) * 4, (k * rated_plen(k, ns) + ns) * 4)
        elif r > conf:
            k = r // conf
            need = max(((47 + ns + 8 + 1 + 3) & ~3) * 4, (k * (rated_plen(k, k * ns) | 4) + k * ns) * 4)
        else:
            continue
        scratch = max(scratch, up16(need))
    rows = up16(mm * ((wide >> 2) | 1) * 8) + ns * 4
    return up16(rows) + 4 * scratch if scratch else rows
