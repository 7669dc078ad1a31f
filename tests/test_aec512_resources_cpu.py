"""The canceller's tick kernel at 512-sample frames (48 kHz with a frame-size setting of 86 to 170, 96 kHz with the default),
checked on the build as tests/test_kernel_resources_cpu.py checks the 256-sample forms (hipcc cross-compiles without a GPU):
  * all three forms (rows / FIFOs / FIFOs + folded resampler) exist;
  * one wave per SIMD, and not one register spilled to scratch (the VGPR and AGPR files together hold the tick's state);
  * at most 40 KB of LDS per wave: four waves per CU fit in its 160 KiB;
  * each form under 64 KB of code (the instruction cache two CUs share).  The two real transforms are functions of their own
    at this size, called from every place that needs one; they are counted on top and must keep the total under 72 KB."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mediastreamer2_amd", "csrc", "aec.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LLVM = "/opt/rocm/lib/llvm/bin"
FORMS = ("aec_tick_kernelILi512ELi0E", "aec_tick_kernelILi512ELi1E", "aec_tick_kernelILi512ELi2E")


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    d = tmp_path_factory.mktemp("aec512_res")
    obj = d / "aec_dev.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o", str(obj)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    dev = d / "aec_gfx950.o"
    r2 = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={obj}",
                         "--targets=hip-amdgcn-amd-amdhsa--gfx950", f"--output={dev}"], capture_output=True, text=True)
    if r2.returncode != 0 or not dev.exists():  # --cuda-device-only may already emit the bare code object
        dev = obj
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", str(dev)], capture_output=True, text=True).stdout
    sizes = {}
    for ln in syms.splitlines():
        if " FUNC " in ln:
            f = ln.split()
            sizes[f[7]] = int(f[2])
    return r.stderr, sizes


def usages(remarks, kernel_substr):
    out = []
    for b in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = b.split()[0]
        if kernel_substr in name:
            out.append((name, {m.group(1).strip(): m.group(2).strip() for m in re.finditer(r"remark:\s+([A-Za-z /\[\]]+):\s+(\S+)", b)}))
    return out


def test_the_three_512_forms_exist_without_spills_and_fit_four_per_cu(build):
    remarks, _ = build
    for k in FORMS:
        found = usages(remarks, k)
        assert len(found) == 1, (k, [n for n, _ in found])
        name, u = found[0]
        assert int(u["VGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
        assert int(u["Occupancy [waves/SIMD]"]) == 1, (name, u)
        assert int(u["LDS Size [bytes/block]"]) <= 40 * 1024, (name, u)


def test_the_512_forms_fit_the_instruction_cache(build):
    _, sizes = build
    forms = {k: v for k, v in sizes.items() if any(f in k for f in FORMS)}
    assert len(forms) == 3, sorted(sizes)
    assert max(forms.values()) < 65536, f"a form of aec_tick_kernel<512> is over the 64 KB instruction cache: {forms}"
    called = {k: v for k, v in sizes.items() if ("w_rfft_forward_lds" in k or "w_rfft_inverse_lds" in k) and "TLdsILi512E" in k}
    assert len(called) == 2, sorted(sizes)
    assert max(forms.values()) + sum(called.values()) < 72 * 1024, (forms, called)


def test_the_fft_debug_entry_has_a_512_form(build):
    remarks, _ = build
    (name, u), = usages(remarks, "fft_debug_kernelILi512E")
    assert int(u["VGPRs Spill"]) == 0, (name, u)
