"""The canceller's tick kernel lives on three resource edges at once; a change that pushes it over any of them costs
performance silently, so the build is checked here (hipcc cross-compiles without a GPU):
  * 256 VGPRs = two waves per SIMD; not one register spilled to scratch at 48 kHz (F = 256);
  * at most 20 KB of LDS per wave = eight waves per CU;
  * under 64 KB of code: the instruction cache two CUs share (99.99 % hits measured at that size)."""
import os
import re
import subprocess

import pytest

from kernel_remarks import compile_unit, usages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    """a build of its own, not kernel_remarks.remarks': the code sizes are read off the object file"""
    d = tmp_path_factory.mktemp("aec_res")
    obj = d / "aec_dev.o"
    return d, obj, compile_unit("aec.hip", obj)


def test_tick_kernel_registers_and_lds(build):
    """every form of the tick kernel (rows / FIFOs / FIFOs + folded resampler: the MODE template parameter)"""
    _, _, remarks = build
    big = list(usages(remarks, "aec_tick_kernelILi256E"))
    assert len(big) == 3, [n for n, _ in big]
    for name, u in big:
        assert int(u["VGPRs"]) <= 256 and int(u["VGPRs Spill"]) == 0, (name, u)
        assert int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)  # (a scalar spilled to memory shows here alone, not as a VGPR spill)
        assert int(u["Occupancy [waves/SIMD]"]) == 2, (name, u)
        assert int(u["LDS Size [bytes/block]"]) <= 20480, (name, u)  # one wave per block: 8 per CU
    for k in ("aec_tick_kernelILi128E", "aec_tick_kernelILi64E"):
        found = usages(remarks, k)
        assert found, f"no remarks for {k}"
        for name, v in found:
            assert int(v["VGPRs Spill"]) <= 12, (name, v)  # the small frames run at 3 / 4 waves per SIMD: a handful of spills is the price


def test_tick_kernel_code_fits_the_instruction_cache(build):
    d, obj, _ = build
    dev = d / "aec_gfx950.o"
    r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={obj}",
                        "--targets=hip-amdgcn-amd-amdhsa--gfx950", f"--output={dev}"], capture_output=True, text=True)
    if r.returncode != 0 or not dev.exists():  # --cuda-device-only may already emit the bare code object
        dev = obj
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", str(dev)], capture_output=True, text=True).stdout
    sizes = {ln.split()[7]: int(ln.split()[2]) for ln in syms.splitlines() if " FUNC " in ln and "aec_tick_kernel" in ln}
    big = {k: v for k, v in sizes.items() if "ILi256E" in k}
    assert len(big) == 3, syms[-2000:]
    assert max(big.values()) < 65536, f"a form of aec_tick_kernel<256> is over the 64 KB instruction cache: {big}"
    headline = [v for k, v in big.items() if "ILi256ELi2E" in k]  # FIFOs + folded resampler: what the headline and the plugin's fused chain launch
    assert headline and headline[0] <= 64 * 1024 - 1536, f"the headline's form has less than 1.5 KB of instruction cache to spare: {headline}"


def test_group_kernels_registers_lds_and_code(build):
    """the small-frame cancellers with several legs per wavefront (aec_group.hpp): the per-leg scalars live in registers, so
    the kernels sit close to the 256 of two waves per SIMD -- nothing may spill to scratch; LDS for eight waves per CU; code
    inside the instruction cache"""
    d, obj, remarks = build
    for k in ("aec_group_kernelILi128E", "aec_group_kernelILi64E"):
        (name, u), = usages(remarks, k)
        assert int(u["VGPRs"]) <= 256 and int(u["VGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)
        assert int(u["Occupancy [waves/SIMD]"]) >= 2, (name, u)
        assert int(u["LDS Size [bytes/block]"]) <= 20480, (name, u)
    dev = d / "aec_gfx950.o"
    if not dev.exists():
        dev = obj
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", str(dev)], capture_output=True, text=True).stdout
    sizes = {ln.split()[7]: int(ln.split()[2]) for ln in syms.splitlines() if " FUNC " in ln and "aec_group_kernel" in ln}
    assert len(sizes) == 2 and max(sizes.values()) < 65536, sizes


# ---- the float mode of the built library

LIB = os.path.join(ROOT, "mediastreamer2_amd", "libmsmi355x.so")
MAKEFILE = os.path.join(ROOT, "mediastreamer2_amd", "csrc", "Makefile")
FLUSHING_FLAGS = ("-fgpu-flush-denormals-to-zero", "-ffast-math", "-Ofast", "-funsafe-math-optimizations")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernel_descriptors(tmp):
    """{kernel name: compute_pgm_rsrc1} of every kernel descriptor (the 64-byte `<kernel>.kd` objects) in the gfx950 code
    objects bundled into libmsmi355x.so: one offload bundle per .hip file, back to back in the .hip_fatbin section"""
    import struct
    fat = tmp / "fat.bin"
    r = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", LIB], capture_output=True, text=True)
    assert r.returncode == 0 and fat.exists(), r.stderr
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), blob)]
    assert starts, "no offload bundle in .hip_fatbin"
    out = {}
    for i, at in enumerate(starts):
        part, co = tmp / f"bundle{i}.bin", tmp / f"gfx950_{i}.co"
        part.write_bytes(blob[at:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True, text=True)
        assert r.returncode == 0 and co.exists() and co.stat().st_size > 0, r.stderr
        elf = co.read_bytes()
        sections = {}   # index -> (address, file offset)
        for ln in subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-SW", str(co)], capture_output=True, text=True).stdout.splitlines():
            m = re.match(r"\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s", ln)
            if m:
                sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
        for ln in subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", str(co)], capture_output=True, text=True).stdout.splitlines():
            f = ln.split()
            if len(f) == 8 and f[7].endswith(".kd") and f[3] == "OBJECT":
                assert int(f[2]) == 64, ln
                addr, off = sections[int(f[6])]
                kd = elf[int(f[1], 16) - addr + off:][:64]
                out[f[7][:-3]] = struct.unpack_from("<I", kd, 48)[0]   # compute_pgm_rsrc1: bytes 48..51 of the descriptor
    return out


def test_every_kernel_keeps_subnormals(tmp_path):
    """The canceller's state is subnormal for as long as a leg is digitally silent (tests/test_gpu_aec_silence.py), and the
    reference's x86 float build keeps those words: every kernel of the built library must run with float_denorm_mode_32 = 3 and
    float_denorm_mode_16_64 = 3 (compute_pgm_rsrc1 bits 16-17 and 18-19: denormals kept as sources and as results), which
    is hipcc's default -- and the Makefile must not name a flag that changes it."""
    if not os.path.exists(LIB):
        import __graft_entry__ as entry
        entry.build()
    kds = kernel_descriptors(tmp_path)
    assert len(kds) >= 30, sorted(kds)
    for want in ("aec_tick_kernel", "aec_group_kernel", "volume", "mix", "resampl", "fifo"):
        assert any(want in k for k in kds), f"no descriptor of a {want} kernel found: {sorted(kds)[:8]}"
    wrong = {k: ((v >> 16) & 3, (v >> 18) & 3) for k, v in kds.items() if (v >> 16) & 15 != 15}
    assert not wrong, f"(float_denorm_mode_32, float_denorm_mode_16_64) != (3, 3) in {len(wrong)} of {len(kds)} kernels: {sorted(wrong.items())[:4]}"
    text = open(MAKEFILE).read()
    assert not [f for f in FLUSHING_FLAGS if f in text], "csrc/Makefile names a flag that flushes subnormals or reorders float arithmetic"
