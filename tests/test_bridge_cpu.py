"""CPU-side checks of the bridge sessions' boundary: include/msmi355x_bridge.h, the BRIDGE_EXPORTS list and the built
library name the same symbols; msmi355x.h (and with it the host double's list) knows none of them; without a GPU a
bridge fails loudly (no CPU fallback)."""
import os
import re
import subprocess

import pytest

import mediastreamer2_amd as ms
from mediastreamer2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mediastreamer2_amd")


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", src)))


def test_bridge_header_and_export_list_agree():
    names = _declared("msmi355x_bridge.h")
    assert names and all(n.startswith("mi_bridge_") for n in names), names
    assert names == sorted(_lib.BRIDGE_EXPORTS)
    assert len(set(_lib.BRIDGE_EXPORTS)) == len(_lib.BRIDGE_EXPORTS)


def test_library_exports_every_bridge_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r"\b(mi_bridge_[a-z0-9_]+)\b", out))
    assert defined == set(_lib.BRIDGE_EXPORTS), sorted(defined ^ set(_lib.BRIDGE_EXPORTS))
    L = _lib.load()
    assert all(hasattr(L, s) for s in _lib.BRIDGE_EXPORTS)
    assert L.mi_abi_version() == 3


def test_main_header_declares_no_bridge_symbol():
    assert not [n for n in _declared("msmi355x.h") if n.startswith("mi_bridge")]
    assert not set(_lib.BRIDGE_EXPORTS) & set(_lib.EXPORTS)
    assert "mi_bridge" not in open(os.path.join(ROOT, "include", "msmi355x.h")).read()


def test_default_config_is_a_g711_bridge():
    cfg = ms.BridgeConfig()
    _lib.load().mi_bridge_default_config(ms.C.byref(cfg))
    assert (cfg.nstreams, cfg.members_per_conference, cfg.rate) == (1024, 32, 8000)
    assert (cfg.in_codec, cfg.out_codec, cfg.plc) == (ms.MI_SESSION_PCMU, ms.MI_SESSION_PCMU, 0)


def test_no_bridge_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(ms.MiError) as e:
        ms.Bridge(None, 6, members=3)
    assert e.value.code == _lib.MI_ENODEV


def test_bridge_header_is_plain_c_and_the_example_builds(tmp_path):
    """the header compiles as C99 on its own, and examples/g711_bridge.c builds against libmsmi355x.so alone; without a
    GPU it exits loudly instead of falling back"""
    cc = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "msmi355x_bridge.h"\nint main(void) { mi_bridge_config c; mi_bridge_default_config(&c); return c.rate != 8000; }\n')
    r = subprocess.run(cc + ["-c", str(probe), "-o", str(tmp_path / "hdr.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = tmp_path / "g711_bridge"
    r = subprocess.run(cc + [os.path.join(ROOT, "examples", "g711_bridge.c"), "-L", PKG, "-lmsmi355x", f"-Wl,-rpath,{PKG}", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    import torch
    if not torch.cuda.is_available():
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 1 and "no CPU fallback" in run.stderr
