"""What creating a bridge decides before it allocates (csrc/bridge_plan.hpp: refusals, kernel family, LDS, pitches), run
without a GPU and without the library: tests/host/bridge_plan_check.cpp, built here with AddressSanitizer + UBSan and run as
a child process, one run per shape.  The expectations are those of the six GPU test_refusals / test_geometry functions and of
tests/test_gpu_bridge_families.py, under the same rules and legs; those tests stay, this one needs no GPU.  The concealer's
own refusals (a leg outside 8 - 48 kHz, a transform radix above 17) are mi_plc_check_rate's in plc.hip, which the plan
calls and the program stands in for: they are not repeated here."""
import os
import subprocess

import pytest

from kernel_remarks import bridge_lds as lds_total

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "bridge_plan_check.cpp")
PCM16, PCMA, PCMU = 0, 1, 2  # MI_SESSION_* (include/msmi355x.h)
MI_EINVAL, MI_ENOTSUP = -1, -4
P16, ULAW = (PCM16, PCM16), (PCMU, PCMU)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bridge_plan") / "bridge_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(rules, conf, members, legs, plc=False):
        """-> (return code, the error text or {name: value} of the plan)"""
        r = subprocess.run([str(exe), rules, str(conf), str(members), str(int(plc))] + [f"{a}:{b}:{c}" for a, b, c in legs],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]  # a sanitizer's report ends the program and is its stderr
        code, _, rest = r.stdout.strip().partition(" ")
        return int(code), (rest if int(code) else dict(kv.split("=") for kv in rest.split()))
    return run


ok8, ok16, ok48 = [(8000, *ULAW)] * 6, [(16000, *P16)] * 6, [(48000, *P16)] * 6
at = lambda rate, n, pair=ULAW: [(rate, *pair)] * n
GATEWAY16 = [(8000, PCMU, PCMU), (8000, PCMA, PCMU), (16000, PCM16, PCM16)]  # tests/test_gpu_bridge_concealed.py's, the first three
# (what the text must contain, rules, conference rate, members, legs, plc), file by file
REFUSALS = [
    # test_gpu_bridge.py
    (["11025"], "create", 11025, 3, at(11025, 6), False),
    # test_gpu_bridge_rates.py
    ([16000], "rated", 8000, 3, at(8000, 5) + at(16000, 1), False),
    (["ratio 4"], "rated", 32000, 3, at(32000, 5) + at(8000, 1), False),
    ([1.5], "rated", 24000, 3, at(24000, 5) + at(16000, 1), False),
    ([16000], "rated", 48000, 3, at(8000, 5) + at(16000, 1), True),
    (["LDS"], "rated", 48000, 50, at(8000, 50), False),
    # test_gpu_bridge_legs.py
    (["leg 5 names codec 7"], "legs", 8000, 3, ok8[:5] + [(8000, PCMU, 7)], False),
    (["leg 3 names codec -1"], "legs", 8000, 3, ok8[:3] + [(8000, -1, PCMU)] + ok8[4:], False),
    (["leg 4"], "legs", 8000, 3, ok8[:4] + [(8000, PCMA, PCMU)] + ok8[5:], True),
    (["leg 5 at 16000"], "legs", 8000, 3, ok8[:5] + [(16000, *P16)], False),
    (["leg 5 at 8000 Hz in a 32000 Hz conference is ratio 4"], "legs", 32000, 3, at(32000, 5, P16) + [(8000, *ULAW)], False),
    # test_gpu_bridge_endpoints.py
    (["leg 5 at 32000", "ratio 4"], "endpoints", 8000, 3, ok8[:5] + [(32000, *P16)], False),
    (["leg 2 at 24000", "1.5"], "endpoints", 16000, 3, ok16[:2] + [(24000, *P16)] + ok16[3:], False),
    (["leg 5 at 44100"], "endpoints", 8000, 3, ok8[:5] + [(44100, *P16)], False),
    (["leg 4's rate 4400"], "endpoints", 8800, 3, at(8800, 4, P16) + at(4400, 2, P16), False),
    (["leg 5 names codec 7"], "endpoints", 8000, 3, ok8[:5] + [(16000, PCMU, 7)], False),
    ([16000, 48000], "endpoints", 8000, 3, at(16000, 5, P16) + at(48000, 1, P16), True),
    (["LDS", "50 members x 480 samples"], "endpoints", 8000, 50, at(48000, 50, P16), False),
    (["leg 5 at 16000 Hz is above"], "legs", 8000, 3, ok8[:5] + [(16000, *P16)], False),
    # test_gpu_bridge_concealed.py
    (["leg 4 names codec 3"], "concealed", 16000, 3, at(16000, 4) + [(16000, 3, PCMU), (16000, *P16)], True),
    (["the concealer batch sits behind one decoder"], "endpoints", 16000, 3, GATEWAY16 * 2, True),
    (["the concealer batch has one rate"], "rated", 16000, 3, [(8000, *ULAW), (16000, *ULAW)] * 3, True),
    # test_gpu_bridge_rational.py
    (["leg 5 at 44100"], "rational", 8000, 3, ok8[:5] + [(44100, *P16)], False),
    (["leg 4 at 32000", "1.333"], "rational", 24000, 3, at(24000, 4, P16) + at(32000, 2, P16), False),
    (["leg 5 at 32000", "ratio 4"], "rational", 8000, 3, ok8[:5] + [(32000, *P16)], False),
    (["leg 4's rate 1200"], "rational", 800, 3, at(800, 4, P16) + at(1200, 2, P16), False),
    (["leg 4's rate 4400"], "rational", 8800, 3, at(8800, 4, P16) + at(4400, 2, P16), False),
    (["leg 5 names codec 3"], "rational", 8000, 3, ok8[:5] + [(12000, PCMU, 3)], False),
    (["leg 2 at 24000", "1.5"], "endpoints", 16000, 3, ok16[:2] + [(24000, *P16)] + ok16[3:], False),
    (["leg 2 at 24000", "1.5"], "concealed", 16000, 3, ok16[:2] + [(24000, *P16)] + ok16[3:], False),
]


@pytest.mark.parametrize("values,rules,conf,members,legs,plc", REFUSALS, ids=[f"{r[1]}-{r[0][0]}" for r in REFUSALS])
def test_refusals(plan, values, rules, conf, members, legs, plc):
    code, text = plan(rules, conf, members, legs, plc)
    assert code == MI_ENOTSUP, text
    for v in values:
        assert str(v) in text, text


def test_what_the_refused_shapes_turn_into_when_legal(plan):
    """the `legal without ...` halves of those tests, and members that do not divide the streams"""
    assert plan("create", 8000, 3, at(8000, 7))[0] == MI_EINVAL
    assert plan("rated", 16000, 3, at(8000, 6))[0] == 0
    assert plan("endpoints", 8000, 3, ok8[:5] + [(16000, *P16)])[1]["tick_bytes"] == "320,320"
    assert plan("rational", 48000, 3, ok48[:5] + [(72000, *P16)])[1]["tick_bytes"] == "1440,1440"
    assert plan("rational", 16000, 3, ok16[:2] + [(24000, *P16)] + ok16[3:])[1]["tick_bytes"] == "480,480"
    room = at(16000, 3) + [(96000, *P16)] + at(16000, 2, P16)
    assert plan("concealed", 16000, 3, room)[1]["tick_bytes"] == "1920,1920"


# tests/test_gpu_bridge_families.py: two 16 kHz conferences of four 16 kHz PCM16 legs, stream 4 choosing the kernel
FAMILIES = {
    "TICK": ("create", (16000, *P16)),
    "RATED": ("rated", (8000, *P16)),
    "LEGS": ("legs", (16000, PCMA, PCMA)),
    "LEGS_RATED": ("legs", (8000, PCMU, PCMU)),
    "UPDOWN": ("endpoints", (48000, *P16)),
    "RATIONAL": ("rational", (24000, *P16)),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_family(plan, family):
    rules, leg4 = FAMILIES[family]
    legs = at(16000, 8, P16)
    legs[4] = leg4
    code, p = plan(rules, 16000, 4, legs)
    assert code == 0 and p["family"] == family, p


@pytest.mark.parametrize("conf,room,cap", [(48000, [(32000, *P16), (48000, *P16)], 43), (16000, [(24000, *P16), (48000, *P16)], 45)])
def test_member_caps_of_the_header(plan, conf, room, cap):
    """include/msmi355x_bridge.h: 32 kHz legs in a 48 kHz conference, up to 43 members; 24 kHz legs in a 16 kHz room that also
    holds 48 kHz members, up to 45.  The cap is planned, one more is refused; 2048 bytes are the kernel's own"""
    wide = max(r for r, _, _ in room) // 100
    code, p = plan("rational", conf, cap, (room * cap)[:cap])
    assert code == 0 and p["family"] == "RATIONAL" and int(p["lds"]) == lds_total(conf, [r for r, _, _ in room], cap) <= 65536 - 2048, p
    code, text = plan("rational", conf, cap + 1, (room * (cap + 1))[:cap + 1])
    assert code == MI_ENOTSUP and "LDS" in text and f"{cap + 1} members x {wide} samples" in text, text
    assert lds_total(conf, [r for r, _, _ in room], cap + 1) > 65536 - 2048


GEOMETRY = [  # (rules, conference rate, members, legs, tick_bytes): the shapes of the three GPU test_geometry functions
    ("rational", 48000, 3, [(8000, *ULAW), (32000, *P16), (48000, *P16)] * 2, (960, 960)),
    ("rational", 16000, 3, [(24000, PCMU, PCM16), (16000, *ULAW), (8000, PCMA, PCMA)], (240, 480)),
    ("create", 8000, 3, at(8000, 6, (PCMA, PCMU)), (80, 80)),
    ("endpoints", 16000, 3, [(8000, *ULAW), (16000, *P16), (48000, *P16)] * 2, (960, 960)),
    ("rated", 48000, 3, [(r, *P16) for r in (8000, 16000, 48000, 8000, 8000, 16000)], (960, 960)),
    ("rated", 48000, 3, at(8000, 6), (80, 80)),
]


@pytest.mark.parametrize("rules,conf,members,legs,tick_bytes", GEOMETRY, ids=[f"{g[0]}-{g[1]}-{g[4][0]}" for g in GEOMETRY])
def test_geometry(plan, rules, conf, members, legs, tick_bytes):
    code, p = plan(rules, conf, members, legs)
    assert code == 0 and tuple(int(v) for v in p["tick_bytes"].split(",")) == tick_bytes, p
    assert int(p["lds"]) == lds_total(conf, [r for r, _, _ in legs], members), p
