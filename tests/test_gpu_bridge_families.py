"""A conference's result does not depend on which kernel serves its bridge (csrc/bridge.hip composes its five kernels from
one set of phases): two 16 kHz conferences of four, the first four 16 kHz PCM16 legs in every variant, the first leg of the
second choosing the kernel by its rate and codec.  Whatever that leg is, the first conference's output rows, meter states and
levels are BIT-EQUAL to the plain bridge's on every tick, and the tail of a wider row is zeros."""
import numpy as np
import pytest

import mediastreamer2_amd as ms
from conftest import synth_pcm

pytestmark = pytest.mark.gpu

PCM16, PCMA, PCMU = ms.MI_SESSION_PCM16, ms.MI_SESSION_PCMA, ms.MI_SESSION_PCMU
L, A, O = ms.MI_MIX_LINKED, ms.MI_MIX_ACTIVE, ms.MI_MIX_OUTPUT
CONF, MM, N, NTICKS, ROW = 16000, 4, 8, 8, 320  # ROW: bytes of a 16 kHz PCM16 tick

# stream 4 as (rate, in_codec, out_codec), the constructor form, and the kernel that shape launches
VARIANTS = {
    "tick<0,0>": ((16000, PCM16, PCM16), None),
    "rated<0,0>": ((8000, PCM16, PCM16), "leg_rates"),
    "legs<false>": ((16000, PCMA, PCMA), "legs"),
    "legs<true>": ((8000, PCMU, PCMU), "legs"),
    "updown": ((48000, PCM16, PCM16), "endpoints"),
    "rational": ((24000, PCM16, PCM16), "rational"),
}


def _bridge(ctx, variant):
    leg4, form = VARIANTS[variant]
    legs = [(CONF, PCM16, PCM16)] * N
    legs[MM] = leg4
    kw = dict(members=MM, rate=CONF, in_codec=PCM16, out_codec=PCM16)
    if form == "leg_rates":
        kw[form] = [l[0] for l in legs]
    elif form:
        kw[form] = legs
    return ms.Bridge(ctx, N, **kw), leg4


def _run(ctx, variant):
    """8 ticks -> (conference 0's rows per tick as bytes at the bridge's pitch, its meter states' bytes, its levels)"""
    br, (rate4, in4, _) = _bridge(ctx, variant)
    try:
        params = [ms.VolumeBatch.default_params() for _ in range(N)]
        params[0].agc_enabled, params[0].remove_dc = 1, 1
        params[1].noise_gate_enabled = 1
        br.set_volume_params(params)
        flags = np.full(N, L | A | O, np.uint8)
        flags[3] = L | A  # its output off
        gain = np.ones(N, np.float32)
        gain[0] = 0.5
        br.set_controls(flags=flags, gain=gain)
        ns = CONF // 100
        sig = np.stack([synth_pcm(70 + s, ns * NTICKS, sigma=12000.0, rate=CONF) for s in range(N)])
        own4 = np.random.default_rng(0xFA4).integers(0, 256, (NTICKS, rate4 // 100 * (1 if in4 else 2)), dtype=np.uint8)
        rows = []
        for t in range(NTICKS):
            if t == 3:
                flags[1] = L | O  # inactive from here on
                br.set_controls(flags=flags)
            h_in, h_present = br.acquire()
            x = h_in.view(np.uint8).reshape(N, -1)
            x[:] = 0
            x[:, :ROW] = np.ascontiguousarray(sig[:, t * ns:(t + 1) * ns]).view(np.uint8)
            x[MM, :ROW] = 0
            x[MM, :own4.shape[1]] = own4[t]
            h_present[2] = t not in (2, 5)
            br.submit()
            rows.append(br.collect().view(np.uint8).reshape(N, -1)[:MM].copy())
        return rows, bytes(br.volume_state(0, MM)), br.levels()[:MM].copy()
    finally:
        br.close()


@pytest.fixture(scope="module")
def plain(ctx):
    rows, state, levels = _run(ctx, "tick<0,0>")
    pcm = np.stack(rows).view(np.int16)
    assert (np.abs(pcm.astype(np.int32)) >= 32767).any(), "the sum must saturate on some samples"
    assert all(r[[0, 1, 2]].any() and not r[3].any() for r in rows), "three pins hear the mix, the fourth's output is off"
    return rows, state, levels


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_conference_is_the_same_under_every_kernel(ctx, plain, variant):
    want_rows, want_state, want_levels = plain
    rows, state, levels = _run(ctx, variant)
    for t in range(NTICKS):
        assert rows[t].shape[1] >= ROW
        np.testing.assert_array_equal(rows[t][:, :ROW], want_rows[t], err_msg=f"tick {t}")
        assert not rows[t][:, ROW:].any(), f"tick {t}: the tail of a wider row is zeros"
    assert state == want_state
    np.testing.assert_array_equal(levels.view(np.uint32), want_levels.view(np.uint32))
