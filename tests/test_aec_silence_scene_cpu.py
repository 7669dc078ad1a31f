"""The premise of tests/test_gpu_aec_silence.py, pinned on the oracle alone (no GPU): when both pins of the echo scene go
to exact zero after a few active frames, the library's canceller -- restated by the oracle as the reference's x86 float
build evaluates it, subnormals kept -- runs for more than a hundred frames on subnormal state, all of E among it, stays
finite and never reaches `adapted`.  So "bit for bit until adaptation" holds through the whole scene and there is
something to compare.  Measured (scene 1; 6 / 10 active frames, 1.5 s of zeros, 6 frames back; no active_frames had to change):

  rate / F / tail          first subnormal word      frames holding one   most subnormal words in E (E has) / in the state
   8 kHz /  64 / 128 ms    13 / 13 frames into the zeros   175 / 175         128 ( 128) /  130
  16 kHz / 128 / 128 ms    34 / 34                         154 / 154         256 ( 256) /  259
  48 kHz / 256 / 128 ms    37 / 38                         244 / 243         512 ( 512) /  515
  48 kHz / 512 / 128 ms    19 / 19                         122 / 122        1024 (1024) / 1027
  16 kHz / 128 / 512 ms    34 / 34                         154 / 154         256 ( 256) /  259
  96 kHz / 512 / 128 ms    19 / 19                         262 / 262        1024 (1024) / 1027

`adapted` is never set and every state word stays finite in all twelve runs (-s prints the figures)."""
import numpy as np
import pytest

import aec_silence as sil


@pytest.fixture(scope="module")
def orc():
    import oracle
    oracle.build()
    oracle.lib()
    return oracle


@pytest.mark.parametrize("rate,F,tail_ms", sil.GEOMETRIES)
@pytest.mark.parametrize("active", sil.ONSETS)
def test_silence_premise(orc, rate, F, tail_ms, active):
    mic, far, span = sil.silence_scene(1, rate, F, active, sil.SILENT_S, sil.BACK_FRAMES, "both")
    assert not mic[span[0] * F:span[1] * F].any() and not far[span[0] * F:span[1] * F].any()
    assert mic[:span[0] * F].any() and far[span[1] * F:].any()
    run = sil.oracle_run(orc, rate, F, tail_ms, mic, far)
    first = int(np.argmax(run["sub"] > 0))
    print(f"\n{rate} / {F} / {tail_ms} ms, {active} active: first subnormal word {first - span[0]} frames into the zeros, "
          f"{int((run['sub'] > 0).sum())} frames hold one, most in E {int(run['sub_E'].max())} of {2 * F}, most in the state {int(run['sub'].max())}")
    sil.assert_premise(run, F, f"{rate}/{F}/{tail_ms}/{active}")
    assert span[0] <= first < span[1], "the first subnormal word appears during the zeros"
    assert run["out"][span[1] * F:].any(), "the canceller's output is not silence after the return"


@pytest.mark.parametrize("mode,most", [("mic", 8), ("far", 0)])
def test_one_pin_at_zero_leaves_the_spectra_normal(orc, mode, most):
    """only the microphone at zero: a few scalars go subnormal (and the filter, still fed by the far end, goes on to adapt:
    such a leg leaves the bit-for-bit contract at that frame); only the far end at zero: nothing goes subnormal and the
    canceller never adapts"""
    rate, F, tail_ms = 16000, 128, 128
    mic, far, span = sil.silence_scene(1, rate, F, 6, sil.SILENT_S, sil.BACK_FRAMES, mode)
    run = sil.oracle_run(orc, rate, F, tail_ms, mic, far)
    assert not run["nonfinite"].any()
    assert run["sub_E"].max() == 0 and run["sub"].max() <= most, (int(run["sub_E"].max()), int(run["sub"].max()))
    if mode == "mic":
        assert run["sub"].max() >= 2
    else:
        assert not run["adapted"].any()


def test_count_words():
    a = np.array([0.0, -0.0, 1e-39, -1e-45, sil.TINY, 1.0, np.inf, np.nan], np.float32)
    assert sil.count_words(a) == (2, 2)
