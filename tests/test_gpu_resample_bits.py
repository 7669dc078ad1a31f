"""The batch resampler kernels pinned to the bits of the commit named in tests/golden/resample_bits.json (recorded there by
tests/golden/make_resample_bits.py): test_gpu_resample.py holds them within 1 LSB of the oracle and the bridge tests hold the
bridge bit-equal to them, so a summation order that changed on both sides at once would pass both.  Not here."""
import json
import os

import pytest

import mediastreamer2_amd as ms
import resample_bits as rb

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_recording_holds_every_case():
    assert GOLDEN["ticks"] == rb.TICKS
    assert sorted(GOLDEN["cases"]) == sorted(rb.case_key(c) for c in rb.CASES)
    assert len(rb.CASES) == 18 and all(len(v) == rb.TICKS for v in GOLDEN["cases"].values())


@pytest.mark.parametrize("case", rb.CASES, ids=rb.case_key)
def test_resampler_bits_are_the_recorded_ones(ctx, case):
    import torch
    want = GOLDEN["cases"][rb.case_key(case)]  # a case the recording lacks is a failure
    got = rb.case_hashes(ms, torch, ctx, case)
    assert got == want, f"{rb.case_key(case)}: ticks {[t for t in range(rb.TICKS) if got[t] != want[t]]} differ from commit {GOLDEN['commit']}"
