#!/usr/bin/env python3
"""Generates tests/golden/g711.npz: the reference's own G.711 conversions over their whole domain.

The values come from oracle/_ref/libg711_ref.so, the reference's src/audiofilters/g711.c compiled unmodified by
oracle/build_ref.sh, which needs the reference tree.  The fixture holds outputs only (every int16 PCM value from -32768 up
encoded per law, every code word from 0 up decoded per law), so the tests compare against the reference build wherever they run.
Run `python tests/golden/make_g711_golden.py` from the repo root after oracle/build_ref.sh has built oracle/_ref.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    R = oracle.g711_ref()
    if R is None:
        sys.exit("make_g711_golden.py: oracle/_ref/libg711_ref.so is not built (oracle/build_ref.sh)")
    pcm = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    codes = np.arange(256, dtype=np.uint8)
    np.savez_compressed(
        os.path.join(HERE, "g711.npz"),
        alaw_encode=np.array([R.Snack_Lin2Alaw(int(v)) for v in pcm], np.uint8),
        ulaw_encode=np.array([R.Snack_Lin2Mulaw(int(v)) for v in pcm], np.uint8),
        alaw_decode=np.array([R.Snack_Alaw2Lin(int(c)) for c in codes], np.int16),
        ulaw_decode=np.array([R.Snack_Mulaw2Lin(int(c)) for c in codes], np.int16))


if __name__ == "__main__":
    main()
