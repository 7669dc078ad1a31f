"""Records tests/golden/resample_bits.json: one SHA-256 per (case, tick) of what mediastreamer2_amd.ResamplerBatch of the
build that is importable puts out for the cases of tests/resample_bits.py.  Run on the GPU, against a build of the commit
the batch kernels are to be pinned to:
    python3 tests/golden/make_resample_bits.py <commit> [output.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import mediastreamer2_amd as ms  # noqa: E402
import resample_bits as rb  # noqa: E402

commit = sys.argv[1]
dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "resample_bits.json")
ctx = ms.Context(0)
cases = {rb.case_key(c): rb.case_hashes(ms, torch, ctx, c) for c in rb.CASES}
ctx.close()
with open(dst, "w") as f:
    json.dump({"commit": commit, "ticks": rb.TICKS, "cases": cases}, f, indent=1)
    f.write("\n")
print(len(cases), "cases ->", dst)
