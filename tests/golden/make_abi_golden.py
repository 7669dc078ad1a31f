#!/usr/bin/env python3
"""Generates tests/golden/ms2_abi.json: what the reference's headers say about every id, enum value, method macro and
struct field list include/ms2_plugin_abi.h restates (tests/test_abi_against_reference_headers.py compares the two).

The headers are parsed, not copied: the fixture holds the parsed values for the names our header declares and nothing
else.  Run from the repo root with the root of a mediastreamer2 source tree:
    python tests/golden/make_abi_golden.py <mediastreamer2 source tree>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_abi_against_reference_headers as abi  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    inc = os.path.join(sys.argv[1], "include", "mediastreamer2")

    def read_ref(*names):
        out = []
        for n in names:
            with open(os.path.join(inc, n)) as f:
                out.append(abi.strip_comments(f.read()))
        return "\n".join(out)
    with open(os.path.join(HERE, "ms2_abi.json"), "w") as f:
        json.dump(abi.reference_facts(read_ref), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
