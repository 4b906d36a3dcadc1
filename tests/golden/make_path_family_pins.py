#!/usr/bin/env python3
"""Writes tests/golden/path_family_pins.json: the SHA-256 of what every case of tests/path_family_cases.py returns on
the device, the `hipcc --version` string of the toolchain that built the library, and what the cases exercise (QE
branches, jump counts) by the CPU restatements — asserted before anything is written.

Run on a GPU, on the library whose bits are to be held:  python tests/golden/make_path_family_pins.py
The fixture pins a state of csrc/; it is regenerated only by a change that MEANS to move the bits."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import hedgehog_jl_amd as hh  # noqa: E402
from tests import oracle_ffi  # noqa: E402
from tests import path_family_cases as pf  # noqa: E402


def main():
    seen = pf.seen(oracle_ffi.load())
    pf.check_seen(seen)
    doc = dict(toolchain=pf.toolchain(), n_paths=pf.N, seen=seen, pins=pf.compute(hh.get_context(0)))
    with open(pf.GOLDEN, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{pf.GOLDEN}: {len(doc['pins'])} cases")


if __name__ == "__main__":
    main()
