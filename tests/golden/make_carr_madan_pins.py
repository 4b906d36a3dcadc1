#!/usr/bin/env python3
"""Writes tests/golden/carr_madan_pins.json: the SHA-256 of what every case of tests/carr_madan_law_cases.py (part 2)
returns on the device, and the `hipcc --version` string of the toolchain that built the library.

Run on a GPU, on the library whose bits are to be held:  python tests/golden/make_carr_madan_pins.py
The fixture pins a state of csrc/hh_fourier.hip; it is regenerated only by a change that MEANS to move the bits."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import hedgehog_jl_amd as hh  # noqa: E402
from tests import carr_madan_law_cases as cl  # noqa: E402


def main():
    doc = dict(toolchain=cl.toolchain(), pins=cl.compute(hh.get_context(0)))
    with open(cl.GOLDEN, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{cl.GOLDEN}: {len(doc['pins'])} cases")


if __name__ == "__main__":
    main()
