#!/usr/bin/env python3
"""Generates tests/golden/reference_definitions.json: every name the reference's src/**/*.jl defines — struct /
function / abstract type / const / assignment / a line that starts with `name(` / a name re-imported by
`import M: …` — as a sorted list.  tests/test_julia_layout.py holds the names julia/*.jl takes from Hedgehog to
this list, so the check needs no copy of the reference.

    python tests/golden/make_reference_definitions.py <Hedgehog.jl checkout>"""
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def defines(src: str, name: str) -> bool:
    e = re.escape(name)
    return re.search(rf"(struct\s+{e}\b|function\s+{e}\b|^\s*{e}\s*\(|abstract type\s+{e}\b|const\s+{e}\b|"
                     rf"^\s*{e}\s*=|import \w+: .*\b{e}\b)", src, re.M) is not None


def main(ref_root: str) -> None:
    files = sorted(glob.glob(os.path.join(ref_root, "src", "**", "*.jl"), recursive=True))
    if not files:
        sys.exit(f"no Julia sources under {ref_root}/src")
    src = "\n".join(open(f).read() for f in files)
    tokens = set(re.findall(r"[A-Za-z_]\w*!?", src))
    tokens |= {t.rstrip("!") for t in tokens}
    names = sorted(t for t in tokens if defines(src, t))
    out = os.path.join(ROOT, "tests", "golden", "reference_definitions.json")
    with open(out, "w") as f:
        json.dump({"what": "names defined in the reference's src/**/*.jl (tests/golden/make_reference_definitions.py)",
                   "names": names}, f, indent=0)
        f.write("\n")
    print(f"{out}: {len(names)} names from {len(files)} files")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
