"""Compare kernels of two gfx950 assembly listings (hipcc --save-temps) function by function.

    python tools/compare_kernel_asm.py OLD.s NEW.s [--match SUBSTRING]

Prints, per kernel symbol present in OLD whose name contains SUBSTRING, whether its instruction lines in NEW are the
same line for line (comments, directives and local label numbers aside) and ends with a count.  Exit status 1 when any
differs or is missing."""
from __future__ import annotations

import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith("."):  # comments, directives, labels
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def main(argv):
    match = argv[argv.index("--match") + 1] if "--match" in argv else ""
    old, new = kernels(argv[1]), kernels(argv[2])
    names = [n for n in old if match in n]
    bad = 0
    for n in names:
        same = new.get(n) == old[n]
        bad += not same
        print(("same      " if same else "DIFFERENT ") + f"{len(old[n]):6d} lines  {n}")
    print(f"{len(names) - bad} of {len(names)} kernels identical line for line")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
