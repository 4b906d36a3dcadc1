#!/usr/bin/env python3
"""Writes tests/golden/route_pins.json: a SHA-256 of what every case of tests/route_cases.py sends to the C-ABI and gets
back, through the recording context (no GPU, nothing is simulated), and every refusal's text.

The file pins the host's behaviour as it stood before the routes were stated in one table.  It is not regenerated: to
check it, run this script in a checkout of the commit before that change, with this script and tests/route_cases.py copied
in, and compare bytes.  Both use the package's public names only.  --full PATH also writes the records themselves."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import route_cases as rc  # noqa: E402


def main():
    records = rc.compute()
    with open(rc.GOLDEN, "w") as f:
        f.write(rc.dump(rc.pins(records)))
    if "--full" in sys.argv:
        with open(sys.argv[sys.argv.index("--full") + 1], "w") as f:
            json.dump(records, f, indent=0, sort_keys=True)
    print(f"{rc.GOLDEN}: {len(records)} records, {sum(1 for r in records.values() if 'raises' in r)} of them refusals")


if __name__ == "__main__":
    main()
