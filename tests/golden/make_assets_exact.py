"""Writes tests/golden/assets_exact.json: the closed forms of the multi-asset tests (tests/assets_cases.py) at 50 digits,
the bivariate normal by quadrature.  CPU only.

  cases     (a), (b) and (e) of tests/assets_cases.py as they stand there: spots, sigmas, weights, correlation, r, T
  prices    per case and closed form, 40 digits: the price, and the price with every off-diagonal correlation set to 0 —
            the reading a simulation on uncorrelated draws would converge to, which the device tests hold their prices
            away from

The issue's table (double precision, five decimals) is asserted against both columns here.

Run from the repository root:  python tests/golden/make_assets_exact.py
"""
import json
import os
import sys

import mpmath as mp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import assets_cases as ac  # noqa: E402


def build():
    prices = {}
    for cid, case in ac.CASES.items():
        full, flat = ac.closed_forms(cid, case), ac.closed_forms(cid, ac.uncorrelated(case))
        with mp.workdps(ac.DPS):
            prices[cid] = {name: dict(price=mp.nstr(full[name], 40), rho0=mp.nstr(flat[name], 40)) for name in full}
        for name in full:
            if (cid, name) in ac.ISSUE_TABLE:
                want, want0 = ac.ISSUE_TABLE[cid, name]
                assert abs(float(full[name]) - want) < 6e-6 and abs(float(flat[name]) - want0) < 6e-6, (cid, name, full[name], flat[name])
    return dict(note="written by tests/golden/make_assets_exact.py; see its docstring", digits=40, asian_shape=list(ac.ASIAN_SHAPE),
                cases=ac.CASES, prices=prices)


def main():
    doc = build()
    with open(ac.GOLDEN, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(ac.GOLDEN, os.path.getsize(ac.GOLDEN), "bytes")
    for cid, rows in doc["prices"].items():
        for name, rec in rows.items():
            print(cid, name, rec["price"][:12], rec["rho0"][:12])


if __name__ == "__main__":
    main()
