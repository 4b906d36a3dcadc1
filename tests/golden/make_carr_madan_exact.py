"""Writes tests/golden/carr_madan_exact.json: truncated Carr–Madan prices and gradients to 30 digits
(oracle/carr_madan_exact.py, mpmath at 50) and, next to each, `e64` — how far the same formulas in
numpy complex128 on a converged rule (oracle/carr_madan_fp64.py) land from it, i.e. fp64 rounding alone.

    python tests/golden/make_carr_madan_exact.py            # rewrite the file (minutes, <= 16 workers)
    python tests/golden/make_carr_madan_exact.py --check ID [ID ...]   # recompute these, compare

Each record: `inputs` as hex floats (S0, K, T, r_drift, discount, alpha, bound, sigma and, for Heston, V0,
kappa, theta, rho), `days` (T = days/365, so that the case can be posed with dates), `cp`, `price` (call, or put
by parity), `grad` (of the CALL, slots S0 V0 κ θ σ ρ r_drift discount) where the case has one, `e64`,
`e64_grad`, `settle` (the converged rule's last move under doubling, relative), `max_sheet` (0: the principal logarithm is the continuous one), `moment_all_T`.

The Heston cases keep the (α+1)-th moment finite for every T — κ − ρσ(α+1) > 0 and (κ − ρσ(α+1))² ≥
σ²α(α+1), asserted below — so that the strip of the transform does not narrow with T; the one exception is
the third Monte Carlo target, which the suite prices as the modelled project runs it (negative σ) and whose
moment is finite at its own expiry (asserted instead).
"""
from __future__ import annotations

import argparse
import json
import math
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mpmath as mp  # noqa: E402

from oracle import carr_madan_exact as exact  # noqa: E402
from oracle import carr_madan_fp64 as fp64  # noqa: E402

OUT = os.path.join(HERE, "carr_madan_exact.json")
DIGITS = 30
H = dict(V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7)   # the suite's Heston set


def heston(id_, alpha, bound, days=365, K=100.0, r=0.03, S0=100.0, cp=1.0, grad=False, **params):
    T = days / 365
    return dict(id=id_, dynamics="heston", S0=S0, K=K, T=T, days=days, r_drift=r, discount=math.exp(-r * T),
                alpha=alpha, bound=bound, cp=cp, grad=grad, **{**H, **params})


def lognormal(id_, alpha, bound, sigma, days=365, K=100.0, r=0.05, S0=100.0, cp=1.0, compat=False, grad=False):
    T = days / 365
    return dict(id=id_, dynamics="lognormal", S0=S0, K=K, T=T, days=days, r_drift=r, discount=math.exp(-r * T),
                alpha=alpha, bound=bound, cp=cp, grad=grad, sigma=sigma, compat_sqrt_alpha=compat)


def cases():
    c = [
        # the three targets of test_carr_madan_heston_targets
        heston("target_mc_heston", 1.0, 32.0, days=366, grad=True),
        heston("target_h252", 1.0, 400.0, days=365, grad=True),
        heston("target_q2", 1.0, 32.0, days=364, r=0.05, V0=1.5, kappa=0.04, theta=0.3, sigma=-0.6, rho=0.04),
        # alpha x bound, thinned to the cells that tell h/alpha apart; strikes and expiries spread over them
        heston("a0.1_b16", 0.1, 16.0, K=80.0, days=91),
        heston("a0.1_b32", 0.1, 32.0, K=125.0, grad=True),
        heston("a0.1_b100", 0.1, 100.0, K=60.0, days=1825, cp=-1.0),
        heston("a0.1_b400", 0.1, 400.0, days=20),
        heston("a0.1_b1000", 0.1, 1000.0, K=160.0, days=10950),
        heston("a0.1_b2000", 0.1, 2000.0, K=100.0, days=37),
        heston("a0.25_b32", 0.25, 32.0, K=160.0, days=1825),
        heston("a0.25_b100", 0.25, 100.0, K=80.0, grad=True),
        heston("a0.25_b400", 0.25, 400.0, K=100.0, days=91, cp=-1.0),
        heston("a0.25_b1000", 0.25, 1000.0, K=125.0, days=20),
        heston("a0.5_b100", 0.5, 100.0, K=60.0),
        heston("a0.5_b400", 0.5, 400.0, K=125.0, days=10950),
        heston("a0.5_b2000", 0.5, 2000.0, K=100.0, days=37),
        heston("a0.75_b100", 0.75, 100.0, K=160.0, days=91),
        heston("a0.75_b400", 0.75, 400.0, K=80.0, days=20),
        heston("a0.75_b1000", 0.75, 1000.0, K=100.0, days=1825, cp=-1.0),
        heston("a1_b16", 1.0, 16.0, K=125.0, days=1825),
        heston("a1_b100", 1.0, 100.0, K=60.0, days=91),
        heston("a1_b400_far_otm", 1.0, 400.0, K=160.0, days=20),
        heston("a1_b1000", 1.0, 1000.0, K=80.0, days=10950),
        heston("a1_b2000", 1.0, 2000.0, K=125.0, days=365),
        heston("a1.5_b400", 1.5, 400.0, K=100.0, days=91),
        heston("a1.5_b1000", 1.5, 1000.0, K=60.0, days=20),
        heston("a4_b16", 4.0, 16.0, K=100.0, days=1825),
        heston("a4_b1000", 4.0, 1000.0, K=160.0, days=365),
        heston("a4_b2000", 4.0, 2000.0, K=80.0, days=91, cp=-1.0),
        # vol of vol from tiny to large; the two smallest are where C = κθ/σ²·(…) cancels
        heston("sigma_0.001", 1.0, 32.0, sigma=0.001),
        heston("sigma_0.001_a0.75_b100", 0.75, 100.0, K=125.0, days=730, sigma=0.001),
        heston("sigma_0.01", 1.0, 32.0, K=80.0, sigma=0.01),
        heston("sigma_0.01_b100", 1.0, 100.0, K=100.0, days=1825, sigma=0.01, cp=-1.0),
        heston("sigma_0.05", 1.0, 32.0, K=125.0, days=730, sigma=0.05, grad=True),
        heston("sigma_1.2", 1.0, 100.0, K=100.0, days=365, sigma=1.2, grad=True),
        # 2κθ < σ²
        heston("feller_violated", 1.0, 100.0, K=80.0, days=730, V0=0.04, kappa=1.0, theta=0.04, sigma=0.6, rho=-0.5,
               grad=True),
        heston("rho_+0.95", 1.0, 100.0, K=125.0, days=365, kappa=3.0, sigma=0.4, rho=0.95, grad=True),
        heston("rho_-0.95", 1.5, 100.0, K=80.0, days=91, rho=-0.95),
        heston("r_negative", 1.0, 32.0, K=100.0, days=730, r=-0.01, grad=True),
        heston("T5_K125", 0.75, 100.0, K=125.0, days=1825, grad=True),
        heston("spot_2500", 1.0, 400.0, S0=2500.0, K=2600.0, days=365),
        # fast-decaying CFs: at bound 100 the truncated tail is < 1e-50, the host test prices them by Gil-Pelaez
        heston("gil_pelaez_K90", 1.0, 100.0, K=90.0, days=730, V0=0.09, kappa=2.0, theta=0.09, sigma=0.3, rho=-0.5),
        heston("gil_pelaez_K120", 1.5, 100.0, K=120.0, days=730, V0=0.09, kappa=2.0, theta=0.09, sigma=0.3, rho=-0.5,
               cp=-1.0),
        # the lognormal law; σ√T·bound >= 12 on the first six (tail < 1e-30: Black–Scholes to 1e-25)
        lognormal("ln_K80", 1.0, 32.0, 0.4, K=80.0),
        lognormal("ln_K100_put", 1.0, 32.0, 0.4, K=100.0, cp=-1.0),
        lognormal("ln_K125", 1.0, 32.0, 0.4, K=125.0, grad=True),
        lognormal("ln_730d", 1.0, 32.0, 0.4, K=110.0, days=730, grad=True),
        lognormal("ln_730d_compat", 1.0, 32.0, 0.4, K=110.0, days=730, compat=True, grad=True),
        lognormal("ln_r_negative", 1.5, 100.0, 0.25, K=90.0, days=1825, r=-0.01),
        lognormal("ln_a0.25_b400", 0.25, 400.0, 0.2, K=100.0, days=91),
        lognormal("ln_a1_b1000_compat", 1.0, 1000.0, 0.2, K=125.0, days=20, compat=True),
    ]
    assert len({x["id"] for x in c}) == len(c)
    for x in c:
        if x["dynamics"] != "heston":
            continue
        x["moment_all_T"] = exact.moment_exists_for_all_T(x["kappa"], x["sigma"], x["rho"], x["alpha"])
        assert x["moment_all_T"] or x["id"] == "target_q2", x["id"]
        assert exact.moment_exists_at(x["kappa"], x["sigma"], x["rho"], x["alpha"], x["T"]), x["id"]
    return c


def _call(task):
    case, name, sign = task
    info = {}
    if name is None:
        return exact.call_price(case, info), info.get("max_sheet", 0)
    moved, h = exact.shifted(case, name, sign)
    return exact.call_price(moved), h


def fp64_fields(c, price, grad):
    """e64, e64_grad, settle of one case: the worst of oracle/carr_madan_fp64.converged's rules against the exact
    price (mpf; a put's by the parity the entry points apply, in floats) and gradient (mpf list or None)."""
    with mp.workdps(exact.DPS):
        res, settle = fp64.converged(c, grad=grad is not None)
        calls = [x[0] for x in res] if grad is not None else res
        p64 = [x if c["cp"] > 0 else x - c["S0"] + c["K"] * c["discount"] for x in calls]
        out = dict(e64=mp.nstr(max(abs(mp.mpf(x) - price) for x in p64), 4), settle=settle)
        if grad is not None:
            out["e64_grad"] = [mp.nstr(max(abs(mp.mpf(float(x[1][j])) - grad[j]) for x in res), 4)
                               for j in range(len(grad))]
        return out


def compute(selected, workers=None):
    """The records of `selected` cases: every exact integral is one task of the pool (workers = 1: in this process)."""
    tasks = []
    for c in selected:
        tasks.append((c, None, 0))
        if c["grad"]:
            tasks += [(c, n, s) for n in exact.GRAD_SLOTS if n in c for s in (+1, -1)]
    tasks_sorted = sorted(range(len(tasks)), key=lambda i: -tasks[i][0]["bound"])   # the long ones first
    if workers == 1:
        res = [_call(tasks[i]) for i in tasks_sorted]
    else:
        with multiprocessing.Pool(min(16, workers or os.cpu_count() or 1)) as pool:
            res = pool.map(_call, [tasks[i] for i in tasks_sorted], chunksize=1)
    results = dict(zip(tasks_sorted, res))
    records, i = [], 0
    with mp.workdps(exact.DPS):
        for c in selected:
            call, sheet = results[i]
            i += 1
            num = {k: v for k, v in c.items() if isinstance(v, float) and k not in ("cp",)}
            put_shift = -mp.mpf(c["S0"]) + mp.mpf(c["K"]) * mp.mpf(c["discount"])
            price = call if c["cp"] > 0 else call + put_shift
            rec = dict(id=c["id"], dynamics=c["dynamics"], days=c["days"], cp=c["cp"],
                       inputs={k: v.hex() for k, v in num.items()}, price=mp.nstr(price, DIGITS), max_sheet=sheet)
            if c["dynamics"] == "heston":
                rec["moment_all_T"] = c["moment_all_T"]
            else:
                rec["compat_sqrt_alpha"] = c["compat_sqrt_alpha"]
            g = None
            if c["grad"]:
                g = []
                for n in exact.GRAD_SLOTS:
                    if n not in c:
                        g.append(mp.mpf(0))
                        continue
                    (up, h), (dn, _) = results[i], results[i + 1]
                    i += 2
                    g.append((up - dn) / (2 * h))
                rec["grad"] = [mp.nstr(x, DIGITS) for x in g]
            rec.update(fp64_fields(c, price, g))
            records.append(rec)
    return records


def check(ids, path=OUT, workers=None):
    """Recompute the named cases; -> list of (id, field) that differ from the file beyond 1e-25 relative."""
    have = {r["id"]: r for r in json.load(open(path))["cases"]}
    bad = []
    todo = [c for c in cases() if c["id"] in ids]
    assert len(todo) == len(ids), "unknown case id"
    for rec in compute(todo, workers):
        old = have[rec["id"]]
        bad += [(rec["id"], k) for k in ("inputs", "max_sheet", "cp", "days") if rec[k] != old[k]]
        pairs = [("price", rec["price"], old["price"])] + \
                [(f"grad[{k}]", a, b) for k, (a, b) in enumerate(zip(rec.get("grad", []), old.get("grad", [])))]
        for name, a, b in pairs:
            a, b = mp.mpf(a), mp.mpf(b)
            if abs(a - b) > mp.mpf("1e-25") * max(abs(b), 1):
                bad.append((rec["id"], name))
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", nargs="+", metavar="ID")
    a = ap.parse_args()
    if a.check:
        bad = check(set(a.check))
        print("differs: %s" % bad if bad else "ok")
        return 1 if bad else 0
    doc = dict(about="truncated Carr-Madan integrals by mpmath at %d digits (oracle/carr_madan_exact.py); "
                     "e64 = |numpy complex128 on a converged rule - exact|; regenerate with "
                     "tests/golden/make_carr_madan_exact.py" % exact.DPS,
               grad_slots=list(exact.GRAD_SLOTS), cases=compute(cases()))
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
