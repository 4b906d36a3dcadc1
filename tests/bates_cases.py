"""Bates (include/hedgehog_mc.h, "Bates (1996): Heston variance with Merton jumps"): what the host and the device tests
share.

  * the step restated generically in the number type by COMPOSITION: tests/qe_cases.step takes (x, v) to (x′, v′) on the
    draws of domain 5, tests/merton_cases._jump forms the jump sum from the draws of domain 4, and the sum is added to
    x′ before the date.  mpmath at 50 digits is the reference, Python floats in the header's operation order are "the
    same formulas in fp64", whose distance from the 50-digit run is e64.  The constants are qe_cases.constants' with
    rdt = (r − λ·expm1(μ_J + ½σ_J²))·dt in the header's order;
  * the draws restated from the oracle's host Philox words: qe_cases.step_normals / step_uniforms (domain 5),
    merton_cases.path_uniforms / box_muller (domain 4);
  * the one-step expectation of exp(x′ − x − r·dt): qe_cases.step_expectation's integral times the Poisson-normal sum;
  * the Carr–Madan rule for ϕ_B in numpy complex128 and the exactly integrated truncated integral
    (oracle/carr_madan_exact.py's integrand with heston_log_cf plus the jump term).

The bar of a statistic is euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A).  A comes from qe_cases' two
magnitude rules (its docstring: a by oracle/euler_exact.py's rules, b the first-order running bound, A the smaller); the
jump's term J = (σ_J·√N)·z + N·μ_J enters both by the same rules: its a is merton_cases._jump's own, its b that of the
same two products and sum in qe_cases.VA arithmetic.  Neither the QE BRANCH nor the jump COUNT is a rounding matter:
tests/golden/make_bates_exact.py asserts on every trajectory of the fixed seeds that both walks take the same branches
with qe_cases.MARGIN to spare and that every jump uniform keeps merton_cases.MARGIN from every exact cumulative boundary.

MUTATIONS of the restatement (tests/test_bates_host.py holds each to the golden rows): `mut` names one of
  r_plain     r in place of r_c                       r_plus     r + λκ̄ in place of r_c
  keep_z      the mirror keeps +z                     odd_words  odd steps read words 0, 1 of their block
  late_jump   the jump applied after the date         mean_T     λ·T in place of λ·dt as the Poisson mean
"""
import json
import math
import os
from fractions import Fraction

import mpmath as mp
import numpy as np

from hedgehog_jl_amd import _ffi
from oracle import carr_madan_exact as cx
from oracle import euler_exact as ex
from tests import merton_cases as mc
from tests import path_bridge_cases as bc
from tests import qe_cases as qc
from tests.carr_madan_law_cases import cm_case
from tests.lognormal_exact_cases import box_muller

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bates_exact.json")
DPS = qc.DPS
VA = qc.VA
MUTATIONS = ("r_plain", "r_plus", "keep_z", "odd_words", "late_jump", "mean_T")
MODELS = qc.MODELS
PATH_N = 257
PATH_SHAPES = ((1, 1), (5, 1), (6, 1), (6, 3))  # (n_steps, monitor_every): 5 is the odd tail of the two-step block
PATH_MEAN = 0.9                                  # λ·dt: N takes 0 … 4 within one case
JUMP = dict(mu_j=-0.1, sigma_j=0.15)
GOLDEN_N, GOLDEN_SHAPE = 64, (5, 1)
# the law test's model: qe_cases.LAW with jumps
LAW = dict(qc.LAW, lam=0.8, **JUMP)


def load_golden():
    return json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else None


def path_seeds():
    return np.arange(1, PATH_N + 1, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03) + np.uint64(13)


def path_case(name, n_steps):
    """the model `name` with jumps whose λ·dt is PATH_MEAN up to rounding"""
    case = MODELS[name]
    return dict(case, lam=PATH_MEAN * n_steps / case["T"], **JUMP)


def path_mean(case, n_steps, span=None):
    """λ·dt as the library forms it: fl(λ · fl(T / n_steps))"""
    return case["lam"] * (case["T"] / n_steps if span is None else span)


# ---- the draws -----------------------------------------------------------------------------------------------------------

def jump_normals(oracle, seeds, n_steps):
    """z[i][k] at 50 digits: the first normal of block (k, 1, 0, 4) — whether the device draws it or not"""
    with mp.workdps(DPS):
        return [[box_muller(oracle.philox([k, 1, 0, mc.DOM_JUMP], mc._key(s)))[0] for k in range(n_steps)] for s in seeds]


def draws(oracle, seeds, n_steps):
    """everything a walk reads: (Z, U) of domain 5, (UJ, zJ) of domain 4"""
    return dict(Z=qc.step_normals(oracle, seeds, n_steps), U=qc.step_uniforms(oracle, seeds, n_steps),
                UJ=mc.path_uniforms(oracle, seeds, n_steps), zJ=jump_normals(oracle, seeds, n_steps))


def counts(UJ, mean, check=True):
    """N[i][k] of every uniform in exact arithmetic; `check`: MARGIN from every boundary and the fp64 loop agrees"""
    if check:
        return mc.counts_of(UJ, mean)
    N = np.empty(UJ.shape, dtype=np.int64)
    for idx, u in np.ndenumerate(UJ):
        N[idx] = mc.poisson_fp64(float(u), mean)
    return N


# ---- the restatement -----------------------------------------------------------------------------------------------------

def _expm1(t, num):
    v = math.expm1(t.v) if num is float else mp.expm1(t.v)
    e = ex._exp(t.v)
    return VA(v, max(abs(v), e * t.a), e * t.b + abs(v))


def compensator(case, num):
    """λ·expm1(μ_J + (½·σ_J)·σ_J), csrc/hh_jump.hip's merton_compensator in its order"""
    lam, mu, sj = (VA(num(case[k])) for k in ("lam", "mu_j", "sigma_j"))
    return lam * _expm1(mu + (VA(num(0.5)) * sj) * sj, num)


def constants(case, n_steps, num, psi_c=0.0, mut=None):
    """qe_cases.constants with rdt = r_c·dt, r_c = r − λκ̄"""
    q = qc.constants(case, n_steps, num, psi_c)
    r, lk = VA(num(case["r_drift"])), compensator(case, num)
    r_c = r if mut == "r_plain" else r + lk if mut == "r_plus" else r - lk
    q["rdt"] = r_c * VA(num(case["T"]) / n_steps)
    return q


def _fma(a, b, c):
    """the correctly rounded a·b + c of doubles"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def jump_of(case, N, z, num, mut=None):
    """J = (σ_J·√N)·z + N·μ_J as a qe_cases.VA: value and a from tests/merton_cases._jump, b by qe_cases' rules on the
    same operations.  In floats the value is the device's: one fma.  mut "sqrt_N": N in place of √N."""
    c = {k: bc.VA(num(case[k])) for k in ("sigma_j", "mu_j")}
    J = mc._jump(c, int(N), bc.VA(z.v, z.a), num, mut)
    n = VA(num(float(N)))
    Jq = (VA(num(case["sigma_j"])) * qc._sqrt(n)) * z + n * VA(num(case["mu_j"]))
    v = J.v
    if num is float:
        v = _fma(case["sigma_j"] * (float(N) if mut == "sqrt_N" else math.sqrt(float(N))), z.v, float(N) * case["mu_j"])
    return VA(v, J.a, Jq.b)


def walk(case, n_steps, num, d, i, N, mirror, mart, record=None, mut=None, psi_c=0.0):
    """one member of trajectory i on the draws d and the jump counts N[k]: -> (xs, v_T), xs the log spot a date after
    step k would see, as VAs"""
    q = constants(case, n_steps, num, 0.0 if mut == "psi_fixed" else psi_c, mut)
    x, v = qc._log_input(num, case["S0"]), VA(num(case["V0"]))
    xs = []
    for k in range(n_steps):
        zv, zx = VA(num(d["Z"][i][k][0])), VA(num(d["Z"][i][k][1]))
        u = VA(num(float(d["U"][i][k])))
        if mirror:
            zv, zx, u = -zv, -zx, q["one"] - u
        x, v = qc.step(q, x, v, zv, zx, u, mart, num, record, mut if mut in qc.MUTATIONS + qc.SWEEP_MUTATIONS else None)
        seen = x
        if N[k] > 0:
            z = VA(num(d["zJ"][i][k]))
            x = x + jump_of(case, N[k], -z if mirror and mut != "keep_z" else z, num, mut)
        xs.append(seen if mut == "late_jump" else x)
    return xs, v


def mutated_counts(case, n_steps, UJ_i, mut):
    """the jump counts of one trajectory as a mutated reading forms them (fp64 loop; no margins asked of a mutation)"""
    U = np.array(UJ_i, dtype=float)
    if mut == "odd_words":
        U = np.array([U[k - 1] if k & 1 else U[k] for k in range(n_steps)])
    mean = path_mean(case, n_steps, span=case["T"] if mut == "mean_T" else None)
    return [mc.poisson_fp64(float(u), mean) for u in U]


def _float_draws(d, i):
    return dict(Z={i: [(float(a), float(b)) for a, b in d["Z"][i]]}, U=d["U"], zJ={i: [float(z) for z in d["zJ"][i]]})


def walks(case, n_steps, d, N, anti, mart, n=None, check=True, psi_c=0.0, unusable=None, mut=None):
    """both runs of every member of the first n trajectories -> [member][path] of (xs_mp, vT_mp, xs_64, vT_64), and what
    the members saw: QE branches and jump counts; `check` and `unusable` as qe_cases.walks takes them"""
    n = len(d["Z"]) if n is None else n
    threshold = 1.5 if psi_c == 0.0 else psi_c
    members = 2 if anti else 1
    out = [[None] * n for _ in range(members)]
    seen = dict(quadratic=0, exponential=0, zero=0, N={})
    with mp.workdps(DPS):
        for i in range(n):
            d64 = _float_draws(d, i)
            for m in range(members):
                rm, r6 = [], []
                xs_mp, v_mp = walk(case, n_steps, mp.mpf, d, i, N[i], m == 1, mart, rm, mut, psi_c)
                xs_64, v_64 = walk(case, n_steps, float, d64, i, N[i], m == 1, mart, r6, mut, psi_c)
                if check and unusable is not None:
                    if not qc.same_branches(rm, r6, threshold):
                        unusable.add(i)
                elif check:
                    for (psi, quad, zero, du), (_, quad6, zero6, _) in zip(rm, r6):
                        assert quad == quad6 and zero == zero6, (i, m)
                        assert abs(psi - mp.mpf(threshold)) > qc.MARGIN and (du is None or abs(du) > qc.MARGIN), (i, m, psi, du)
                for _, quad, zero, _ in rm:
                    seen["quadratic" if quad else "exponential"] += 1
                    seen["zero"] += bool(zero)
                for k in range(n_steps):
                    seen["N"][int(N[i][k])] = seen["N"].get(int(N[i][k]), 0) + 1
                out[m][i] = (xs_mp, v_mp, xs_64, v_64)
    return out, seen


reference = qc.reference  # -> want [member][path][row] (row 5 is var_T), e64, A


# ---- one step's expectation ------------------------------------------------------------------------------------------------

def step_expectation(case, n_steps, v, mart=True, mut=None, terms=80):
    """E exp(x′ − x − r·dt) of one Bates step from the state v: qe_cases.step_expectation's integral of
    exp(drift′ + ½·var′) over the variance step — Z_x integrated in closed form — times exp((r_c − r)·dt), times the
    Poisson-normal sum Σ_n e^{−m} mⁿ/n! · exp(n·μ_J + ½·n·σ_J²), m = λ·dt, at the working precision"""
    qe_part, branch, _, _ = qc.step_expectation(case, n_steps, v, lambda vn, drift, var: mp.exp(drift + var / 2), mart=mart)
    lam, mu, sj = (mp.mpf(case[k]) for k in ("lam", "mu_j", "sigma_j"))
    dt = mp.mpf(case["T"]) / n_steps
    lk = lam * mp.expm1(mu + sj * sj / 2)
    shift = mp.mpf(0) if mut == "r_plain" else lk if mut == "r_plus" else -lk   # (what stands for r_c) − r
    m = lam * dt
    w, total = mp.exp(-m), mp.mpf(0)
    for n in range(terms):
        if n:
            w = w * m / n
        total += w * mp.exp(n * mu + n * sj * sj / 2)
    return qe_part * mp.exp(shift * dt) * total, branch


# ---- Carr–Madan ------------------------------------------------------------------------------------------------------------

def log_cf(case):
    """tests/carr_madan_law_cases.py's law, exactly: log ϕ = heston_log_cf at the compensated drift +
    λT·(exp(iμ_J·t − σ_J²t²/2) − 1) at t = v − i(α+1)"""
    lam, mu, sj = (cx._mpf(case[k]) for k in ("lam", "mu_j", "sigma_j"))
    p = {k: cx._mpf(case[k]) for k in ("S0", "K", "T", "r_drift", "discount", "alpha", "bound", "V0", "kappa", "theta",
                                        "sigma", "rho")}
    p["compat_sqrt_alpha"] = False
    p["r_drift"] = p["r_drift"] - lam * mc.kappa_bar(case)
    alpha = p["alpha"]
    assert cx.moment_exists_at(p["kappa"], p["sigma"], p["rho"], alpha, p["T"]), "no (α+1)-th moment"
    unwrapped = cx.UnwrappedLog(p, p["bound"])

    def f(v):
        t = mp.mpc(v, -(alpha + 1))
        return cx.heston_log_cf(p, t, lambda z: unwrapped(v, z)) + lam * p["T"] * (mp.exp(mp.mpc(0, 1) * t * mu - sj * sj * t * t / 2) - 1)
    return f


def phi(case, u):
    """… and as hh_fourier.hip's BatesLaw forms it, in numpy complex128: HestonLaw's expression with r_c in it, the jump
    term added to the exponent last"""
    T = case["T"]
    kap, th, sg, rho, V0 = (case[k] for k in ("kappa", "theta", "sigma", "rho", "V0"))
    iu = 1j * u
    r_c = case["r_drift"] - case["lam"] * math.expm1(case["mu_j"] + 0.5 * case["sigma_j"] * case["sigma_j"])
    kri = kap - rho * sg * iu
    u2 = u * u
    d1 = np.sqrt(kri * kri + (sg * sg) * (iu + u2))
    g = (kri - d1) / (kri + d1)
    ed = np.exp(-d1 * T)
    one_m_ged = 1.0 - g * ed
    Cc = (kap * th / (sg * sg)) * (T * (kri - d1) - 2.0 * np.log(one_m_ged / (1.0 - g)))
    Dv = (1.0 / (sg * sg)) * ((kri - d1) * ((1.0 - ed) / one_m_ged))
    e = Cc + V0 * Dv + math.log(case["S0"]) * iu + (r_c * T) * iu
    e = e + (case["lam"] * T) * (np.exp(case["mu_j"] * iu - (0.5 * case["sigma_j"] * case["sigma_j"]) * u2) - 1.0)
    return np.exp(e)


cm_bar = mc.cm_bar

# the Carr–Madan cases: a Feller-violating model (carr_madan_cases' own, 2κθ = 0.08 against σ² = 0.36, with its α and
# bound), a put, λ = 0, σ_J = 0, a short expiry
_FELLER_OK = dict(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r_drift=0.03, T=1.0)
CM_CASES = {
    "feller_violated": cm_case(dict(_FELLER_OK, kappa=1.0, sigma=0.6, rho=-0.5, T=2.0, lam=0.8, **JUMP), 80.0, None, None),
    "put": cm_case(dict(_FELLER_OK, lam=0.8, **JUMP), 90.0, 1.0, 32.0, cp=-1.0),
    "no_jumps": cm_case(dict(_FELLER_OK, lam=0.0, **JUMP), 105.0, 1.0, 32.0),
    "fixed_jump": cm_case(dict(_FELLER_OK, lam=1.5, mu_j=-0.08, sigma_j=0.0), 110.0, 1.0, 32.0),
    "short": cm_case(dict(_FELLER_OK, T=0.1, lam=2.0, **JUMP), 95.0, 1.0, 32.0),
}


def cm_cases():
    """CM_CASES with the Feller-violating case's α and bound taken from tests/carr_madan_cases.py"""
    from tests import carr_madan_cases as cmc
    _, ref = cmc.BY_ID["feller_violated"]
    out = dict(CM_CASES)
    out["feller_violated"] = dict(out["feller_violated"], alpha=ref["alpha"], bound=ref["bound"])
    return out


# ---- the C structs of a case ---------------------------------------------------------------------------------------------

model_of = qc.model_of
config_of = qc.config_of


def jump_struct(case):
    return _ffi.make_jump(case["lam"], case["mu_j"], case["sigma_j"])
