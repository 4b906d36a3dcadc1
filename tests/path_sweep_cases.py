"""The sweep of the path-statistics kernels over model VALUES: the table of named cases per family, the admissibility
checks of include/hedgehog_mc.h restated in Python (once, here), and the evaluation of a case by the restatements the
families' own tests use (qe_cases, bates_cases, merton_cases) — what tests/golden/make_path_sweep.py,
tests/test_path_sweep_host.py and tests/test_gpu_path_sweep.py share.

The fixed-model tests of each family pin the arithmetic on one or two hand-picked models; these cases look for a
dependence on the values.  A case has one of two origins:
  edge   written by hand (EDGE below): one row per edge of the admitted region and per degenerate value of the step —
         ρ ∈ {0.6, 0, ±1}, ψ_c ∈ {1, 2, 1.25}, V0 = 0, κ·dt tiny and huge, σ²/(2κθ) up to HH_QE_MAX_PSI, Poisson means
         from 0 to HH_JUMP_MAX_MEAN, σ_J = 0, large |μ_J|, σ ∈ {1e-8, 2} — run on every shape of SHAPES, with and
         without the start, with and without mirrors;
  drawn  DRAWN_N models per family from numpy.random.default_rng(SEED): log-uniform in the scale parameters, uniform in ρ
         and in the switches, a draw the header does not admit rejected; stored in tests/golden/path_sweep.json as hex
         floats, so that every machine forms the same doubles, and READ from there (draw_models is the maker's).  One
         shape, DRAWN_SHAPE, with the start and with mirrors.
FAMILIES covered: the quadratic-exponential scheme ("qe": hh_mc_path_stats_qe / hh_mc_solve_path_qe), Bates ("bates":
hh_mc_path_stats_bates / hh_mc_solve_path_bates), the Merton path form ("merton_path": hh_mc_solve_path_jump), the Merton
terminal law ("merton_terminal": hh_mc_solve_jump) and several assets ("assets": hh_mc_path_stats_assets /
hh_mc_solve_path_assets; d ∈ {1, 2, 3, 8}, every index kind, correlations of ±0.999, a zero and a negative weight, an
asset without volatility) and local volatility ("localvol": hh_mc_path_stats_lv / hh_mc_solve_path_lv under
HH_EXTREMES_BRIDGE and HH_EXTREMES_MONITORED; the five localvol_cases.SURFACES with S0 on the lowest node, on the highest
node and off the grid, r < 0, T before the first and past the last table time).
The Euler statistics ("euler": hh_mc_path_stats_ex / hh_mc_solve_path_ex) are swept in their BRIDGE form on the rows
path_bridge_cases.walk restates — S_T, CMAX_S and CMIN_S: lognormal σ ∈ {1e-8, 2}; Heston in both em_split readings with
ρ ∈ {±1, 0}, a negative vol-of-vol, V0 = 0 and a model that clips on at least MIN_CLIP_FRACTION of its member-steps; a
trajectory whose two runs could clip differently (oracle/euler_exact._usable) is left out.  The four other rows of that
family have no 50-digit restatement in the tree; the device test holds them to the HH_EXTREMES_MONITORED call bit for bit
and to finiteness, no more.

Local volatility leaves no trajectory out: the lookup is bilinear with clamping, continuous in the state, so a cell or a
clamp the two runs decide differently — as they must where S0 sits exactly on a node — changes σ by a rounding, and that
is measured in e64 like every other rounding.  The rows record how many states lay off the grid on each side.

n_paths = N_PATHS = 65: one full wave and a one-lane second wave.  The seeds are each family's own path_seeds()[:65].

USABLE trajectories.  A trajectory on which the fp64 run and the 50-digit run could take different discrete decisions —
a QE branch with |ψ − ψ_c| or |U − p| within qe_cases.MARGIN, a jump uniform within merton_cases.MARGIN of a cumulative
boundary — is left out of the comparison, mirrors included; at most MAX_UNUSABLE = 0.02 of a case's trajectories (one of
65) may be.  That is a condition on the INPUTS, checked by the maker with the reference alone: a drawn model that breaks
it is replaced by the next draw, an edge row gets another value of the same kind.

The bar of every number is euler_tangent_cases.path_bar(e64, A), imported; nothing here widens it.  Away from the pinned
models the ε·A term of the QE restatement grows to 1e-6 of a path's scale, so `bars` NARROWS it: the smaller of path_bar and
FP64_SIZED = 1e-9 of the path's scale (`scales`), the project's own figure for a bar that is fp64-sized
(euler_tangent_cases.assert_bars_are_fp64_sized).  The host test asserts that the fp64 restatement keeps a factor 20 inside
it (20·e64 <= 1e-9 of scale) on every case but the two of ILL_CONDITIONED, whose fp64 run is itself far from the 50-digit
run by construction.  On those two the 50-digit bar holds almost nothing, so the device is ALSO held to the fp64
restatement — the same formulas on the same rounded constants, 1 − E among them — within 1e-9 of scale (`reference`'s f64).
"""
import json
import math
import os

import mpmath as mp
import numpy as np

from hedgehog_jl_amd import _ffi
from tests import assets_cases as ac
from tests import bates_cases as bt
from tests import euler_tangent_cases as etc
from tests import localvol_cases as lc
from tests import merton_cases as mc
from tests import path_bridge_cases as bc
from tests import path_payoff_cases as pc
from tests import qe_cases as qc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_sweep.json")
FAMILIES = ("qe", "bates", "merton_path", "merton_terminal", "assets", "localvol", "euler")
SEED = 20261020
DRAWN_N = 24
DRAWN_BY_FAMILY = {}    # family -> a smaller drawn table, where its reference is too slow for DRAWN_N (none is)
N_PATHS = 65
SHAPES = ((1, 1), (5, 1), (6, 3))       # (n_steps, monitor_every): 5 half-reads the Philox block that feeds two steps
DRAWN_SHAPE = (5, 1)
TERMINAL_OFFSETS = (0, 2 ** 33 - 1)     # the terminal law's "shapes": path_offset
TERMINAL_SIZES = (1, 63, 65)
MAX_UNUSABLE = etc.MAX_UNUSABLE
CAP = int(MAX_UNUSABLE * N_PATHS)       # trajectories of a case that may be left out: 1
INV, UNS = _ffi.HH_ERR_INVALID, _ffi.HH_ERR_UNSUPPORTED
MAX_PSI, MAX_MEAN = _ffi.HH_QE_MAX_PSI, _ffi.HH_JUMP_MAX_MEAN
INF = float("inf")
FP64_SIZED = 1e-9
# Cases whose fp64 restatement is itself far from the 50-digit run BY CONSTRUCTION, so that their 50-digit bars are wide:
ILL_CONDITIONED = {
    "qe:kappa_dt_small": "1 − E keeps 2 to 5 significant bits, and c1, c2 and θ·(1 − E) inherit them",
    "qe:sigma_1e-6": "K0, K1·v and K2·v′ are of size κθ·dt/σ = 1e4 and cancel to the size of one step's drift",
}


# ---- the admissibility checks of the header, restated -------------------------------------------------------------------

def _finite(*xs):
    return all(math.isfinite(x) for x in xs)


def compensator(lam, mu_j, sigma_j):
    """λ·expm1(μ_J + (½·σ_J)·σ_J): csrc/hh_jump.h's merton_compensator"""
    try:
        return lam * math.expm1(mu_j + (0.5 * sigma_j) * sigma_j)
    except OverflowError:
        return INF


def jump_defect(lam, mu_j, sigma_j, span):
    """-> None, or (code, text) of the first check of hh_api.hip's check_jump that fails; span: what one draw covers"""
    if not (lam >= 0.0) or not math.isfinite(lam):
        return INV, "jump lambda must be finite and >= 0"
    if not (sigma_j >= 0.0) or not math.isfinite(sigma_j):
        return INV, "jump sigma_j must be finite and >= 0"
    if not math.isfinite(mu_j):
        return INV, "jump mu_j must be finite"
    if not math.isfinite(compensator(lam, mu_j, sigma_j)):
        return INV, "exp(mu_j + sigma_j^2/2) must be finite"
    if not (lam * span <= MAX_MEAN):
        return INV, "is above HH_JUMP_MAX_MEAN"
    return None


def qe_defect(model, n_steps, psi_c, mart, r_drift=None):
    """-> None, or (code, text) of the first failing check of a quadratic-exponential entry point: the scalars every path
    entry point checks, then check_qe (the constants formed on r_drift — Bates passes the compensated rate)"""
    m = model
    r = m["r_drift"] if r_drift is None else r_drift
    if not (m["S0"] > 0.0 and m["T"] > 0.0 and abs(m["rho"]) <= 1.0
            and _finite(m["S0"], m["T"], m["sigma"], m["r_drift"], m["V0"], m["kappa"], m["theta"])):
        return INV, "S0, T > 0, |rho| <= 1, model scalars finite"
    if not (m["kappa"] > 0.0 and m["theta"] > 0.0 and m["sigma"] > 0.0 and m["V0"] >= 0.0):
        return INV, "kappa, theta, sigma must be > 0 and V0 >= 0"
    if not ((m["sigma"] * m["sigma"]) / (2.0 * m["kappa"] * m["theta"]) <= MAX_PSI):
        return INV, "is above HH_QE_MAX_PSI"
    if not (psi_c == 0.0 or 1.0 <= psi_c <= 2.0):
        return INV, "psi_c must be 0 (the default 1.5) or lie in [1, 2]"
    q = qc.constants(dict(m, r_drift=r), n_steps, float, psi_c)
    if not _finite(*[q[k].v for k in ("E", "c1", "c2", "th_ome", "rdt", "K0", "K1", "K2", "K3", "A", "k13")]):
        return INV, "the step's constants are not finite"
    if not (q["th_ome"].v > 0.0 and q["c2"].v > 0.0):
        return INV, "rounds to 0"
    if mart and q["A"].v > 0.0:
        return UNS, "run without it"
    return None


def lognormal_defect(model):
    m = model
    if not (m["S0"] > 0.0 and m["T"] > 0.0 and _finite(m["S0"], m["T"], m["sigma"], m["r_drift"])):
        return INV, "model scalars"
    return None


def assets_defect(model, kind):
    """-> None, or (code, text) of the first failing check of a multi-asset entry point (run_path_stats, check_assets)"""
    m, d = model, len(model["spots"])
    if not (m["T"] > 0.0 and _finite(m["T"], m["r_drift"])):
        return INV, "T > 0, r_drift and discount finite"
    if not 1 <= d <= ac.MAX:
        return INV, "must lie in 1 .."
    if kind not in ac.KINDS:
        return INV, "unknown index_kind"
    for i in range(d):
        if not (m["spots"][i] > 0.0 and math.isfinite(m["spots"][i])):
            return INV, "the spot must be finite and > 0"
        if not (m["sigmas"][i] >= 0.0 and math.isfinite(m["sigmas"][i])):
            return INV, "sigma must be finite and >= 0"
        if not math.isfinite(m["weights"][i]):
            return INV, "the weight must be finite"
        if kind in (ac.BEST, ac.WORST) and not m["weights"][i] > 0.0:
            return INV, "a best-of / worst-of weight must be > 0"
    if kind == ac.SUM and not any(w != 0.0 for w in m["weights"]):
        return INV, "every weight of the weighted sum is zero"
    if ac.corr_defect(m["corr"]):
        return INV, "correlation: " + ac.corr_defect(m["corr"])
    if ac.cholesky_fp64(m["corr"]) is None:
        return INV, "the correlation matrix is not positive definite"
    return None


def surface_of(case):
    """the case's surface dict: localvol_cases.surface(name), its volatilities scaled by case["vol_scale"]"""
    surf = lc.surface(case["surface"])
    return dict(surf, vols=surf["vols"] * case["vol_scale"])


def localvol_defect(model, surf):
    """-> None, or (code, text) of the first failing check of a local-volatility entry point (run_path_stats without
    model->sigma, then check_localvol)"""
    m, vols, times = model, np.asarray(surf["vols"]), [float(t) for t in surf["times"]]
    if not (m["S0"] > 0.0 and m["T"] > 0.0 and _finite(m["S0"], m["T"], m["r_drift"])):
        return INV, "S0, T > 0, |rho| <= 1, model scalars finite"
    if len(times) < 1 or vols.shape[1] < 2:
        return INV, "the surface needs n_times >= 1 and n_x >= 2"
    if vols.size > _ffi.HH_LV_MAX_NODES:
        return INV, "is above HH_LV_MAX_NODES"
    if not math.isfinite(surf["x_lo"]):
        return INV, "x_lo must be finite"
    if not (surf["h"] > 0.0 and math.isfinite(surf["h"]) and math.isfinite(1.0 / surf["h"])):
        return INV, "h must be finite and > 0"
    for j, t in enumerate(times):
        if not (t >= 0.0 and math.isfinite(t)):
            return INV, "must be finite and >= 0"
        if j and not t > times[j - 1]:
            return INV, "times must be strictly increasing"
    if not (np.all(np.isfinite(vols)) and np.all(vols > 0.0)):
        return INV, "must be finite and > 0"
    return None


def euler_defect(model):
    m = model
    if not (m["S0"] > 0.0 and m["T"] > 0.0 and abs(m["rho"]) <= 1.0
            and _finite(m["S0"], m["T"], m["sigma"], m["r_drift"], m["V0"], m["kappa"], m["theta"])):
        return INV, "S0, T > 0, |rho| <= 1, model scalars finite"
    return None


def lam_of(case, n_steps):
    """λ of a case whose Poisson mean of one draw is case["mean"]: the largest double not above mean/span whose product
    with the span, as the library forms it, is not above the mean's cap"""
    span = case["model"]["T"] / n_steps if case["family"] != "merton_terminal" else case["model"]["T"]
    lam = case["mean"] / span
    while lam * span > max(case["mean"], 0.0) and case["mean"] == MAX_MEAN:
        lam = math.nextafter(lam, 0.0)
    return lam


def jump_model(case, n_steps):
    """the case's model with its jumps at this step count, in the form bates_cases / merton_cases take"""
    return dict(case["model"], lam=lam_of(case, n_steps), mu_j=case["mu_j"], sigma_j=case["sigma_j"], n_steps=n_steps,
                antithetic=1)


def defect(case, n_steps=5):
    """the header's verdict on a case at a step count: None when admitted"""
    fam, m = case["family"], case["model"]
    if fam == "qe":
        return qe_defect(m, n_steps, case["psi_c"], case["mart"])
    if fam == "assets":
        return assets_defect(m, case["kind"])
    if fam == "euler":
        return euler_defect(m)
    if fam == "localvol":
        return localvol_defect(m, case.get("surf") or surface_of(case))
    jm = jump_model(case, n_steps)
    span = m["T"] if fam == "merton_terminal" else m["T"] / n_steps
    if fam == "bates":
        base = qe_defect(m, n_steps, case["psi_c"], 0)   # the scalars first, as run_path_stats orders them
        if base and base[1].startswith("S0"):
            return base
        return jump_defect(jm["lam"], jm["mu_j"], jm["sigma_j"], span) or \
            qe_defect(m, n_steps, case["psi_c"], case["mart"], m["r_drift"] - compensator(jm["lam"], jm["mu_j"], jm["sigma_j"]))
    return lognormal_defect(m) or jump_defect(jm["lam"], jm["mu_j"], jm["sigma_j"], span)


# ---- the edge table -----------------------------------------------------------------------------------------------------

FELLER = qc.MODELS["feller"]                  # 2κθ = 0.16 against σ² = 0.25
STRADDLE = dict(FELLER, sigma=0.8)            # σ²/(2κθ) = 4: ψ runs from below 1 to 4 within a case
JUMP = dict(mu_j=-0.1, sigma_j=0.15)


def _psi_max_model(ratio):
    """κ = 1, θ = 0.04 and the σ whose σ²/(2κθ), as the library forms it, is the largest double not above `ratio`"""
    m = dict(FELLER, kappa=1.0, theta=0.04, sigma=math.sqrt(ratio * 0.08))
    while (m["sigma"] * m["sigma"]) / (2.0 * m["kappa"] * m["theta"]) > ratio:
        m["sigma"] = math.nextafter(m["sigma"], 0.0)
    return m


def _qe(name, model, psi_c=0.0, mart=0, **expect):
    return dict(family="qe", origin="edge", name=name, model=model, psi_c=psi_c, mart=mart, expect=expect)


def _bates(name, model, mean, mu_j, sigma_j, psi_c=0.0, mart=0, **expect):
    return dict(family="bates", origin="edge", name=name, model=model, psi_c=psi_c, mart=mart, mean=mean, mu_j=mu_j,
                sigma_j=sigma_j, expect=expect)


def _merton(family, name, mean, mu_j=-0.1, sigma_j=0.15, **over):
    return dict(family=family, origin="edge", name=name, model=dict({k: mc.BASE[k] for k in ("S0", "sigma", "r_drift", "T")}, **over),
                mean=mean, mu_j=mu_j, sigma_j=sigma_j, expect=dict(max_N=40) if mean == MAX_MEAN else {})


QE_EDGE = [
    # ρ > 0: A > 0, so without the correction only (REJECTED holds the corrected call to HH_ERR_UNSUPPORTED)
    _qe("rho_+0.6", dict(FELLER, rho=0.6), A_positive=True),
    _qe("rho_0", dict(FELLER, rho=0.0), mart=1, K1_is_K2=True),
    _qe("rho_0_plain", dict(FELLER, rho=0.0), K1_is_K2=True),
    _qe("rho_-1", dict(FELLER, rho=-1.0), mart=1, K3_zero=True),
    _qe("rho_-1_plain", dict(FELLER, rho=-1.0), K3_zero=True),
    _qe("rho_+1", dict(FELLER, rho=1.0), K3_zero=True, A_positive=True),
    # ψ_c at its ends and inside, on a model whose ψ crosses each of them within the case
    _qe("psi_c_1.0", STRADDLE, psi_c=1.0, mart=1, both_branches=True),
    _qe("psi_c_2.0", STRADDLE, psi_c=2.0, both_branches=True),
    _qe("psi_c_1.25", STRADDLE, psi_c=1.25, mart=1, both_branches=True),
    _qe("V0_0", dict(FELLER, V0=0.0), mart=1),
    _qe("V0_0_rho_+0.9", dict(FELLER, V0=0.0, rho=0.9)),
    # κ·T = 2e-15: 1 − E is 18 ulps of 2⁻⁵³ on one step and 3 on six, and still above 0
    _qe("kappa_dt_small", dict(FELLER, kappa=2e-15, sigma=3e-4, T=1.0), mart=1, small_ome=True),
    # κ·T = 4200: E = exp(−700) on six steps, exp(−840) on five, 0.0 on one
    _qe("kappa_dt_large", dict(FELLER, kappa=4200.0, sigma=20.0, T=1.0), mart=1, tiny_E=True),
    _qe("psi_max_1e6", _psi_max_model(1e6), mart=1),
    _qe("psi_max_0.99e9", _psi_max_model(0.99 * MAX_PSI)),
    # σ small: ψ ≪ 1 in every state, t = 2/ψ above 1e9
    _qe("sigma_1e-6", dict(FELLER, sigma=1e-6), mart=1, all_quadratic=True),
]

BATES_EDGE = [
    _bates("rho_+0.6_mean_8", dict(FELLER, rho=0.6), 8.0, -0.1, 0.15, A_positive=True),
    _bates("rho_0_mean_1e-3", dict(FELLER, rho=0.0), 1e-3, -0.1, 0.15, mart=1, K1_is_K2=True),
    _bates("rho_-1_mean_64", dict(FELLER, rho=-1.0), MAX_MEAN, -0.1, 0.15, mart=1, K3_zero=True, max_N=40),
    _bates("rho_+1_mean_0", dict(FELLER, rho=1.0), 0.0, -0.1, 0.15, K3_zero=True, A_positive=True),
    _bates("rho_+1_mean_8_sigma_j_0", dict(FELLER, rho=1.0), 8.0, -0.1, 0.0, K3_zero=True, A_positive=True),
    _bates("psi_c_1.0_mean_64_mu_j_-2", STRADDLE, MAX_MEAN, -2.0, 0.15, psi_c=1.0, mart=1, both_branches=True, max_N=40),
    _bates("psi_c_2.0_mean_8_mu_j_+1", STRADDLE, 8.0, 1.0, 0.15, psi_c=2.0, both_branches=True),
    _bates("psi_c_1.25_mean_1e-3_sigma_j_0", STRADDLE, 1e-3, -0.1, 0.0, psi_c=1.25, mart=1, both_branches=True),
    _bates("psi_c_2.0_mean_0.9", STRADDLE, 0.9, -0.1, 0.15, psi_c=2.0, mart=1, both_branches=True),
    _bates("rho_-1_mean_2.5_mu_j_+1", dict(FELLER, rho=-1.0), 2.5, 1.0, 0.15, K3_zero=True),
]


def _merton_edge(family):
    return [
        _merton(family, "mean_0", 0.0), _merton(family, "mean_1e-3", 1e-3), _merton(family, "mean_2.5", 2.5),
        _merton(family, "mean_8", 8.0), _merton(family, "mean_64", MAX_MEAN),
        _merton(family, "sigma_j_0", 2.5, sigma_j=0.0), _merton(family, "mu_j_-2", 2.5, mu_j=-2.0),
        _merton(family, "mu_j_+1", 8.0, mu_j=1.0), _merton(family, "mu_j_-2_mean_64", MAX_MEAN, mu_j=-2.0),
        _merton(family, "sigma_1e-8", 0.9, sigma=1e-8), _merton(family, "sigma_2", 0.9, sigma=2.0),
    ]


def _assets(name, model, kind, **expect):
    return dict(family="assets", origin="edge", name=name, model=model, kind=kind, expect=expect)


def _pair(rho, **over):
    return dict(ac.path_case(2), corr=[[1.0, rho], [rho, 1.0]], **over)


ASSETS_EDGE = [
    _assets("d1_sum", ac.path_case(1), ac.SUM), _assets("d2_best", ac.path_case(2), ac.BEST),
    _assets("d2_worst", ac.path_case(2), ac.WORST), _assets("d3_sum", ac.path_case(3), ac.SUM),
    _assets("d3_geo", ac.path_case(3), ac.GEO), _assets("d8_sum", ac.path_case(8), ac.SUM),
    _assets("d8_geo", ac.path_case(8), ac.GEO), _assets("d8_best", ac.path_case(8), ac.BEST),
    _assets("d8_worst", ac.path_case(8), ac.WORST),
    # the factor's last diagonal entry is sqrt(1 − 0.999²) = 0.0447
    _assets("corr_+0.999_sum", _pair(0.999), ac.SUM, thin_factor=True),
    _assets("corr_-0.999_geo", _pair(-0.999), ac.GEO, thin_factor=True),
    _assets("corr_-0.999_best", _pair(-0.999), ac.BEST, thin_factor=True),
    _assets("weight_0", dict(ac.path_case(3), weights=[0.5, 0.0, 0.5]), ac.SUM),
    # 100 − 0.3·90: a spread that stays above 0 on every trajectory (the reference takes its logarithm: asserted there)
    _assets("spread", dict(ac.path_case(2), weights=[1.0, -0.3]), ac.SUM, negative_weight=True),
    _assets("sigma_i_0_best", dict(ac.path_case(3), sigmas=[0.2, 0.0, 0.25]), ac.BEST),
    _assets("sigma_i_0_sum", dict(ac.path_case(3), sigmas=[0.2, 0.0, 0.25]), ac.SUM),
]

def _node_spot(surf, top):
    """S0 whose log, as Python forms it, lands on the surface's lowest (highest) node: u = (log S0 − x_lo)/h is exactly 0
    (n_x − 1) where a double within 64 ulps of the node's spot gives that, the nearest such double otherwise"""
    n_x, inv_h = surf["vols"].shape[1], 1.0 / surf["h"]
    want = float(n_x - 1) if top else 0.0
    best = s0 = math.exp(surf["x_lo"] + (surf["h"] * (n_x - 1) if top else 0.0))
    for up in (True, False):
        t = s0
        for _ in range(64):
            if abs((math.log(t) - surf["x_lo"]) * inv_h - want) < abs((math.log(best) - surf["x_lo"]) * inv_h - want):
                best = t
            t = math.nextafter(t, INF if up else 0.0)
    return best


def _lv(name, surface, vol_scale=1.0, **over):
    expect = {k: over.pop(k) for k in ("on_node", "off_low", "off_high") if k in over}
    return dict(family="localvol", origin="edge", name=name, model=dict(lc.MODEL, **over), surface=surface, vol_scale=vol_scale,
                expect=expect)


def _localvol_edge():
    rows = []
    for name in lc.SURFACES:
        surf = lc.surface(name)
        rows.append(_lv(f"{name}_S0_lowest_node", name, S0=_node_spot(surf, False), on_node=0))
        rows.append(_lv(f"{name}_S0_highest_node", name, S0=_node_spot(surf, True), on_node=1))
        rows.append(_lv(f"{name}_S0_off_grid", name, S0=math.exp(surf["x_lo"] - 0.5), off_low=True))
    rows.append(_lv("narrow_r_below_0", "narrow", r_drift=-0.02, off_low=True, off_high=True))
    rows.append(_lv("two_by_3_T_before_the_first_time", "two_by_3", T=0.1))     # every step before times[0] = 0.25
    rows.append(_lv("narrow_T_past_the_last_time", "narrow", T=3.0, off_low=True, off_high=True))   # times end at 0.8
    return rows


LOCALVOL_EDGE = _localvol_edge()


def _euler(name, model, dynamics="heston", em_split=1, **expect):
    return dict(family="euler", origin="edge", name=name, model=model, dynamics=dynamics, em_split=em_split, expect=expect)


def _euler_edge():
    flat = dict(bc.H252, V0=0.0, kappa=0.0, theta=0.0, rho=0.0)
    rows = [_euler("lognormal_sigma_1e-8", dict(flat, sigma=1e-8), "lognormal"),
            _euler("lognormal_sigma_2", dict(flat, sigma=2.0), "lognormal")]
    for split in (1, 0):
        tag = "split" if split else "classic"
        rows += [_euler(f"{tag}_rho_+1", dict(bc.H252, rho=1.0), em_split=split),
                 _euler(f"{tag}_rho_-1", dict(bc.H252, rho=-1.0), em_split=split),
                 _euler(f"{tag}_rho_0", dict(bc.H252, rho=0.0), em_split=split),
                 _euler(f"{tag}_vol_of_vol_below_0", dict(bc.H252, sigma=-0.3), em_split=split),
                 _euler(f"{tag}_V0_0", dict(bc.H252, V0=0.0), em_split=split),
                 _euler(f"{tag}_clipped", bc.CLIPPED, em_split=split, clips=True)]
    return rows


EULER_EDGE = _euler_edge()

EDGE = dict(qe=QE_EDGE, bates=BATES_EDGE, merton_path=_merton_edge("merton_path"), merton_terminal=_merton_edge("merton_terminal"),
            assets=ASSETS_EDGE, localvol=LOCALVOL_EDGE, euler=EULER_EDGE)


def _nudge(x, up):
    return math.nextafter(x, INF if up else -INF)


def rejected(family):
    """For each admissibility boundary the edge table touches, the value just OUTSIDE it: (name, case, n_steps, code,
    text).  The value just inside is one of EDGE's rows."""
    by = {c["name"]: c for c in EDGE[family]}
    out = []

    def row(name, base, code, text, n_steps=5, **change):
        c = dict(by[base])
        c["model"] = dict(c["model"], **{k: v for k, v in change.items() if k in c["model"]})
        c.update({k: v for k, v in change.items() if k not in c["model"]})
        out.append((name, c, n_steps, code, text))

    if family in ("qe", "bates"):
        lo, hi, pos = ("rho_-1", "rho_+1", "rho_+0.6") if family == "qe" else ("rho_-1_mean_64", "rho_+1_mean_0", "rho_+0.6_mean_8")
        row("rho_above_+1", hi, INV, "S0, T > 0, |rho| <= 1, model scalars finite", rho=_nudge(1.0, True))
        row("rho_below_-1", lo, INV, "S0, T > 0, |rho| <= 1, model scalars finite", rho=_nudge(-1.0, False))
        row("correction_with_A_positive", pos, UNS, "run without it", mart=1)
        row("correction_with_rho_+1", hi, UNS, "run without it", mart=1)
        p1, p2 = ("psi_c_1.0", "psi_c_2.0") if family == "qe" else ("psi_c_1.0_mean_64_mu_j_-2", "psi_c_2.0_mean_8_mu_j_+1")
        row("psi_c_below_1", p1, INV, "psi_c must be 0 (the default 1.5) or lie in [1, 2]", psi_c=_nudge(1.0, False))
        row("psi_c_above_2", p2, INV, "psi_c must be 0 (the default 1.5) or lie in [1, 2]", psi_c=_nudge(2.0, True))
    if family == "qe":
        row("V0_below_0", "V0_0", INV, "kappa, theta, sigma must be > 0 and V0 >= 0", V0=-5e-324)
        row("kappa_dt_rounds_to_0", "kappa_dt_small", INV, "rounds to 0", kappa=1e-17, sigma=1e-6)
        over = dict(by["psi_max_0.99e9"]["model"])
        over["sigma"] = math.sqrt(MAX_PSI * 0.08)
        while not (over["sigma"] * over["sigma"]) / (2.0 * over["kappa"] * over["theta"]) > MAX_PSI:
            over["sigma"] = math.nextafter(over["sigma"], INF)
        row("psi_max_above_1e9", "psi_max_0.99e9", INV, "is above HH_QE_MAX_PSI", sigma=over["sigma"])
    if family == "bates":
        row("mean_above_64", "rho_-1_mean_64", INV, "is above HH_JUMP_MAX_MEAN", mean=_nudge(MAX_MEAN, True) * (1 + 1e-12))
        row("sigma_j_below_0", "rho_+1_mean_8_sigma_j_0", INV, "jump sigma_j must be finite and >= 0", sigma_j=-5e-324)
        row("lambda_below_0", "rho_+1_mean_0", INV, "jump lambda must be finite and >= 0", mean=-1e-300)
    if family == "euler":
        text = "S0, T > 0, |rho| <= 1, model scalars finite"
        row("rho_above_+1", "split_rho_+1", INV, text, rho=_nudge(1.0, True))
        row("rho_below_-1", "classic_rho_-1", INV, text, rho=_nudge(-1.0, False))
        row("T_0", "lognormal_sigma_2", INV, text, T=0.0)
    if family == "localvol":
        cap = surface_of(by["cap_S0_off_grid"])
        more = dict(cap, times=np.append(cap["times"], 1.0), vols=np.vstack([cap["vols"], cap["vols"][-1:]]))
        row("one_row_more_than_the_cap", "cap_S0_off_grid", INV, "is above HH_LV_MAX_NODES", surf=more)
        one = surface_of(by["one_row_S0_off_grid"])
        row("h_0", "one_row_S0_off_grid", INV, "h must be finite and > 0", surf=dict(one, h=0.0))
        zero = one["vols"].copy()
        zero[0, 1] = 0.0
        row("a_volatility_of_0", "one_row_S0_off_grid", INV, "must be finite and > 0", surf=dict(one, vols=zero))
        row("T_0", "two_by_3_T_before_the_first_time", INV, "S0, T > 0, |rho| <= 1, model scalars finite", T=0.0)
    if family == "assets":
        below = [0.2, -5e-324, 0.25]
        row("sigma_i_below_0", "sigma_i_0_best", INV, "sigma must be finite and >= 0", sigmas=below)
        row("best_of_weight_0", "sigma_i_0_best", INV, "a best-of / worst-of weight must be > 0", weights=[0.5, 0.0, 0.5])
        row("every_weight_0", "weight_0", INV, "every weight of the weighted sum is zero", weights=[0.0, 0.0, 0.0])
        row("corr_+1", "corr_+0.999_sum", INV, "the correlation matrix is not positive definite", corr=[[1.0, 1.0], [1.0, 1.0]])
    if family in ("merton_path", "merton_terminal"):
        row("mean_above_64", "mean_64", INV, "is above HH_JUMP_MAX_MEAN", mean=_nudge(MAX_MEAN, True) * (1 + 1e-12))
        row("sigma_j_below_0", "sigma_j_0", INV, "jump sigma_j must be finite and >= 0", sigma_j=-5e-324)
        row("lambda_below_0", "mean_0", INV, "jump lambda must be finite and >= 0", mean=-1e-300)
    return out


# ---- the drawn table ----------------------------------------------------------------------------------------------------

def _logu(rng, lo, hi):
    return float(math.exp(rng.uniform(math.log(lo), math.log(hi))))


def draw_models(family):
    """the endless stream of a family's draws, inadmissible ones left out; the maker takes the first DRAWN_N whose
    unusable share is within the cap"""
    rng = np.random.default_rng([SEED, FAMILIES.index(family)])
    k = 0
    while True:
        if family in ("qe", "bates"):
            model = dict(S0=_logu(rng, 1.0, 1000.0), V0=_logu(rng, 1e-4, 0.5), kappa=_logu(rng, 0.05, 20.0),
                         theta=_logu(rng, 0.005, 0.5), sigma=_logu(rng, 0.01, 3.0), rho=float(rng.uniform(-1.0, 1.0)),
                         r_drift=float(rng.uniform(-0.05, 0.1)), T=_logu(rng, 0.05, 5.0))
            case = dict(family=family, origin="drawn", model=model, mart=int(rng.integers(0, 2)),
                        psi_c=0.0 if rng.integers(0, 2) else float(rng.uniform(1.0, 2.0)), expect={})
        elif family == "euler":
            model = dict(S0=_logu(rng, 1.0, 1000.0), V0=_logu(rng, 1e-4, 0.5), kappa=_logu(rng, 0.05, 20.0),
                         theta=_logu(rng, 0.005, 0.5), sigma=_logu(rng, 0.01, 1.5), rho=float(rng.uniform(-1.0, 1.0)),
                         r_drift=float(rng.uniform(-0.05, 0.1)), T=_logu(rng, 0.05, 5.0))
            case = dict(family=family, origin="drawn", model=model, dynamics="heston" if rng.integers(0, 4) else "lognormal",
                        em_split=int(rng.integers(0, 2)), expect={})
        elif family == "localvol":
            model = dict(S0=_logu(rng, 40.0, 250.0), r_drift=float(rng.uniform(-0.05, 0.1)), T=_logu(rng, 0.05, 5.0))
            case = dict(family=family, origin="drawn", model=model, surface=lc.SURFACES[int(rng.integers(0, len(lc.SURFACES)))],
                        vol_scale=_logu(rng, 0.25, 4.0), expect={})
        elif family == "assets":
            d = int(rng.integers(1, ac.MAX + 1))
            B = rng.normal(size=(d, d)) + 2.0 * float(rng.uniform(0.0, 1.0)) * rng.normal(size=(d, 1))  # a common factor
            G = B @ B.T
            Cm = G / np.sqrt(np.outer(np.diag(G), np.diag(G)))
            corr = [[1.0 if i == j else float(Cm[min(i, j)][max(i, j)]) for j in range(d)] for i in range(d)]
            model = dict(spots=[_logu(rng, 10.0, 1000.0) for _ in range(d)], sigmas=[_logu(rng, 0.01, 1.0) for _ in range(d)],
                         weights=[float(rng.uniform(0.05, 1.0)) for _ in range(d)], corr=corr,
                         r_drift=float(rng.uniform(-0.05, 0.1)), T=_logu(rng, 0.05, 5.0))
            case = dict(family=family, origin="drawn", model=model, kind=int(ac.KINDS[int(rng.integers(0, 4))]), expect={})
        else:
            model = dict(S0=_logu(rng, 1.0, 1000.0), sigma=_logu(rng, 1e-3, 2.0), r_drift=float(rng.uniform(-0.05, 0.1)),
                         T=_logu(rng, 0.05, 5.0))
            case = dict(family=family, origin="drawn", model=model, expect={})
        if family not in ("qe", "assets", "localvol", "euler"):
            case.update(mean=_logu(rng, 1e-3, MAX_MEAN), mu_j=float(rng.uniform(-2.0, 1.0)),
                        sigma_j=0.0 if rng.integers(0, 8) == 0 else _logu(rng, 1e-3, 1.0))
        case["name"] = f"draw_{k:02d}"
        k += 1
        if defect(case, DRAWN_SHAPE[0]) is None:
            yield case


_FLOATS = ("psi_c", "mean", "mu_j", "sigma_j", "vol_scale")


def _hex(v):
    return [_hex(t) for t in v] if isinstance(v, list) else float(v).hex()


def _unhex(v):
    return [_unhex(t) for t in v] if isinstance(v, list) else float.fromhex(v)


def to_hex(case):
    rec = {k: v for k, v in case.items() if k not in ("model", "expect", "origin") + _FLOATS}
    rec["model"] = {k: _hex(v) for k, v in case["model"].items()}
    rec.update({k: float(case[k]).hex() for k in _FLOATS if k in case})
    return rec


def from_hex(rec):
    case = {k: v for k, v in rec.items() if k not in ("model",) + _FLOATS}
    case["model"] = {k: _unhex(v) for k, v in rec["model"].items()}
    case.update({k: float.fromhex(rec[k]) for k in _FLOATS if k in rec})
    case.update(origin="drawn", expect={})
    return case


def load_golden():
    return json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else None


DOC = load_golden()


def cases(family, need_fixture=True):
    """the family's named cases: the edge table, then the drawn models of the fixture (which must be there: a test module
    collected without it would run the edge rows alone and look complete)"""
    if DOC is None and need_fixture:
        raise FileNotFoundError(f"{GOLDEN} is missing: run tests/golden/make_path_sweep.py")
    drawn = [from_hex(r) for r in DOC["drawn"].get(family, [])] if DOC else []
    return EDGE[family] + drawn


def shapes_of(case):
    """the (n_steps, monitor_every) a case runs on — for the terminal law (path_offset, 1)"""
    if case["family"] == "merton_terminal":
        return tuple((off, 1) for off in TERMINAL_OFFSETS)
    return SHAPES if case["origin"] == "edge" else (DRAWN_SHAPE,)


def starts_of(case):
    if case["family"] == "merton_terminal":
        return (0,)
    return (0, 1) if case["origin"] == "edge" else (1,)


def antis_of(case):
    return (0, 1) if case["origin"] == "edge" or case["family"] == "merton_terminal" else (1,)


def case_id(case):
    return f"{case['family']}:{case['name']}"


# ---- seeds, draws, evaluation --------------------------------------------------------------------------------------------

def euler_seeds():
    return np.arange(1, N_PATHS + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)   # path_bridge_cases.live_seeds' form


def euler_case(case, n_steps, dW):
    """the case in the form path_bridge_cases.reference takes, mirrors included"""
    return dict(case["model"], dynamics=case["dynamics"], em_split=case["em_split"], n_steps=n_steps, antithetic=1, dW=dW)


def euler_dynamics(case):
    return (_ffi.HH_HESTON, 2) if case["dynamics"] == "heston" else (_ffi.HH_LOGNORMAL, 1)


def seeds_of(family):
    if family == "euler":
        return euler_seeds()
    return {"qe": qc.path_seeds, "bates": bt.path_seeds, "merton_path": mc.path_seeds, "assets": ac.path_seeds,
            "localvol": lc.path_seeds}[family]()[:N_PATHS]


_memo = {}


def cached(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def host_increments(oracle, seeds, n_steps, T):
    """dW[path][step] of the lognormal path kernels for these seeds, from the oracle's host fill (one tile)"""
    tiled = oracle.wiener_fill(_ffi.HH_LOGNORMAL, 0.0, T, n_steps, seeds)
    return bc.increments_of(tiled, len(seeds), n_steps, 1)[:, :, 0]


def draws(oracle, family, key):
    """what a family's walk reads at a step count (terminal law: a path_offset), memoised: T-free draws only"""
    def make():
        if family == "qe":
            s = seeds_of(family)
            return dict(Z=qc.step_normals(oracle, s, key), U=qc.step_uniforms(oracle, s, key))
        if family == "bates":
            return bt.draws(oracle, seeds_of(family), key)
        if family == "euler":
            return dict(U=bc.bridge_uniforms(oracle, seeds_of(family), key))
        if family == "localvol":
            s = seeds_of(family)
            return dict(Z=lc.step_normals(oracle, s, key), U=bc.bridge_uniforms(oracle, s, key))
        if family == "assets":   # of all HH_MAX_ASSETS assets: a case of d assets reads the first d
            return dict(z=ac.asset_normals(oracle, seeds_of(family), key))
        if family == "merton_path":
            s = seeds_of(family)
            with mp.workdps(mc.DPS):
                z = [[mc.box_muller(oracle.philox([k, 1, 0, mc.DOM_JUMP], mc._key(t)))[0] for k in range(key)] for t in s]
            return dict(UJ=mc.path_uniforms(oracle, s, key), z=z)
        return dict(UJ=mc.terminal_uniforms(oracle, mc.TERMINAL_SEED, key, N_PATHS),
                    z=mc.terminal_normals(oracle, mc.TERMINAL_SEED, key, N_PATHS))
    return cached(("draws", family, key), make)


def _histogram(N):
    vals, cnt = np.unique(np.asarray(N), return_counts=True)
    return {int(v): int(c) for v, c in zip(vals, cnt)}


def walk(oracle, case, key, dW=None, mut=None):
    """A case at one step count (terminal law: one path_offset), mirrors included, memoised when unmutated.
    -> dict: usable [path] (bool), counts (what the case exercised), and what `reference` needs.  dW: the Merton path
    form's diffusion increments when the caller has the device's own; the oracle's host fill otherwise."""
    fam = case["family"]

    def make():
        d = draws(oracle, fam, key)
        bad = set()
        out = dict(counts={})
        if fam == "qe":
            out["runs"], counts = qc.walks(case["model"], key, d["Z"], d["U"], 1, case["mart"], mut=mut, psi_c=case["psi_c"],
                                           unusable=bad)
            out["counts"].update(counts)
        elif fam == "euler":   # the whole reference here: its usable mask and clip count come out of the same two runs
            dyn, ncomp = euler_dynamics(case)
            inc = dW
            if inc is None:
                tiled = oracle.wiener_fill(dyn, case["model"]["rho"], case["model"]["T"], key, seeds_of(fam))
                inc = bc.increments_of(tiled[:key * ncomp * 256], N_PATHS, key, ncomp)
            ref = out["ref"] = bc.reference(euler_case(case, key, inc), d["U"])
            bad.update(int(i) for i in np.flatnonzero(~ref["usable"]))
            out["counts"].update(clip_fraction=ref["clip_fraction"])
        elif fam == "localvol":
            surf = out["surf"] = surface_of(case)
            u0 = (math.log(case["model"]["S0"]) - surf["x_lo"]) * (1.0 / surf["h"])
            out.update(Z=d["Z"], U=d["U"])
            out["counts"].update(u_start=u0, nodes=int(surf["vols"].size))
        elif fam == "assets":
            dd = len(case["model"]["spots"])
            out["z"] = [[row[:dd] for row in path] for path in d["z"]]
            L = ac.cholesky_fp64(case["model"]["corr"])
            out["counts"].update(d=dd, kind=case["kind"], L_last=L[-1], weights_below_0=sum(w < 0.0 for w in case["model"]["weights"]),
                                 weights_0=sum(w == 0.0 for w in case["model"]["weights"]),
                                 sigmas_0=sum(t == 0.0 for t in case["model"]["sigmas"]))
        elif fam == "bates":
            jm = jump_model(case, key)
            mean = bt.path_mean(jm, key)
            N = out["N"] = mc.counts_of(d["UJ"], mean, unusable=bad) if mean > 0.0 else np.zeros(d["UJ"].shape, dtype=np.int64)
            out["runs"], seen = bt.walks(jm, key, d, N, 1, case["mart"], psi_c=case["psi_c"], unusable=bad, mut=mut)
            out["counts"].update({k: seen[k] for k in ("quadratic", "exponential", "zero")}, N=_histogram(N))
        else:
            terminal = fam == "merton_terminal"
            jm = jump_model(case, 1 if terminal else key)
            mean = jm["lam"] * jm["T"] if terminal else mc.path_mean(jm)
            N = mc.counts_of(d["UJ"], mean, unusable=bad) if mean > 0.0 else np.zeros(d["UJ"].shape, dtype=np.int64)
            out.update(N=N, model=jm)
            out["counts"]["N"] = _histogram(N)
            if terminal:
                out["z"] = d["z"]
            else:
                out["dW"] = host_increments(oracle, seeds_of(fam), key, jm["T"]) if dW is None else dW
                out["z"] = [[t if N[i][k] > 0 else None for k, t in enumerate(row)] for i, row in enumerate(d["z"])]
        if fam in ("qe", "bates"):
            q = qc.constants(case["model"], key, float, case["psi_c"])
            out["counts"].update(K3=q["K3"].v, E=q["E"].v, ome=1.0 - q["E"].v, A=q["A"].v, K1_is_K2=bool(q["K1"].v == q["K2"].v))
        usable = np.ones(N_PATHS, dtype=bool)
        usable[sorted(bad)] = False
        out["usable"] = usable
        out["counts"]["unusable"] = int((~usable).sum())
        return out
    if mut is not None or dW is not None:
        return make()
    return cached(("walk", case_id(case), key), make)


def reference(case, walked, every, include_start):
    """-> dict(want [member][path][row] mpf, e64, A [member][path][row], members = 2, rows): the family's own reference
    on the walked case; the terminal law has the one row S_T"""
    fam = case["family"]
    if fam in ("qe", "bates"):
        ref = qc.reference(case["model"], walked["runs"], every, include_start)
        f64 = np.array([[[t.v for t in qc.rows_of(case["model"], xs, float, every, include_start) + [vT]]
                         for _, _, xs, vT in mem] for mem in walked["runs"]])
        return dict(ref, rows=6, f64=f64)
    if fam == "euler":   # the bridge rows depend on neither the dates nor the start
        r = walked["ref"]
        return dict(want=r["want"], e64=r["e64"], A=r["A"], members=2, rows=3)
    if fam == "localvol":
        ref = lc.reference(case["model"], walked["surf"], len(walked["Z"][0]), walked["Z"], walked["U"], 1, every, include_start)
        walked["counts"].setdefault("where", {}).update({f"{len(walked['Z'][0])}x{every}+{include_start}":
                                                         [ref["counts"].get(k, 0) for k in (-1, 0, 1)]})
        return dict(ref, rows=7)
    if fam == "assets":
        ref = ac.path_reference(case["model"], case["kind"], walked["z"], 1, every, include_start)
        assert all(t[0] > 0 for mem in ref["want"] for t in mem), case_id(case)   # a spread's index stays above 0
        return dict(ref, rows=5)
    if fam == "merton_path":
        ref = mc.path_reference(walked["model"], walked["dW"], walked["N"], walked["z"], every, include_start)
        return dict(ref, rows=5)
    ref = mc.terminal_reference(walked["model"], walked["z"], walked["N"])
    return dict(want=[[[t] for t in mem] for mem in ref["want"]], e64=ref["e64"][:, :, None], A=ref["A"][:, :, None],
                members=2, rows=1)


def scales(ref):
    """what a bar is measured against, [member][path][row]: the value itself; for the four spot rows the path's largest
    monitored spot (a minimum's magnitude is, by path_bridge_cases._pick, that of the larger operand); 1 at least for the
    sum of logs; for var_T the case's median at least (a small v′ is a square of a difference)"""
    vals = np.array([[[abs(float(t)) for t in row] for row in mem] for mem in ref["want"]])
    scale = vals.copy()
    if ref["rows"] == 3:   # S_T, CMAX_S, CMIN_S
        return np.repeat(vals[:, :, 1:2], 3, axis=2)
    if ref["rows"] >= 5:
        for r in (0, 2, 3, 4, 5, 6)[:4 if ref["rows"] < 7 else 6]:   # with bridge rows: the continuous maximum
            scale[:, :, r] = vals[:, :, 2 if ref["rows"] < 7 else 5]
        scale[:, :, 1] = np.maximum(vals[:, :, 1], 1.0)
    if ref["rows"] == 6:
        scale[:, :, 5] = np.maximum(vals[:, :, 5], np.median(vals[:, :, 5]))
    return scale


def bars(case, ref):
    """the bars a case's numbers are held to: path_bar(e64, A), and never more than FP64_SIZED of the path's scale — but on
    the ILL_CONDITIONED rows, where the fp64 restatement itself is farther than that from the 50-digit run"""
    b = etc.path_bar(ref["e64"], ref["A"])
    return b if case_id(case) in ILL_CONDITIONED else np.minimum(b, FP64_SIZED * scales(ref))


def digest(ref, usable):
    """per row, the sum of the 50-digit reference over the usable members, to 30 digits"""
    with mp.workdps(qc.DPS):
        return [mp.nstr(mp.fsum(ref["want"][m][i][row] for m in range(ref["members"]) for i in np.flatnonzero(usable)), 30)
                for row in range(ref["rows"])]


def combos(case):
    """every (shape key, monitor_every, include_start) a case's reference is formed on"""
    return [(key, every, start) for key, every in shapes_of(case) for start in starts_of(case)]


def check_expectations(case, walks_by_key):
    """the counts that show a case exercises what it is for (asserted by the maker and by the host test)"""
    e = case["expect"]
    keys = list(walks_by_key)
    multi = [k for k in keys if case["family"] == "merton_terminal" or k > 1]   # on one step every member shares one ψ
    for k, w in walks_by_key.items():
        c = w["counts"]
        assert c["unusable"] <= CAP, (case_id(case), k, c["unusable"])
        if e.get("K3_zero"):
            assert c["K3"] == 0.0, (case_id(case), k, c["K3"])
        if e.get("K1_is_K2"):
            assert c["K1_is_K2"], (case_id(case), k)
        if e.get("A_positive"):
            assert c["A"] > 0.0, (case_id(case), k, c["A"])
        if e.get("small_ome"):
            assert 0.0 < c["ome"] <= 32 * 2.0 ** -53, (case_id(case), k, c["ome"])
        if e.get("all_quadratic"):
            assert c["exponential"] == 0, (case_id(case), k, c)
        if e.get("clips") and k > 1:
            assert c["clip_fraction"] >= etc.MIN_CLIP_FRACTION, (case_id(case), k, c["clip_fraction"])
        if "on_node" in e:
            assert abs(c["u_start"] - (c["nodes"] // len(lc.surface(case["surface"])["times"]) - 1) * e["on_node"]) < 1e-9, (case_id(case), c["u_start"])
        if e.get("off_low") and "where" in c and k > 1:
            assert all(v[0] > 0 for v in c["where"].values()), (case_id(case), c["where"])
        if e.get("off_high") and "where" in c and k > 1:
            assert all(v[2] > 0 for v in c["where"].values()), (case_id(case), c["where"])
        if e.get("thin_factor"):
            assert 0.0 < c["L_last"] < 0.05, (case_id(case), c["L_last"])
        if e.get("negative_weight"):
            assert c["weights_below_0"] > 0, case_id(case)
        if e.get("max_N"):
            assert max(c["N"]) >= e["max_N"], (case_id(case), k, c["N"])
    if e.get("both_branches"):
        assert multi and all(walks_by_key[k]["counts"]["quadratic"] > 0 and walks_by_key[k]["counts"]["exponential"] > 0
                             for k in multi), case_id(case)
    if e.get("tiny_E"):
        assert all(walks_by_key[k]["counts"]["E"] < 1e-300 for k in keys), case_id(case)
        assert any(walks_by_key[k]["counts"]["E"] > 0.0 for k in keys), case_id(case)


def json_counts(counts):
    return {k: ({str(n): c for n, c in v.items()} if isinstance(v, dict) else v) for k, v in counts.items()}


# ---- the C structs of a case ---------------------------------------------------------------------------------------------

def qe_struct(case):
    return _ffi.make_qe(case["psi_c"], case["mart"])


def jump_struct(case, n_steps):
    jm = jump_model(case, n_steps)
    return _ffi.make_jump(jm["lam"], jm["mu_j"], jm["sigma_j"])


def localvol_struct(case):
    return lc.localvol_of(case.get("surf") or surface_of(case))


def assets_struct(case):
    return ac.assets_of(case["model"], case["kind"])


def payoffs_of(case):
    """one payoff of every kind the case admits — the list of the families' own tests, struck around the case's own spot:
    a drawn S0 runs from 1 to 1000, where strikes near 100 would leave most rows identically zero"""
    if case["family"] == "assets":
        spread = any(w < 0.0 for w in case["model"]["weights"])   # the geometric Asian is refused on a spread
        return [p for p in ac.payoff_list(case["model"], case["kind"]) if not (spread and p.kind == _ffi.HH_PAYOFF_ASIAN_GEOM)]
    s = case["model"]["S0"] / 100.0
    return [pc.payoff(pc.VANILLA, 100.0 * s, 1.0), pc.payoff(pc.ARITH, 98.0 * s, 1.0), pc.payoff(pc.GEOM, 101.0 * s, -1.0),
            pc.payoff(pc.BARRIER, 95.0 * s, 1.0, pc.DOWN_OUT, 80.0 * s, 1.5 * s), pc.payoff(pc.DCASH, 102.0 * s, 1.0, cash=3.0),
            pc.payoff(pc.DASSET, 99.0 * s, -1.0), pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FLOAT, 0.0, 1.0),
            pc.payoff(_ffi.HH_PAYOFF_LOOKBACK_FIXED, 100.0 * s, 1.0)]


def model_struct(case):
    if case["family"] == "assets":
        return ac.model_of(case["model"])
    if case["family"] == "localvol":
        return lc.model_of(case["model"])
    if case["family"] == "euler":
        return qc.model_of(case["model"])
    return qc.model_of(case["model"]) if case["family"] in ("qe", "bates") else mc.model_of(case["model"])
