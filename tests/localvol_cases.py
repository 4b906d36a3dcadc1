"""Local volatility on a tabulated surface (include/hedgehog_mc.h, "Local volatility on a tabulated surface"): what the
host and the device tests share.

  * the lookup and the step in PYTHON FLOATS, operation for operation as csrc/hh_localvol.h writes them (row_of, cell_of,
    sigma_of, step_of; fma by exact rational arithmetic, rounded once): the same IEEE operations in the same order, so
    tests/c/localvol_host_check.cpp must give their bits;
  * the same step restated generically in the number type (member): mpmath at 50 digits is the reference, Python floats
    "the same formulas in fp64", whose distance from the 50-digit run is e64; every value carries qe_cases.VA's two
    running magnitudes and the bar of a statistic is euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A), imported.
    The row j_k is the float run's in both (a host-formed integer); the CELL of a state is no rounding matter: the
    lookup is continuous across a cell edge and across both clamps, so a state within rounding of an edge gets the same
    σ from either side to rounding;
  * the draws of the lognormal Euler kernel from the oracle's host Philox: the normals of block (h, 0, 0, 0) restated at
    50 digits by hh_rng.h's formulas, the bridge uniforms of block (k, 0, 0, 3);
  * the CEV model's closed form (Schroder) at mpmath precision, and its local volatility.
"""
import json
import math
import os
from fractions import Fraction

import mpmath as mp
import numpy as np

from hedgehog_jl_amd import _ffi
from oracle import euler_exact as ex
from tests.lognormal_exact_cases import box_muller
from tests.path_bridge_cases import bridge_uniforms  # noqa: F401  (the device tests draw them here)
from tests.qe_cases import VA, _div, _expo, _log_input, _pick, _sqrt

DPS = ex.DPS
DOM_EULER = 0
PATH_N = 257
PATH_SHAPES = ((1, 1), (3, 1), (12, 4))  # (n_steps, monitor_every)
MODEL = dict(S0=100.0, r_drift=0.03, T=1.0)
X0 = math.log(MODEL["S0"])


# ---- the header's operations in Python floats: bit for bit -------------------------------------------------------------

def fma(a, b, c):
    """one rounding of a·b + c"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def row_of(times, t):
    """hh_localvol.h: localvol_row -> (j, w)"""
    n = len(times)
    if n < 2:
        return 0, 0.0
    j = 0
    while j + 2 < n and times[j + 1] <= t:
        j += 1
    w = (t - times[j]) / (times[j + 1] - times[j])
    w = 0.0 if w < 0.0 else w
    w = 1.0 if w > 1.0 else w
    return j, w


def cell_of(x, x_lo, inv_h, n_x):
    """hh_localvol.h: localvol_cell -> (i, f, where): where = -1 clamped below, +1 above, 0 inside the grid"""
    u = (x - x_lo) * inv_h
    top = float(n_x - 1)
    where = -1 if u < 0.0 else 1 if u > top else 0
    u = 0.0 if u < 0.0 else u
    u = top if u > top else u
    i = min(int(u), n_x - 2)
    return i, u - float(i), where


def sigma_of(vols, n_x, j, w, two_rows, i, f):
    """hh_localvol.h: localvol_sigma on the row-major table `vols`"""
    c0, c1 = vols[j * n_x + i], vols[j * n_x + i + 1]
    if two_rows:
        c0 = fma(w, vols[(j + 1) * n_x + i] - c0, c0)
        c1 = fma(w, vols[(j + 1) * n_x + i + 1] - c1, c1)
    return fma(f, c1 - c0, c0)


def step_of(x, sigma, r, dt, dW):
    """hh_localvol.h: localvol_step"""
    g = r - 0.5 * sigma * sigma
    return fma(sigma, dW, fma(dt, g, x))


def get_sigma(surface, t, x):
    """σ(t, x) of a surface dict (times, vols [n_times][n_x] array, x_lo, h) by the operations above"""
    vols = np.asarray(surface["vols"], dtype=np.float64)
    n_t, n_x = vols.shape
    j, w = row_of([float(s) for s in surface["times"]], float(t))
    i, f, _ = cell_of(float(x), float(surface["x_lo"]), 1.0 / float(surface["h"]), n_x)
    return sigma_of([float(v) for v in vols.reshape(-1)], n_x, j, w, n_t > 1, i, f)


# ---- the surfaces of the device tests ------------------------------------------------------------------------------------

def _wavy(n_t, n_x, x_lo, h):
    """a smooth positive table that varies in both directions"""
    j, i = np.meshgrid(np.arange(n_t), np.arange(n_x), indexing="ij")
    x = x_lo + h * i
    return 0.22 + 0.05 * np.sin(3.0 * (x - X0) + 0.7 * j) + 0.02 * j / max(n_t - 1, 1) - 0.04 * (x - X0)


def surface(name):
    """name -> dict(times, vols, x_lo, h).  T = 1 in every case.
      one_row    (1, 2): no second row, one cell, wide: every state inside
      two_by_3   (2, 3): times 0.25 and 0.5 — steps before, between (12 steps) and after them
      narrow     (5, 33): 33 nodes over log S0 ± 0.08 — at σ ≈ 0.2 and dt >= 1/12 states leave the grid on both sides;
                 times 0.2 .. 0.8 start after 0 and end before T: both time clamps
      cap        (32, 256): HH_LV_MAX_NODES, the full 64 KiB
      long_row   (1, 8192): a row longer than the workgroup's load stride"""
    if name == "one_row":
        n_t, n_x, x_lo, h, times = 1, 2, X0 - 2.0, 4.0, [0.0]
    elif name == "two_by_3":
        n_t, n_x, x_lo, h, times = 2, 3, X0 - 0.5, 0.5, [0.25, 0.5]
    elif name == "narrow":
        n_t, n_x, x_lo, h, times = 5, 33, X0 - 0.08, 0.005, [0.2, 0.35, 0.5, 0.65, 0.8]
    elif name == "cap":
        n_t, n_x, x_lo, h, times = 32, 256, X0 - 1.0, 2.0 / 255, [0.03 * (j + 1) for j in range(32)]
    elif name == "long_row":
        n_t, n_x, x_lo, h, times = 1, 8192, X0 - 1.0, 2.0 / 8191, [0.5]
    else:
        raise KeyError(name)
    vols = _wavy(n_t, n_x, x_lo, h)
    assert vols.min() > 0.05
    return dict(times=np.array(times), vols=vols, x_lo=x_lo, h=h)


SURFACES = ("one_row", "two_by_3", "narrow", "cap", "long_row")


def path_seeds():
    return np.arange(1, PATH_N + 1, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03) + np.uint64(11)


def _key(seed):
    return [int(seed) & 0xFFFFFFFF, int(seed) >> 32]


def step_normals(oracle, seeds, n_steps):
    """Z[i][k] at 50 digits: step k takes component k & 1 of the Box–Muller pair of block (k >> 1, 0, 0, 0) under seeds[i]"""
    with mp.workdps(DPS):
        out = []
        for s in seeds:
            pairs = [box_muller(oracle.philox([h, 0, 0, DOM_EULER], _key(s))) for h in range((n_steps + 1) // 2)]
            out.append([pairs[k >> 1][k & 1] for k in range(n_steps)])
        return out


# ---- the restatement, generic in the number type ---------------------------------------------------------------------------

def _neg2log(u, num):
    l = ex._log(num(u))
    m = 2 * max(abs(l), 1)
    return VA(-2 * l, m, m)


def _half(m):
    return VA(m.v / 2, m.a / 2, m.b / 2)


def _bridge(x0, x1, q, L, sign):
    d = x1 - x0
    root = _sqrt(d * d + q * L)
    return _half(x0 + x1 + (root if sign > 0 else -root))


def _lookup(surf, num, x, j, w, counts):
    vols, n_x = surf["vols"], surf["vols"].shape[1]
    u = (x - VA(num(float(surf["x_lo"])))) * VA(num(1.0 / float(surf["h"])))
    top = n_x - 1
    if u.v < 0:
        u, where = VA(num(0.0)), -1
    elif u.v > top:
        u, where = VA(num(float(top))), 1
    else:
        where = 0
    if counts is not None:
        counts[where] = counts.get(where, 0) + 1
    i = min(int(u.v), n_x - 2)
    f = u - VA(num(float(i)))

    def node(jj, ii):
        return VA(num(float(vols[jj, ii])))
    c0, c1 = node(j, i), node(j, i + 1)
    if vols.shape[0] > 1:
        c0 = c0 + w * (node(j + 1, i) - c0)
        c1 = c1 + w * (node(j + 1, i + 1) - c1)
    return c0 + f * (c1 - c0)


def member(model, surf, n_steps, num, Z, U, mirror, monitor_every, include_start, counts=None):
    """The seven rows of one member (enum hh_path_stat; CMAX_S, CMIN_S from the bridge draws U[k] = (U1, U2)) as VAs.
    Z[k]: the step's normal; the mirror takes −dW on its own state and its own σ, and the bridge draws swapped."""
    half = VA(num(0.5))
    r = VA(num(model["r_drift"]))
    dt = VA(num(model["T"]) / n_steps)
    sqrt_dt = _sqrt(dt)
    times = [float(t) for t in surf["times"]]
    dt64 = model["T"] / n_steps
    x = _log_input(num, model["S0"])
    rows = None
    cmax = cmin = x

    def take(S, xs):
        nonlocal rows
        rows = [S, xs, S, S, S] if rows is None else \
            [rows[0] + S, rows[1] + xs, _pick(rows[2], S, True), _pick(rows[3], S, False), S]

    if include_start:
        take(VA(num(model["S0"])), x)
    for k in range(n_steps):
        j, _ = row_of(times, float(k) * dt64)
        if len(times) > 1:
            tk = VA(num(float(k))) * dt
            w = _div(tk - VA(num(times[j])), VA(num(times[j + 1])) - VA(num(times[j])))
            w = VA(num(0.0)) if w.v < 0 else VA(num(1.0)) if w.v > 1 else w
        else:
            w = VA(num(0.0))
        sg = _lookup(surf, num, x, j, w, counts)
        z = VA(num(Z[k]))
        dW = sqrt_dt * (-z if mirror else z)
        x0 = x
        g = r - (half * sg) * sg
        x = (x + dt * g) + sg * dW
        L1, L2 = _neg2log(U[k][0], num), _neg2log(U[k][1], num)
        if mirror:
            L1, L2 = L2, L1
        q = (sg * sg) * dt
        cmax = _pick(_pick(cmax, _bridge(x0, x, q, L1, +1), True), x, True)
        cmin = _pick(_pick(cmin, _bridge(x0, x, q, L2, -1), False), x, False)
        if (k + 1) % monitor_every == 0:
            take(_expo(x), x)
    return rows + [_expo(cmax), _expo(cmin)]


def reference(model, surf, n_steps, Z, U, anti, monitor_every, include_start):
    """-> want [member][path][row] (mpf), e64 and A (float arrays [member][path][7]), counts {-1, 0, +1: steps}"""
    members = 2 if anti else 1
    n = len(Z)
    want = [[None] * n for _ in range(members)]
    e64, A = np.zeros((members, n, 7)), np.zeros((members, n, 7))
    counts = {}
    with mp.workdps(DPS):
        for i in range(n):
            for m in range(members):
                ref = member(model, surf, n_steps, mp.mpf, Z[i], U[i], m == 1, monitor_every, include_start)
                f64 = member(model, surf, n_steps, float, [float(t) for t in Z[i]], U[i], m == 1, monitor_every,
                             include_start, counts)
                want[m][i] = [t.v for t in ref]
                A[m, i] = [float(t.A) for t in ref]
                e64[m, i] = [float(abs(mp.mpf(b.v) - a.v)) for a, b in zip(ref, f64)]
    return dict(want=want, e64=e64, A=A, members=members, counts=counts)


# ---- the C structs of a case ---------------------------------------------------------------------------------------------

def model_of(model=MODEL, strike=100.0, cp=1.0, sigma=float("nan")):
    """model->sigma is not read by the local-vol entry points: NaN unless a test asks for the lognormal kernel"""
    return _ffi.make_model(S0=model["S0"], V0=0.0, kappa=0.0, theta=0.0, sigma=sigma, rho=0.0, r=model["r_drift"],
                           T=model["T"], strike=strike, cp=cp)


def config_of(n, n_steps, seeds, anti=0, **kw):
    return _ffi.make_config(_ffi.HH_LOGNORMAL, _ffi.HH_EULER_MARUYAMA, n, n_steps=n_steps, antithetic=anti, seeds=seeds, **kw)


def localvol_of(surf):
    return _ffi.make_localvol(surf["times"], surf["vols"], surf["x_lo"], surf["h"])


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "localvol_exact.json")


def load_golden():
    """the fixture of tests/golden/make_localvol_exact.py: its JSON with the two arrays beside it loaded in place —
    "fine" [5][21][257], "coarse" [n_centre][5] on the nodes "coarse_nodes" """
    doc = json.load(open(GOLDEN))
    for k in ("coarse", "fine"):
        doc[k] = np.load(GOLDEN.replace(".json", f"_{k}.npy"))
    return doc


# ---- the CEV model: dS = rS dt + δ S^β dW, 0 < β < 1 -----------------------------------------------------------------------

CEV = dict(S0=100.0, r=0.03, beta=0.5, sigma0=0.25)  # δ = σ0·S0^{1−β}: σ(S) = σ0·(S/S0)^{β−1}


def cev_sigma(S):
    return CEV["sigma0"] * (np.asarray(S, dtype=np.float64) / CEV["S0"]) ** (CEV["beta"] - 1.0)


def ncx2_cdf(z, k, lam):
    """the noncentral chi-square CDF χ²(z; k, λ) = Σ_j e^{−λ/2}(λ/2)^j/j! · P(k/2 + j, z/2) at the working precision; the
    Poisson weights are summed outwards from their mode, P by its recurrence P(a + 1, y) = P(a, y) − y^a e^{−y}/Γ(a + 1)"""
    z, k, lam = mp.mpf(z), mp.mpf(k), mp.mpf(lam)
    y, m = z / 2, lam / 2
    j0 = int(mp.floor(m))
    w0 = mp.exp(-m + j0 * mp.log(m) - mp.loggamma(j0 + 1))
    a0 = k / 2 + j0
    P0 = mp.gammainc(a0, 0, y, regularized=True)
    t0 = mp.exp(a0 * mp.log(y) - y - mp.loggamma(a0 + 1))  # y^a e^{−y}/Γ(a + 1)
    tiny = mp.mpf(10) ** (-mp.mp.dps - 5)
    total = w0 * P0
    w, P, t, a, j = w0, P0, t0, a0, j0
    while True:  # upwards
        P, j = P - t, j + 1
        w = w * m / j
        a = a + 1
        t = t * y / a
        total += w * P
        if w < tiny and j > m:
            break
    w, P, t, a, j = w0, P0, t0, a0, j0
    while j > 0:  # downwards
        t = t * a / y
        a = a - 1
        w = w * j / m
        j -= 1
        P = P + t
        total += w * P
        if w < tiny:
            break
    return total


def cev_call(T, K):
    """Schroder's closed form for 0 < β < 1"""
    S0, r, beta = mp.mpf(CEV["S0"]), mp.mpf(CEV["r"]), mp.mpf(CEV["beta"])
    T, K = mp.mpf(T), mp.mpf(K)
    delta = mp.mpf(CEV["sigma0"]) * S0 ** (1 - beta)
    v = delta ** 2 / (2 * r * (beta - 1)) * (mp.exp(2 * r * (beta - 1) * T) - 1)
    D = K * mp.exp(-r * T)
    a = D ** (2 * (1 - beta)) / ((1 - beta) ** 2 * v)
    b = 1 / (1 - beta)
    c = S0 ** (2 * (1 - beta)) / ((1 - beta) ** 2 * v)
    return S0 * (1 - ncx2_cdf(a, b + 2, c)) - D * ncx2_cdf(c, b, a)
