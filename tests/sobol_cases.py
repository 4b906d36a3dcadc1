"""The quasi-Monte Carlo fill restated (include/hedgehog_mc.h, "Quasi-Monte Carlo"), for tests/test_sobol_host.py,
tests/test_gpu_sobol.py and tests/golden/make_sobol_exact.py: the point rule in numpy, the digital shift from Philox in
numpy, the Brownian-bridge table and the kernel's walk of it in Python, the fill at 50 digits with its bars, and the
numpy restatement of a randomised QMC price that sizes the convergence conditions.  TEST INFRASTRUCTURE ONLY.

The bars of the fill.  Every value carries oracle/euler_exact.py's running magnitude A (|x| + |y| for a sum, A·|c| for a
product with an exact constant), so that tests/euler_tangent_cases.path_bar(e64, A) = 20·max(e64, ε·A) bounds what any
careful fp64 evaluation of the same operations may differ by — e64 being the distance of the Python-float run of the same
operations from the 50-digit run.  The normal enters with tests/math_bars.py's bar for normal_quantile: NQ ulp, taken
as NQ·ε·|z|, carried linearly through wl·W_l + wr·W_r + sd·z, the difference, the correlation and sqrt_dt, and ADDED.
The table's numbers (wl, wr, sd), sqrt_dt, ρ and sqrt(1 − ρ²) are inputs of the kernel: the fp64 numbers the host forms."""
import json
import math
import os

import mpmath as mp
import numpy as np

from hedgehog_jl_amd import _ffi
from tests import euler_tangent_cases as etc
from tests.math_bars import BARS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sobol_exact.json")
DPS = 50
EPS = 2.0 ** -52
NQ = BARS["nquant"]
DOM_SOBOL = 7
MAX_DIMS = 4096
TILE = 256
INCREMENTAL, BRIDGE = 0, 1
BRIDGE_STEPS = (1, 2, 3, 5, 8, 252)

# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------
POINT_COUNTS = (1, 255, 256, 257, 513)
POINT_OFFSETS = (0, 1, 2 ** 20 - 3, 2 ** 32 - 513)
POINT_DIMS = (0, 1, 503, 4095)
FILL_SHAPES = ((1, 1), (2, 1), (3, 1), (5, 2), (8, 2), (16, 2), (252, 2))
FILL_POINTS = 257
FILL_RHOS = (0.0, -0.7)
FILL_T = 1.5
FILL_SEED, FILL_RANDOMIZATION = 0x9E3779B97F4A7C15, 3
SHIFT_SEED = 0x0123456789ABCDEF
# the Heston model of the convergence conditions (the issue's) and their fixed seeds; tests/golden/make_sobol_exact.py
# keeps a seed only where the numpy restatement clears conditions (c) and (d) by 1.25x
HESTON = dict(S0=100.0, K=100.0, r=0.03, T=1.0, V0=0.04, theta=0.04, kappa=1.5, sigma=0.5, rho=-0.7)
LOGNORMAL = dict(S0=100.0, K=100.0, r=0.03, T=1.0, sigma=0.2)
CONV_SEED = 20261020
CONV_R = 16
CONV_N_EXACT, CONV_N_HESTON = 2 ** 12, 2 ** 14
CONV_MARGIN = 1.25


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- the point rule --------------------------------------------------------------------------------------------------------

def directions(dims):
    """[len(dims)][32] direction words from hh_sobol_directions (host arithmetic: no GPU)"""
    lib = _ffi.load_library()
    out = np.zeros((len(dims), 32), dtype=np.uint32)
    for k, d in enumerate(dims):
        assert lib.hh_sobol_directions(int(d), out[k].ctypes.data) == 0, d
    return out


def expand(poly, m_init):
    """the 32 direction words of a dimension from its polynomial (both end bits included) and initial values, in Python
    integers: m_j = m_(j−s) ^ 2^s·m_(j−s) ^ the XOR of 2^k·m_(j−k) over the inner coefficients a_k = bit s − k of poly;
    poly = 1 (dimension 0): every m = 1"""
    s = poly.bit_length() - 1
    m = list(m_init[:s]) if s else [1] * 32
    for j in range(len(m), 32):
        t = m[j - s] ^ (m[j - s] << s)
        for k in range(1, s):
            if (poly >> (s - k)) & 1:
                t ^= m[j - k] << k
        m.append(t)
    return [(m[j] << (31 - j)) & 0xFFFFFFFF for j in range(32)]


def points(v, idx):
    """words [dim][point] of points idx (uint64 array below 2^32) from direction words v [dim][32]: Gray-code order"""
    i = np.asarray(idx, dtype=np.uint64)
    g = (i ^ (i >> np.uint64(1))).astype(np.uint32)
    x = np.zeros((v.shape[0], g.size), dtype=np.uint32)
    for b in range(32):
        x ^= np.where((g >> np.uint32(b)) & np.uint32(1), v[:, b:b + 1], np.uint32(0)).astype(np.uint32)
    return x


def philox4x32_10(ctr, key):
    """Philox4x32-10 on arrays: ctr [4][n] uint32, key (k0, k1) -> [4][n] (hh_rng.h's rounds)"""
    c = [np.asarray(t, dtype=np.uint64) for t in ctr]
    k0, k1 = int(key[0]), int(key[1])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.array(c).astype(np.uint32)


def shift_words(dims, randomization, seed):
    """the shift word of each dimension: word d & 3 of block (d >> 2, r, 0, kDomSobol) keyed by the seed's two halves"""
    d = np.asarray(dims, dtype=np.uint64)
    z = np.zeros_like(d)
    blk = philox4x32_10([d >> np.uint64(2), z + np.uint64(randomization), z, z + np.uint64(DOM_SOBOL)],
                        (seed & 0xFFFFFFFF, seed >> 32))
    return blk[(d & np.uint64(3)).astype(np.int64), np.arange(d.size)]


def words(dims, idx, shifted=False, randomization=0, seed=0):
    x = points(directions(dims), idx)
    return x ^ shift_words(dims, randomization, seed)[:, None] if shifted else x


def u_of(x):
    """(x + 1/2)·2^-32, exact"""
    return (np.asarray(x, dtype=np.float64) + 0.5) * 2.0 ** -32


# ---- the bridge ------------------------------------------------------------------------------------------------------------

def bridge_nodes(n):
    """[(l, m, r, depth, wl, wr, sd)] in construction order; node 0 is the terminal value (l = 0, m = r = n)"""
    nodes = [(0, n, n, 0, 0.0, 0.0, math.sqrt(float(n)))]
    queue, head = [(0, n, 0)], 0
    while head < len(queue):
        l, r, depth = queue[head]
        head += 1
        if r - l < 2:
            continue
        m = (l + r) // 2
        a, b, ln = float(m - l), float(r - m), float(r - l)
        nodes.append((l, m, r, depth, b / ln, a / ln, math.sqrt(a * b / ln)))
        queue += [(l, m, depth + 1), (m, r, depth + 1)]
    return nodes


def bridge_matrix(n):
    """A [n + 1][n]: W_t = Σ_j A[t][j]·z_j"""
    A = np.zeros((n + 1, n))
    for j, (l, m, r, _, wl, wr, sd) in enumerate(bridge_nodes(n)):
        A[m] = (wl * A[l] + wr * A[r] if j else 0.0)
        A[m, j] += sd
    return A


def bridge_ops(n):
    """the kernel's walk (csrc/hh_sobol.h, sobol_bridge_ops): [(emit, index, slot_l, slot_r, slot_m, wl, wr, sd)], n_slots"""
    nodes = bridge_nodes(n)
    node_of, slot_of, slots = {}, {0: 0, n: 1}, 2
    for j, nd in enumerate(nodes[1:], 1):
        node_of[nd[1]], slot_of[nd[1]] = j, 2 + nd[3]
        slots = max(slots, 3 + nd[3])
    ops, stack = [(0, 0, 0, 0, 1, 0.0, 0.0, nodes[0][6])], [(0, n)]
    while stack:
        l, r = stack.pop()
        if r - l == 1:
            ops.append((1, l, slot_of[l], slot_of[r], 0, 0.0, 0.0, 0.0))
            continue
        m = (l + r) // 2
        nd = nodes[node_of[m]]
        ops.append((0, node_of[m], slot_of[l], slot_of[r], slot_of[m], nd[4], nd[5], nd[6]))
        stack += [(m, r), (l, m)]
    return ops, slots


def walk(ops, n_slots, z):
    """the unit-variance steps d[k] the walk writes from the normals z[j] (floats): what the kernel does, slot by slot"""
    slot, d, written = [0.0] * n_slots, {}, []
    for emit, index, sl, sr, sm, wl, wr, sd in ops:
        if emit:
            d[index] = slot[sr] - slot[sl]
            written.append(index)
        else:
            slot[sm] = wl * slot[sl] + (wr * slot[sr] + sd * z[index])
    return d, written


# ---- the fill at 50 digits, with magnitudes --------------------------------------------------------------------------------

def quantiles_mp(u):
    """Φ⁻¹ of the exact fp64 numbers u at the working precision: one 50-digit Φ at the fp64 quantile z0, then the inverse's
    Taylor series in δ = (u − Φ(z0))/φ(z0) to third order — |δ| is below 1e-14, so the remainder is below 1e-56"""
    from scipy.special import ndtri
    r2, s2pi = mp.sqrt(2), mp.sqrt(2 * mp.pi)
    out = []
    for t, z0 in zip(u, ndtri(np.asarray(u, dtype=np.float64))):
        z0 = mp.mpf(float(z0))
        d = (mp.mpf(float(t)) - mp.erfc(-z0 / r2) / 2) * s2pi * mp.exp(z0 * z0 / 2)
        out.append(z0 + d + z0 * d * d / 2 + (2 * z0 * z0 + 1) * d ** 3 / 6)
    return out


class V:
    """value v, magnitude a, and q: what the normals' own bars may move it by — numbers, or arrays over the points (v an
    object array of mpf in the 50-digit run)"""
    __slots__ = ("v", "a", "q")

    def __init__(self, v, a, q):
        self.v, self.a, self.q = v, a, q

    def __add__(self, o):
        return V(self.v + o.v, self.a + o.a, self.q + o.q)

    def __sub__(self, o):
        return V(self.v - o.v, self.a + o.a, self.q + o.q)

    def scale(self, c):
        return V(self.v * c, self.a * abs(c), self.q * abs(c))


def steps_of(n_steps, construction, z):
    """the unit-variance steps [k] of one factor from its normals z[j] (V), in the header's operation order"""
    if construction == INCREMENTAL:
        return list(z)
    W = {0: None}
    for j, (l, m, r, _, wl, wr, sd) in enumerate(bridge_nodes(n_steps)):
        inner = z[j].scale(sd)
        if j and W[r] is not None:
            inner = W[r].scale(wr) + inner
        W[m] = W[l].scale(wl) + inner if j and W[l] is not None else inner
    return [W[k + 1] - W[k] if W[k] is not None else W[k + 1] for k in range(n_steps)]


def increments(n_steps, ncomp, rho, T, d):
    """dW[k][comp] (V) from the unit-variance steps d[comp][k] (V)"""
    sqrt_dt = math.sqrt(T / float(n_steps))
    rho_c = math.sqrt(1.0 - rho * rho)
    out = []
    for k in range(n_steps):
        row = [d[0][k].scale(sqrt_dt)]
        if ncomp == 2:
            row.append((d[0][k].scale(rho) + d[1][k].scale(rho_c)).scale(sqrt_dt))
        out.append(row)
    return out


_z_cache, _steps_cache = {}, {}


def normals_mp(x):
    """50-digit quantiles of the words x [dim][point] as an object array, computed once per word"""
    x = np.asarray(x)
    new = sorted({int(w) for w in x.ravel()} - _z_cache.keys())
    with mp.workdps(DPS):
        _z_cache.update(zip(new, quantiles_mp([(w + 0.5) * 2.0 ** -32 for w in new])))
    out = np.empty(x.shape, dtype=object)
    for idx, w in np.ndenumerate(x):
        out[idx] = _z_cache[int(w)]
    return out


def fill_reference(n_steps, ncomp, construction, rho, T, x):
    """(hi, lo, bar), each [point][step][comp]: the 50-digit value as hi + lo in two floats (|got − value| is then
    |(got − hi) − lo|, the first difference being exact wherever got is within a factor two of hi) and its bar — of the
    fill of the points whose words are x [ncomp·n_steps][point]"""
    zq = normals_mp(x)
    n = x.shape[1]
    hi, lo, bars = (np.zeros((n, n_steps, ncomp)) for _ in range(3))
    to_float = np.frompyfunc(float, 1, 1)
    with mp.workdps(DPS):
        zf = to_float(zq).astype(np.float64)
        zm = [[V(zq[ncomp * j + c], np.abs(zf[ncomp * j + c]), NQ * EPS * np.abs(zf[ncomp * j + c])) for j in range(n_steps)]
              for c in range(ncomp)]
        z64 = [[V(zf[ncomp * j + c], np.abs(zf[ncomp * j + c]), 0.0) for j in range(n_steps)] for c in range(ncomp)]
        key = (n_steps, ncomp, construction, x.tobytes())
        if key not in _steps_cache:  # the steps do not depend on ρ and T: the cases that differ in those share them
            _steps_cache[key] = tuple([steps_of(n_steps, construction, zs[c]) for c in range(ncomp)] for zs in (zm, z64))
        ref = increments(n_steps, ncomp, rho, T, _steps_cache[key][0])
        f64 = increments(n_steps, ncomp, rho, T, _steps_cache[key][1])
        for k in range(n_steps):
            for c in range(ncomp):
                hi[:, k, c] = to_float(ref[k][c].v).astype(np.float64)
                lo[:, k, c] = to_float(ref[k][c].v - hi[:, k, c].astype(object)).astype(np.float64)
                e64 = np.abs((f64[k][c].v - hi[:, k, c]) - lo[:, k, c])
                bars[:, k, c] = etc.path_bar(e64, ref[k][c].a) + ref[k][c].q
    return hi, lo, bars


def fill_errors(got, hi, lo):
    """|got − (hi + lo)| elementwise"""
    return np.abs((np.asarray(got) - hi) - lo)


def untile(buf, n_points, n_steps, ncomp):
    """tile-major dW[tile][step][comp][256] -> ([point][step][comp], the padded lanes of the last tile)"""
    t = np.asarray(buf).reshape(-1, n_steps, ncomp, TILE)
    flat = t.transpose(0, 3, 1, 2).reshape(-1, n_steps, ncomp)
    return flat[:n_points], flat[n_points:]


# ---- the numpy restatement of a randomised QMC price (tests/golden/make_sobol_exact.py) ------------------------------------

def normals_np(n_steps, ncomp, n_points, randomization, seed):
    """z [ncomp·n_steps][point] in fp64 (scipy's quantile: the law, not the device's bits)"""
    from scipy.special import ndtri
    dims = np.arange(ncomp * n_steps)
    return ndtri(u_of(words(dims, np.arange(n_points, dtype=np.uint64), True, randomization, seed)))


def steps_np(n_steps, construction, z):
    """unit-variance steps [k][point] of one factor from z [j][point]"""
    if construction == INCREMENTAL:
        return z
    W = bridge_matrix(n_steps) @ z
    return np.diff(W, axis=0)


def heston_euler_payoffs(model, n_steps, d1, d2):
    """call payoffs of the split-step Euler scheme of DESIGN.md on unit-variance steps d1, d2 [k][point] (independent
    factors), discounted"""
    dt = model["T"] / n_steps
    sq, rho = math.sqrt(dt), model["rho"]
    rho_c = math.sqrt(1.0 - rho * rho)
    x = np.full(d1.shape[1], math.log(model["S0"]))
    v = np.full(d1.shape[1], model["V0"])
    for k in range(n_steps):
        dW1, dW2 = sq * d1[k], sq * (rho * d1[k] + rho_c * d2[k])
        vp = np.maximum(v, 0.0)
        kx = x + dt * (model["r"] - 0.5 * vp)
        kv = v + dt * model["kappa"] * (model["theta"] - vp)
        g = np.sqrt(np.maximum(kv, 0.0))
        x, v = kx + g * dW1, kv + model["sigma"] * g * dW2
    return math.exp(-model["r"] * model["T"]) * np.maximum(np.exp(x) - model["K"], 0.0)


def rqmc(estimates):
    """(mean, standard error) of R randomisations' estimates: the sample standard deviation over sqrt(R)"""
    e = np.asarray(estimates, dtype=np.float64)
    return float(e.mean()), (float(e.std(ddof=1)) / math.sqrt(e.size) if e.size > 1 else float("nan"))
