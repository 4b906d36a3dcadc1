"""Exact sums, a high-precision least-squares fit and a derived decision margin for one LSM regression row
(hedgehog.jl_amd/csrc/hh_lsm.hip: rowstat_of, add_powers / add_moments, solve_normal_equations_wave,
exercise_now).

TEST INFRASTRUCTURE ONLY.  oracle/lsm_oracle.py is a second fp64 solver (SVD least squares); this module is the
exact reference the kernels' row fit is held against.

Exact sums.  Every fp64 is an integer times a power of two, so a sum of fp64 terms is exact in Python integers
(`exact_sum`, `exact_power_sums`).  The power sums Σ z^m and moment sums Σ z^k y of the reference are the sums of
the EXACT real powers of the fp64 regressors, not of fp64-rounded powers.

High-precision fit.  The normal equations G c = B (G_jk = Σ z^(j+k)) are solved with mpmath at `DPS` digits.
Fitted values, not coefficients, are compared: they are unique even when G is singular (m <= D distinct points:
the fit interpolates; repeated spots: the per-value means).  The reference mirrors the device's drop rule in
exact arithmetic: column c is kept when its exact pivot — the Schur complement of G_cc on the columns kept before
it — exceeds DROP · G_cc, and dropped otherwise.  Dropping an exactly dependent column leaves the fitted values
unchanged; a column within the rounding margin of the threshold makes the row AMBIGUOUS (every decision of the
row counts as a near-tie).

Decision margin.  The device decides `pay > cont` with cont = Horner(ĉ, ẑ), ĉ the fp64 solution of the fp64
normal equations.  δ_i bounds |cont_i − f*_i| to first order (f* the exact fitted value).  With u = 2^-53,
S_m = Σ|z|^m, T_k = Σ|y||z|^k and c, w_i = G_KK^-1 v_K(z_i) on the kept columns K:

  * sums: |ΔP_m| <= u (h + (m − 1) + θ m) S_m and |ΔB_k| <= u (h + k + θ k + e_y) T_k.  h is the depth of the
    summation tree (each term takes part in at most h roundings, |fl(Σ) − Σ| <= γ_h Σ|t|); m − 1 (k) roundings
    form a power by repeated products (pw *= z); θ = 4 covers the regressor itself: the device's
    ẑ = fl(fl(x − μ)·isd) and the reference's z are each within 2u of an affine image of x, and fitted values do
    not depend on the affine map, so |Δz^m| <= m θ u |z|^m; e_y ulps cover y (its rounding and the discount
    table's exp()).
  * solve: LDLᵀ without pivoting of a positive semidefinite G, and the two triangular solves, are backward
    stable: (G + E) ĉ = B with |E| <= γ_(3N+1) |L||D||Lᵀ| (Higham, Accuracy and Stability, Thm 10.4), and for a
    Gram matrix (|L||D||Lᵀ|)_jk <= sqrt(G_jj G_kk) (Cauchy–Schwarz).  The device forms each multiplier and each
    back-substitution quotient as x·rcp(p) with a reciprocal of <= 1 ulp: N + 3 more roundings.  So
    |E_jk| <= c_s u sqrt(S_2j S_2k), c_s = 4N + 4.
  * propagation: Δf_i = w_iᵀ(ΔB − ΔG c) to first order, so
        |Δf_i| <= Σ_k |w_ik| (|ΔB_k| + Σ_j (|ΔP_(j+k)| + |E_jk|) |c_j|).
  * evaluation: Horner in ẑ, |Δ| <= γ_2D Σ|c_k||z|^k (Higham Eq. 5.3), plus k θ u |c_k||z_i|^k for the
    regressor.
  * second order: with η = ||D^-1 ΔG D^-1||_2 · ||(D^-1 G D^-1)^-1||_2 (D = diag sqrt(G_kk)) the Neumann series
    of (G + ΔG)^-1 converges, and the remainder is at most the first-order term again, when η <= 1/2:
    δ_i = 2 × the first-order sum.  Rows with η > 1/2 get δ = ∞.

Nothing in δ is fitted to an observed error: test_lsm_exact_host.py shows the ratio of observed error to δ on a
restatement of the device's fit, and the GPU tests use the same bound with the device's own depth h.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction

import mpmath
import numpy as np

U = 2.0 ** -53
DPS = 60
DROP = 1e-13          # the device's drop rule: pivot <= DROP · (its own diagonal entry) -> coefficient 0
THETA = 4.0           # ulps of the regressor (see the module docstring)

# ---- the device's summation tree (hh_lsm.hip header) -------------------------------------------------------------

WG, WAVES, LANES, REC_LANES, REC_WAVES = 512, 8, 64, 256, 4


def lsm_q(ntot: int) -> int:
    """Trajectories per lane: the smallest of 2, 4, 8, 16 with which the ensemble fits 256 chunks (lsm_q)."""
    q, cap = 2, 1 << 18
    while q < 16 and ntot > cap:
        q, cap = 2 * q, 2 * cap
    return q


def lsm_nch(ntot: int) -> int:
    per = WG * lsm_q(ntot)
    return (ntot + per - 1) // per


def tree_depth(ntot: int) -> int:
    """Roundings a term can take part in on its way through the device's summation tree: Q − 1 in order within a
    lane (the first addition, to zero, is exact), 6 butterfly levels over 64 lanes, 7 additions of the 8 waves in
    order, ceil(nch/256) − 1 in order within a record lane, 6 butterfly levels, 3 additions of the 4 waves."""
    q, nch = lsm_q(ntot), lsm_nch(ntot)
    return (q - 1) + 6 + (WAVES - 1) + (-(-nch // REC_LANES) - 1) + 6 + (REC_WAVES - 1)


def _butterfly(a):
    """64 lanes (last axis) -> total of lane 0, pairs (l, l^32), (l, l^16), …, (l, l^1)."""
    idx = np.arange(LANES)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[..., idx ^ off]
    return a[..., 0]


def tree_sum(terms):
    """The device's canonical sum of terms[..., ntot] in fp64, in its order (trajectory
    p = chunk·512·Q + j·512 + lane; a lane adds its Q terms in order, a wave by the butterfly, the chunk its 8
    waves in order; chunk records dealt to 256 lanes, added in order, butterfly, 4 waves in order)."""
    terms = np.asarray(terms, dtype=np.float64)
    ntot = terms.shape[-1]
    q, nch = lsm_q(ntot), lsm_nch(ntot)
    pad = np.zeros(terms.shape[:-1] + (nch * WG * q,))
    pad[..., :ntot] = terms
    a = pad.reshape(terms.shape[:-1] + (nch, q, WAVES, LANES))
    lane = np.zeros(terms.shape[:-1] + (nch, WAVES, LANES))
    for j in range(q):
        lane = lane + a[..., j, :, :]
    wav = _butterfly(lane)                      # [..., nch, 8]
    rec = wav[..., 0]
    for w in range(1, WAVES):
        rec = rec + wav[..., w]                 # [..., nch]
    nrl = -(-nch // REC_LANES)
    r = np.zeros(terms.shape[:-1] + (nrl * REC_LANES,))
    r[..., :nch] = rec
    r = r.reshape(terms.shape[:-1] + (nrl, REC_LANES))
    acc = np.zeros(terms.shape[:-1] + (REC_LANES,))
    for k in range(nrl):
        acc = acc + r[..., k, :]
    wv = _butterfly(acc.reshape(terms.shape[:-1] + (REC_WAVES, LANES)))
    tot = wv[..., 0]
    for w in range(1, REC_WAVES):
        tot = tot + wv[..., w]
    return tot


# ---- exact sums ----------------------------------------------------------------------------------------------------

def exact_sum(a) -> Fraction:
    """Σ a (fp64 array) exactly: mantissas as integers, grouped by exponent (each half of a 53-bit mantissa is
    below 2^27, so 2^21 of them add exactly in a double)."""
    a = np.asarray(a, dtype=np.float64).ravel()
    if a.size == 0:
        return Fraction(0)
    if not np.all(np.isfinite(a)):
        raise ValueError("exact_sum of a non-finite value")
    assert a.size < 2 ** 26
    m, e = np.frexp(a)
    M = np.ldexp(m, 53).astype(np.int64)            # a = M · 2^(e − 53), |M| < 2^53
    s = np.sign(M)
    A = np.abs(M)
    hi, lo = (s * (A >> 26)).astype(np.float64), (s * (A & ((1 << 26) - 1))).astype(np.float64)
    e0 = int(e.min())
    idx = (e - e0).astype(np.int64)
    sh, sl = np.bincount(idx, hi), np.bincount(idx, lo)
    tot = 0
    for k in np.nonzero((sh != 0) | (sl != 0))[0]:
        tot += ((int(sh[k]) << 26) + int(sl[k])) << int(k)
    return Fraction(tot) * Fraction(2) ** (e0 - 53)


def _int_mantissas(x):
    """fp64 x -> (python ints M, python ints shift, e0) with x = M · 2^(shift + e0), shift >= 0."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    M = np.ldexp(m, 53).astype(np.int64)
    e = e.astype(np.int64) - 53
    e0 = int(e.min()) if x.size else 0
    return [int(v) for v in M], [int(v) for v in (e - e0)], e0


def exact_power_sums(z, y=None, kmax=16):
    """Exact Σ z_i^m (m = 0..kmax), or Σ z_i^m y_i when y is given, of the real powers of the fp64 z_i, as
    mpmath numbers at the working precision."""
    Mz, sz, ez = _int_mantissas(z)
    if y is not None:
        My, sy, ey = _int_mantissas(y)
    else:
        My, sy, ey = [1] * len(Mz), [0] * len(Mz), 0
    out = []
    pw = list(My)            # M_z^m · M_y
    for m in range(kmax + 1):
        # term i = pw_i · 2^(m sz_i + sy_i) · 2^(m ez + ey)
        tot = 0
        for p, a, b in zip(pw, sz, sy):
            if p:
                tot += p << (m * a + b)
        out.append(mpmath.ldexp(mpmath.mpf(tot), m * ez + ey))
        pw = [p * q for p, q in zip(pw, Mz)]
    return out


# ---- fp64 restatement of the device's row fit --------------------------------------------------------------------

def rowstat(n, sx, sxx):
    """rowstat_of: (n, Σx, Σx²) -> (μ, 1/std) as the device forms them (IEEE division and square root, no fused
    operations: the library is built with -ffp-contract=off)."""
    n, sx, sxx = np.float64(n), np.float64(sx), np.float64(sxx)
    if not n > 0:
        return 0.0, 1.0
    mu = sx / n
    var = sxx / n - mu * mu
    return float(mu), float(np.float64(1.0) / np.sqrt(var)) if var > 0 else 1.0


def device_z(x, mu, isd):
    return (np.asarray(x, dtype=np.float64) - np.float64(mu)) * np.float64(isd)


def device_powers(z, kmax):
    """[kmax+1][n]: z^0 … z^kmax formed as the device does (pw = 1; pw *= z)."""
    out = np.empty((kmax + 1, len(z)))
    pw = np.ones(len(z))
    for k in range(kmax + 1):
        out[k] = pw
        pw = pw * z
    return out


def device_moment_terms(z, y, degree):
    out = np.empty((degree + 1, len(z)))
    pw = np.asarray(y, dtype=np.float64).copy()
    for k in range(degree + 1):
        out[k] = pw
        pw = pw * z
    return out


def device_solve(B, n, P, degree):
    """solve_normal_equations_wave: elimination without pivoting, multipliers r·rcp(pivot), a column whose pivot is
    not above DROP · (its diagonal entry) dropped; returns the coefficients (0 for a dropped column)."""
    N = degree + 1
    Pv = lambda i: float(n) if i == 0 else float(P[i])
    r = [[Pv(j + k) for k in range(N)] + [float(B[j])] for j in range(N)]
    inv = [0.0] * N
    for c in range(N):
        p = r[c][c]
        dead = not (p > DROP * Pv(2 * c))
        inv[c] = 0.0 if dead else 1.0 / p
        if not dead:
            for j in range(c + 1, N):
                f = r[j][c] * inv[c]
                for k in range(c, N + 1):
                    r[j][k] = r[j][k] - f * r[c][k]
    cf = [0.0] * N
    for c in range(N - 1, -1, -1):
        s = r[c][N]
        for k in range(c + 1, N):
            s = s - r[c][k] * cf[k]
        cf[c] = s * inv[c]
    return np.array(cf)


def horner(coef, z):
    z = np.asarray(z, dtype=np.float64)
    cont = np.full(z.shape, coef[-1])
    for c in range(len(coef) - 2, -1, -1):
        cont = cont * z + coef[c]
    return cont


def device_row_fit(x, y, degree, ntot=None):
    """The device's regression of one row, in fp64, summed in the device's tree order: x, y are the in-the-money
    spots and continuation values.  Returns (fitted values at x, (μ, isd), coefficients).  ntot: size of the
    ensemble the tree is laid out for (the out-of-the-money trajectories add zeros; default len(x))."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(x)
    if n == 0:
        return np.zeros(0), (0.0, 1.0), np.zeros(degree + 1)
    stats = tree_sum(_padded(np.stack([np.ones(n), x, x * x]), ntot))
    mu, isd = rowstat(*stats)
    z = device_z(x, mu, isd)
    P = tree_sum(_padded(device_powers(z, 2 * degree), ntot))
    B = tree_sum(_padded(device_moment_terms(z, y, degree), ntot))
    coef = device_solve(B, stats[0], P, degree)
    return horner(coef, z), (mu, isd), coef


def _padded(a, ntot):
    if ntot is None or ntot == a.shape[-1]:
        return a
    out = np.zeros(a.shape[:-1] + (ntot,))
    out[..., :a.shape[-1]] = a
    return out


# ---- the exact fit and its margin --------------------------------------------------------------------------------

@dataclass
class RowFit:
    fitted: np.ndarray       # exact fitted values f*_i (to ~2^-64 relative of Σ|c_k||z_i|^k)
    delta: np.ndarray        # δ_i (inf where the row is not decidable to first order)
    kept: list               # columns the drop rule keeps in exact arithmetic
    ambiguous: bool          # a pivot within its rounding margin of the drop threshold
    eta: float               # the second-order control (first order valid for eta <= 1/2)
    z: np.ndarray            # the regressor the reference used


def reference_z(x):
    """A standardised regressor for the reference: z = fl(fl(x − μ)·isd) with μ, 1/std of the exact moments."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if n == 0:
        return x.copy()
    s1, s2 = exact_sum(x), exact_sum_sq(x)
    mu = s1 / n
    var = s2 / n - mu * mu
    isd = 1.0 / math.sqrt(var) if var > 0 else 1.0
    return device_z(x, float(mu), isd)


def exact_sum_sq(x) -> Fraction:
    Mx, sx, ex = _int_mantissas(x)
    tot = 0
    for p, a in zip(Mx, sx):
        tot += (p * p) << (2 * a)
    return Fraction(tot) * Fraction(2) ** (2 * ex)


def exact_row_fit(x, y, degree, h, e_y=1.0, theta=THETA, drop=DROP, z=None):
    """Exact least-squares fit of y on the polynomials of degree `degree` in x (fitted values), with the device's
    drop rule mirrored in exact arithmetic, and δ_i for a device fit whose sums carry tree depth h.
    x, y: the in-the-money spots and continuation values (fp64).  z: the regressor (default reference_z(x)) —
    pass the device's ẑ when the device's sums are the exact sums fed to it."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, N = len(x), degree + 1
    if n == 0:
        return RowFit(np.zeros(0), np.zeros(0), [], False, 0.0, x.copy())
    z = reference_z(x) if z is None else np.asarray(z, dtype=np.float64)
    with mpmath.workdps(DPS):
        P = exact_power_sums(z, kmax=2 * degree)
        B = exact_power_sums(z, y, kmax=degree)
        G = mpmath.matrix(N, N)
        for j in range(N):
            for k in range(N):
                G[j, k] = P[j + k]
        # bounds (fp64 is accurate enough for them)
        az, ay = np.abs(z), np.abs(y)
        pw = device_powers(az, 2 * degree)
        S = np.array([math.fsum(r) for r in pw])
        T = np.array([math.fsum(r * ay) for r in pw[:N]])
        m_ = np.arange(2 * degree + 1)
        eP = U * (h + np.maximum(m_ - 1, 0) + theta * m_) * S
        eP[0] = 0.0                                   # P[0] is the count n: exact
        kk = np.arange(N)
        eB = U * (h + kk + theta * kk + e_y) * T
        cs = 4 * N + 4
        sq = np.sqrt(S[2 * kk])
        Emat = cs * U * np.outer(sq, sq)
        dG = np.array([[eP[j + k] for k in range(N)] for j in range(N)]) + Emat
        # the drop rule in exact arithmetic
        kept, ambiguous = [], False
        for c in range(N):
            gcc = G[c, c]
            if kept:
                GK = mpmath.matrix([[G[a, b] for b in kept] for a in kept])
                gK = mpmath.matrix([G[a, c] for a in kept])
                a_ = mpmath.lu_solve(GK, gK)
                piv = gcc - sum(gK[i] * a_[i] for i in range(len(kept)))
                at = np.array([-float(a_[i]) for i in range(len(kept))] + [1.0])
            else:
                piv, at = gcc, np.array([1.0])
            idx = kept + [c]
            dpiv = float(np.abs(at) @ dG[np.ix_(idx, idx)] @ np.abs(at))
            thr = drop * gcc
            if piv - dpiv > thr * (1 + 1e-12):
                kept.append(c)
            elif not (piv + dpiv <= thr * (1 - 1e-12)):
                ambiguous = True
                if piv > thr:
                    kept.append(c)
        K = kept
        GK = mpmath.matrix([[G[a, b] for b in K] for a in K])
        BK = mpmath.matrix([B[a] for a in K])
        cK = mpmath.lu_solve(GK, BK)
        GKi = GK ** -1
    cK_f = np.array([float(v) for v in cK])
    # f*_i in extended precision from the mp coefficients (hi + lo doubles)
    cK_lo = np.array([float(cK[i] - mpmath.mpf(cK_f[i])) for i in range(len(K))])
    zl = z.astype(np.longdouble)
    fitted = np.zeros(n, dtype=np.longdouble)
    for i, a in enumerate(K):
        fitted += (np.longdouble(cK_f[i]) + np.longdouble(cK_lo[i])) * zl ** a
    fitted = fitted.astype(np.float64)
    # first-order δ on the kept columns
    Gi = np.array([[float(GKi[i, j]) for j in range(len(K))] for i in range(len(K))])
    VK = np.stack([z ** a for a in K])                     # [|K|][n]
    W = Gi @ VK
    W = np.abs(W) + (len(K) + 1) * U * (np.abs(Gi) @ np.abs(VK))
    dGK = dG[np.ix_(K, K)]
    beta = eB[K] + dGK @ np.abs(cK_f)
    first = beta @ W
    hor = np.zeros(n)
    for i, a in enumerate(K):
        hor += (2 * degree + theta * a) * abs(cK_f[i]) * az ** a
    first = first + U * hor
    # second-order control
    Dk = np.sqrt(np.array([float(G[a, a]) for a in K]))
    Dk[Dk == 0] = 1.0
    Gs = Gi * np.outer(Dk, Dk)
    dGs = dGK / np.outer(Dk, Dk)
    eta = float(np.linalg.norm(Gs, 2) * np.linalg.norm(dGs, 2)) if len(K) else 0.0
    delta = 2.0 * first if eta <= 0.5 else np.full(n, np.inf)
    if ambiguous:
        delta = np.full(n, np.inf)
    # the reference values themselves carry ~2^-63 relative of Σ|c||z|^k: add it to δ
    delta = delta + 2.0 ** -60 * (len(K) + 2) * np.sum([abs(cK_f[i]) * az ** a for i, a in enumerate(K)], axis=0)
    return RowFit(fitted, delta, K, ambiguous, eta, z)


def decisions(pay, fit: RowFit):
    """(exercise per the exact fit, near-tie mask |pay − f*| <= δ)."""
    pay = np.asarray(pay, dtype=np.float64)
    return pay > fit.fitted, np.abs(pay - fit.fitted) <= fit.delta
