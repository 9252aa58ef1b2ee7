"""Numpy statement of the exact tail p-value of the interaction score test (csrc/tail_pvalue.hip).

For Q = sum_j lam_j chi2_1 (the weights kept by SKAT's filter, as Davies integrates them) and K(t) = -1/2 sum log(1 - 2 lam_j t):

    P(Q > q) = (1 / 2 pi i) int exp(K(t) - t q) / t dt   along   t(u) = c + i sigma u + mu u^2,  u in [-U, U]
    c        the saddle point of K(t) - t q - log t:  K'(c) = q + 1 / c,  in (0, 1 / (2 lam_max)) when q > E[Q];
             in (-inf, 0) when q <= E[Q], where the contour passes left of the pole at 0 and gives P(Q > q) - 1
    sigma    (K''(c) + 1 / c^2)^(-1/2);   mu = KAPPA / q

The parabola meets the real axis only at c: it keeps the pole at 0 on one side and wraps the branch cut
[1 / (2 lam_max), inf), so the integrand falls off like a Gaussian in u and the trapezoid rule over the nodes
u_m = m U / M (m = -M..M; by conjugate symmetry m = 0..M) converges geometrically.  exp(K(c) - c q) is taken out
of the sum, so log p comes out directly, below the double range of p too.  Every complex factor is formed
relative to its value at c, 1 - w_j d with w_j = 2 lam_j / (1 - 2 lam_j c) and d = t - c, and taken on the
principal branch: it meets the real axis only at d = 0, where it is 1.

One weight kept: p = erfc(sqrt(q / (2 lam))), log p through erfcx below 1e-300.
"""
import math

import numpy as np
from scipy.special import erfc, erfcx

U = 20.0            # half-width of the contour in u
M = 128             # nodes on u in (0, U]: 2 M + 1 = 257 over [-U, U]
KAPPA = 0.1         # q mu: exp(-t q) adds exp(-KAPPA u^2) to the integrand's decay
NEWTON_MAX = 200

CONVERGED, NOT_BRACKETED, NON_FINITE, NO_WEIGHTS = 0, 1, 2, 3


def kept_weights(lam):
    """SKAT's Get_Lambda filter as davies.hip applies it: lam > mean(lam[lam >= 0]) / 1e5, order kept."""
    lam = np.asarray(lam, float)
    pos = lam[lam >= 0]
    thr = pos.sum() / pos.size / 100000.0 if pos.size else np.inf
    return lam[lam > thr]


def _derivs(w, q, c):
    s = 1.0 - 2.0 * w * c
    return np.sum(w / s) - q - 1.0 / c, np.sum(2.0 * w * w / (s * s)) + 1.0 / (c * c)


def saddle(w, q):
    """(c, ok): the root of h(c) = K'(c) - q - 1/c by Newton steps kept inside a bracket that halves when a step would
    leave it.  h increases on both (0, 1/(2 lam_max)) and (-inf, 0)."""
    upper = q > np.sum(w)
    if upper:
        lo, hi = 0.0, 0.5 / np.max(w)
    else:
        lo, hi = -2.0 * (0.5 * w.size + 1.0) / q, 0.0     # h(lo) <= (k/2 + 1)/|lo| - q < 0
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        return np.nan, False
    c = 0.5 * (lo + hi)
    for _ in range(NEWTON_MAX):
        h, dh = _derivs(w, q, c)
        if h < 0:
            lo = c
        else:
            hi = c
        step = h / dh
        cn = c - step
        if not (lo < cn < hi):
            cn = 0.5 * (lo + hi)
        if abs(cn - c) <= 1e-14 * abs(c) or not (hi - lo > 4e-16 * abs(c)):
            return cn, True
        c = cn
    return c, False


def tail_pvalue(q, lam):
    """(p, log p, status) for one variant: Q = q, eigenvalues lam of F (any order)."""
    lam = np.asarray(lam, float)
    q = float(q)
    if not (np.isfinite(q) and np.all(np.isfinite(lam))):
        return np.nan, np.nan, NON_FINITE
    w = kept_weights(lam)
    if w.size == 0:
        return np.nan, np.nan, NO_WEIGHTS
    if q <= 0.0:
        return 1.0, 0.0, CONVERGED
    if w.size == 1:
        x = math.sqrt(q / (2.0 * w[0]))
        p = float(erfc(x))
        logp = math.log(p) if p > 1e-300 else math.log(erfcx(x)) - x * x
        return p, logp, CONVERGED
    c, ok = saddle(w, q)
    if not ok:
        return np.nan, np.nan, NOT_BRACKETED
    s = 1.0 - 2.0 * w * c
    kc = -0.5 * np.sum(np.log1p(-2.0 * w * c))
    sigma = 1.0 / math.sqrt(np.sum(2.0 * w * w / (s * s)) + 1.0 / (c * c))
    mu = KAPPA / q
    wr = 2.0 * w / s
    u = np.arange(1, M + 1) * (U / M)
    u2 = u * u
    # log(1 - wr d), d = mu u^2 + i sigma u: |.|^2 - 1 = wr u^2 (wr (sigma^2 + mu^2 u^2) - 2 mu), arg = atan2(-wr sigma u, 1 - wr mu u^2)
    x = wr[None, :] * u2[:, None] * (wr[None, :] * (sigma * sigma + mu * mu * u2[:, None]) - 2.0 * mu)
    re_log = 0.5 * np.sum(np.log1p(x), axis=1)
    im_log = np.sum(np.arctan2(-wr[None, :] * sigma * u[:, None], 1.0 - wr[None, :] * mu * u2[:, None]), axis=1)
    d = mu * u2 + 1j * sigma * u
    g = np.exp(-0.5 * (re_log + 1j * im_log) - d * q) / (c + d) * (sigma - 2j * mu * u)
    terms = g.real
    terms[-1] *= 0.5
    S = (U / M) / math.pi * (0.5 * sigma / c + np.sum(terms))
    A = kc - c * q
    if c > 0:
        if not (S > 0 and np.isfinite(S)):
            return np.nan, np.nan, NON_FINITE
        logp = A + math.log(S)
        return math.exp(logp), logp, CONVERGED
    F = -math.exp(A) * S              # P(Q <= q)
    if not (0.0 <= F < 1.0):
        return np.nan, np.nan, NON_FINITE
    return 1.0 - F, math.log1p(-F), CONVERGED


def tail_pvalues(Q, lam):
    """Row-wise tail_pvalue: Q (count,), lam (count, k).  Returns (p, log p, status) arrays."""
    Q = np.asarray(Q, float).ravel()
    lam = np.asarray(lam, float).reshape(Q.size, -1)
    out = [tail_pvalue(q, l) for q, l in zip(Q, lam)]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out], np.int32))
