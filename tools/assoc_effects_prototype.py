"""The numpy statement of cellregmap_amd/csrc/assoc_effects.hip: effect size, standard error and
ML scale of the alternative model y ~ [W, g] of an association test at a fixed variance ratio delta, from the sums over the
rotated space that the kernel forms -- no n x n matrix.

With (Q0, S0) the economic decomposition of Sigma(rho*), t_u = Q0'u and w_k = 1 / ((1 - delta) S0_k + delta),

    u'K^-1v = sum_k t_u[k] t_v[k] w_k + (u'v - sum_k t_u[k] t_v[k]) / delta          K = (1 - delta) Sigma + delta I

for u, v among the columns of W, g and y.  Then L = chol(W'K^-1W), z_g = L^-1 W'K^-1g, z_y = L^-1 W'K^-1y and

    schur = g'K^-1g - z_g'z_g        num = g'K^-1y - z_g'z_y        beta = num / schur
    rss   = y'K^-1y - z_y'z_y - num^2 / schur        scale = rss / n        beta_se = sqrt(scale / schur)

(the kernel's fast form takes L and z_y from the gene's prepared record; its full-refit form factorises the whole
[W, g] block, whose last pivot is sqrt(schur) -- the same numbers).  tests/test_assoc_effects_prototype_cpu.py holds this
file to the dense longdouble reference.

    python tools/assoc_effects_prototype.py        a small self-check against numpy's dense solve
"""
import math

import numpy as np

EFFECT_OK, EFFECT_G_IN_SPAN_W, EFFECT_NO_FIT, EFFECT_NON_FINITE = 0, 1, 2, 3


def metric_products(T, S0, plain, delta):
    """[W, g, y]'K^-1[W, g, y] from the rotated columns ``T`` (r x m) and their plain products ``plain`` (m x m)."""
    w = 1.0 / ((1.0 - delta) * S0 + delta)
    return (T.T * w) @ T + (plain - T.T @ T) / delta


def effects_at(y, W, g, Q0, S0, delta, tau=1e-12):
    """(beta, beta_se, scale, schur, status) at ``delta``; ``tau``: the fast scanner's rank rule schur <= tau g'K^-1g."""
    y, g = np.asarray(y, float).ravel(), np.asarray(g, float).ravel()
    W = np.asarray(W, float).reshape(y.size, -1)
    c = W.shape[1]
    Z = np.column_stack([W, g, y])
    H = metric_products(Q0.T @ Z, np.asarray(S0, float), Z.T @ Z, float(delta))
    L = np.linalg.cholesky(H[:c, :c])
    zg = _forward(L, H[:c, c])
    zy = _forward(L, H[:c, c + 1])
    schur = H[c, c] - zg @ zg
    num = H[c, c + 1] - zg @ zy
    rss0 = H[c + 1, c + 1] - zy @ zy
    if not schur > tau * H[c, c]:
        return np.nan, np.nan, rss0 / y.size, schur, EFFECT_G_IN_SPAN_W
    scale = (rss0 - num * num / schur) / y.size
    beta, se = num / schur, math.sqrt(scale / schur) if scale >= 0 else np.nan
    ok = np.isfinite(beta) and np.isfinite(se)
    return beta, se, scale, schur, EFFECT_OK if ok else EFFECT_NON_FINITE


def _forward(L, b):
    z = np.zeros_like(b)
    for i in range(b.size):
        z[i] = (b[i] - L[i, :i] @ z[:i]) / L[i, i]
    return z


def log_pvalue(alt_lml, null_lml):
    """log erfc(sqrt(lrs / 2)), lrs = max(2 (alt - null), 0), in the kernel's three branches: near 1 through erf, in the
    middle the logarithm of erfc, below 1e-300 log(erfcx(x)) - x^2."""
    from scipy.special import erfcx

    lrs = max(2.0 * (alt_lml - null_lml), 0.0)
    h = 0.5 * lrs
    x = math.sqrt(h)
    if x < 0.5:
        return math.log1p(-math.erf(x))
    p = math.erfc(x)
    return math.log(p) if p > 1e-300 else math.log(float(erfcx(x))) - h


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    n, c, k = 120, 3, 7
    hS = rng.normal(size=(n, k))
    U, s, _ = np.linalg.svd(hS, full_matrices=False)
    Q0, S0 = U, s * s
    W = np.column_stack([np.ones(n), rng.normal(size=(n, c - 1))])
    g = rng.normal(size=n)
    y = 0.4 * g + hS @ rng.normal(size=k) + rng.normal(size=n)
    for delta in (1e-3, 0.3, 0.97):
        beta, se, scale, schur, status = effects_at(y, W, g, Q0, S0, delta)
        Ki = np.linalg.inv((1 - delta) * hS @ hS.T + delta * np.eye(n))
        X = np.column_stack([W, g])
        A = np.linalg.inv(X.T @ Ki @ X)
        b = A @ (X.T @ Ki @ y)
        s2 = (y @ Ki @ y - (X.T @ Ki @ y) @ b) / n
        print("delta %.3g: beta %.12g (dense %.12g)  se %.12g (dense %.12g)  status %d"
              % (delta, beta, b[-1], se, math.sqrt(s2 * A[-1, -1]), status))
        assert abs(beta - b[-1]) <= 1e-9 * abs(b[-1]) and abs(se - math.sqrt(s2 * A[-1, -1])) <= 1e-9 * se
