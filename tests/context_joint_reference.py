"""The joint fixed-effect GxC test in extended precision (plain helper module, not a test).

Per variant g (include/crm_hip.h: crm_scan_interaction_contexts_joint) at a given point
(rho, delta), with the kept candidates x_j = g o C_j, j in ``keep``:

    H0: X = [W, C, g]            H1: [X, x_j for j in keep],  delta frozen
    Sigma = (1 - delta) hS hS' + delta I       s = y'Py / n       lml = -1/2 (n log 2 pi + n + n log s + log|Sigma|)

``joint_test`` is ``pinned_reference.pinned_ml`` of X and of [X, kept candidates] -- Sigma formed and factorised in
``numpy.longdouble``, [y, X, candidates] whitened, the whitened design matrices orthonormalised by Gram-Schmidt run twice --
with the one factorisation shared by the two models (tests/test_context_joint_reference_cpu.py holds it to ``pinned_ml``
itself), and beta and its standard error by the same whitening: with Rx, ry the whitened candidates and y projected off
the whitened X,

    S = Rx'Rx = Ls Ls'     beta = S^-1 Rx'ry     rss1 = |ry off [X, candidates]|^2     beta_se_j = sqrt(rss1 / n (S^-1)_jj)

``oracle_joint_at`` is the float64 oracle at the same point: ``pinned_reference._LMMAt`` pinned at delta on both design
matrices, beta from its own solve and beta_se from its own X'K^-1X.  Its distance to ``joint_test`` is the yardstick
(``pinned_reference.limits``).  ``device_form`` states in numpy float64 what the kernel computes: the phi metric, the
Schur complement against [X0, g] and the Cholesky factor in column order with the drop rule.  ``log_chi2_sf`` is the
closed-form tail.
"""
import math

import numpy as np

import pinned_reference as pr

LD = pr.LD
TINY, ONE_LESS = 2.2250738585072014e-308, 1 - 2.220446049250313e-16


def joint_test(y, X, g, C, gram, delta, keep=None):
    """{null_lml, null_scale, alt_lml, beta [kept], beta_se [kept]} in longdouble; [X, kept candidates] of full column
    rank, ``gram`` = hS hS' in longdouble."""
    y = np.asarray(y, LD).ravel()
    X = np.asarray(X, LD)
    n, c = X.shape
    cand = np.asarray(g, LD).reshape(-1, 1) * np.asarray(C, LD)
    if keep is not None:
        cand = cand[:, list(keep)]
    kk = cand.shape[1]
    L = pr._cholesky(pr._sigma(None, delta, gram, n))
    white = pr._forward(L, np.column_stack([y, X, cand]))
    logdet = 2 * np.sum(np.log(np.diag(L)))

    def lml(rss):
        return -(n * pr.LOG2PI + n + n * np.log(rss / n) + logdet) / 2

    basis0, _ = pr._orthonormal(white[:, 1:1 + c])
    ry = pr._off(basis0, white[:, 0])
    rss0 = ry @ ry
    basis1, _ = pr._orthonormal(white[:, 1:])
    r1 = pr._off(basis1, white[:, 0])
    rss1 = r1 @ r1
    Rx = np.column_stack([pr._off(basis0, white[:, 1 + c + j]) for j in range(kk)])
    Ls = pr._cholesky(Rx.T @ Rx)
    Li = pr._forward(Ls, np.eye(kk, dtype=LD))
    beta = Li.T @ (Li @ (Rx.T @ ry))
    se = np.sqrt(rss1 / n * np.sum(Li * Li, axis=0))
    return {"null_lml": lml(rss0), "null_scale": rss0 / n, "alt_lml": lml(rss1), "beta": beta, "beta_se": se}


def oracle_joint_at(y, X, Q0, S0, g, C, delta, keep=None):
    """The float64 oracle at the same point: its LMM pinned at ``delta`` on X and on [X, kept candidates]."""
    cand = np.asarray(g, float).reshape(-1, 1) * np.asarray(C, float)
    if keep is not None:
        cand = cand[:, list(keep)]
    kk = cand.shape[1]
    QS = ((Q0,), np.asarray(S0, float))
    x = np.log(float(delta)) - np.log1p(-float(delta))
    null = pr._LMMAt(y, X, QS, restricted=False)
    null._at = float(delta)
    null_lml = -null._neg_lml_at(x)
    alt = pr._LMMAt(y, np.column_stack([X, cand]), QS, restricted=False)
    alt._at = float(delta)
    alt_lml = -alt._neg_lml_at(x)
    XKX = alt._cache[0]
    cov = alt._Vt.T @ np.linalg.solve(XKX, alt._Vt)
    return {"null_lml": null_lml, "null_scale": null.scale, "alt_lml": alt_lml, "beta": alt.beta[-kk:],
            "beta_se": np.sqrt(alt.scale * np.diag(cov)[-kk:])}


def errors(got, ref):
    """Distances of a record to the reference's, as ``context_lrt_reference.errors`` states them: lml (the null's and the
    alternative's, relative), lrs (2 (alt - null), absolute, relative to |null lml| of the reference), beta
    (``pinned_reference.vector_error``) and beta_se (relative, the largest over the kept candidates)."""
    row = pr.ml_errors({"lml": got["alt_lml"], "lrs": (got["alt_lml"], got["null_lml"])},
                       {"lml": ref["alt_lml"], "lrs": (ref["alt_lml"], ref["null_lml"])})
    return {"lml": max(pr.relative(got["null_lml"], ref["null_lml"]), row["lml"]), "lrs": row["lrs"],
            "beta": pr.vector_error(got["beta"], ref["beta"]),
            "beta_se": max(pr.relative(a, b) for a, b in zip(got["beta_se"], ref["beta_se"]))}


def device_form(y, X, Q0, S0, g, C, delta):
    """The kernel's arithmetic in numpy float64: every product a'K^-1b = a'b / delta - sum_s phi_s ta_s tb_s, the factor L
    of X'K^-1X, V = L^-1 X'K^-1X_c, S = X_c'K^-1X_c - V'V, m = X_c'K^-1y - V'z, the Cholesky factor of S in column order
    (a pivot <= 1e-12 x_j'K^-1x_j drops the candidate), u, rss1, beta and beta_se.  Returns the record of ``joint_test``
    with ``dof`` and ``dropped`` [k] added; beta and beta_se have k entries (NaN where dropped)."""
    y = np.asarray(y, float).ravel()
    X = np.asarray(X, float)
    n = y.size
    S0 = np.asarray(S0, float)
    Xc = np.asarray(g, float).reshape(-1, 1) * np.asarray(C, float)
    k = Xc.shape[1]
    phi = (1 - delta) * S0 / (delta * ((1 - delta) * S0 + delta))
    logdet = float(np.log((1 - delta) * S0 + delta).sum()) + (n - S0.size) * np.log(delta)

    def metric(A, B):
        tA, tB = Q0.T @ A, Q0.T @ B
        return A.T @ B / delta - (tA.T * phi) @ tB

    A = metric(X, X)
    L = np.linalg.cholesky(A)
    yc = y[:, None]
    z = np.linalg.solve(L, metric(X, yc))[:, 0]
    rss0 = float(metric(yc, yc)[0, 0] - z @ z)
    V = np.linalg.solve(L, metric(X, Xc))
    full = metric(Xc, Xc)
    S = full - V.T @ V
    m = metric(Xc, yc)[:, 0] - V.T @ z
    Ls = np.zeros((k, k))
    kept = np.zeros(k, bool)
    for j in range(k):
        d = S[j, j] - Ls[j, :j] @ Ls[j, :j]
        if not d > 1e-12 * full[j, j]:
            Ls[j, :j] = 0.0
            Ls[j, j] = 1.0
            continue
        kept[j] = True
        Ls[j, j] = np.sqrt(d)
        Ls[j + 1:, j] = (S[j + 1:, j] - Ls[j + 1:, :j] @ Ls[j, :j]) / Ls[j, j]
    u = np.zeros(k)
    for j in range(k):
        if kept[j]:
            u[j] = (m[j] - Ls[j, :j] @ u[:j]) / Ls[j, j]
    rss1 = rss0 - float(u @ u)
    Li = np.linalg.solve(Ls, np.eye(k))
    s1 = max(rss1 / n, 1.4901161193847656e-08)

    def lml(s):
        return -(n * float(pr.LOG2PI) + n + n * np.log(s) + logdet) / 2

    beta = np.where(kept, Li.T @ u, np.nan)
    se = np.where(kept, np.sqrt(s1 * np.sum(Li * Li, axis=0)), np.nan)
    return {"null_lml": lml(max(rss0 / n, 1.4901161193847656e-08)), "null_scale": rss0 / n, "alt_lml": lml(s1), "beta": beta,
            "beta_se": se, "dof": int(kept.sum()), "dropped": ~kept}


def log_chi2_sf(dof, lrs):
    """log Q(dof / 2, lrs / 2) in float64 by the finite sums the kernel uses (all terms positive):
    dof even: Q = e^-x sum_{i < dof / 2} x^i / i!;  dof odd: Q = erfc(sqrt x) + e^-x sum_{i = 1}^{(dof - 1) / 2}
    x^(i - 1/2) / Gamma(i + 1/2), in log form through erfcx; dof = 1 with the three branches of the per-context kernel."""
    from scipy.special import erfcx

    x = 0.5 * float(lrs)
    sx = math.sqrt(x)
    if dof == 1:
        if sx < 0.5:
            return math.log1p(-math.erf(sx))
        p = math.erfc(sx)
        return math.log(p) if p > 1e-300 else math.log(float(erfcx(sx))) - x
    if dof % 2 == 0:
        t = total = 1.0
        for i in range(1, dof // 2):
            t *= x / i
            total += t
        return math.log(total) - x
    t = total = sx * 1.1283791670955126
    for i in range(1, (dof - 1) // 2):
        t *= x / (i + 0.5)
        total += t
    return math.log(float(erfcx(sx)) + total) - x


def _mp():
    import mpmath as mp

    mp.mp.dps = 50
    return mp


def mp_log_pvalue(dof, lrs):
    """log of the upper tail of chi^2_dof at max(lrs, 0) in mpmath."""
    mp = _mp()
    x = mp.mpf(max(float(lrs), 0.0)) / 2
    return float(mp.log(mp.gammainc(mp.mpf(dof) / 2, x, mp.inf, regularized=True)))


def mp_pvalue(dof, lrs):
    """``lrt_pvalues`` of the statistic with the tail in mpmath: lrs clipped from below at the smallest normal double, the
    p-value to [2.2e-308, 1 - 2.2e-16]."""
    mp = _mp()
    x = mp.mpf(max(float(lrs), TINY)) / 2
    return min(max(float(mp.gammainc(mp.mpf(dof) / 2, x, mp.inf, regularized=True)), TINY), ONE_LESS)


def tail_tolerance(dof, log_p):
    """One rounding per recurrence term plus the exponential and the logarithm."""
    return (dof + 16) * 2.2e-16 * max(1.0, abs(log_p))
