"""The per-context fixed-effect GxC tests in extended precision (plain helper module, not a test).

Per variant g and context column C_j (include/crm_hip.h: crm_scan_interaction_contexts) at a
given point (rho, delta):

    H0: X = [W, C, g]            H1_j: [X, x_j],  x_j = g o C_j,  delta frozen
    Sigma = (1 - delta) hS hS' + delta I       s = y'Py / n       lml = -1/2 (n log 2 pi + n + n log s + log|Sigma|)

``context_tests`` is ``pinned_reference.pinned_ml`` of X and of [X, x_j] -- Sigma formed and factorised in
``numpy.longdouble``, [y, X, x_1 .. x_k] whitened, the whitened X orthonormalised by Gram-Schmidt run twice -- with the one
factorisation shared by the k + 1 models of a variant (tests/test_context_lrt_reference_cpu.py holds it to ``pinned_ml``
itself), and beta and its standard error by the same whitening: with rx, ry the whitened x_j and y projected off the
whitened X,

    d = rx'rx      m = rx'ry      beta = m / d      rss1 = ry'ry - m^2 / d      beta_se = sqrt(rss1 / n / d)

``oracle_context_at`` is the float64 oracle's own composition at the same point: its ``LMM`` with X = [W, C, g] pinned at
delta, then ``get_fast_scanner().fast_scan(g[:, None] * C)`` (oracle/lmm.py:247-267), and beta / beta_se from the same
A = [X, x_j]'K^-1[X, x_j] the scanner forms.  Its distance to ``context_tests`` is the yardstick
(``pinned_reference.limits``).
"""
import numpy as np

import pinned_reference as pr
from oracle.lmm import FastScanner

LD = pr.LD


def context_tests(y, X, g, C, gram, delta):
    """{null_lml, null_scale, alt_lml [k], beta [k], beta_se [k]} in longdouble; X = [W, C, g] of full column rank,
    ``gram`` = hS hS' in longdouble."""
    y = np.asarray(y, LD).ravel()
    X = np.asarray(X, LD)
    n, c = X.shape
    cand = np.asarray(g, LD).reshape(-1, 1) * np.asarray(C, LD)
    L = pr._cholesky(pr._sigma(None, delta, gram, n))
    white = pr._forward(L, np.column_stack([y, X, cand]))
    basis, _ = pr._orthonormal(white[:, 1:1 + c])
    ry = pr._off(basis, white[:, 0])
    logdet = 2 * np.sum(np.log(np.diag(L)))
    rss0 = ry @ ry

    def lml(rss):
        return -(n * pr.LOG2PI + n + n * np.log(rss / n) + logdet) / 2

    out = {"null_lml": lml(rss0), "null_scale": rss0 / n, "alt_lml": [], "beta": [], "beta_se": []}
    for j in range(cand.shape[1]):
        rx = pr._off(basis, white[:, 1 + c + j])
        d, m = rx @ rx, rx @ ry
        rss1 = rss0 - m * m / d
        out["alt_lml"].append(lml(rss1))
        out["beta"].append(m / d)
        out["beta_se"].append(np.sqrt(rss1 / n / d))
    return out


def oracle_context_at(y, X, Q0, S0, g, C, delta):
    """The float64 oracle at the same point: {null_lml, null_scale, alt_lml, beta, beta_se} (arrays of k)."""
    cand = np.asarray(g, float).reshape(-1, 1) * np.asarray(C, float)
    lmm = pr._LMMAt(y, X, ((Q0,), np.asarray(S0, float)), restricted=False)
    lmm._at = float(delta)
    null_lml = -lmm._neg_lml_at(np.log(lmm._at) - np.log1p(-lmm._at))
    alt = FastScanner(lmm).fast_scan(cand)["lml"]
    # beta and its standard error from the scanner's own terms (oracle/lmm.py:252-265)
    n = lmm._n
    yKy, XKy, XKX, _ = lmm._terms(lmm._at)
    w = 1.0 / ((1.0 - lmm._at) * lmm._S0 + lmm._at)
    tC = lmm._Q0.T @ cand
    beta, se = np.empty(cand.shape[1]), np.empty(cand.shape[1])
    for j in range(cand.shape[1]):
        x, tx = cand[:, j], tC[:, j]
        xKx = float((tx * w) @ tx) + (float(x @ x) - float(tx @ tx)) / lmm._at
        xKy = float((tx * w) @ lmm._ty) + (float(x @ lmm._y) - float(tx @ lmm._ty)) / lmm._at
        xKX = lmm._tXr.T @ (w * tx) + (lmm._tX.T @ x - lmm._tXr.T @ tx) / lmm._at
        A = np.block([[XKX, xKX[:, None]], [xKX[None, :], np.array([[xKx]])]])
        b = np.concatenate([XKy, [xKy]])
        sol = np.linalg.lstsq(A, b, rcond=None)[0]
        s = (yKy - float(b @ sol)) / n
        schur = xKx - float(xKX @ np.linalg.lstsq(XKX, xKX, rcond=None)[0])
        beta[j], se[j] = sol[-1], np.sqrt(s / schur)
    return {"null_lml": null_lml, "null_scale": lmm.scale, "alt_lml": alt, "beta": beta, "beta_se": se}


def errors(got, ref, cols=None):
    """Distances of a record to the reference's, as ``pinned_reference.ml_errors`` states them: lml (the null's and every
    alternative's, relative), lrs (2 (alt - null), absolute, relative to |null lml| of the reference), beta_se (relative,
    the largest over the contexts ``cols``; default all) and beta (``pinned_reference.vector_error`` over those contexts:
    the largest gap relative to the largest |beta| of the variant -- a context without an effect has a beta that is
    the rounding of a cancellation, in the oracle as anywhere, and no relative error of its own)."""
    k = len(ref["alt_lml"])
    cols = list(range(k) if cols is None else cols)
    out = {"lml": pr.relative(got["null_lml"], ref["null_lml"]), "lrs": 0.0, "beta_se": 0.0}
    for j in cols:
        row = pr.ml_errors({"lml": got["alt_lml"][j], "lrs": (got["alt_lml"][j], got["null_lml"])},
                           {"lml": ref["alt_lml"][j], "lrs": (ref["alt_lml"][j], ref["null_lml"])})
        out["lml"], out["lrs"] = max(out["lml"], row["lml"]), max(out["lrs"], row["lrs"])
        out["beta_se"] = max(out["beta_se"], pr.relative(got["beta_se"][j], ref["beta_se"][j]))
    out["beta"] = pr.vector_error([got["beta"][j] for j in cols], [ref["beta"][j] for j in cols])
    return out
