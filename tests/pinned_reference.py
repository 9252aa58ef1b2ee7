"""An extended-precision reference for the score test at a pinned point (plain helper module, not a test).

Where a null-fit search stops within its tolerance is decided by rounding noise, so a comparison of two searches can ask
for 1e-6 at most.  At a FIXED point (rho, delta), however, Q, F, the restricted log-likelihood and the scale are closed-form
functions of the inputs: ``pinned`` evaluates them in ``numpy.longdouble`` (eps 1.1e-19) straight from the dense textbook
definitions -- Sigma is formed, factorised by a Cholesky written out here, [y, X, half_dK] are whitened and projected off
the whitened X by Gram-Schmidt run twice.  No spectral decomposition, no Q0, no LAPACK: nothing is shared with the device's
path or with the float64 oracle's implicit forms (oracle/scoretest.py, oracle/lmm.py).

    Sigma = (1 - delta) hS hS' + delta I          df = n - rank X          s = y' P y / df
    Q = 1/2 |half_dK' P y|^2 / s^2                F = 1/2 half_dK' P half_dK / s
    lml = -1/2 (df log 2 pi + df + df log s + log|Sigma| + log|X' Sigma^-1 X| - log|X'X|)

with P = Sigma^-1 - Sigma^-1 X (X' Sigma^-1 X)^-1 X' Sigma^-1 (oracle/lmm.py: ``lml()`` for ``restricted=True`` is the same
number: its n log s + log|X'K^-1X / s| is df log s + log|X'K^-1X|).

``oracle_at`` is the float64 oracle's own evaluation at the same point; its distance to ``pinned`` is what float64 can
achieve on a problem and the yardstick of tests/test_gpu_pinned.py (``limits``).

A problem whose reference cannot be evaluated -- Sigma not positive definite in longdouble, X without full column rank --
raises: nothing is left out silently.
"""
import numpy as np

from oracle.lmm import LMM
from oracle.scoretest import LowRankCov, Projection, score_F, score_Q

LD = np.longdouble
if np.finfo(LD).eps > 1e-18:
    raise RuntimeError("numpy.longdouble on this host has eps %.3g: the pinned-point reference needs an extended type "
                       "(eps <= 1e-18) and does not stand in for one with float64" % float(np.finfo(LD).eps))

LOG2PI = np.log(8 * np.arctan(LD(1)))      # (numpy.pi is a double)
FLOOR_PER_CELL = 2.2e-16      # an n-length float64 sum in the worst order
CEILING = 1e-11               # the tightest figure the suite asserts between two forms of the library
PATHS = 32                    # device stages rounded independently, against the oracle's three products with Q0


def _cholesky(A, block=32):
    """Lower Cholesky factor of a symmetric matrix, blocked: panels column by column, the trailing block by one product."""
    A = np.array(A, LD)
    n = A.shape[0]
    for j0 in range(0, n, block):
        j1 = min(n, j0 + block)
        for j in range(j0, j1):
            d = A[j, j] - A[j, j0:j] @ A[j, j0:j]
            if not d > 0:
                raise np.linalg.LinAlgError("Sigma is not positive definite in longdouble (pivot %d: %.3g)" % (j, float(d)))
            A[j, j] = np.sqrt(d)
            A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, j0:j] @ A[j, j0:j]) / A[j, j]
        if j1 < n:
            panel = A[j1:, j0:j1]
            A[j1:, j1:] -= panel @ panel.T
    return np.tril(A)


def _forward(L, B, block=32):
    """L^-1 B for a lower triangular L."""
    B = np.array(B, LD)
    n = L.shape[0]
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        if i0:
            B[i0:i1] -= L[i0:i1, :i0] @ B[:i0]
        for i in range(i0, i1):
            B[i] = (B[i] - L[i, i0:i] @ B[i0:i]) / L[i, i]
    return B


def _orthonormal(Z):
    """Gram-Schmidt on the columns of Z, twice; returns (orthonormal basis, log|Z'Z|).  A column that loses ten digits
    against the ones before it makes the rank of X a matter of thresholds: raised, not decided here."""
    Q = np.array(Z, LD)
    logdet = LD(0)
    for j in range(Q.shape[1]):
        before = np.sqrt(Q[:, j] @ Q[:, j])
        for _ in range(2):
            if j:
                Q[:, j] -= Q[:, :j] @ (Q[:, :j].T @ Q[:, j])
        norm = np.sqrt(Q[:, j] @ Q[:, j])
        if not norm > 1e-10 * before:
            raise ValueError("column %d of X lies in the span of the columns before it: no pinned reference" % j)
        logdet += 2 * np.log(norm)
        Q[:, j] /= norm
    return Q, logdet


def pinned(y, X, half_S, half_dK, delta, gram=None):
    """(Q, F, lml, scale) in longdouble at the background half factor ``half_S`` (= hS at rho*) and ``delta``;
    X = [W, g], half_dK = g[idx_G] o E0[idx_E].  ``gram``: hS hS' in longdouble where the caller can form it in fewer
    operations than the product of an n x 1000 factor (``kronecker_gram``); ``half_S`` is then not read."""
    y = np.asarray(y, LD).ravel()
    X, D = np.asarray(X, LD), np.asarray(half_dK, LD)
    n, c = X.shape
    delta = LD(delta)
    if gram is None:
        hS = np.asarray(half_S, LD)
        gram = hS @ hS.T
    Sigma = (1 - delta) * np.asarray(gram, LD)
    Sigma[np.diag_indices(n)] += delta
    L = _cholesky(Sigma)
    white = _forward(L, np.column_stack([y, X, D]))
    wy, Z, wD = white[:, 0], white[:, 1:1 + c], white[:, 1 + c:]
    basis, logdet_XSX = _orthonormal(Z)
    ry = wy - basis @ (basis.T @ wy)
    ry -= basis @ (basis.T @ ry)
    rD = wD - basis @ (basis.T @ wD)
    rD -= basis @ (basis.T @ rD)
    df = n - c
    s = (ry @ ry) / df
    u = rD.T @ ry
    Q = (u @ u) / (2 * s * s)
    F = (rD.T @ rD) / (2 * s)
    logdet_Sigma = 2 * np.sum(np.log(np.diag(L)))
    logdet_XX = _orthonormal(X)[1]
    lml = -(df * LOG2PI + df + df * np.log(s) + logdet_Sigma + logdet_XSX - logdet_XX) / 2
    return Q, F, lml, s


class _LMMAt(LMM):
    """The oracle's LMM with delta given as a number instead of through logistic(logit(delta)), which returns a
    neighbouring double: the two evaluations are to meet at the same point exactly."""
    _at = 0.5

    @property
    def delta(self):
        return self._at


def oracle_at(y, X, Q0, S0, half_dK, delta, projection=Projection):
    """The float64 oracle's (Q, F, lml, scale) at ``delta`` on the economic decomposition (Q0, S0) of hS hS':
    ``LMM._neg_lml_at`` for the likelihood and the scale, then the implicit forms of oracle/scoretest.py as
    oracle/crm.py: scan_interaction strings them together.  ``projection``: the class that stands for P (the CPU test
    passes deliberately wrong ones)."""
    delta = float(delta)
    lmm = _LMMAt(y, X, ((Q0,), np.asarray(S0, float)), restricted=True)
    lmm._at = delta
    lml = -lmm._neg_lml_at(np.log(delta) - np.log1p(-delta))
    P = projection(LowRankCov(Q0, np.asarray(S0, float), lmm.v0, lmm.v1), np.asarray(X, float))
    y = np.asarray(y, float).ravel()
    return score_Q(P, half_dK, y), score_F(P, half_dK), lml, lmm.scale


def half_factor(rho, E1, hK=None, Ls=None):
    """hS at a grid point, as oracle/crm.py: OracleCellRegMap builds it (modes A / B / C)."""
    if Ls:
        return np.concatenate([np.sqrt(rho) * E1] + [np.sqrt(1 - rho) * np.asarray(L, float) for L in Ls], axis=1)
    if hK is not None:
        return np.concatenate([np.sqrt(rho) * E1, np.sqrt(1 - rho) * np.asarray(hK, float)], axis=1)
    return np.asarray(E1, float)


def kronecker_gram(rho, E1, hK, us):
    """hS hS' of mode C in longdouble without the n x (k1 + k2 m) factor: with L_i = diag(us[:, i]) hK the sum of the
    L_i L_i' is the Hadamard product (hK hK') o (us us') -- the same doubles, O(n^2 (m + k)) operations."""
    E1, hK, us = (np.asarray(a, LD) for a in (E1, hK, us))
    return LD(rho) * (E1 @ E1.T) + (1 - LD(rho)) * ((hK @ hK.T) * (us @ us.T))


def errors(got, ref):
    """Distances of (Q, F, lml, scale) to the reference's, as floats: Q relative to max(|Q|, tr F) (a score vector that
    nearly vanishes leaves Q itself ill-conditioned), F to max|F|, lml and the scale relative."""
    Q, F, lml, s = ref
    gQ, gF, glml, gs = got
    return {"Q": float(abs(LD(gQ) - Q) / max(abs(Q), np.trace(F))),
            "F": float(np.abs(np.asarray(gF, LD) - F).max() / np.abs(F).max()),
            "lml": float(abs(LD(glml) - lml) / abs(lml)),
            "scale": float(abs(LD(gs) - s) / s)}


def worst(rows):
    """Per quantity, the largest of several ``errors`` records."""
    return {k: max(r[k] for r in rows) for k in rows[0]}


def limits(oracle_errors, n):
    """What a device form may be off by, per quantity: 32 x the float64 oracle's own error against ``pinned`` at the same
    points, never below n x 2.2e-16 and never above 1e-11."""
    return {k: float(min(CEILING, max(PATHS * v, n * FLOOR_PER_CELL))) for k, v in oracle_errors.items()}


def pick(p, block=None):
    """At most three variants by fixed index: the first, the one at p // 2 and the last; with ``block`` (variants per block
    or tile of the form under test) the middle one moves into the second block where p reaches it."""
    mid = p // 2 if block is None or p <= block else max(p // 2, block)
    return sorted({0, min(mid, p - 1), p - 1})
