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

The effect sizes and the association likelihood-ratio tests are closed forms at a point the device reports as well:

    K = v0 (rho U U' + (1 - rho) L L') + v1 I     beta = (M' K^-1 M)^-1 M' K^-1 y     u = U' K^-1 (y - M beta)
    ML:  s = y' P y / n                           lml = -1/2 (n log 2 pi + n + n log s + log|Sigma|)

(``pinned_effects``, ``pinned_ml``; U = g o E0, M = [W, g, E0]).  Where the device reports no point -- the association
scan that refits delta per variant -- ``pinned_ml_max`` maximises the reference itself over x = logit(delta) by three-point
parabolas, which also gives the curvature that turns the search's tolerance on x into one on the likelihood (it is
``pinned_max`` with ``restricted=False``; ``grid_lmls`` uses the restricted one for the effect sizes' grid).  Their
float64 yardsticks are ``oracle_effects_at`` and ``oracle_ml_at``; ``effects_errors`` / ``ml_errors`` are the records
``limits`` reads.

The null fits of the interaction scan at every grid point (tests/test_gpu_pinned_null_model.py) are held the same way from
both sides: ``null_trial_reference`` is ``pinned_max`` of the restricted likelihood per (variant, grid point) -- or the
value at the clamp of the logistic where the maximum sits there --, ``stop_allowance`` how far in x a faithful search may
stop from it, ``trial_shares`` the checks on one trial record as shares of their bounds, ``selection_from_records`` /
``selection_against_reference`` the two checks on the choice of rho*; ``oracle_null_at`` is the yardstick.
"""
import numpy as np

from oracle.lmm import LMM, FastScanner
from oracle.scoretest import LowRankCov, Projection, cov_solve, score_F, score_Q
from oracle.sugar import economic_qs_linear

LD = np.longdouble
if np.finfo(LD).eps > 1e-18:
    raise RuntimeError("numpy.longdouble on this host has eps %.3g: the pinned-point reference needs an extended type "
                       "(eps <= 1e-18) and does not stand in for one with float64" % float(np.finfo(LD).eps))

LOG2PI = np.log(8 * np.arctan(LD(1)))      # (numpy.pi is a double)
FLOOR_PER_CELL = 2.2e-16      # an n-length float64 sum in the worst order
CEILING = 1e-11               # the tightest figure the suite asserts between two forms of the library
PATHS = 32                    # device stages rounded independently, against the oracle's three products with Q0
# ``grid_lmls`` maximises the reference itself at the two best grid values whenever they are this close (relative).  It is
# 100 x CEILING on purpose: ``argmax_or_tie`` is only ever asked with a limit that ``limits`` returned, which is at most
# CEILING, so every pair it can call tied -- or just not tied -- has been maximised in longdouble, not read at a float64
# optimum; pairs further apart than this are separated by far more than that read can be off.
REFINE_WITHIN = 100 * CEILING


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


def pinned(y, X, half_S, half_dK, delta, gram=None, logdet_XX=None):
    """(Q, F, lml, scale) in longdouble at the background half factor ``half_S`` (= hS at rho*) and ``delta``;
    X = [W, g], half_dK = g[idx_G] o E0[idx_E].  ``gram``: hS hS' in longdouble where the caller can form it in fewer
    operations than the product of an n x 1000 factor (``kronecker_gram``); ``half_S`` is then not read.  ``logdet_XX``:
    log|X'X| as ``log_gram(X)`` returns it, for a caller that evaluates many points on one X."""
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
    if logdet_XX is None:
        logdet_XX = _orthonormal(X)[1]
    lml = -(df * LOG2PI + df + df * np.log(s) + logdet_Sigma + logdet_XSX - logdet_XX) / 2
    return Q, F, lml, s


def log_gram(X):
    """log|X'X| in longdouble, as ``pinned`` forms it."""
    return _orthonormal(np.asarray(X, LD))[1]


def _sigma(half_S, delta, gram, n):
    """(1 - delta) hS hS' + delta I in longdouble."""
    if gram is None:
        hS = np.asarray(half_S, LD)
        gram = hS @ hS.T
    Sigma = (1 - LD(delta)) * np.asarray(gram, LD)
    Sigma[np.diag_indices(n)] += LD(delta)
    return Sigma


def _off(basis, v):
    """v projected off an orthonormal basis, twice."""
    v = v - basis @ (basis.T @ v)
    return v - basis @ (basis.T @ v)


def pinned_ml(y, X, half_S, delta, gram=None):
    """(lml, scale) of the ML likelihood in longdouble at ``delta``: s = y'Py / n, lml = -1/2 (n log 2 pi + n + n log s +
    log|Sigma|) -- what the association scan's null fit (X = W) and its alternatives (X = [W, g]) return."""
    y = np.asarray(y, LD).ravel()
    X = np.asarray(X, LD)
    n = y.size
    L = _cholesky(_sigma(half_S, delta, gram, n))
    white = _forward(L, np.column_stack([y, X]))
    basis, _ = _orthonormal(white[:, 1:])
    ry = _off(basis, white[:, 0])
    s = (ry @ ry) / n
    lml = -(n * LOG2PI + n + n * np.log(s) + 2 * np.sum(np.log(np.diag(L)))) / 2
    return lml, s


def _logistic(x):
    return 1 / (1 + np.exp(-LD(x)))


def pinned_max(y, X, half_S, x0, restricted=False, gram=None):
    """(L*, x*, curvature): the maximum over x = logit(delta) of ``pinned_ml`` (``restricted``: of ``pinned``'s lml), the
    x where it is taken and -L'' there, by three-point parabolas in longdouble: from x0 (the float64 oracle's optimum)
    with h = 1e-3 until the vertex stays within h, then once with h = 1e-4 around it.  A stencil that is not concave has
    no vertex: raised."""
    y = np.asarray(y, LD).ravel()
    if gram is None:
        hS = np.asarray(half_S, LD)
        gram = hS @ hS.T
    none = np.zeros((y.size, 0))
    logdet_XX = log_gram(X) if restricted else None

    def f(x):
        if restricted:
            return pinned(y, X, None, none, _logistic(x), gram=gram, logdet_XX=logdet_XX)[2]
        return pinned_ml(y, X, None, _logistic(x), gram=gram)[0]

    def vertex(x, h):
        lo, mid, hi = f(x - h), f(x), f(x + h)
        second = (hi - 2 * mid + lo) / (h * h)
        if not second < 0:
            raise ValueError("the likelihood is not concave around x = %.6g (second difference %.3g)" % (float(x), float(second)))
        return x - (hi - lo) / (2 * h) / second, -second

    x, h = LD(x0), LD(10) ** -3
    for _ in range(4):
        new, _ = vertex(x, h)
        moved, x = abs(new - x), new
        if moved <= h:
            break
    else:
        raise ValueError("no maximum within 4e-3 of x0 = %.6g" % float(x0))
    x, curvature = vertex(x, LD(10) ** -4)
    return f(x), x, curvature


def pinned_ml_max(y, X, half_S, x0, gram=None):
    """``pinned_max`` of the ML likelihood: the reference of a scan that refits delta per variant."""
    return pinned_max(y, X, half_S, x0, restricted=False, gram=gram)


def refit_allowance(x, curvature):
    """What a search with rtol = atol = 1e-6 on x may leave of the likelihood: half the curvature times the square of three
    tolerances (brent_search.h and oracle/brent.py stop when the bracket is within 2 tol of the best point)."""
    return float(curvature) / 2 * (3 * (1e-6 * abs(float(x)) + 1e-6)) ** 2


CLAMP = 2.220446049250313e-16     # delta is held to [CLAMP, 1 - CLAMP]: oracle/lmm.py (epsilon.tiny) and nullfit.hip (EPS_TINY) alike


def _logit(delta):
    d = LD(delta)
    return np.log(d) - np.log1p(-d)


def null_trial_reference(y, X, half_S, x0, gram=None):
    """(L*, x*, curvature, clamp) of one null fit -- one variant at one grid value -- from the reference alone:
    ``pinned_max(restricted=True)`` started from ``x0``, the x of the float64 oracle's polished fit there (as ``grid_lmls``
    does).  Where that fit sits at a clamp of the logistic (delta = CLAMP or 1 - CLAMP: the likelihood is monotone up to
    it, so no stencil around x0 has a vertex) the reference's value at the clamp is returned with x* = logit of the
    clamp's delta, curvature None and the clamp's delta as the mark (None: an interior maximum).  Anything else that has no maximum near x0 raises (``pinned_max``)."""
    x0 = float(x0)
    delta0 = 1 / (1 + np.exp(-x0)) if x0 > 0 else np.exp(x0) / (np.exp(x0) + 1)
    for clamp in (CLAMP, 1 - CLAMP):
        if (delta0 <= clamp) if clamp < 0.5 else (delta0 >= clamp):
            none = np.zeros((np.asarray(y).size, 0))
            return pinned(y, X, half_S, none, clamp, gram=gram)[2], _logit(clamp), None, clamp
    return pinned_max(y, X, half_S, x0, restricted=True, gram=gram) + (None,)


def stop_allowance(x, curvature, top, lim):
    """How far in x = logit(delta) a faithful search may stop from the maximum x*: three tolerances 1e-6 |x*| + 1e-6 (the
    same three as ``refit_allowance``: brent_search.h and oracle/brent.py stop when the bracket is within 2 tol of the best
    point, and the best point is at most one more from the bracket's middle), plus the radius inside which the search
    cannot tell points apart at all.  Around x* the likelihood is L* - curvature / 2 (x - x*)^2; the objective the search
    compares carries rounding noise of up to ``lim`` |L*| (the lml limit of ``limits``), so two points whose true values
    differ by less than that may be ordered either way: every x with curvature / 2 (x - x*)^2 <= lim |L*|, that is
    |x - x*| <= sqrt(2 lim |L*| / curvature), can be taken for the best one."""
    x, curvature = float(x), float(curvature)
    return 3 * (1e-6 * abs(x) + 1e-6) + float(np.sqrt(2 * lim * abs(float(top)) / curvature))


def trial_shares(rec, ref_at, trial, lim):
    """The checks b, c and d of tests/test_gpu_pinned_null_model.py on one trial record, as shares of their bounds (a share
    above 1 is a failure; the caller asserts).  ``rec``: (lml, delta, scale) of the search under test; ``ref_at``: the
    reference's (lml, scale) at that delta; ``trial``: ``null_trial_reference``; ``lim``: {"lml", "scale"} of ``limits``."""
    lml, delta, scale = (LD(v) for v in rec[:3])
    top, x, curvature, clamped = trial
    noise = lim["lml"] * abs(top)
    out = {"lml": float(abs(lml - ref_at[0]) / abs(ref_at[0])) / lim["lml"],
           "scale": float(abs(scale - ref_at[1]) / ref_at[1]) / lim["scale"]}
    if clamped is not None:
        # d: the reference at the search's delta is not below the reference at the clamp by more than the noise; and the
        # delta is the clamp's own double (one memoised point on both sides)
        out["clamp value"] = float((top - ref_at[0]) / noise)
        out["clamp delta"] = 0.0 if float(delta) == clamped else float("inf")
    else:
        out["short of L*"] = float((top - lml) / (refit_allowance(x, curvature) + noise))
        out["above L*"] = float((lml - top) / noise)
        out["stop"] = float(abs(_logit(delta) - x)) / stop_allowance(x, curvature, top, lim["lml"])
    return out


def selection_from_records(lmls, rho_index):
    """e: is ``rho_index`` the first index of the maximum of the trial lmls (the reference's ``>`` in its loop over the grid)?"""
    lmls = np.asarray(lmls, float)
    return bool(np.all(np.isfinite(lmls))) and int(rho_index) == int(np.argmax(lmls))


def selection_against_reference(tops, rho_index, limit):
    """f: (accepted, tie) -- without a tie the index is the reference's; with one it is among the grid points within
    ``limit`` x |largest| of the largest."""
    best, tie = argmax_or_tie(tops, limit)
    if not tie:
        return int(rho_index) == best, False
    tied = [i for i, v in enumerate(tops) if abs(tops[best] - v) <= limit * abs(tops[best])]
    return int(rho_index) in tied, True


def pinned_effects(y, M, U, half_L, rho, v0, v1, beta=None):
    """(beta, u) in longdouble at (rho, v0, v1): K = v0 (rho U U' + (1 - rho) L L') + v1 I is formed and factorised, [y, M, U]
    whitened, the whitened M orthonormalised (Gram-Schmidt twice; R = basis' Z) and beta back-substituted from
    R beta = basis' y; u = U' K^-1 (y - M beta).  M = [W, g, E0], U = g o E0; ``half_L = None``: no L (mode A).
    ``beta`` given: u for that beta (estimate_aggregate_environment takes it from a fit under another covariance)."""
    y = np.asarray(y, LD).ravel()
    M, U = np.asarray(M, LD), np.asarray(U, LD)
    n, m = M.shape
    rho, v0, v1 = LD(rho), LD(v0), LD(v1)
    K = (v0 * rho) * (U @ U.T)
    if half_L is not None:
        hL = np.asarray(half_L, LD)
        K += (v0 * (1 - rho)) * (hL @ hL.T)
    K[np.diag_indices(n)] += v1
    white = _forward(_cholesky(K), np.column_stack([y, M, U]))
    wy, Z, wU = white[:, 0], white[:, 1:1 + m], white[:, 1 + m:]
    if beta is not None:
        beta = np.asarray(beta, LD)
        return beta, wU.T @ (wy - Z @ beta)
    basis, _ = _orthonormal(Z)                  # (raises where M is not of full column rank)
    R = basis.T @ Z
    t = basis.T @ wy
    t += basis.T @ (wy - basis @ t)
    beta = np.zeros(m, LD)
    for j in range(m - 1, -1, -1):
        beta[j] = (t[j] - R[j, j + 1:] @ beta[j + 1:]) / R[j, j]
    return beta, wU.T @ (wy - Z @ beta)


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


def oracle_null_at(y, X, Q0, S0, delta):
    """The float64 oracle's restricted (lml, scale) at ``delta``: the null-fit half of ``oracle_at``."""
    lmm = _LMMAt(y, X, ((Q0,), np.asarray(S0, float)), restricted=True)
    lmm._at = float(delta)
    lml = -lmm._neg_lml_at(np.log(lmm._at) - np.log1p(-lmm._at))
    return lml, lmm.scale


def pinned_solve(half_S, v0, v1, rhs):
    """(v0 hS hS' + v1 I)^-1 rhs in longdouble: K = C C', the inverse of C by forward substitution on the identity."""
    hS, rhs = np.asarray(half_S, LD), np.asarray(rhs, LD)
    n = hS.shape[0]
    K = LD(v0) * (hS @ hS.T)
    K[np.diag_indices(n)] += LD(v1)
    Ci = _forward(_cholesky(K), np.eye(n))
    return Ci.T @ (Ci @ rhs)


def effects_half(U, half_L, rho):
    """The per-SNP covariance half [sqrt(rho) U, sqrt(1 - rho) L] (oracle/crm.py: predict_interaction)."""
    if half_L is None:
        return np.sqrt(rho) * np.asarray(U, float)
    return np.concatenate([np.sqrt(rho) * np.asarray(U, float), np.sqrt(1 - rho) * np.asarray(half_L, float)], axis=1)


def oracle_effects_at(y, M, U, half_L, rho, v0, v1, fit=None, beta=None):
    """The float64 oracle's (beta, u, lml, scale) at the same point: its ``LMM`` (restricted) pinned at
    delta = v1 / (v0 + v1), then ``LowRankCov`` / ``cov_solve`` on y - M beta as oracle/crm.py: predict_interaction strings
    them together.  ``fit``: called on the pinned LMM and the decomposition, returns (beta, u) -- the CPU test passes
    imitated kernel slips.  ``beta`` given: u on y - M beta, as ``pinned_effects``."""
    y = np.asarray(y, float).ravel()
    U = np.asarray(U, float)
    delta = float(v1) / (float(v0) + float(v1))
    (Q0,), S0 = economic_qs_linear(effects_half(U, half_L, float(rho)), return_q1=False)
    lmm = _LMMAt(y, M, ((Q0,), S0), restricted=True)
    lmm._at = delta
    lml = -lmm._neg_lml_at(np.log(delta) - np.log1p(-delta))
    if fit is not None:
        beta, u = fit(lmm, Q0, S0)
    elif beta is not None:
        u = U.T @ cov_solve(LowRankCov(Q0, S0, float(v0), float(v1)), y - np.asarray(M, float) @ beta)
    else:
        beta = lmm.beta
        u = U.T @ cov_solve(LowRankCov(Q0, S0, float(v0), float(v1)), y - lmm.mean())
    return beta, u, lml, lmm.scale


def oracle_ml_at(y, X, Q0, S0, delta, G=None):
    """The float64 oracle's ML (lml, scale) at ``delta`` (``LMM._neg_lml_at``, restricted=False) and, with ``G``, its
    ``FastScanner``'s alternative lmls of the columns of G at that frozen delta."""
    delta = float(delta)
    lmm = _LMMAt(y, X, ((Q0,), np.asarray(S0, float)), restricted=False)
    lmm._at = delta
    lml = -lmm._neg_lml_at(np.log(delta) - np.log1p(-delta))
    alt = None if G is None else FastScanner(lmm).fast_scan(np.asarray(G, float))["lml"]
    return lml, lmm.scale, alt


def grid_lmls(y, X, half_of, grid, restricted):
    """The reference's maximised lml per grid value: the float64 oracle's polished fit gives x = logit(delta), the
    reference is evaluated there (a lower bound of its maximum, short by half the curvature times the square of the
    polish's 1e-12); where the best two come within ``REFINE_WITHIN`` of each other both are maximised by ``pinned_max``."""
    y = np.asarray(y, float).ravel()
    none = np.zeros((y.size, 0))
    xs, out = [], []
    for rho in grid:
        hS = half_of(float(rho))
        lmm = LMM(y, X, economic_qs_linear(hS, return_q1=False), restricted=restricted)
        lmm.fit(verbose=False, polish=True)
        xs.append(lmm._x)
        out.append(pinned(y, X, hS, none, lmm.delta)[2] if restricted else pinned_ml(y, X, hS, lmm.delta)[0])
    order = np.argsort(np.asarray(out, float))[::-1]
    if len(out) > 1 and abs(out[order[0]] - out[order[1]]) <= REFINE_WITHIN * abs(out[order[0]]):
        for i in order[:2]:
            out[i] = pinned_max(y, X, half_of(float(grid[i])), xs[i], restricted=restricted)[0]
    return out


def argmax_or_tie(lmls, limit):
    """(index of the largest, whether the two largest are within ``limit`` x |largest| of each other)."""
    order = np.argsort(np.asarray(lmls, float))[::-1]
    tie = len(lmls) > 1 and abs(lmls[order[0]] - lmls[order[1]]) <= limit * abs(lmls[order[0]])
    return int(order[0]), bool(tie)


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


def relative(got, ref):
    return float(abs(LD(got) - ref) / abs(ref))


def vector_error(got, ref):
    """max|got - ref| relative to the largest magnitude of the reference vector.  A reference that is zero throughout
    (beta_gxe at rho = 0) is met by zeros only."""
    ref = np.asarray(ref, LD)
    gap, top = np.abs(np.asarray(got, LD) - ref).max(), np.abs(ref).max()
    if top == 0:
        return 0.0 if gap == 0 else float("inf")
    return float(gap / top)


def effects_errors(got, ref):
    """``got`` and ``ref``: dicts with some of beta, u, beta_gxe (vectors: ``vector_error``), lml, scale (relative)."""
    return {k: (relative if k in ("lml", "scale") else vector_error)(got[k], ref[k]) for k in got}


def ml_errors(got, ref):
    """``got`` and ``ref``: dicts with lml and some of scale (relative) and lrs -- the pair (alt lml, null lml), the
    statistic 2 (alt - null) held absolutely, relative to |null lml| of the reference."""
    out = {}
    for k in got:
        if k == "lrs":
            (ga, gn), (ra, rn) = got[k], ref[k]
            out[k] = float(abs(2 * (LD(ga) - LD(gn)) - 2 * (ra - rn)) / abs(rn))
        else:
            out[k] = relative(got[k], ref[k])
    return out


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
