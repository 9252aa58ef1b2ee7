"""Numpy statement of the batched effect-size route (csrc/effects_multi.hip).

For one (y, W, E0, L, g): the REML objective of oracle/lmm.py for LMM(y, M = [W, g, E0], QS(rho)) with
Sigma_p(rho) = rho U U' + (1 - rho) L L', U = g o E0, evaluated from ONE decomposition L L' = Q_L S_L Q_L' and a
k0 x k0 capacitance matrix per evaluation:

    N        = delta I + a Q_L S_L Q_L',  a = (1 - delta)(1 - rho),  w_j = 1 / (delta + a S_L[j])
    u'N^-1 v = sum_j w_j t_u[j] t_v[j] + c(u, v) / delta,  t_u = Q_L'u,  c(u, v) = u'v - t_u't_v  (once per pair)
    C        = I / ((1 - delta) rho) + U'N^-1 U
    u'D^-1 v = u'N^-1 v - (U'N^-1 u)' C^-1 (U'N^-1 v)
    log|D|   = sum_j log(delta + a S_L[j]) + (n - r_L) log delta + log|C| + k0 log((1 - delta) rho)

``L``: None (mode A: no kinship term), an n x m cell-level factor, or a list of halves (get_L_values' Hadamard halves).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from oracle import brent  # noqa: E402
from oracle.lmm import LOG2PI, _logistic, _rsolve  # noqa: E402
from oracle.sugar import LOGMAX, epsilon  # noqa: E402

RHO_GRID = np.linspace(0, 1, 11)


def l_decomposition(L, n):
    """(Q_L, S_L) of L L' from the thin SVD of the concatenated halves; squared singular values below 1e-12 of the
    largest are dropped (the library's rule for its backgrounds)."""
    if L is None:
        return np.zeros((n, 0)), np.zeros(0)
    if isinstance(L, (list, tuple)) or hasattr(L, "hK"):
        L = np.concatenate([np.asarray(x, float) for x in L], axis=1)
    U, s, _ = np.linalg.svd(np.asarray(L, float), full_matrices=False)
    S = s * s
    keep = S > 1e-12 * S.max(initial=0.0)
    return U[:, keep], S[keep]


class WoodburyEffects:
    """The restricted fit of [W, g, E0] under Sigma_p(rho) for one pair, through the rank-k0 form."""

    def __init__(self, y, W, E0, g, L=None, rho_grid=None, QS=None):
        self.y = np.asarray(y, float).ravel()
        n = self.y.shape[0]
        self.W = np.asarray(W, float)
        self.E0 = np.asarray(E0, float)
        self.g = np.asarray(g, float).reshape(n, 1)
        self.rho_grid = (np.array([1.0]) if L is None else RHO_GRID) if rho_grid is None else np.asarray(rho_grid, float)
        self.Q, self.S = QS if QS is not None else l_decomposition(L, n)
        self.n = n
        self.cW, self.k0 = self.W.shape[1], self.E0.shape[1]
        self.M = np.concatenate((self.W, self.g, self.E0), axis=1)
        self.U = self.g * self.E0
        P = self.M.shape[1]
        self.P = P
        Z = np.concatenate((self.M, self.y[:, None], self.U), axis=1)   # [X, y, U]
        T = self.Q.T @ Z
        self.T = T
        self.cnum = Z.T @ Z - T.T @ T          # complement numerators, once per pair
        self.XX = self.M.T @ self.M

    def _ninv(self, rho, delta):
        """Z'N^-1 Z over Z = [X, y, U]."""
        a = (1.0 - delta) * (1.0 - rho)
        w = 1.0 / (delta + a * self.S)
        return (self.T.T * w) @ self.T + self.cnum / delta, float(np.log(delta + a * self.S).sum())

    def terms(self, rho, delta):
        """(yKy, XKy, XKX, logdet) of oracle/lmm.py: _terms with K = D(delta) of Sigma_p(rho), X = M as given."""
        P, k0 = self.P, self.k0
        H, lsum = self._ninv(rho, delta)
        logdet = lsum + (self.n - self.S.shape[0]) * np.log(delta)
        if rho > 0.0:
            C = H[P + 1:, P + 1:] + np.eye(k0) / ((1.0 - delta) * rho)
            Lc = np.linalg.cholesky(C)
            Zc = np.linalg.solve(Lc, H[P + 1:, :P + 1])
            H = H[:P + 1, :P + 1] - Zc.T @ Zc
            logdet += 2.0 * np.log(np.diag(Lc)).sum() + k0 * np.log((1.0 - delta) * rho)
        else:
            H = H[:P + 1, :P + 1]
        return float(H[P, P]), H[:P, P], H[:P, :P], logdet

    def state(self, rho, delta):
        yKy, XKy, XKX, logdet = self.terms(rho, delta)
        beta = _rsolve(XKX, XKy)
        df = self.n - self.P
        scale = max((yKy - float(XKy @ beta)) / df, epsilon.small)
        val = -0.5 * (df * LOG2PI + df + self.n * np.log(scale) + logdet)
        sgn0, ld0 = np.linalg.slogdet(self.XX)
        sgn1, ld1 = np.linalg.slogdet(XKX / scale)
        if sgn0 != 1.0 or sgn1 != 1.0:
            raise ValueError("The determinant of X'X / H should be positive.")
        val += 0.5 * (ld0 - ld1)
        return float(val), beta, scale

    def lml(self, rho, delta):
        return self.state(rho, delta)[0]

    def fit_rho(self, rho):
        """oracle/brent.py's search (bracket + Brent, rtol = atol = 1e-6) over x = logit(delta): (delta, lml)."""
        x, _, _ = brent.minimize(lambda x: -self.lml(rho, _logistic(x)), a=-LOGMAX, b=LOGMAX, rtol=1e-6, atol=1e-6)
        delta = _logistic(float(x))
        return delta, self.lml(rho, delta)

    def fit(self):
        """Best grid point (strict >, first wins): (rho, delta, lml)."""
        best = (None, None, -np.inf)
        for rho in self.rho_grid:
            delta, lml = self.fit_rho(float(rho))
            if lml > best[2]:
                best = (float(rho), delta, lml)
        return best

    def blup(self, rho, delta):
        """(beta, u = U'K^-1 (y - M beta), v0, v1) at (rho, delta); K = scale D."""
        _, beta, scale = self.state(rho, delta)
        P, k0 = self.P, self.k0
        H, _ = self._ninv(rho, delta)
        B = H[P + 1:, :P + 1]                   # U'N^-1 [X, y]
        t = B[:, P] - B[:, :P] @ beta           # U'N^-1 r
        if rho > 0.0:
            C = H[P + 1:, P + 1:] + np.eye(k0) / ((1.0 - delta) * rho)
            t = np.linalg.solve(C, t) / ((1.0 - delta) * rho)   # U'D^-1 r
        return beta, t / scale, scale * (1.0 - delta), scale * delta

    def betas(self, maf, rho=None, delta=None):
        """(beta_g, beta_gxe (n,)) of predict_interaction; at the given (rho, delta) or at the fitted optimum."""
        if rho is None:
            rho, delta, _ = self.fit()
        beta, u, v0, _ = self.blup(rho, delta)
        beta_gxe = (v0 * rho) * self.E0 @ u / np.sqrt(2 * maf * (1 - maf))
        return float(beta[self.cW]), beta_gxe
