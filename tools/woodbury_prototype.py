"""Numpy statement of the unrelated-donor form of the score test (scan_plan.hip: kin_wb; assemble.hip: woodbury_kernel).

With a diagonal donor-level kinship hKd hKd' = diag(kappa_d), the covariance of the null model

    K0 = v0 Sigma(rho) + v1 I,   Sigma(rho) = rho E1 E1' + (1 - rho) blockdiag_d kappa_d us_d us_d'

is inverted donor by donor: G_d = us_d'us_d = U_d diag(lambda_d) U_d', Phi_d = us_d U_d lambda_d^-1/2 (orthonormal),
s_p = (1 - rho) kappa_d lambda_dj over the positions p = (d, j), and with N = v1 I + v0 sum_p s_p phi_p phi_p'

    u'N^-1 v  = (u'v - sum_p w_p (Phi'u)_p (Phi'v)_p) / v1,          w_p = a_p / (1 + a_p),  a_p = (v0 / v1) s_p
    u'K0^-1 v = u'N^-1 v - v0 rho (E1'N^-1 u)' C^-1 (E1'N^-1 v),      C = I + v0 rho E1'N^-1 E1.

Directions of us_d below k2 eps lambda_max (k2 > the donor's cells) carry no variance and are dropped, as on the device.
Q and F then follow the reference's PMat / ScoreStatistic (cellregmap/_math.py:79-128) with X = [W, g], the test
direction g o E0.
"""
import numpy as np

EPS = np.finfo(float).eps


def donor_basis(us, group, groups):
    """Per donor: (cells of the donor, Phi_d, lambda_d) with the directions below rounding dropped."""
    out = []
    k2 = us.shape[1]
    for d in range(groups):
        cells = np.flatnonzero(group == d)
        u = us[cells]
        lam, U = np.linalg.eigh(u.T @ u)
        keep = lam > k2 * EPS * max(lam.max(), 0.0)
        out.append((cells, u @ U[:, keep] / np.sqrt(lam[keep]), lam[keep]))
    return out


class WoodburyInverse:
    """u'K0^-1 v for K0 = v0 Sigma(rho) + v1 I on a diagonal donor kinship (kappa: hKd hKd' diagonal)."""

    def __init__(self, E1, us, group, kappa, rho, v0, v1):
        groups = len(kappa)
        self.basis = donor_basis(us, group, groups)
        self.v1 = v1
        self.w = []
        for (cells, Phi, lam), kap in zip(self.basis, kappa):
            a = (v0 / v1) * (1.0 - rho) * kap * lam
            self.w.append(a / (1.0 + a))          # 0 at rho = 1 and at v0 = 0; no division by zero
        self.E1 = E1
        self.g = v0 * rho
        if self.g > 0.0:
            ME = self._n_inv(E1, E1)
            self.C = np.eye(E1.shape[1]) + self.g * ME
            self.L = np.linalg.cholesky(self.C)

    def _n_inv(self, U, V):
        acc = U.T @ V
        for (cells, Phi, _), w in zip(self.basis, self.w):
            acc = acc - (Phi.T @ U[cells]).T @ (w[:, None] * (Phi.T @ V[cells]))
        return acc / self.v1

    def form(self, U, V):
        out = self._n_inv(U, V)
        if self.g > 0.0:
            left = np.linalg.solve(self.L, self._n_inv(self.E1, U))
            right = np.linalg.solve(self.L, self._n_inv(self.E1, V))
            out = out - self.g * left.T @ right
        return out


def score_QF(y, W, g, gtest, E0, E1, us, group, kappa, rho, v0, v1):
    """Q and F of one variant: fixed effects X = [W, g], test direction gtest o E0."""
    K = WoodburyInverse(E1, us, group, kappa, rho, v0, v1)
    X = np.column_stack([W, g])
    D = gtest[:, None] * E0
    y = y[:, None]
    XKX, XKy, DKX = K.form(X, X), K.form(X, y), K.form(D, X)
    coef_y = np.linalg.lstsq(XKX, XKy, rcond=None)[0]
    coef_D = np.linalg.lstsq(XKX, DKX.T, rcond=None)[0]
    u = K.form(D, y) - DKX @ coef_y
    Q = 0.5 * float(u[:, 0] @ u[:, 0])
    F = 0.5 * (K.form(D, D) - DKX @ coef_D)
    return Q, F
