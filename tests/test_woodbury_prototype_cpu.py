"""The unrelated-donor form of the score test (tools/woodbury_prototype.py, the algebra of scan.hip: kin_wb and
assemble.hip: woodbury_kernel) against the reference's spectral form restated in oracle/scoretest.py, on ragged cohorts:
unequal donor sizes and kappa_d, k2 > n_d for some donors, E1 != E2 != E0, rho* in {0, 0.3, 1}, delta at its upper clamp."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import scoretest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototype():
    spec = importlib.util.spec_from_file_location("woodbury_prototype", os.path.join(ROOT, "tools", "woodbury_prototype.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cohort(seed):
    rng = np.random.default_rng(seed)
    sizes = np.array([3, 9, 14, 5, 22, 2, 11])          # k2 = 6 > 3, 5 and 2 cells
    group = np.repeat(np.arange(sizes.size), sizes)
    n = group.size
    kappa = rng.uniform(0.3, 2.5, size=sizes.size)
    E0, E1, E2 = rng.normal(size=(n, 4)), rng.normal(size=(n, 3)), rng.normal(size=(n, 6))
    W = np.column_stack([np.ones(n), rng.normal(size=n)])
    return rng, group, kappa, E0, E1, E2, W


def _spectral(E1, E2, group, kappa, rho):
    """Q0, S0 of Sigma(rho) = rho E1E1' + (1 - rho) (K o E2E2'), K = kappa on the donor blocks, its kept spectrum."""
    same = group[:, None] == group[None, :]
    K = np.where(same, kappa[group][:, None], 0.0)
    S = rho * E1 @ E1.T + (1.0 - rho) * K * (E2 @ E2.T)
    s, Q = np.linalg.eigh(S)
    keep = s > S.shape[0] * np.finfo(float).eps * s.max()
    return Q[:, keep], s[keep]


@pytest.mark.parametrize("rho", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("clamp", [False, True], ids=["fit", "delta-at-clamp"])
def test_woodbury_form_equals_the_spectral_form(rho, clamp):
    proto = _prototype()
    rng, group, kappa, E0, E1, E2, W = _cohort(11)
    n = group.size
    y = rng.normal(size=n)
    scale = 1.7
    delta = 1.0 - 2.220446049250313e-16 if clamp else 0.35
    v0, v1 = scale * (1.0 - delta), scale * delta
    Q0, S0 = _spectral(E1, E2, group, kappa, rho)
    for seed in range(3):
        g = np.random.default_rng(seed).normal(size=n)
        gtest = g[np.random.default_rng(seed + 9).permutation(n)]
        K = scoretest.LowRankCov(Q0, S0, v0, v1)
        P = scoretest.Projection(K, np.column_stack([W, g]))
        half = gtest[:, None] * E0
        q_ref = np.asarray(scoretest.score_Q(P, half, y[:, None])).item()
        F_ref = scoretest.score_F(P, half)
        q, F = proto.score_QF(y, W, g, gtest, E0, E1, E2, group, kappa, rho, v0, v1)
        tol = max(abs(q_ref), np.trace(F_ref))
        assert abs(q - q_ref) <= 1e-12 * tol, (q, q_ref)
        assert np.abs(F - F_ref).max() <= 1e-12 * np.abs(F_ref).max()


def test_dropped_directions_are_the_donors_without_enough_cells():
    proto = _prototype()
    _, group, _, _, _, E2, _ = _cohort(3)
    basis = proto.donor_basis(E2, group, group.max() + 1)
    for cells, Phi, lam in basis:
        assert Phi.shape[1] == min(cells.size, E2.shape[1])
        assert np.allclose(Phi.T @ Phi, np.eye(Phi.shape[1]), atol=1e-12)
