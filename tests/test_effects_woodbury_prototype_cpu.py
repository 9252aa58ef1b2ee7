"""tools/effects_woodbury_prototype.py (the numpy statement of the batched effect-size route)
against the oracle's LMM on each SNP's own decomposition of [sqrt(rho) g o E0, sqrt(1 - rho) L..]."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

from effects_woodbury_prototype import WoodburyEffects  # noqa: E402
from oracle import crm as ocrm  # noqa: E402
from oracle.lmm import LMM  # noqa: E402
from oracle.sugar import economic_qs_linear  # noqa: E402
from cellregmap_amd.synth import make_cohort  # noqa: E402

DELTAS = [1e-6, 1e-4, 1e-2, 0.1, 0.5, 0.9, 0.99, 1 - 1e-4, 1 - 1e-6]


def _case(kind):
    c = make_cohort(8, 12, 3, 3, seed=17)
    rng = np.random.default_rng(4)
    n = c.y.shape[0]
    g = c.G[:, [1]]
    if kind == "mode_a":
        return c, g, None, c.W
    if kind == "cell_level":       # a cell-level factor; g varies within donors
        return c, rng.normal(size=(n, 1)), [rng.normal(size=(n, 6))], np.column_stack([c.W, rng.normal(size=n)])
    halves = ocrm.khatri_rao_halves(c.hK, c.E)
    if kind == "hadamard":         # Hadamard halves, g varying within donors
        return c, g + 0.3 * rng.normal(size=(n, 1)), halves, c.W
    return c, g, halves, c.W       # unrelated donors, donor-constant g: g o E0 in span(L)


def _oracle(c, W, g, halves, rho, delta):
    M = np.concatenate((W, g, c.E), axis=1)
    hS = np.concatenate([np.sqrt(rho) * g * c.E] + [np.sqrt(1 - rho) * L for L in (halves or [])], axis=1)
    lmm = LMM(c.y, M, economic_qs_linear(hS, return_q1=False), restricted=True)
    lmm._x = float(np.log(delta / (1 - delta)))
    lmm._update()
    return lmm


@pytest.mark.parametrize("kind", ["mode_a", "cell_level", "hadamard", "span"])
def test_lml_and_beta_at_fixed_rho_and_delta(kind):
    c, g, halves, W = _case(kind)
    proto = WoodburyEffects(c.y, W, c.E, g, L=halves)
    for rho in proto.rho_grid[::2] if halves is not None else proto.rho_grid:
        for delta in DELTAS:
            lmm = _oracle(c, W, g, halves, rho, delta)
            d = lmm.delta
            lml, beta, _ = proto.state(float(rho), d)
            # (the observed floor: the oracle's own rounding of c(u, v) / delta at the ends of the sweep, where the
            # complement numerators of U cancel to ~1e-16 of u'u and are divided by delta = 1e-6)
            tol = 1e-10 if 1e-4 <= d <= 1 - 1e-4 else 1e-8
            assert abs(lml - lmm.lml()) <= tol * abs(lmm.lml()), (kind, rho, d, lml, lmm.lml())
            scale = np.max(np.abs(lmm.beta))
            assert np.max(np.abs(beta - lmm.beta)) <= tol * 100 * scale, (kind, rho, d, beta, lmm.beta)


@pytest.mark.parametrize("kind", ["mode_a", "hadamard", "span"])
def test_betas_at_the_oracle_optimum(kind):
    """With the oracle's polished optimum (rho*, delta*) fed in, beta_g and beta_gxe match estimate_betas(polish=True)."""
    c, g, halves, W = _case(kind)
    maf = np.array([0.3])
    grid = [1.0] if halves is None else ocrm.RHO_GRID
    best, best_rho = None, None
    for rho in grid:
        M = np.concatenate((W, g, c.E), axis=1)
        hS = np.concatenate([np.sqrt(rho) * g * c.E] + [np.sqrt(1 - rho) * L for L in (halves or [])], axis=1)
        lmm = LMM(c.y, M, economic_qs_linear(hS, return_q1=False), restricted=True)
        lmm.fit(verbose=False, polish=True)
        if best is None or lmm.lml() > best.lml():
            best, best_rho = lmm, rho
    crm = ocrm.OracleCellRegMap(c.y, c.E, W=W, Ls=halves, polish=True)
    obg, obgxe = crm.predict_interaction(g, maf)
    proto = WoodburyEffects(c.y, W, c.E, g, L=halves)
    bg, bgxe = proto.betas(maf[0], rho=float(best_rho), delta=best.delta)
    assert abs(bg - obg[0]) <= 1e-9 * max(abs(obg[0]), 1e-3), (bg, obg)
    assert np.max(np.abs(bgxe - obgxe[0, :, 0])) <= 1e-9 * np.max(np.abs(obgxe)), (np.max(np.abs(bgxe - obgxe[0, :, 0])))


def test_the_fit_picks_the_oracle_grid_point():
    c, g, halves, W = _case("hadamard")
    proto = WoodburyEffects(c.y, W, c.E, g, L=halves)
    rho, delta, lml = proto.fit()
    crm = ocrm.OracleCellRegMap(c.y, c.E, W=W, Ls=halves)
    obg, _ = crm.predict_interaction(g, np.array([0.3]))
    bg, _ = proto.betas(0.3, rho=rho, delta=delta)
    assert abs(bg - obg[0]) <= 1e-4 * max(abs(obg[0]), 1e-3)
