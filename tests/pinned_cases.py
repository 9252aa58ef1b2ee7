"""The cohorts of tests/test_gpu_pinned_effects.py and tests/test_gpu_pinned_association.py (plain helper module, not a
test): built here so that tests/test_pinned_reference_cpu.py can hold every one of them to the condition the GPU tests
rely on -- at the float64 oracle's own optimum, 32 x the oracle's error against the longdouble reference stays below the
1e-11 ceiling, so that the ceiling never sets a limit.  A cohort that fails that check is replaced here.

All cohorts stay at or below 320 cells: one longdouble evaluation of the reference is then well under a second.
"""
import numpy as np

from cellregmap_amd.synth import make_cohort
from oracle import crm as ocrm
from oracle.lmm import LMM
from oracle.sugar import economic_qs_linear

import pinned_reference as pr

# ---- effect sizes ---------------------------------------------------------------------------------------------------------
# name -> (donors, cells per donor, k0, columns of W, columns of E2 or None for mode A, variants, seed)
# packed width = cW + 2 k0 + 2; r_L = donors x columns of E2
EFFECTS = {
    "width 10, r_L 24": (8, 15, 3, 2, 3, 70, 3),              # 120 cells; 70 variants: two variant blocks
    "width 10, mode A": (8, 15, 3, 2, None, 4, 3),
    "width 66, r_L 40": (8, 22, 31, 2, 5, 3, 12),             # 176 cells; r_L above 32 and no multiple of it
    "width 130, r_L 10": (5, 31, 63, 2, 2, 3, 13),            # 155 cells; the last width of the batched form
    "k0 65, mode A": (10, 20, 65, 1, None, 2, 8),             # 200 cells; width 133: the per-SNP path serves it
}

# the (phenotype, variant) pairs the GPU tests name, per cohort -- the three phenotypes on variant 1 first; on the smallest
# cohort every phenotype also on the variants at the edges of the variant block and of the pair chunk.  The CPU suite
# holds the ceiling condition on each of them.  (Phenotype 2 carries the g o E0 effect of variant 1 alone.  With that
# effect at 3 x the noise, as this cohort first had it, the fit on any other variant puts the unexplained variance into
# v0 = 6.3 at rho <= 0.2 and the float64 oracle's own beta is off by up to 1.5e-12 there, 4.8 x what the ceiling leaves
# room for; at 1 x the noise -- rho* = 1 on variant 1 still -- it is 8e-14 at most, so the cohort was replaced.)
EFFECTS_HELD = {
    "width 10, r_L 24": [(0, 1), (1, 1), (2, 1), (1, 0), (1, 63), (1, 64), (1, 69), (2, 0), (2, 63), (2, 64), (2, 69),
                         (0, 0), (1, 2), (2, 2), (0, 2)],
    "width 10, mode A": [(0, 1), (1, 1), (2, 1)],
    "width 66, r_L 40": [(0, 1), (1, 1), (2, 1)],
    "width 130, r_L 10": [(0, 1), (1, 1), (2, 1)],
    "k0 65, mode A": [(1, 0), (2, 1)],
}


class EffectsCase:
    """Y holds three phenotypes: one driven by the L component (rho* = 0 on variant 1), a mixture (interior), one driven
    by g o E0 of variant 1 (rho* = 1)."""

    def __init__(self, name):
        donors, cells, k0, cW, e2, variants, seed = EFFECTS[name]
        co = make_cohort(donors, cells, k0, variants, seed=seed)
        rng = np.random.default_rng(seed + 500)
        n = co.y.size
        self.name, self.n, self.k0, self.cW = name, n, k0, cW
        self.W = np.column_stack([np.ones(n)] + [rng.normal(size=n) for _ in range(cW - 1)])
        self.E0, self.G, self.hK = co.E, co.G, co.hK
        self.maf = np.clip(np.minimum(co.G.mean(0) / 2, 1 - co.G.mean(0) / 2), 0.05, 0.5)
        self.E2 = None if e2 is None else (co.E if e2 == k0 else rng.normal(size=(n, e2)))
        self.half_L = None if e2 is None else np.concatenate(ocrm.khatri_rao_halves(co.hK, self.E2), axis=1)
        self.grid = [1.0] if e2 is None else list(ocrm.RHO_GRID)
        part_l = np.zeros(n) if e2 is None else (self.half_L @ rng.normal(size=self.half_L.shape[1])) / np.sqrt(e2)
        part_gxe = co.G[:, 1] * (co.E @ rng.normal(size=k0)) / np.sqrt(k0)
        noise = rng.normal(size=(n, 3))
        self.Y = np.column_stack([3.0 * part_l + noise[:, 0], 1.5 * part_l + 1.5 * part_gxe + noise[:, 1],
                                  (1.0 if k0 == 3 else 2.0) * part_gxe + noise[:, 2]])

    def operands(self, i, v):
        """(y, M, U) of the pair (phenotype i, variant v)."""
        g = self.G[:, [v]]
        return self.Y[:, i], np.concatenate((self.W, g, self.E0), axis=1), g * self.E0


def effects_records(cs, y, M, U, rho, v0, v1, got=None, norm=1.0):
    """(the reference's record, the float64 oracle's at the same point -- or that of ``got`` = (beta, u, lml, scale)):
    dicts with beta, u, beta_gxe = norm v0 rho E0 u, the restricted lml and the scale at delta = v1 / (v0 + v1)."""
    LD = pr.LD
    beta, u = pr.pinned_effects(y, M, U, cs.half_L, rho, v0, v1)
    _, _, lml, s = pr.pinned(y, M, pr.effects_half(U, cs.half_L, rho), np.zeros((y.size, 0)), LD(v1) / (LD(v0) + LD(v1)))
    ref = {"beta": beta, "u": u, "beta_gxe": (LD(norm) * LD(v0) * LD(rho)) * (np.asarray(cs.E0, LD) @ u), "lml": lml, "scale": s}
    b, uu, l, sc = pr.oracle_effects_at(y, M, U, cs.half_L, rho, v0, v1) if got is None else got
    return ref, {"beta": b, "u": uu, "beta_gxe": (v0 * rho) * (cs.E0 @ uu) * norm, "lml": l, "scale": sc}


def oracle_effects_point(y, M, U, half_L, grid):
    """(rho, v0, v1, lml) of the oracle's own fit: oracle/crm.py: predict_interaction's loop over the grid."""
    best = None
    for rho in grid:
        lmm = LMM(y, M, economic_qs_linear(pr.effects_half(U, half_L, rho), return_q1=False), restricted=True)
        lmm.fit(verbose=False)
        if best is None or lmm.lml() > best[3]:
            best = (float(rho), lmm.v0, lmm.v1, lmm.lml())
    return best


# ---- association ------------------------------------------------------------------------------------------------------------
# name -> (donors, cells per donor, contexts, covariate columns, mode, seed, what drives the phenotype)
# spectrum rank: contexts (mode A), contexts + donors at the interior grid points (mode B); past 256 contexts (the limit
# of E0) the background's contexts go in as E1 and E0 keeps the first three of them
ASSOCIATION = {
    "c 1, mode B": (10, 15, 3, 1, "B", 61, "mix"),                  # 150 cells, register null-fit kernel
    "c 9, mode B": (12, 15, 3, 9, "B", 62, "kinship"),              # 180 cells, LDS kernel at its first count
    "c 62, mode B": (12, 15, 3, 62, "B", 63, "contexts"),           # ... at its last
    "c 70, mode B": (12, 15, 3, 70, "B", 64, "mix"),                # 63..128 columns
    "c 128, mode A": (10, 20, 5, 128, "A", 65, "contexts"),         # 200 cells, CMAX
    "rank 260, mode A": (10, 30, 260, 2, "A", 66, "contexts"),      # 300 cells: past one 256-thread stride, no multiple
    "rank 260, mode B": (30, 10, 230, 3, "B", 67, "mix"),           # 300 cells, 230 + 30 at the interior points
}
DRIVE = {"kinship": (0.0, 3.0), "contexts": (6.0, 0.0), "mix": (2.0, 1.0)}


class AssociationCase:
    def __init__(self, name, variants=3):
        donors, cells, k, c, mode, seed, drive = ASSOCIATION[name]
        co = make_cohort(donors, cells, k, variants, seed=seed)
        rng = np.random.default_rng(seed + 500)
        n = co.y.size
        self.name, self.n, self.mode = name, n, mode
        self.E1, self.hK, self.donor_of_cell, self.donors = co.E, (co.hK if mode == "B" else None), co.donor_of_cell, donors
        self.E = co.E if k <= 256 else co.E[:, :3]
        self.W = np.column_stack([np.ones(n)] + [rng.normal(size=n) for _ in range(c - 1)])
        self.G = co.G + 0.05 * rng.normal(size=co.G.shape)
        self.grid = [1.0] if mode == "A" else list(ocrm.RHO_GRID)
        self.y = self.phenotype(rng, drive) + 0.3 * self.G[:, 0]

    def phenotype(self, rng, drive):
        a, b = DRIVE[drive]
        y = a * (self.E1 @ rng.normal(size=self.E1.shape[1])) / np.sqrt(self.E1.shape[1]) + rng.normal(size=self.n)
        if self.hK is not None:
            y = y + b * (self.hK @ rng.normal(size=self.hK.shape[1]))
        return y

    def half(self, rho):
        return pr.half_factor(rho, self.E1, hK=self.hK)


def oracle_null(y, W, half_of, grid):
    """(rho, the fitted LMM, (Q0, S0)) of the oracle's ML null model (oracle/crm.py: null_fit)."""
    best = None
    for rho in grid:
        (Q0,), S0 = economic_qs_linear(half_of(rho), return_q1=False)
        lmm = LMM(y, W, ((Q0,), S0), restricted=False)
        lmm.fit(verbose=False)
        if best is None or lmm.lml() > best[1].lml():
            best = (float(rho), lmm, (Q0, S0))
    return best
