"""The cohorts of tests/test_gpu_context_joint.py (plain helper module, not a test): the six of
tests/context_lrt_cases.py and four wider ones built the same way on the simulator's cohorts, so that
tests/test_context_joint_reference_cpu.py can hold every one of them to the conditions the GPU tests rely on.

name -> (donors, cells per donor, contexts k, columns of W, mode, seed, what drives the phenotype, columns of E1 or None),
as tests/context_lrt_cases.py states its own; c = rank([W, C]) = columns of W + k.

    k 33, c 35     the first off-diagonal pair of candidate groups (32 + 1)
    k 50, c 51     BASELINE config 3's widths
    k 64, c 66     two full groups: the limit the call has to serve
    k 48, c 128    the largest footprint: V leaves LDS for the variant's global scratch row
Seeds and drives are chosen so that every fitted delta is interior (0.35 .. 0.89), the first wide cohort, whose
background holds 60 contexts of which 33 are tested, has its gene-level null on the interior grid point rho = 0.6, and
every held variant's candidate set is well conditioned: with ten donors a rare genotype is carried by one donor's
30 .. 40 cells only, fewer than the candidates g o C_j tested on them, and the set is then dependent up to the 5 % noise
(``candidate_condition`` above 1 000 for one variant each of seeds 182 at k = 50 and 191 at k = 33; every product
a'K^-1b = a'b / delta - sum_s phi_s ta_s tb_s carries the rounding of a difference, the float64 oracle's included, and
beta inherits it times that condition number).  tests/test_context_joint_reference_cpu.py holds ``candidate_condition``
below 100 on every cohort.
"""
import numpy as np

from cellregmap_amd.synth import make_cohort
from oracle import crm as ocrm

import context_lrt_cases as cc

WIDE = {
    "k 33, c 35, mode B": (10, 30, 33, 2, "B", 181, "contexts", 60),       # 300 cells, spectrum 70; the null at rho = 0.6
    "k 50, c 51, mode B": (10, 36, 50, 1, "B", 202, "mix", None),          # 360 cells, spectrum 60
    "k 64, c 66, mode B": (10, 40, 64, 2, "B", 193, "mix", None),          # 400 cells, spectrum 74
    "k 48, c 128, mode B": (10, 40, 48, 80, "B", 184, "mix", None),        # 400 cells, spectrum 58
}
CASES = dict(cc.CASES)
CASES.update(WIDE)


class JointCase(cc.ContextCase):
    """A cohort of ``CASES``: ``context_lrt_cases.ContextCase`` for its six, the same construction for the wide ones."""

    def __init__(self, name, variants=3):
        if name in cc.CASES:
            super().__init__(name, variants)
            return
        donors, cells, k, cW, mode, seed, drive, e1 = WIDE[name]
        co = make_cohort(donors, cells, k if e1 is None else e1, variants, seed=seed)
        rng = np.random.default_rng(seed + 500)
        n = co.y.size
        self.name, self.n, self.k, self.mode, self.donors = name, n, k, mode, donors
        self.E1, self.hK, self.donor_of_cell = co.E, (co.hK if mode == "B" else None), co.donor_of_cell
        self.C = np.ascontiguousarray(co.E[:, :k])
        self.W = np.column_stack([np.ones(n)] + [rng.normal(size=n) for _ in range(cW - 1)])
        self.G = co.G + 0.05 * rng.normal(size=co.G.shape)
        self.grid = [1.0] if mode == "A" else list(ocrm.RHO_GRID)
        a, b = cc.DRIVE[drive]
        y = a * (self.E1 @ rng.normal(size=self.E1.shape[1])) / np.sqrt(self.E1.shape[1]) + rng.normal(size=n)
        if self.hK is not None:
            y = y + b * (self.hK @ rng.normal(size=self.hK.shape[1]))
        self.y = y + 0.3 * self.G[:, 0] + 0.4 * self.G[:, 0] * self.C[:, k - 1]


_cases = {}


def case(name):
    """One object per cohort and process (the six narrow ones are ``context_lrt_cases.case``'s own objects)."""
    if name in cc.CASES:
        return cc.case(name)
    if name not in _cases:
        _cases[name] = JointCase(name)
    return _cases[name]


def candidate_condition(cs, j):
    """Condition number of the Gram of variant j's candidates g o C_k, projected off [W, C, g] and scaled to unit length."""
    Q, _ = np.linalg.qr(cs.X(j))
    R = cs.G[:, [j]] * cs.C
    R = R - Q @ (Q.T @ R)
    return float(np.linalg.cond(R / np.linalg.norm(R, axis=0)) ** 2)
