"""The cohorts of tests/test_gpu_context_lrt.py (plain helper module, not a test), built on the simulator's cohorts like
tests/pinned_cases.py, so that tests/test_context_lrt_reference_cpu.py can hold every one of them to the conditions the GPU
tests rely on: at the float64 oracle's own optimum 32 x the oracle's error against the longdouble reference stays below
the 1e-11 ceiling, the refitted optima have delta in (1e-3, 1 - 1e-3), and the gene-level nulls of the mode-B cohorts fall
on more than one grid point.

name -> (donors, cells per donor, contexts k, columns of W, mode, seed, what drives the phenotype, columns of E1 or None)
c = rank([W, C]) = columns of W + k; spectrum rank: k (mode A), E1's columns + donors at the interior grid points (mode B).
With ``E1`` columns given, the background's contexts are E1 (a random effect of their own) and the tested contexts C are
its first k columns.
"""
import numpy as np

from cellregmap_amd.synth import make_cohort
from oracle import crm as ocrm
from oracle.lmm import LMM
from oracle.sugar import economic_qs_linear

import pinned_reference as pr

CASES = {
    "k 1, c 2, mode B": (12, 15, 1, 1, "B", 71, "kinship", None),          # 180 cells, spectrum 13; one candidate
    "k 3, c 9, mode B": (12, 15, 3, 6, "B", 72, "mix", None),              # 180 cells, spectrum 15; odd k
    "k 5, c 62, mode B": (10, 20, 5, 57, "B", 73, "kinship", None),        # 200 cells, spectrum 15; 64 Gram rows
    "k 17, c 70, mode B": (10, 20, 17, 53, "B", 74, "mix", None),          # 200 cells, spectrum 27; past one 16-column tile
    "k 3, c 128, mode A": (10, 30, 3, 125, "A", 75, "contexts", 15),       # 300 cells, spectrum 15; 130 Gram rows
    "k 5, rank 260, mode B": (30, 10, 5, 2, "B", 76, "contexts", 230),     # 300 cells, spectrum 260 at the interior points
}
DRIVE = {"kinship": (0.0, 3.0), "contexts": (4.0, 0.0), "mix": (2.0, 1.0)}


class ContextCase:
    def __init__(self, name, variants=3):
        donors, cells, k, cW, mode, seed, drive, e1 = CASES[name]
        co = make_cohort(donors, cells, k if e1 is None else e1, variants, seed=seed)
        rng = np.random.default_rng(seed + 500)
        n = co.y.size
        self.name, self.n, self.k, self.mode, self.donors = name, n, k, mode, donors
        self.E1, self.hK, self.donor_of_cell = co.E, (co.hK if mode == "B" else None), co.donor_of_cell
        self.C = np.ascontiguousarray(co.E[:, :k])
        self.W = np.column_stack([np.ones(n)] + [rng.normal(size=n) for _ in range(cW - 1)])
        self.G = co.G + 0.05 * rng.normal(size=co.G.shape)
        self.grid = [1.0] if mode == "A" else list(ocrm.RHO_GRID)
        a, b = DRIVE[drive]
        y = a * (self.E1 @ rng.normal(size=self.E1.shape[1])) / np.sqrt(self.E1.shape[1]) + rng.normal(size=n)
        if self.hK is not None:
            y = y + b * (self.hK @ rng.normal(size=self.hK.shape[1]))
        # a persistent effect of variant 0 and one that changes with the last context
        self.y = y + 0.3 * self.G[:, 0] + 0.4 * self.G[:, 0] * self.C[:, k - 1]

    def half(self, rho):
        return pr.half_factor(rho, self.E1, hK=self.hK)

    def X0(self):
        return np.column_stack([self.W, self.C])

    def X(self, j):
        return np.column_stack([self.W, self.C, self.G[:, j]])

    def device_kw(self):
        kw = {"E1": self.E1}
        if self.hK is not None:
            kw["hK"] = self.hK
        return kw


_cases = {}


def case(name):
    """One object per cohort and process."""
    if name not in _cases:
        _cases[name] = ContextCase(name)
    return _cases[name]


def oracle_gene_null(cs):
    """(rho, the fitted LMM, (Q0, S0)) of the oracle's gene-level ML null LMM(y, [W, C], QS(rho)): first strict maximum."""
    best = None
    for rho in cs.grid:
        (Q0,), S0 = economic_qs_linear(cs.half(rho), return_q1=False)
        lmm = LMM(cs.y, cs.X0(), ((Q0,), S0), restricted=False)
        lmm.fit(verbose=False)
        if best is None or lmm.lml() > best[1].lml():
            best = (float(rho), lmm, (Q0, S0))
    return best
