"""The cohorts of tests/test_gpu_context_many.py (plain helper module, not a test): cohorts of tests/context_lrt_cases.py
and tests/context_joint_cases.py -- their constructions imported, not restated -- each carrying several phenotypes, so that
tests/test_context_many_cases_cpu.py can hold every phenotype to the conditions the GPU tests rely on.

name -> (per-context or joint, [(what drives the phenotype, seed), ...]).  Phenotype i of a cohort is drawn the way the
cohort's constructor draws its own y, from the generator ``default_rng(seed)``, with the drive named (``DRIVE`` of
tests/context_lrt_cases.py: all three settings occur in every cohort; no seed twice in a cohort, since two drives of one seed
scale the same draws); the cohort's W, C, G, E1 and hK are shared.

    k 3, c 9, mode B       per-context; odd k
    k 17, c 70, mode B     per-context; past one candidate tile
    k 3, c 128, mode A     per-context; a single grid point, so all genes form one rho group
    k 5, rank 260, mode B  per-context; a background of 230 contexts of its own: several rho groups in one call
    k 33, c 35, mode B     joint; the first off-diagonal pair of candidate groups; a background of 60 contexts of its own
    k 48, c 128, mode B    joint; V in the variant's global scratch row, one row per (gene, variant)
Which grid point a null falls on.  In the cohorts whose background contexts ARE the tested contexts (E1 = C: the first two and
the last) C sits among the fixed effects, the rho E1 E1' part of the covariance is projected out, the likelihood does not
depend on rho and the first strict maximum is rho = 0 for every phenotype, whatever drives it (24 drive x seed pairs each
tried) -- one rho group, like mode A's single grid point.  The two cohorts with a background of their own (``MIXED``) are
the ones where the grid point follows the phenotype: there the seeds are chosen so that the oracle's gene-level nulls fall
on at least two grid points, one of them shared by two or more phenotypes and one held by exactly one (a rho group of
several genes and a group of one in the same call).  Every phenotype of every cohort meets the conditions of the
single-phenotype cohorts: refitted delta in (1e-3, 1 - 1e-3), 32 x the oracle's error below the 1e-11 ceiling
(tests/test_context_many_cases_cpu.py).  ``candidate_condition`` depends on W, C and G alone: it is the base cohort's.
"""
import copy

import numpy as np

import context_joint_cases as jc
import context_lrt_cases as cc

COHORTS = {
    "k 3, c 9, mode B": (False, [("mix", 1), ("mix", 2), ("kinship", 3), ("kinship", 4), ("contexts", 6), ("contexts", 7)]),
    "k 17, c 70, mode B": (False, [("mix", 2), ("mix", 3), ("kinship", 1), ("contexts", 4), ("contexts", 7)]),
    "k 3, c 128, mode A": (False, [("kinship", 1), ("contexts", 2), ("contexts", 4), ("mix", 3), ("mix", 5)]),
    "k 5, rank 260, mode B": (False, [("mix", 2), ("mix", 5), ("kinship", 6), ("contexts", 1), ("contexts", 3), ("contexts", 4)]),
    "k 33, c 35, mode B": (True, [("contexts", 2), ("contexts", 8), ("mix", 3), ("mix", 5), ("kinship", 6), ("contexts", 4)]),
    "k 48, c 128, mode B": (True, [("mix", 4), ("mix", 5), ("kinship", 1), ("kinship", 2), ("contexts", 3)]),
}
# the cohorts whose phenotypes fall on several grid points (see above)
MIXED = ("k 5, rank 260, mode B", "k 33, c 35, mode B")


def draw_phenotype(cs, drive, seed):
    """y of the cohort ``cs`` as its constructor draws it: drive x contexts + noise (+ drive x kinship), the persistent effect
    of variant 0 and the one that changes with the last context."""
    rng = np.random.default_rng(seed)
    a, b = cc.DRIVE[drive]
    y = a * (cs.E1 @ rng.normal(size=cs.E1.shape[1])) / np.sqrt(cs.E1.shape[1]) + rng.normal(size=cs.n)
    if cs.hK is not None:
        y = y + b * (cs.hK @ rng.normal(size=cs.hK.shape[1]))
    return y + 0.3 * cs.G[:, 0] + 0.4 * cs.G[:, 0] * cs.C[:, cs.k - 1]


def with_phenotype(cs, y):
    """The cohort ``cs`` with the phenotype ``y`` (a view: everything else is shared)."""
    view = copy.copy(cs)
    view.y = y
    return view


_cohorts = {}


def cohort(name):
    """(the base cohort, [one view per phenotype]) -- one object per cohort and process."""
    if name not in _cohorts:
        base = jc.case(name)
        _cohorts[name] = (base, [with_phenotype(base, draw_phenotype(base, drive, seed)) for drive, seed in COHORTS[name][1]])
    return _cohorts[name]


def is_joint(name):
    return COHORTS[name][0]
