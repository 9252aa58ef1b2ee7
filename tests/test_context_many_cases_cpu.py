"""CPU checks behind tests/test_gpu_context_many.py: every phenotype of every cohort of tests/context_many_cases.py meets the
conditions the single-phenotype GPU tests rely on -- asserted with the oracle, ``oracle_gene_null`` and the rows of
tests/test_context_lrt_reference_cpu.py and tests/test_context_joint_reference_cpu.py -- and the phenotypes of a cohort fall on
the grid points the many calls are to be tried on: several rho groups in one call, one of several genes and one of one."""
import numpy as np
import pytest

import context_joint_cases as jc
import context_lrt_cases as cc
import context_many_cases as mc
import pinned_reference as pr
from test_context_joint_reference_cpu import _oracle_rows as _joint_rows
from test_context_lrt_reference_cpu import _oracle_rows as _each_rows

PHENOTYPES = [(name, i) for name in mc.COHORTS for i in range(len(mc.COHORTS[name][1]))]

_nulls = {}


def _gene_null(name, i):
    if (name, i) not in _nulls:
        rho, lmm, _ = cc.oracle_gene_null(mc.cohort(name)[1][i])
        _nulls[name, i] = (rho, float(lmm.delta))
    return _nulls[name, i]


def test_the_cohorts_are_the_shapes_asked_for():
    assert set(mc.COHORTS) == {"k 3, c 9, mode B", "k 17, c 70, mode B", "k 3, c 128, mode A", "k 5, rank 260, mode B",
                               "k 33, c 35, mode B", "k 48, c 128, mode B"}
    assert {name for name in mc.COHORTS if mc.is_joint(name)} == {"k 33, c 35, mode B", "k 48, c 128, mode B"}
    from cellregmap_amd import _engine  # noqa: F401  (the package imports without a GPU)

    for name, (_, draws) in mc.COHORTS.items():
        base, views = mc.cohort(name)
        assert base is jc.case(name) and 5 <= len(views) == len(draws) <= 7, name
        assert {drive for drive, _ in draws} == set(cc.DRIVE), name           # the three settings
        assert len({seed for _, seed in draws}) == len(draws), name              # several seeds, none twice
        for v in views:                                                       # views: everything but y is the cohort's own
            assert v.G is base.G and v.C is base.C and v.W is base.W and v.y is not base.y
        ys = np.column_stack([v.y for v in views])
        assert np.linalg.matrix_rank(ys) == len(views), name
    # V leaves LDS on the last cohort and on no other: (c + 1) k doubles beside the rest, context_joint.hip's rule
    k, c = 48, 128
    R, Rp, Kp = c + 2, (c + 2 + 15) // 16 * 16, (k + 15) // 16 * 16
    base_doubles = R * (R + 1) // 2 + (k + 1) * (k + 2) // 2 + (max(Rp, Kp) + 32) * 33 + 256 + 64 + 32 + 8
    assert 8 * base_doubles <= 160 * 1024 < 8 * (base_doubles + (c + 1) * k)


@pytest.mark.parametrize("name,i", PHENOTYPES)
def test_every_phenotype_meets_the_conditions_of_the_single_phenotype_cohorts(name, i):
    base, views = mc.cohort(name)
    v = views[i]
    if mc.is_joint(name):
        rho, delta0, rows = _joint_rows(v)
        ora, deltas = pr.worst([r[1] for r in rows]), [r[0] for r in rows]
    else:
        rho, rows = _each_rows(v.y, v.W, v.C, v.G, v.half, v.grid)
        ora, deltas = pr.worst([e for _, e in rows]), [d for d, _ in rows]
        delta0 = _gene_null(name, i)[1]
    assert rho == _gene_null(name, i)[0]
    print("%s, phenotype %d %s (rho %.1f, delta0 %.3f): 32 x the oracle's error: %s" % (
        name, i, mc.COHORTS[name][1][i], rho, delta0, ", ".join("%s %.2e" % (k, 32 * e) for k, e in sorted(ora.items()))))
    for key, e in ora.items():
        assert pr.PATHS * e <= pr.CEILING, (name, i, key, e)                  # the ceiling never sets a limit
    for delta in deltas + [delta0]:                                          # optima away from the clamps
        assert 1e-3 < delta < 1 - 1e-3, (name, i, delta)
    if i == 0:                                                               # (depends on W, C and G alone)
        for j in pr.pick(base.G.shape[1]):
            assert jc.candidate_condition(base, j) < 100.0, (name, j, jc.candidate_condition(base, j))


@pytest.mark.parametrize("name", list(mc.COHORTS))
def test_the_grid_points_of_a_cohorts_nulls(name):
    base, views = mc.cohort(name)
    rhos = [_gene_null(name, i)[0] for i in range(len(views))]
    counts = {r: rhos.count(r) for r in set(rhos)}
    print(name, rhos)
    if name in mc.MIXED:
        assert base.mode == "B" and base.E1.shape[1] > base.k
        assert len(counts) >= 2, rhos                                        # at least two grid points
        assert max(counts.values()) >= 2, rhos                               # one shared by two or more phenotypes
        assert min(counts.values()) == 1, rhos                               # one held by exactly one
    else:
        # E1 = C sits among the fixed effects (or mode A's single grid point): one rho group, whatever drives y
        assert base.mode == "A" or base.E1.shape[1] == base.k
        assert len(counts) == 1, rhos
