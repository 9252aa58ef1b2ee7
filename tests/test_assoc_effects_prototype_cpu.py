"""tools/assoc_effects_prototype.py -- the numpy statement of the effects kernels' algebra, sums over the rotated space and
no n x n matrix -- against the dense longdouble generalised least squares of
tests/assoc_effects_reference.py, on the cohorts and covariate widths of tests/test_gpu_association_effects.py and at the
oracle's own variance ratios (fast: the null model's delta; full refit: the optimum of each variant's ML fit).

This is also where the GPU test's tolerance comes from.  e64, the worst relative gap of the float64 oracle's own route
(``LMM._terms`` at delta, then ``_rsolve``) to the truth over every compared test, is measured here:

    measured e64 = 1.557e-12 (cohort A, mode B, one covariate column, beta; every other case stays below 3.2e-13)
    assoc_effects_reference.E64 = 1.6e-12 (two digits, rounded up)   ->   TOLERANCE = max(8 x 1.6e-12, 1e-12) = 1.28e-11

The prototype meets that bound (its worst gap here: 6.9e-13), which shows the bound is reachable in float64 by the kernel's
route before any GPU run.  Every compared test has delta inside [1e-4, 1 - 1e-4] (asserted), so the looser floor for
planted tests outside that range is never used on these cohorts.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

import assoc_effects_reference as ar  # noqa: E402
from assoc_effects_prototype import EFFECT_G_IN_SPAN_W, EFFECT_OK, effects_at, log_pvalue  # noqa: E402

WORST = {}


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("name", list(ar.CASES))
def test_prototype_meets_the_tolerance_and_e64_is_what_the_header_says(name, fast):
    cs = ar.case(name)
    rho, null_delta = ar.oracle_null(cs)
    Q0, S0 = cs.qs(rho)
    comp = cs.compared()
    if fast:
        deltas = np.full(len(comp), null_delta)
    else:
        deltas = np.array([ar.oracle_alt_delta(cs, rho, cs.G[:, j]) for j in comp])
    assert np.all((deltas >= ar.DELTA_RANGE[0]) & (deltas <= ar.DELTA_RANGE[1])), (name, deltas.min(), deltas.max())
    truth = ar.dense_truth(cs.y, cs.W, cs.G[:, comp], cs.gram(rho), deltas)
    o64 = np.array([ar.oracle64(cs.y, cs.W, cs.G[:, j], Q0, S0, d) for j, d in zip(comp, deltas)]).T
    got = [effects_at(cs.y, cs.W, cs.G[:, j], Q0, S0, d) for j, d in zip(comp, deltas)]
    assert all(g[4] == EFFECT_OK for g in got)
    e64 = float(ar.gaps(o64, truth).max())
    gap = float(ar.gaps(np.array([g[:3] for g in got]).T, truth).max())
    WORST[(name, fast)] = (e64, gap)
    print("\n[effects] %s, %s: rho %.1f, delta %.3g .. %.3g, r %d: e64 %.2e, prototype %.2e (tolerance %.2e)"
          % (name, "fast" if fast else "full refit", rho, deltas.min(), deltas.max(), S0.size, e64, gap, ar.TOLERANCE))
    assert e64 <= ar.E64, (name, e64)
    assert gap <= ar.TOLERANCE, (name, gap)


def test_planted_columns_of_cohort_a():
    """The column of W falls under the fast scanner's rank rule; so does the one 1e-9 away from it (its Schur complement is
    1e-18 of g'K^-1g: lost in the rounding of the sums); the causal variant's statistic is in the hundreds."""
    cs = ar.case("A, mode C, c 3")
    rho, delta = ar.oracle_null(cs)
    Q0, S0 = cs.qs(rho)
    for j in (ar.SPAN, ar.BOUNDARY):
        beta, se, scale, schur, status = effects_at(cs.y, cs.W, cs.G[:, j], Q0, S0, delta)
        assert status == EFFECT_G_IN_SPAN_W and np.isnan(beta) and np.isnan(se) and scale > 0
    beta, se, scale, schur, status = effects_at(cs.y, cs.W, cs.G[:, ar.CAUSAL], Q0, S0, delta)
    z2 = (beta / se) ** 2
    assert status == EFFECT_OK and cs.n * math.log1p(z2 / cs.n) > 200     # (the fast scanner's statistic in closed form)


def test_sign_and_scale_of_the_variant():
    cs = ar.case("A, mode B, c 1")
    rho, delta = ar.oracle_null(cs)
    Q0, S0 = cs.qs(rho)
    g = cs.G[:, 5]
    b1, s1, sc1, _, _ = effects_at(cs.y, cs.W, g, Q0, S0, delta)
    b2, s2, sc2, _, _ = effects_at(cs.y, cs.W, -2.0 * g, Q0, S0, delta)
    assert abs(b2 + b1 / 2) <= 1e-13 * abs(b1) and abs(s2 - s1 / 2) <= 1e-13 * s1 and abs(sc2 - sc1) <= 1e-13 * sc1


@pytest.mark.parametrize("lrs", [0.0, 1e-300, 1e-8, 1.0, 30.0, 1400.0, 1500.0, 5000.0])
def test_log_pvalue_branches_against_mpmath(lrs):
    """1400 and 1500 straddle the switch at p = 1e-300; 1e-300 and 1e-8 sit where erfc rounds to 1 - O(eps)."""
    got = log_pvalue(lrs / 2, 0.0)
    want = ar.mp_log_sf(lrs)
    assert abs(got - want) <= 1e-12 * abs(want), (lrs, got, float(want))
    if lrs == 0.0:
        assert got == 0.0
