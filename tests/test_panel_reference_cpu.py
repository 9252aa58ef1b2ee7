"""tests/panel_reference.py is right, and its bound discriminates: a faithful float64 evaluation of the standardisation
stays well inside it in any summation order, and every plausible slip of a kernel -- the wrong divisor, unweighted donors,
a lost partial sum of one wavefront or of the stride loop, the raw-moment variance, a single-precision mean -- leaves it
by a factor of at least four on the cohorts the GPU test (tests/test_gpu_panel_ingest.py) runs.  That is what lets the GPU
test fail for a subtly wrong kernel.

Measured with these cohorts (worst |got - ref| / bound per cohort a, b, c, d; "-" where the slip changes nothing at that size):

    faithful, donors in order / permuted / reversed     0.025    0.059    0.15     0.18
    sd with n - 1                                       2.8e12   7.4e10   5.2e9    3.7e9
    donors instead of cells                             1.6e14   1.6e13   3.9e13   4.7e13
    donors 64..127 left out of the mean                 -        2.2e13   4.9e14   4.5e14
    donors 64..127 left out of the variance             -        6.2e11   7.7e14   7.2e14
    donors from 256 on left out of the variance         -        -        3.5e11   2.0e14
    variance as sum w g^2 / n - mean^2                  -        45       34       30
    mean rounded to float32                             2.8e6    4.9e7    7.0e7    9.9e7
"""
import decimal
from fractions import Fraction

import numpy as np
import pytest

import panel_reference as pr

SLIPS = ("n_minus_1", "donors_not_cells", "mean_without_64_127", "var_without_64_127", "var_without_256_on", "raw_moments",
         "mean_float32")


def _seq_sum(a):
    return np.cumsum(a, axis=0)[-1]          # strictly one donor after the other, in the order given


def evaluate64(D, w, order, slip=None):
    """The standardised panel in float64, two passes, the donors summed in ``order``; ``slip``: one of SLIPS."""
    idx = np.asarray(order)
    g = D.astype(np.float64)[idx]
    wt = (np.ones(idx.shape[0]) if slip == "donors_not_cells" else w.astype(np.float64)[idx])[:, None]
    n = wt.sum()
    mid = ((idx >= 64) & (idx < 128))[:, None]
    mean = _seq_sum(np.where(mid & (slip == "mean_without_64_127"), 0.0, wt * g)) / n
    if slip == "mean_float32":
        mean = mean.astype(np.float32).astype(np.float64)
    c = g - mean
    dropped = (mid & (slip == "var_without_64_127")) | ((idx >= 256)[:, None] & (slip == "var_without_256_on"))
    var = _seq_sum(np.where(dropped, 0.0, wt * c * c)) / (n - 1 if slip == "n_minus_1" else n)
    if slip == "raw_moments":
        var = _seq_sum(wt * g * g) / n - mean * mean
    out = np.empty_like(g)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[idx] = c / np.sqrt(var)
    return out


def _ratio(got, ref, bound):
    r = np.abs(got.astype(pr.LD) - ref) / bound.astype(pr.LD)
    return float(np.where(np.isfinite(r), r, np.inf).max())     # (a NaN or an infinity is outside any bound)


def _to_decimal(x):
    hi = float(x)
    return decimal.Decimal(hi) + decimal.Decimal(float(x - pr.LD(hi)))     # exact: a longdouble is two doubles' worth


def test_reference_equals_exact_rational_arithmetic():
    rng = np.random.default_rng(3)
    m, p = 7, 5
    D = rng.integers(0, 3, size=(m, p)).astype(np.int8)
    D[:, 3] = 120 + D[:, 0]
    D[:, 4] = -128 + D[:, 1]
    D[:3, 0] = (0, 1, 2)
    D[:3, 1] = (2, 0, 1)
    D[:3, 2] = (0, 0, 1)
    donor = rng.permutation(np.repeat(np.arange(m), [3, 1, 7, 2, 0, 12, 5])).astype(np.int32)
    ref, _ = pr.standardised(D, donor)
    w, n, mean_ld, var_ld = pr.moments(D, donor)
    assert n == 30 and list(w) == [3, 1, 7, 2, 0, 12, 5]
    assert np.array_equal(pr.indicator(donor, m).sum(0), w) and np.array_equal(pr.indicator(donor, m).argmax(1), donor)
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        unit = decimal.Decimal(2) ** -63                      # longdouble's 2u, as 2^-52 is float64's in the bound
        for j in range(p):
            mean = sum(Fraction(int(w[d]) * int(D[d, j]), n) for d in range(m))
            var = sum(int(w[d]) * (int(D[d, j]) - mean) ** 2 for d in range(m)) / n
            assert var > 0
            sd = (decimal.Decimal(var.numerator) / decimal.Decimal(var.denominator)).sqrt()
            mean_d = decimal.Decimal(mean.numerator) / decimal.Decimal(mean.denominator)
            assert abs(_to_decimal(mean_ld[j]) - mean_d) <= unit * abs(mean_d)
            assert abs(_to_decimal(var_ld[j]) - sd * sd) <= unit * (m + 8) * sd * sd
            for d in range(m):
                exact = (int(D[d, j]) - mean_d) / sd
                tol = unit * ((abs(int(D[d, j])) + abs(mean_d)) / sd + (m + 8) * abs(exact))
                assert abs(_to_decimal(ref[d, j]) - exact) <= tol, (d, j)


def test_monomorphic_means_zero_variance_of_the_expanded_column():
    D = np.array([[0, 1, 5], [0, 1, 5], [1, 1, 5], [0, 2, 5]], np.int8)
    donor = np.array([0, 0, 1, 3, 3, 3], np.int32)             # donor 2 has no cell
    assert list(pr.monomorphic(D, donor)) == [True, False, True]
    assert list(pr.monomorphic(D, np.array([0, 1, 2, 3], np.int32))) == [False, False, True]
    _, _, _, var = pr.moments(D, donor)
    assert list(var == 0) == [True, False, True]
    with pytest.raises(ValueError, match="monomorphic"):
        pr.standardised(D, donor)


@pytest.mark.parametrize("name", sorted(pr.COHORTS))
def test_cohorts_are_what_the_gpu_test_needs(name):
    c = pr.cohort(name)
    m, p, ldd, empty = pr.COHORTS[name]
    D, donor = c["D"], c["donor_of_cell"]
    assert D.shape == (m, p) and D.dtype == np.int8 and c["wide"].shape == (m, ldd)
    assert np.array_equal(c["wide"][:, c["col0"]:c["col0"] + p], D)
    w = pr.cell_counts(donor, m)
    assert w.max() <= 12 and (w == 0).sum() == (empty is not None) and (empty is None or w[empty] == 0)
    assert not np.array_equal(donor, np.sort(donor)) and len(set(w)) > 1          # shuffled cells, ragged donors
    assert not pr.monomorphic(D, donor).any()                  # no column is monomorphic over the cells
    for j, kind in enumerate(c["kinds"]):
        col = D[:, j].astype(int)
        if kind == "single":
            assert (col != 0).sum() == 1 and w[np.flatnonzero(col)[0]] > 0
        elif kind == "top":
            assert col.min() >= 120 and col.max() <= 122
        elif kind == "bottom":
            assert col.min() >= -128 and col.max() <= -126 and (col == -128).any()
        else:
            assert col.min() >= 0 and col.max() <= 2
    assert set(c["kinds"]) == set(pr.KINDS[:max(1, min(p, len(pr.KINDS)))])


def test_faithful_float64_is_inside_the_bound_and_every_slip_is_outside():
    worst_faithful = {}
    factors = {s: {} for s in SLIPS}
    for name in sorted(pr.COHORTS):
        c = pr.cohort(name)
        D, donor, m = c["D"], c["donor_of_cell"], c["m"]
        ref, bound = pr.standardised(D, donor)
        w = pr.cell_counts(donor, m)
        orders = (np.arange(m), np.random.default_rng(m).permutation(m), np.arange(m)[::-1])
        worst_faithful[name] = max(_ratio(evaluate64(D, w, o), ref, bound) for o in orders)
        for s in SLIPS:
            factors[s][name] = _ratio(evaluate64(D, w, orders[0], s), ref, bound)
    print("faithful float64, worst |got - ref| / bound per cohort:", {k: "%.3g" % v for k, v in worst_faithful.items()})
    for s in SLIPS:
        print("%-22s" % s, {k: "%.3g" % v for k, v in factors[s].items()})
    assert max(worst_faithful.values()) <= 1.0, worst_faithful
    for s in SLIPS:
        assert max(factors[s].values()) >= 4.0, (s, factors[s])
