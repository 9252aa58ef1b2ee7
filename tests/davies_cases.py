"""The (Q, weights) table on which Davies' and Liu's p-values are held to long-double and mpmath references, at every
width at which csrc/davies.hip takes another trip of a loop (plain helper module, not a test; imported by
tests/test_oracle_davies_widths_cpu.py and tests/test_gpu_davies_widths.py).

Everything is deterministic (fixed seeds).  A case is one row of a launch of the Davies hook: ``k`` weights in ascending
order and a statistic ``q``.  Except in the ``filter`` rows every weight is past SKAT's filter, so the kernel integrates
exactly the row it is given.
"""
from collections import namedtuple

import numpy as np

# 2..7: every phase of the rescale at (j & 3) == 0; 63..66 and 127..129: around one and two trips of the lane-strided loops
WIDTHS = (2, 3, 4, 5, 6, 7, 12, 50, 63, 64, 65, 66, 127, 128, 129, 200, 256)
Q_FRACTIONS = (0.05, 0.2, 0.6, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0, 20.0, 60.0)      # times sum(lam)
SHAPES = ("gamma", "flat", "geometric", "dominant")
AUX_WIDTHS = (12, 65, 129, 256)
AUX_HEADS = ((3.0, 6.0), (1.0, 3.0, 6.0), (5.0,))
AUX_Q = (2.0, 7.0, 20.0)
# Q far above / below the mean: the cut-off search ends the algorithm (cdf 1: Liu's value is returned; cdf 0: p = 1)
EARLY_FRACTIONS = (1e-9, 500.0)
# Liu alone, out to where p leaves the double range
LIU_FAR_FRACTIONS = (100.0, 300.0, 1000.0, 3000.0)
FILTER_WIDTHS = (65, 129)

Case = namedtuple("Case", "name k lam q kind")     # kind: "davies", "aux", "early", "liu_far", "filter"


def _seed(*parts):
    return np.random.default_rng([2026, *parts])


def weights(shape, r):
    """r ascending weights past SKAT's filter (lam > mean / 1e5)."""
    rng = _seed(SHAPES.index(shape), r)
    j = np.arange(r)
    if shape == "gamma":
        lam = rng.gamma(0.7, 1.0, size=r)
        lam = lam + 1e-3 * lam.mean()                 # (a gamma(0.7) draw can fall below the filter's threshold)
    elif shape == "flat":
        lam = 1.0 + 0.01 * rng.random(r)              # never exactly equal: see the note on Liu's branch in the CPU tests
    elif shape == "geometric":
        lam = np.maximum(0.9 ** j, 1e-3 * (1.0 + (r - j) / r))   # (0.9^j alone falls below the filter's threshold past j = 100)
    elif shape == "dominant":
        lam = 1e-3 * (1.0 + rng.random(r))
        lam[-1] = 1.0
    else:
        raise ValueError(shape)
    lam = np.sort(lam)
    assert np.all(lam > lam.mean() / 1e5)
    return lam


def aux_weights(head, r):
    """The published AS 155 weights (6, 3, 1) -- or a part of them -- over r - len(head) weights of 3e-4 (1 + U): the main
    integration alone would need more abscissas than 1.5 x 3 / sqrt(acc), so the auxiliary one runs first."""
    rng = _seed(99, r, len(head))
    lam = np.r_[np.sort(3e-4 * (1.0 + rng.random(r - len(head)))), np.asarray(head, float)]
    assert np.all(np.diff(lam) > 0) and np.all(lam > lam.mean() / 1e5)
    return lam


def kept(lam):
    """SKAT's Get_Lambda filter as the kernel applies it."""
    lam = np.asarray(lam, float)
    nonneg = lam[lam >= 0]
    return lam[lam > nonneg.sum() / nonneg.size / 100000.0]


def filter_rows(k):
    """Rows of k weights of which the filter leaves r < k: most weights scaled by 1e-9, a few set to -1e-12; the last row
    keeps a single weight (Liu's value is returned)."""
    rng = _seed(7, k)
    rows = []
    for i, (survivors, frac) in enumerate(((5, 2.0), (k - 3, 1.0), (64, 4.0), (1, 3.0))):
        lam = np.sort(rng.gamma(0.7, 1.0, size=k) + 1e-3)
        lam[: k - survivors] *= 1e-9
        lam[: min(3, k - survivors)] = -1e-12
        lam = np.sort(lam)
        assert kept(lam).size == survivors
        rows.append(Case(f"filter-k{k}-keep{survivors}", k, lam, frac * kept(lam).sum(), "filter"))
    return rows


def _build():
    cases = []
    for r in WIDTHS:
        for shape in SHAPES:
            lam = weights(shape, r)
            for f in Q_FRACTIONS:
                cases.append(Case(f"{shape}-r{r}-q{f:g}", r, lam, f * lam.sum(), "davies"))
        lam = weights("gamma", r)
        for f in EARLY_FRACTIONS:
            cases.append(Case(f"early-r{r}-q{f:g}", r, lam, f * lam.sum(), "early"))
        for shape in ("gamma", "flat"):
            lam = weights(shape, r)
            for f in LIU_FAR_FRACTIONS:
                cases.append(Case(f"liufar-{shape}-r{r}-q{f:g}", r, lam, f * lam.sum(), "liu_far"))
    for r in AUX_WIDTHS:
        for head in AUX_HEADS:
            lam = aux_weights(head, r)
            for q in AUX_Q:
                cases.append(Case(f"aux-r{r}-head{len(head)}-q{q:g}", r, lam, q, "aux"))
    for k in FILTER_WIDTHS:
        cases.extend(filter_rows(k))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


CASES = _build()


def by_width():
    """{k: [cases]} in table order: one launch of the hook per width."""
    out = {}
    for c in CASES:
        out.setdefault(c.k, []).append(c)
    return out
