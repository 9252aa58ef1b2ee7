"""Cohorts whose donor-level panels hand variants at CHOSEN positions from the collapsed path to the dense one (plain helper
module, not a test; tests/test_gpu_dense_repeats.py and tests/test_dense_repeat_cases_cpu.py use it).

A grouped panel is scanned on the collapsed path; a variant that keeps less than COLLINEAR_TAU = 1e-2 of its squared norm
outside span(W) is scanned again on the dense path and that result overwrites the first (csrc/scan.hip: scan_core).  The
repeats are host-side index arithmetic, restated here as the documentation gives it (``repeat_runs``):

  * the marked variants of a call over ``count`` variants, as positions relative to its first variant, in order;
  * more than a quarter of the call's variants marked: one run over everything;
  * otherwise neighbours at most 32 variants apart merge into one run ``(off, len)``, unmarked variants between them included.

Cohort: 9 donors of 5 .. 37 cells (203 cells: no multiple of 16, one donor below 16 cells), cells shuffled; 3 contexts;
W = [1, w[donor], z] with w donor-level and z cell-level noise.  Every genotype column is donor-constant:

  * ordinary columns: donor-level normal draws that keep at least 0.1 of ||g||^2 outside span(W) (a factor 10 above tau);
  * marked columns: g = W[:, :2] a + e u with u donor-constant, orthogonal to span(W) and of unit norm, and e such that
    e^2 / ||g||^2 = 1e-3 (a factor 10 below tau).  Every marked column has its own a, and the phenotype carries a planted
    GxE effect of every marked column, so that neighbouring variants differ clearly in Q and p.

``shares`` evaluates every column's share in float64 by lstsq and ``layout`` asserts both margins on what it returns.

The "dosages" layout is ordinary input that takes the same path: unstandardised int8 allele counts with W = [1]; three
columns mid-panel are 2 on every donor but the one of 5 cells, which has 1 -- 0.6 % of ||g||^2 outside span(1)."""
from types import SimpleNamespace

import numpy as np

CELLS = (5, 17, 19, 21, 23, 24, 27, 30, 37)
K0 = 3
TAU = 1e-2                      # csrc/scan_pass.h: COLLINEAR_TAU
MARKED_SHARE, ORDINARY_SHARE = 1e-3, 0.1
MERGE_GAP = 32

#: name -> (variants of the panel, marked columns, first, count of the call)
LAYOUTS = {
    # runs [3, 34] (gap 31: merged), [67, 67] (gap 33: separate), [127, 128] (across the boundary of 128-variant blocks)
    # and [299, 299] (the last variant)
    "scattered": (300, (3, 34, 67, 127, 128, 299), 0, 300),
    # the same columns with two more marks, called over [130, 280): runs at offsets 1 and 132, both > 0
    "window": (300, (3, 34, 67, 127, 128, 131, 262, 299), 130, 150),
    # 11 of 40: more than a quarter, the whole range again
    "quarter": (40, (1, 4, 5, 9, 13, 18, 22, 27, 31, 36, 39), 0, 40),
    "dosages": (24, (9, 11, 14), 0, 24),
}


def repeat_runs(marked, count):
    """[(off, len)] of the dense repeats of a call over ``count`` variants whose marked positions (relative to the call's
    first variant) are ``marked``."""
    near = sorted(int(v) for v in marked)
    assert all(0 <= v < count for v in near) and len(set(near)) == len(near)
    if not near:
        return []
    if 4 * len(near) > count:
        return [(0, int(count))]
    runs, start, last = [], near[0], near[0]
    for v in near[1:]:
        if v - last > MERGE_GAP:
            runs.append((start, last - start + 1))
            start = v
        last = v
    runs.append((start, last - start + 1))
    return runs


def shares(G, W):
    """Per column of G: the share of its squared norm outside span(W), in float64 by least squares."""
    G, W = np.asarray(G, float), np.asarray(W, float)
    coef = np.linalg.lstsq(W, G, rcond=None)[0]
    R = G - W @ coef
    return np.sum(R * R, axis=0) / np.sum(G * G, axis=0)


_base = {}


def base(seed=11):
    """(y, E, hK, donor_of_cell, W) of the cohort, cells shuffled; built once and left unchanged."""
    if seed not in _base:
        from cellregmap_amd.synth import make_cohort

        assert sum(CELLS) == 203 and sum(CELLS) % 16 != 0 and min(CELLS) < 16 and len(CELLS) == 9
        c = make_cohort(len(CELLS), max(CELLS), K0, 1, seed=seed, g_causals=(), gxe_causals=())
        rng = np.random.default_rng(seed)
        keep = np.concatenate([np.flatnonzero(c.donor_of_cell == d)[:m] for d, m in enumerate(CELLS)])
        keep = keep[rng.permutation(keep.size)]
        donor = c.donor_of_cell[keep]
        w = rng.normal(size=len(CELLS))
        W = np.column_stack([np.ones(keep.size), w[donor], rng.normal(size=keep.size)])
        _base[seed] = SimpleNamespace(y=c.y[keep], E=c.E[keep], hK=c.hK[keep], donor=donor, W=W)
    return _base[seed]


def _donor_constant_complement(b):
    """Orthonormal basis (cells x 6) of the donor-constant vectors orthogonal to span(W).  A donor-constant u is orthogonal
    to the cell-level column z exactly when it is orthogonal to z's donor means."""
    m = len(CELLS)
    Z = np.zeros((b.y.size, m))
    Z[np.arange(b.y.size), b.donor] = 1.0
    counts = Z.sum(0)
    against = Z.T @ b.W                                  # u_d . (Z' W) = u' W for u = Z u_d
    # null space of against' in the donor coordinates, made orthonormal in the cell metric diag(counts)
    _, _, Vt = np.linalg.svd((against / np.sqrt(counts)[:, None]).T)
    Ud = Vt[b.W.shape[1]:].T / np.sqrt(counts)[:, None]     # m x (m - 3)
    U = Z @ Ud
    assert np.abs(U.T @ U - np.eye(U.shape[1])).max() < 1e-12 and np.abs(b.W.T @ U).max() < 1e-11
    return Ud


_layouts = {}


def layout(name, seed=11):
    """The named layout: ``Gd`` (donors x variants), ``donor`` (cells,), ``G`` = Gd[donor], ``marked`` (columns of the
    panel), ``first``/``count`` of the call, ``in_range`` (marked positions relative to ``first``), ``runs``, and the
    cohort's ``y`` (with the planted effects), ``E``, ``hK``, ``W``; ``dosage`` (int8) for "dosages".  Built once."""
    if (name, seed) in _layouts:
        return _layouts[(name, seed)]
    p, marked, first, count = LAYOUTS[name]
    b = base(seed)
    rng = np.random.default_rng([seed, sorted(LAYOUTS).index("scattered" if name == "window" else name)])
    m, n = len(CELLS), b.y.size
    out = SimpleNamespace(name=name, donor=b.donor, E=b.E, hK=b.hK, marked=tuple(marked), first=first, count=count,
                          dosage=None)
    if name == "dosages":
        out.W = np.ones((n, 1))
        maf = rng.uniform(0.2, 0.5, size=p)
        Gd = np.zeros((m, p), np.int8)
        for j in range(p):
            while True:
                col = rng.binomial(2, maf[j], size=m).astype(np.int8)
                if col.std() > 0 and shares(col[b.donor, None].astype(float), out.W)[0] >= ORDINARY_SHARE:
                    break
            Gd[:, j] = col
        for j in marked:                                 # the common homozygote on every donor but the smallest
            Gd[:, j] = 2
            Gd[int(np.argmin(CELLS)), j] = 1
        out.dosage = Gd
        out.Gd = Gd.astype(float)
        out.marked_max, out.ordinary_min = 0.7 * TAU, ORDINARY_SHARE       # (0.6 % by the arithmetic of the docstring)
        out.y = b.y.copy()
    else:
        out.W = b.W
        Ud = _donor_constant_complement(b)
        Gd = np.empty((m, p))
        for j in range(p):
            while True:
                col = rng.normal(size=m)
                if shares(col[b.donor, None], b.W)[0] >= 1.5 * ORDINARY_SHARE:
                    break
            Gd[:, j] = col
        # (drawn for every column, so that "window" holds the columns of "scattered" with two more marks)
        a = np.column_stack([rng.choice([-1.0, 1.0], size=p) * rng.uniform(0.5, 2.0, size=p), rng.normal(size=p)])
        mix = rng.normal(size=(p, Ud.shape[1]))
        alpha = rng.normal(size=(p, K0))
        y = b.y.copy()
        Wd = np.column_stack([np.ones(m), [b.W[b.donor == d, 1][0] for d in range(m)]])
        for j in marked:
            in_span = Wd @ a[j]
            norm2 = float(np.sum(in_span[b.donor] ** 2))
            u = Ud @ (mix[j] / np.linalg.norm(mix[j]))             # unit norm over the cells
            Gd[:, j] = in_span + np.sqrt(MARKED_SHARE / (1.0 - MARKED_SHARE) * norm2) * u
            g = Gd[b.donor, j]
            y = y + 0.25 * (1 + marked.index(j) % 3) * g / np.sqrt(np.mean(g * g)) * (b.E @ alpha[j])
        out.Gd = Gd
        out.marked_max, out.ordinary_min = 1.001 * MARKED_SHARE, ORDINARY_SHARE
        out.y = y
    out.G = np.ascontiguousarray(out.Gd[b.donor])
    out.in_range = tuple(j - first for j in marked if first <= j < first + count)
    out.runs = repeat_runs(out.in_range, count)
    check_margins(out)
    _layouts[(name, seed)] = out
    return out


def check_margins(lay):
    """Marked columns a clear factor under tau, every other a factor 10 above it; returns the shares."""
    s = shares(lay.G, lay.W)
    is_marked = np.zeros(s.size, bool)
    is_marked[list(lay.marked)] = True
    assert np.all(s[is_marked] <= lay.marked_max) and lay.marked_max < TAU, (lay.name, s[is_marked])
    assert np.all(s[~is_marked] >= lay.ordinary_min) and lay.ordinary_min >= 10 * TAU, (lay.name, s[~is_marked].min())
    if lay.dosage is None:
        assert np.all(np.abs(s[is_marked] / MARKED_SHARE - 1) < 1e-6), s[is_marked]
    return s
