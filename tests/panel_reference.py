"""Long-double reference of what the genotype panel builders put on the device, and the cohorts both the CPU and the GPU
tests of the builders run on.  Plain numpy: no GPU, no library import.

From donor-level int8 dosages ``D`` (m x p) and the donor index of every cell, the standardised panel is, per variant j,

    w_d    = cells of donor d,            n = sum_d w_d
    mean_j = sum_d w_d D_dj / n
    var_j  = sum_d w_d (D_dj - mean_j)^2 / n          (population variance of the EXPANDED column)
    ref_dj = (D_dj - mean_j) / sqrt(var_j)

all in ``numpy.longdouble`` (64-bit mantissa: eps 1.1e-19, 2000 times below float64's).

The bound a float64 implementation is held to is a priori -- it comes from the operations, not from any implementation:

    |got_dj - ref_dj| <= 2^-52 * ( (|D_dj| + |mean_j|) / sd_j  +  (m + 8) |ref_dj| )

First term: the mean is one rounded quotient of an exact integer sum (relative error u = 2^-53) and the difference
D - mean one more rounding, at most u (|D| + |mean|) absolute each side of it -- 2^-52 takes both -- carried through the
division by sd.  Second term: var is a sum of m non-negative terms, whatever the order or the tree (relative error at most
(m - 1) u, plus 3 u per term for the products and the perturbed differences, already counted above to first order), and the
square root halves it; the division by n, the square root, the final division and its rounding are one u each: (m + 8) * 2^-52
leaves a factor of two over m u / 2 + 4 u and does not grow with the size of the dosages.

Monomorphic variants: a variant is monomorphic -- and cannot be standardised -- when its EXPANDED column has zero variance,
i.e. when all donors that have at least one cell carry the same dosage.  A donor without cells does not count.
"""
import numpy as np

LD = np.longdouble
if np.finfo(LD).eps > 1e-18:
    raise RuntimeError("numpy.longdouble on this host has eps %.3g: the panel reference needs an extended type "
                       "(eps <= 1e-18) and does not stand in for one with float64" % float(np.finfo(LD).eps))

U2 = 2.0 ** -52


def cell_counts(donor_of_cell, m):
    """w_d: the number of cells of every donor (int64, length m)."""
    donor_of_cell = np.asarray(donor_of_cell)
    assert donor_of_cell.ndim == 1 and donor_of_cell.min() >= 0 and donor_of_cell.max() < m
    return np.bincount(donor_of_cell, minlength=m).astype(np.int64)


def moments(D, donor_of_cell):
    """``(w, n, mean, var)`` of the expanded columns: w int64 (m,), n int, mean and var longdouble (p,)."""
    D = np.asarray(D)
    assert D.ndim == 2 and D.dtype == np.int8
    w = cell_counts(donor_of_cell, D.shape[0])
    n = int(w.sum())
    wl, Dl = w.astype(LD)[:, None], D.astype(LD)
    mean = (wl * Dl).sum(0) / LD(n)
    var = (wl * (Dl - mean) ** 2).sum(0) / LD(n)
    return w, n, mean, var


def monomorphic(D, donor_of_cell):
    """bool (p,): the variants whose expanded column has zero variance (decided on the integers, no rounding)."""
    D = np.asarray(D)
    held = D[cell_counts(donor_of_cell, D.shape[0]) > 0]
    return (held == held[0]).all(0)


def standardised(D, donor_of_cell):
    """``(ref, bound)``: the standardised donor-level panel in longdouble (m x p) and the a-priori bound (float64, m x p) on
    |got - ref| of a float64 implementation.  Refuses monomorphic variants."""
    D = np.asarray(D)
    if monomorphic(D, donor_of_cell).any():
        raise ValueError("a monomorphic variant cannot be standardised")
    _, _, mean, var = moments(D, donor_of_cell)
    sd = np.sqrt(var)
    Dl = D.astype(LD)
    ref = (Dl - mean) / sd
    bound = LD(U2) * ((np.abs(Dl) + np.abs(mean)) / sd + LD(D.shape[0] + 8) * np.abs(ref))
    return ref, bound.astype(np.float64)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the entries (the comparison is made in longdouble)."""
    return float((np.abs(np.asarray(got).astype(LD) - ref) / bound.astype(LD)).max())


def indicator(donor_of_cell, m):
    """Z (n x m float64): Z[i, d] = 1 where cell i belongs to donor d, else 0."""
    donor_of_cell = np.asarray(donor_of_cell)
    Z = np.zeros((donor_of_cell.shape[0], m))
    Z[np.arange(donor_of_cell.shape[0]), donor_of_cell] = 1.0
    return Z


# ---- the cohorts -----------------------------------------------------------------------------------------------------
# name -> (donors m, variants p, leading dimension of the int8 source, donor left without a cell or None)
COHORTS = {"a": (9, 1, 1, None), "b": (65, 7, 7, None), "c": (257, 129, 140, None), "d": (300, 128, 128, 17)}
# the kinds of column, dealt in turn: allele frequency 0.5 / 0.2 / 0.05, a single carrier donor, dosages offset to the top
# and to the bottom of the int8 range (where the raw-moment form of the variance cancels)
KINDS = ("af50", "af20", "af05", "single", "top", "bottom")
_cache = {}


def _column(kind, m, has_cells, rng):
    if kind == "single":
        col = np.zeros(m, np.int64)
        col[rng.choice(np.flatnonzero(has_cells))] = 1
        return col
    af = {"af50": 0.5, "af20": 0.2, "af05": 0.05, "top": 0.3, "bottom": 0.3}[kind]
    col = rng.binomial(2, af, size=m)
    held = np.flatnonzero(has_cells)
    if (col[held] == col[held[0]]).all():       # (a rare allele among few donors: give one donor a copy)
        col[held[-1]] = (col[held[-1]] + 1) % 3
    return col + {"top": 120, "bottom": -128}.get(kind, 0)


def cohort(name):
    """The cohort of that name (built once per process, arrays read-only): a dict with ``D`` int8 (m x p), ``wide`` -- the int8
    matrix (m x ldd) of which D is the column window starting at ``col0`` --, ``donor_of_cell`` int32 (n,) in shuffled cell
    order with 1..12 cells per donor (none for ``empty_donor``), ``kinds`` (the kind of every column), ``m``, ``p``, ``ldd``."""
    if name in _cache:
        return _cache[name]
    m, p, ldd, empty = COHORTS[name]
    rng = np.random.default_rng([0x9A4E1, sorted(COHORTS).index(name)])
    cells = rng.integers(1, 13, size=m)
    if empty is not None:
        cells[empty] = 0
    donor_of_cell = rng.permutation(np.repeat(np.arange(m), cells)).astype(np.int32)
    kinds = [KINDS[j % len(KINDS)] for j in range(p)]
    D = np.stack([_column(k, m, cells > 0, rng) for k in kinds], axis=1).astype(np.int8)
    col0 = (ldd - p) // 2
    wide = rng.integers(-128, 128, size=(m, ldd)).astype(np.int8)
    wide[:, col0:col0 + p] = D
    out = {"name": name, "m": m, "p": p, "ldd": ldd, "col0": col0, "empty_donor": empty, "kinds": kinds,
           "D": np.ascontiguousarray(wide[:, col0:col0 + p]), "wide": wide, "donor_of_cell": donor_of_cell}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[name] = out
    return out
