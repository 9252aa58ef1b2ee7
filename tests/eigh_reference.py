"""A long-double reference for the symmetric eigenproblem, the error measures and the bound that the eigen-solver tests
share, and the builders of their cases (tests/test_eigh_reference_cpu.py keeps all of it honest on the CPU;
tests/test_gpu_eigh_edges.py and tests/test_gpu_eigh2_edges.py hold the device to it).

Reference: Householder tridiagonalisation of the dense matrix and Sturm-count bisection of the tridiagonal, vectorised over
the eigenvalue index, 90 halvings of the Gershgorin interval -- plain numpy in ``np.longdouble`` (64-bit mantissa on x86:
eps 1.1e-19, and an exponent range in which the square of 1e-200 does not underflow).

Measures of a candidate (lam, Z) of A, formed in long double:
    eig    max |lam - ref|
    resid  max |A - Z diag(lam) Z'|
    orth   max |Z'Z - I|

Bound: each measure <= FACTOR * max(LAPACK's value of the same measure on the same matrix, n * eps * scale), with
scale = max |ref| (1 for orth), eps = 2.2e-16.  LAPACK is ``np.linalg.eigh`` (resid, orth) and ``np.linalg.eigvalsh``
(eig).  The floor n * eps * scale is the textbook backward-stability order: it keeps a matrix on which LAPACK happens to be
exact from demanding exactness.  FACTOR = 8 is a margin over an independent backward-stable solver of the same precision
(the device sums in another order, on the FP64 matrix pipe).
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(float).eps)
FACTOR = 8.0
HALVINGS = 90
MEASURES = ("eig", "resid", "orth")


# ---- the reference ----------------------------------------------------------------------------------------------------
def tridiagonalise(A):
    """(d, e) of Q'AQ for a dense symmetric A, by Householder reflections in long double."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    for k in range(n - 2):
        x = A[k + 1:, k]
        s2 = np.dot(x[1:], x[1:])
        if s2 == 0:
            continue
        alpha = x[0]
        nrm = np.sqrt(alpha * alpha + s2)
        beta = -nrm if alpha >= 0 else nrm
        tau = (beta - alpha) / beta
        v = x / (alpha - beta)
        v[0] = 1
        A22 = A[k + 1:, k + 1:]
        p = tau * (A22 @ v)
        w = p - (tau * np.dot(p, v) / 2) * v
        A22 -= np.outer(v, w) + np.outer(w, v)
        A[k + 1:, k] = 0
        A[k + 1, k] = beta
        A[k, k + 1:] = A[k + 1:, k]
    return np.diag(A).copy(), np.diag(A, -1).copy()


def tridiagonal_eigenvalues(d, e):
    """Ascending eigenvalues of T(d, e) by bisection on the Sturm count (number of eigenvalues below x = number of
    negative pivots of T - x I), all indices at once."""
    d = np.asarray(d, dtype=LD)
    n = d.size
    e = np.asarray(e, dtype=LD)[: n - 1]
    if n == 1:
        return d.copy()
    e2 = e * e
    ae = np.abs(e)
    rad = np.r_[ae, LD(0)] + np.r_[LD(0), ae]
    glo, ghi = (d - rad).min(), (d + rad).max()
    span = max(ghi - glo, abs(glo), abs(ghi))
    glo, ghi = glo - span * LD(2) ** -60, ghi + span * LD(2) ** -60
    pivmin = np.finfo(LD).tiny * max(LD(1), e2.max())
    lo = np.full(n, glo, dtype=LD)
    hi = np.full(n, ghi, dtype=LD)
    idx = np.arange(n)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for _ in range(HALVINGS):
            x = (lo + hi) / 2
            q = d[0] - x
            q = np.where(np.abs(q) < pivmin, -pivmin, q)
            count = (q < 0).astype(np.int64)
            for i in range(1, n):
                q = d[i] - x - e2[i - 1] / q
                q = np.where(np.abs(q) < pivmin, -pivmin, q)
                count += q < 0
            below = count > idx          # at least idx + 1 eigenvalues lie below x: eigenvalue idx is below x
            hi = np.where(below, x, hi)
            lo = np.where(below, lo, x)
    return (lo + hi) / 2


def is_tridiagonal(A):
    A = np.asarray(A)
    return A.shape[0] < 3 or not np.any(np.tril(A, -2))


def reference_eigenvalues(A):
    """Ascending eigenvalues of the symmetric A in long double (a tridiagonal A goes to the bisection as it is)."""
    A = np.asarray(A)
    if is_tridiagonal(A):
        return tridiagonal_eigenvalues(np.diag(A), np.diag(A, -1))
    return tridiagonal_eigenvalues(*tridiagonalise(A))


# ---- measures and the bound -------------------------------------------------------------------------------------------
def measures(A, lam, Z, ref):
    """(eig, resid, orth) of the candidate (lam, Z) of A, formed in long double."""
    A, lam, Z = np.asarray(A, dtype=LD), np.asarray(lam, dtype=LD), np.asarray(Z, dtype=LD)
    n = A.shape[0]
    eig = np.abs(lam - ref).max()
    resid = np.abs(A - (Z * lam) @ Z.T).max()
    orth = np.abs(Z.T @ Z - np.eye(n, dtype=LD)).max()
    return float(eig), float(resid), float(orth)


def lapack_measures(A, ref):
    A = np.asarray(A, dtype=float)
    lam, Z = np.linalg.eigh(A)
    _, resid, orth = measures(A, lam, Z, ref)
    eig = float(np.abs(np.linalg.eigvalsh(A).astype(LD) - ref).max())
    return eig, resid, orth


def floors(n, ref):
    scale = float(np.abs(ref).max())
    return n * EPS * scale, n * EPS * scale, n * EPS


class Held:
    """One candidate against the bound: ``dev``, ``lapack``, ``limit`` and ``ratio`` (the device's measure over
    max(LAPACK's, floor)) per measure, ``violations`` as a list of texts."""

    def __init__(self, name, A, lam, Z, ref=None, factor=FACTOR, lapack=None):
        A = np.asarray(A, dtype=float)
        self.name, self.n = name, A.shape[0]
        self.ref = reference_eigenvalues(A) if ref is None else ref
        self.dev = measures(A, lam, Z, self.ref)
        self.lapack = lapack_measures(A, self.ref) if lapack is None else lapack
        base = [max(l, f) for l, f in zip(self.lapack, floors(self.n, self.ref))]
        self.limit = [factor * b for b in base]
        self.ratio = [dv / b if b > 0 else (0.0 if dv == 0 else np.inf) for dv, b in zip(self.dev, base)]
        finite = bool(np.all(np.isfinite(lam)) and np.all(np.isfinite(Z)))
        self.violations = [f"{name} (n = {self.n}): {m} {dv:.3e} > {lim:.3e} (LAPACK {la:.3e}, ratio {r:.1f})"
                           for m, dv, lim, la, r in zip(MEASURES, self.dev, self.limit, self.lapack, self.ratio)
                           if not dv <= lim]
        if not finite:
            self.violations.append(f"{name} (n = {self.n}): not finite")

    def line(self):
        f = lambda t: " ".join(f"{x:9.2e}" for x in t)  # noqa: E731
        return (f"[eigh-hold] {self.name:<46s} n={self.n:<5d} dev {f(self.dev)} | lapack {f(self.lapack)} | ratio "
                + " ".join(f"{r:6.2f}" for r in self.ratio))


def hold(name, A, lam, Z, ref=None, factor=FACTOR):
    """Print the case's line (device, LAPACK, ratio per measure) and return the violated measures as texts."""
    h = Held(name, A, lam, Z, ref=ref, factor=factor)
    print(h.line())
    return h.violations


def hold_spectrum(name, lam, A, ref=None, factor=FACTOR):
    """The eigenvalue measure alone (a candidate spectrum without vectors)."""
    A = np.asarray(A, dtype=float)
    n = A.shape[0]
    ref = reference_eigenvalues(A) if ref is None else ref
    dev = float(np.abs(np.asarray(lam, dtype=LD) - ref).max())
    la = float(np.abs(np.linalg.eigvalsh(A).astype(LD) - ref).max())
    base = max(la, floors(n, ref)[0])
    ratio = dev / base if base > 0 else (0.0 if dev == 0 else np.inf)
    print(f"[eigh-hold] {name:<46s} n={n:<5d} dev {dev:9.2e} | lapack {la:9.2e} | ratio {ratio:6.2f}")
    ok = dev <= factor * base and bool(np.all(np.isfinite(lam)))
    return [] if ok else [f"{name} (n = {n}): eig {dev:.3e} > {factor * base:.3e} (LAPACK {la:.3e}, ratio {ratio:.1f})"]


# ---- cases ------------------------------------------------------------------------------------------------------------
def tridiag(d, e):
    d, e = np.asarray(d, float), np.asarray(e, float)
    n = d.size
    return np.diag(d) + np.diag(e[: n - 1], 1) + np.diag(e[: n - 1], -1)


def top_split(n):
    """Where the divide-and-conquer tree (eigh_dc.hip: build_tree) cuts a tridiagonal of order n first."""
    return ((n + 15) // 16 // 2) * 16


DC_ORDERS = (32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 130, 256, 257)
DC_ORDERS_ALL_STRUCTURES = (33, 65, 129, 257)
DC_FEW = ("a", "b", "c", "d")
DC_ALL = ("a", "b", "c", "d", "e", "f", "g", "h", "i")


def dc_structure(kind, n):
    """(d, e) of the tridiagonal of order n that puts the top merge (cut after row m - 1, m = top_split(n)) into the state
    named in the module that uses it:
      a  distinct diagonal, one coupling e[m-1]: z has two non-zeros, k = 2
      b  the same with d[m-1] == d[m]: the pair rotates into one pole, k = 1
      c  e[m-1] = 0 exactly, both halves coupled inside: rho = 0, k = 0
      d  a block and its mirror image glued by 1e-9 at the cut (mirrored, so that the cut's d[m-1] -= |e|, d[m] -= |e| meets
         corresponding entries and the halves stay twins): every surviving pole has a twin and rotates into it
      e  Wilkinson's W+ of that order
      f  diagonal logspace(0, -12, n), couplings 1e-3 of the geometric mean of their neighbours
      g  constant diagonal and couplings (1-2-1 Toeplitz): nothing deflates, k = n
      h  couplings of 1e-200, whose squares underflow in double
      i  a random tridiagonal: many poles, partial deflation (its eigenvectors localise, so from order 65 up a share of z
         falls under the tolerance; the structure in which nothing deflates is g)
    """
    m = top_split(n)
    rng = np.random.default_rng(1000 * n + ord(kind))
    e = np.zeros(n)
    if kind in ("a", "b"):
        d = rng.permutation(np.linspace(1.0, 2.0, n))
        if kind == "b":
            d[m] = d[m - 1]
        e[m - 1] = 0.5
    elif kind == "c":
        d = rng.normal(size=n)
        e[: n - 1] = rng.normal(size=n - 1)
        e[m - 1] = 0.0
    elif kind == "d":
        h = min(m, n - m)
        bd, be = rng.normal(size=h), rng.normal(size=h - 1)
        d = 3.0 + np.arange(n) / n           # the rows outside the two blocks: distinct, uncoupled
        d[m - h:m], e[m - h:m - 1] = bd, be
        d[m:m + h], e[m:m + h - 1] = bd[::-1], be[::-1]
        e[m - 1] = 1e-9
    elif kind == "e":
        d = np.abs(np.arange(n) - (n - 1) / 2.0)
        e[: n - 1] = 1.0
    elif kind == "f":
        d = np.logspace(0, -12, n)
        e[: n - 1] = 1e-3 * np.sqrt(d[:-1] * d[1:])
    elif kind == "g":
        d = np.full(n, 2.0)
        e[: n - 1] = -1.0
    elif kind == "h":
        d = rng.permutation(np.linspace(1.0, 2.0, n))
        e[: n - 1] = 1e-200
    elif kind == "i":
        d = rng.normal(size=n)
        e[: n - 1] = rng.normal(size=n - 1)
    else:
        raise ValueError(kind)
    return d, e


def top_merge_inputs(d, e):
    """What the top merge of the divide-and-conquer tree sees of T(d, e): the cut halves' spectra (lam), the last row of the
    left half's vectors and the first row of the right half's (z), the size of the left half and the coupling -- the
    arguments of the deflation plan (eigh_dc.hip: plan_merge; hook crm_test_dc_plan).  The halves by LAPACK."""
    d, e = np.array(d, float), np.asarray(e, float)
    n = d.size
    m = top_split(n)
    beta = e[m - 1]
    d[m - 1] -= abs(beta)
    d[m] -= abs(beta)
    l1, Q1 = np.linalg.eigh(tridiag(d[:m], e[:m - 1]))
    l2, Q2 = np.linalg.eigh(tridiag(d[m:], e[m:n - 1]))
    return np.r_[l1, l2], np.r_[Q1[-1], Q2[0]], m, beta


def dc_cases(n):
    kinds = DC_ALL if n in DC_ORDERS_ALL_STRUCTURES else DC_FEW
    return {k: tridiag(*dc_structure(k, n)) for k in kinds}


def dc_batch(n=97):
    """One batched call whose matrices deflate differently: c, d, e, i and the identity."""
    names = ["c", "d", "e", "i", "identity"]
    return names, np.stack([tridiag(*dc_structure(k, n)) for k in names[:4]] + [np.eye(n)])


def background_kinds(n=130, seed=0):
    """Dense matrices of the kinds a background has (tests/test_gpu_eigh.py), at order n."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    X = rng.normal(size=(n, 40))
    third = [n - 2 * (n // 3), n // 3, n // 3]
    cases = {
        "rank-40 Gram": X @ X.T,
        "three clusters": (Q * np.repeat([1.0, 2.0, 3.0], third)) @ Q.T,
        "graded over 12 decades": (Q * np.logspace(0, -12, n)) @ Q.T,
    }
    H = rng.normal(size=(2 * n + 40, n))
    C = H.T @ H
    for rho in (0.0, 1.0):
        D = np.r_[np.full(10, np.sqrt(rho)), np.full(n - 10, np.sqrt(1 - rho))]
        cases[f"D C D rho={rho:g}"] = D[:, None] * C * D[None, :]
    return {k: 0.5 * (A + A.T) for k, A in cases.items()}


def graded_gram(dim, seed, decades):
    """H'H with the columns of H graded over `decades` decades (the 256-reflector back-transformation's matrices)."""
    rng = np.random.default_rng(seed)
    H = rng.normal(size=(dim + 200, dim)) * np.logspace(0, -decades, dim)
    return H.T @ H


def family_scaling(dim, rho, lead=64):
    """The diagonal of D(rho) of the two-stage solver's family: sqrt(rho) on the leading block, sqrt(1 - rho) behind."""
    return np.r_[np.full(lead, np.sqrt(rho)), np.full(max(dim - lead, 0), np.sqrt(1 - rho))][:dim]


# ---- planted slips (what the measures must see) -----------------------------------------------------------------------
def slip_eigenvalue(lam, Z, scale):
    lam = lam.copy()
    lam[lam.size // 2] += 1e-12 * scale
    return lam, Z


def slip_swapped_columns(lam, Z, scale):
    Z = Z.copy()
    j = lam.size // 2
    Z[:, [j, j + 1]] = Z[:, [j + 1, j]]
    return lam, Z


def slip_rotated_column(lam, Z, scale):
    Z = Z.copy()
    j = lam.size // 2
    Z[:, j] = Z[:, j] + 1e-11 * Z[:, j + 1]
    return lam, Z


SLIPS = {"eigenvalue moved by 1e-12 scale": slip_eigenvalue, "two columns swapped": slip_swapped_columns,
         "column rotated by 1e-11": slip_rotated_column}
